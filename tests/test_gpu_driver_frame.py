"""What the driver-loop frame (csrc/driver_loop.hpp) owns, for every agent whose kernel is written on it: the learner's state / action / episode-step
load and store, the step cap, the five statistics and both episode-end conventions.

Per row: 130 learners (two waves and a two-lane tail inside one 256-thread block), max_episode_steps = 7, a fixed seed, train(40) with
statistics; then the same run cut as train(13) + train(27) in a second ctx, and as train(3) + train(37) in a third: CartPole's terminal episodes
all end within the first 7 steps, so only a cut below 7 puts some of them in the second launch.
  MountainCar order 1   no episode reaches the goal in 7 steps: truncation only
  CartPole order 1      episodes end both ways.  From the restart state no pole falls within 7 steps (a constant push needs 9), so the learners
                        start from pole angles spread over (-0.2, 0.2) rad of the +-0.209 rad limit: the outer ones fall in their first episode
EXPECTED was recorded from the library as it stood BEFORE the frame existed (the parent commit's build, loaded through RSRL_HIP_LIB), with
`python tests/test_gpu_driver_frame.py`: the integers as they are, the two f32-per-launch sums by their f64 bit pattern, the final states, actions
and episode steps by a digest.  Every recorded row has episodes_truncated > 0, every CartPole row episodes > episodes_truncated."""
import hashlib
import struct

import numpy as np
import pytest

import rsrl_amd as ra

pytestmark = pytest.mark.gpu

N, CAP, STEPS, CUTS, SEED = 130, 7, 40, (13, 3), 11
EG, SM = dict(policy=ra.EPSILON_GREEDY), dict(policy=ra.SOFTMAX, alpha=0.001)
AGENTS = {
    "TD": dict(algo=ra.TD, policy=ra.RANDOM),
    "TDLambda": dict(algo=ra.TD_LAMBDA, policy=ra.RANDOM, lam=0.5),
    "GreedyGQ": dict(algo=ra.GREEDY_GQ, lr_td=0.001, **EG),
    "SARSALambda": dict(algo=ra.SARSA_LAMBDA, lam=0.5, **EG),
    "QLambda": dict(algo=ra.Q_LAMBDA, lam=0.5, **EG),
    "QSigma": dict(algo=ra.Q_SIGMA, sigma=0.5, n_steps=2, **EG),
    "ActorCritic": dict(algo=ra.ACTOR_CRITIC, **SM),
    "QActorCritic": dict(algo=ra.Q_ACTOR_CRITIC, **SM),
    "TDActorCritic": dict(algo=ra.TD_ACTOR_CRITIC, **SM),
    "REINFORCE": dict(algo=ra.REINFORCE, **SM),
    "BaselineREINFORCE": dict(algo=ra.BASELINE_REINFORCE, **SM),
}
DOMAINS = {"MountainCar": ra.MOUNTAIN_CAR, "CartPole": ra.CART_POLE}
ROWS = [(d, a) for d in DOMAINS for a in AGENTS]
INTS = ("env_steps", "episodes", "episodes_truncated", "sum_episode_steps")

# (domain, agent): (env_steps, episodes, episodes_truncated, sum_episode_steps, sum_abs_td_error bits, sum_reward bits, digest)
EXPECTED = {
    ('MountainCar', 'TD'): (5200, 650, 650, 4550, '0000c0b4633ab440', '000000000050b4c0', 'c39561aa438ad717'),
    ('MountainCar', 'TDLambda'): (5200, 650, 650, 4550, '0000801bdec4a440', '000000000050b4c0', 'c39561aa438ad717'),
    ('MountainCar', 'GreedyGQ'): (5200, 650, 650, 4550, '000040f2d345b440', '000000000050b4c0', 'd1a401e1e081bf31'),
    ('MountainCar', 'SARSALambda'): (5200, 650, 650, 4550, '00002017f25db140', '000000000050b4c0', '3a95291cfed50add'),
    ('MountainCar', 'QLambda'): (5200, 650, 650, 4550, '0000c074f9d0af40', '000000000050b4c0', '44a420d8b59680e8'),
    ('MountainCar', 'QSigma'): (5200, 650, 650, 4550, '0000c06df73eb440', '000000000050b4c0', '75cc682eb3f46ca0'),
    ('MountainCar', 'ActorCritic'): (5200, 650, 650, 4550, '000080366f4bb440', '000000000050b4c0', 'c39561aa438ad717'),
    ('MountainCar', 'QActorCritic'): (5200, 650, 650, 4550, '000040cd864bb440', '000000000050b4c0', 'c39561aa438ad717'),
    ('MountainCar', 'TDActorCritic'): (5200, 650, 650, 4550, '0000002b663ab440', '000000000050b4c0', '4350036e370ab643'),
    ('MountainCar', 'REINFORCE'): (5200, 650, 650, 4550, '000080422d4dd340', '000000000050b4c0', 'b5b3647f69063833'),
    ('MountainCar', 'BaselineREINFORCE'): (5200, 650, 650, 4550, '000080422d4dd340', '000000000050b4c0', 'b5b3647f69063833'),
    ('CartPole', 'TD'): (5200, 658, 642, 4578, '00000012899c3240', '00000000000030c0', '4aea066381928836'),
    ('CartPole', 'TDLambda'): (5200, 658, 642, 4578, '000000742a756c40', '00000000000030c0', '4aea066381928836'),
    ('CartPole', 'GreedyGQ'): (5200, 659, 641, 4585, '000000526be83240', '00000000000032c0', '254edf7c4bdd7271'),
    ('CartPole', 'SARSALambda'): (5200, 659, 641, 4585, '0000e0e8772ed140', '00000000000032c0', 'fd7d29e1317a3294'),
    ('CartPole', 'QLambda'): (5200, 659, 641, 4585, '00007063cd51a040', '00000000000032c0', '4fa60d3f1bce8f9d'),
    ('CartPole', 'QSigma'): (5200, 659, 641, 4585, '0000008e94503240', '00000000000032c0', '05956142ed3dc82c'),
    ('CartPole', 'ActorCritic'): (5200, 659, 641, 4585, '000000944a4c3840', '00000000000032c0', '76cf95f81310a2db'),
    ('CartPole', 'QActorCritic'): (5200, 659, 641, 4585, '000000944a4c3840', '00000000000032c0', '76cf95f81310a2db'),
    ('CartPole', 'TDActorCritic'): (5200, 659, 641, 4585, '000000f0a3003540', '00000000000032c0', '76cf95f81310a2db'),
    ('CartPole', 'REINFORCE'): (5200, 659, 641, 4585, '0000000000003240', '00000000000032c0', '76cf95f81310a2db'),
    ('CartPole', 'BaselineREINFORCE'): (5200, 659, 641, 4585, '0000000000003240', '00000000000032c0', '76cf95f81310a2db'),
}


def run(domain, agent, cuts):
    """-> (the statistics of every train() call, (states, actions, episode_steps) at the end)"""
    with ra.Context(domain=DOMAINS[domain], order=1, n_envs=N, seed=SEED, max_episode_steps=CAP, lr=0.01, gamma=0.99, **AGENTS[agent]) as c:
        c.reset()
        if domain == "CartPole":
            s = np.zeros((c.D, N), dtype=np.float32)
            s[2] = np.linspace(-0.2, 0.2, N, dtype=np.float32)
            c.states = s
        stats = [c.train(n) for n in cuts]
        return stats, (c.states, c.actions, c.episode_steps)


def bits(x):
    return struct.pack("<d", x).hex()


def digest(end):
    h = hashlib.sha256()
    for arr in end:
        h.update(np.ascontiguousarray(arr).tobytes())
    return h.hexdigest()[:16]


def record(domain, agent):
    (st,), end = run(domain, agent, (STEPS,))
    return tuple(st[k] for k in INTS) + (bits(st["sum_abs_td_error"]), bits(st["sum_reward"]), digest(end))


@pytest.mark.parametrize("domain,agent", ROWS, ids=[f"{d}-{a}" for d, a in ROWS])
def test_frame_holds_the_parents_run(domain, agent):
    exp = EXPECTED[(domain, agent)]
    assert exp[2] > 0 and (domain != "CartPole" or exp[1] > exp[2])          # the row exercises what it is there for
    (whole,), end = run(domain, agent, (STEPS,))
    got = tuple(whole[k] for k in INTS) + (bits(whole["sum_abs_td_error"]), bits(whole["sum_reward"]), digest(end))
    print(domain, agent, got)
    assert got == exp
    for cut in CUTS:
        parts, end2 = run(domain, agent, (cut, STEPS - cut))
        for k in INTS:
            assert parts[0][k] + parts[1][k] == whole[k], (cut, k)
        if domain == "CartPole" and cut < CAP:                 # terminal episodes on both sides of the launch boundary
            assert all(p["episodes"] > p["episodes_truncated"] for p in parts), cut
        for x, y in zip(end, end2):
            assert np.array_equal(x, y), cut


if __name__ == "__main__":                               # re-record (against RSRL_HIP_LIB, when set): the rows of EXPECTED
    for row in ROWS:
        print(f"    {row!r}: {record(*row)!r},", flush=True)
