"""What the least-squares kernels' lane-group layout does around the agents' rules, held to the library as it stood before their shared pieces
(kernels_lstd.hpp: GroupId / GroupGiven, the Handler::handle prologue of k_handle_lstd, k_handle_tdac_lstd, k_handle_tdac_beta; tdcritic_target, the
actor-critics' TDCritic block) were taken out -- and what any later frame for k_train_lstd, k_train_tdac_lstd, k_train_tdac_beta, k_train_lstd_batch
would have to keep: the group index and the idle lanes r >= F, the step cap, the five statistics with their f64 sums counted once per group, both
episode-end conventions and the caller-supplied transition.  (That lane 0 ALONE stores the learner is not observable: every lane holds the same bits.)

Per row: 67 learners (at G = 4 two 256-thread blocks, the second with 3 learners in a partial wave; at G = 16 / 32 / 64 a ragged last block),
max_episode_steps = 7, a fixed seed, train(40) with statistics; then the same run in fresh contexts as train(13) + train(27) and as
train(3) + train(37); then, in a fresh context after train(7) (theta is no longer zero), one handle() (handle_transitions() for LSTD /
LSTDLambda, two rows, lengths 0 / 1 / 2) on crafted transitions.  Orders 1, 2, 4, 5 of MountainCar give F = 4 = G, 9 < 16, 25 < 32, 36 < 64.
From the restart state a cap of 7 gives truncation only on every domain here, so the starts are this module's own (start_states):
  MountainCar, ContinuousMountainCar   every eighth learner stands at x = 0.56, v = 0.06: its first step reaches the goal whatever the action
  CartPole   the poles spread over (-0.2, 0.2) rad with an outward 1.5 rad/s (tests/test_gpu_wave_frame.py's recipe): the outer ones fall in the
             first steps, later ones after the cut at 3; the poles within 0.03 rad of upright start with episode_steps = 5, so that the cap
             cuts them at their second step -- a terminal and a truncated episode on both sides of the cut at 3
  Acrobot    every eighth learner starts with both links swung up (theta1 = 2.6 rad at 2 rad/s); every eighth other one with episode_steps = 4
A preset episode_steps of LSTD / LSTDLambda comes with a record for the steps it claims (the start state, reward 0).
LSTD / LSTDLambda: A starts at 1e-6 I, so a 7-row episode that cannot fill A (F = 25 and 36) still meets no exactly zero pivot: every solve
commits at every order (the recorded sum of singular_solves is 0 in every row; it is part of the row that is compared).
The episode counts were checked on the CPU before recording: `python scripts/group_frame_counts.py` steps the f32 oracle's domains from
start_states with the driver loop's Random draws and prints terminal / truncated episodes for the whole run and on both sides of each cut.
That covers the Random-policy rows and, by the starts' construction, the actor-critics on MountainCar / Acrobot (their first steps end whatever
the action).  The CartPole iLSTD-AC row was NOT pre-computed -- the project's numpy restatements hold single transitions, no driver loop with the
Gibbs actor's samples: its counts (389 episodes, 334 truncated) are the parent's recorded ones, and the cut assertions below check them at run time.
EXPECTED was recorded from the library as it stood BEFORE the frame existed (the parent commit's build, loaded through RSRL_HIP_LIB), with
`python tests/test_gpu_group_frame.py`: the integers as they are, the two f64 sums by their bit pattern, the end state -- states, actions,
episode steps, get_weights, every learner's f64 least-squares state with singular_solves, the policy weights, the episode record -- by a
digest, handle()'s TD errors by a digest of their bytes and the state after it by a digest."""
import hashlib
import struct

import numpy as np
import pytest

import rsrl_amd as ra

pytestmark = pytest.mark.gpu

N, CAP, STEPS, CUTS, SEED = 67, 7, 40, (13, 3), 11
AGENTS = {
    "RecursiveLSTD": dict(algo=ra.RECURSIVE_LSTD, policy=ra.RANDOM, alpha=0.05),
    "iLSTD": dict(algo=ra.ILSTD, policy=ra.RANDOM, alpha=0.05, n_steps=2),
    "iLSTD-AC": dict(algo=ra.ILSTD_ACTOR_CRITIC, policy=ra.SOFTMAX, lr=0.05, alpha=0.3, tau=1.0, n_steps=2),
    "LSTD": dict(algo=ra.LSTD, policy=ra.RANDOM),
    "LSTDLambda": dict(algo=ra.LSTD_LAMBDA, policy=ra.RANDOM, lam=0.8),
    "Beta-AC": dict(algo=ra.ILSTD_ACTOR_CRITIC, policy=ra.BETA, lr=0.05, alpha=0.3, n_steps=2),
}
BATCH, ACTOR = ("LSTD", "LSTDLambda"), ("iLSTD-AC", "Beta-AC")
DOMAINS = {"MountainCar": ra.MOUNTAIN_CAR, "CartPole": ra.CART_POLE, "Acrobot": ra.ACROBOT, "ContinuousMountainCar": ra.CONTINUOUS_MOUNTAIN_CAR}
DISCRETE = [("MountainCar", o) for o in (1, 2, 4, 5)] + [("CartPole", 1), ("Acrobot", 1)]
ROWS = [(d, o, a) for a in AGENTS if a != "Beta-AC" for d, o in DISCRETE] + [("ContinuousMountainCar", o, "Beta-AC") for o in (1, 2, 4, 5)]
INTS = ("env_steps", "episodes", "episodes_truncated", "sum_episode_steps")

# (domain, order, agent): (env_steps, episodes, episodes_truncated, sum_episode_steps, sum_abs_td_error bits, sum_reward bits, end-state digest,
#                          the sum of singular_solves (LSTD / LSTDLambda, else 0), digest of handle()'s TD errors, digest of the state after handle())
EXPECTED = {
    ('MountainCar', 1, 'RecursiveLSTD'): (2680, 344, 335, 2354, 'f903bda2e8dda440', '0000000000dea4c0', '3b9a25b1cc3f07ed', 0, '38c434bd0e3209d8', 'b958ac9380710775'),
    ('MountainCar', 2, 'RecursiveLSTD'): (2680, 344, 335, 2354, 'e0471905c9dda440', '0000000000dea4c0', '4b21e0a091fd80ce', 0, '578164c12e9ac638', 'b073fc8986dffbf2'),
    ('MountainCar', 4, 'RecursiveLSTD'): (2680, 344, 335, 2354, '1212feb86cdda440', '0000000000dea4c0', 'a66865cd4ebe058d', 0, 'bfb3360b7a3d3518', 'cb3ec0fc62d08b60'),
    ('MountainCar', 5, 'RecursiveLSTD'): (2680, 344, 335, 2354, '1fca2e9d29dda440', '0000000000dea4c0', '6d524c5def775ee5', 0, '80a5a0cb63f51494', '9a1428dca4ba9a7a'),
    ('CartPole', 1, 'RecursiveLSTD'): (2680, 390, 334, 2537, '336862ab0e014c40', '0000000000004cc0', '890a6ccea640d79b', 0, 'c52eb083d137fbe7', 'ef0db4d1471bea7b'),
    ('Acrobot', 1, 'RecursiveLSTD'): (2680, 352, 343, 2410, '659dfd5963dda440', '0000000000dea4c0', '230d043498b4a027', 0, 'aead83200c96a440', '46ef8fe404482dc1'),
    ('MountainCar', 1, 'iLSTD'): (2680, 344, 335, 2354, '2367b98782d79740', '0000000000dea4c0', 'cf639579c75a93f2', 0, '8671a419711a3db8', '8ac5f75ab12bf6b6'),
    ('MountainCar', 2, 'iLSTD'): (2680, 344, 335, 2354, '30bf38e6f1e29540', '0000000000dea4c0', '9d8c9e5e454fe0fd', 0, '62dbcff4855d8cd1', '5a1cfee6f433df0c'),
    ('MountainCar', 4, 'iLSTD'): (2680, 344, 335, 2354, '0d3f2f6484089440', '0000000000dea4c0', '00ffebfaf3146f94', 0, '848c7a1c9baa7ca3', '797677df1c9d882b'),
    ('MountainCar', 5, 'iLSTD'): (2680, 344, 335, 2354, '24a0d75ab7689340', '0000000000dea4c0', '0c7e5892aef74be3', 0, '63a8cde8aeb50f31', '0ca78324dd2558ef'),
    ('CartPole', 1, 'iLSTD'): (2680, 390, 334, 2537, '1444c24f627f5d40', '0000000000004cc0', 'c18c02c6a14055de', 0, 'f898e76460b72301', '4b8119a29ae8f469'),
    ('Acrobot', 1, 'iLSTD'): (2680, 352, 343, 2410, 'f4b8bc43cf1e9e40', '0000000000dea4c0', 'c8b4496e8e719e3a', 0, '8d4006f10b5033df', 'e4759f589e861a2d'),
    ('MountainCar', 1, 'iLSTD-AC'): (2680, 344, 335, 2354, 'd4a0f8ec1ace9740', '0000000000dea4c0', 'e92f879ba271024e', 0, '32cb383a09ea30bb', '7c9fbacc11ff3cef'),
    ('MountainCar', 2, 'iLSTD-AC'): (2680, 344, 335, 2354, '7096222e08ac9540', '0000000000dea4c0', 'a407d93d22746672', 0, '46d0ca936f9461cc', 'f27d751acf5f8a60'),
    ('MountainCar', 4, 'iLSTD-AC'): (2680, 344, 335, 2354, '68551ba412499340', '0000000000dea4c0', '04e1104971f5e316', 0, '3803aa62278aa8b1', 'd3e1ba91eb5104a6'),
    ('MountainCar', 5, 'iLSTD-AC'): (2680, 344, 335, 2354, '96cff5573d599240', '0000000000dea4c0', '70735bd262a96490', 0, 'a456b373c78c578d', 'c1c7b2228ff24e9e'),
    ('CartPole', 1, 'iLSTD-AC'): (2680, 389, 334, 2530, '3584d11664e85940', '0000000000804bc0', 'de869f13992a48be', 0, '9407466d16bbf5e4', '3c850d9d4ca798fe'),
    ('Acrobot', 1, 'iLSTD-AC'): (2680, 352, 343, 2410, '48dcf7b8f1249e40', '0000000000dea4c0', 'a78fa85d308f0464', 0, '47da66c29c7707f0', '2047e929434beec2'),
    ('MountainCar', 1, 'LSTD'): (2680, 344, 335, 2354, '4a11737b256e8240', '0000000000dea4c0', 'aac493acf30c7fcc', 0, '17dff860a7adb48c', '0b557c40636b2d00'),
    ('MountainCar', 2, 'LSTD'): (2680, 344, 335, 2354, '19570535f55f8040', '0000000000dea4c0', '5ac72a01988e30b2', 0, '90bdf5501fb27e86', '2bedd877a8d838aa'),
    ('MountainCar', 4, 'LSTD'): (2680, 344, 335, 2354, '98a3bace40c37f40', '0000000000dea4c0', 'ccd49a9ed87f047b', 0, '36e451f632b4922b', 'd46822e94ffa3671'),
    ('MountainCar', 5, 'LSTD'): (2680, 344, 335, 2354, '67bb90f3036d7f40', '0000000000dea4c0', '80dc336553a17523', 0, 'ba7a86ebdf41ffd6', 'a4adc04a3888342d'),
    ('CartPole', 1, 'LSTD'): (2680, 390, 334, 2537, '98386ca053605e40', '0000000000004cc0', '9ad32e2c5605a5c3', 0, '6066a1b3d39fba0f', '4c260938eb1918a1'),
    ('Acrobot', 1, 'LSTD'): (2680, 352, 343, 2410, 'ca70ed108f74bb40', '0000000000dea4c0', '780247b3c2562c82', 0, '46673bc80af5c751', '264029915dc3d80b'),
    ('MountainCar', 1, 'LSTDLambda'): (2680, 344, 335, 2354, '095b09e28b8c7e40', '0000000000dea4c0', '447d44f1da078e55', 0, '4b0d459e43ee0815', '80dcd3b21b287454'),
    ('MountainCar', 2, 'LSTDLambda'): (2680, 344, 335, 2354, 'f0f1e502fac37e40', '0000000000dea4c0', '6d7061aa3b9cb74f', 0, '5beb03c547aee879', '2b9611e976b9338d'),
    ('MountainCar', 4, 'LSTDLambda'): (2680, 344, 335, 2354, 'c4abf08a7f1f7f40', '0000000000dea4c0', '9323785a1e6be2d6', 0, '44ee93dbd286c687', 'b63aa55a58e21f45'),
    ('MountainCar', 5, 'LSTDLambda'): (2680, 344, 335, 2354, 'c1b4e94209c77f40', '0000000000dea4c0', '19ad9f98578ed892', 0, '68d75a6733b8105a', '3ef8cefe0fff4ef7'),
    ('CartPole', 1, 'LSTDLambda'): (2680, 390, 334, 2537, '8b5745f057056040', '0000000000004cc0', 'e9865d273d05cdfb', 0, 'fa443a7081f1efa3', 'fa508b0a3f7e163c'),
    ('Acrobot', 1, 'LSTDLambda'): (2680, 352, 343, 2410, 'b42bd2b4aabfd040', '0000000000dea4c0', '73fb103a0d7c5515', 0, 'fe21a6f99865399f', '97480f1f2e226409'),
    ('ContinuousMountainCar', 1, 'Beta-AC'): (2680, 344, 335, 2354, '2c53bbc735309840', '0000000000dea4c0', '09ad3daea3124752', 0, 'dd62d45ef722b056', '1f2576d2b3674bc0'),
    ('ContinuousMountainCar', 2, 'Beta-AC'): (2680, 344, 335, 2354, '2eb3f257e35b9640', '0000000000dea4c0', 'c5e730193d3eb4a0', 0, '71372412884722e1', 'f5f7e174a32b2e78'),
    ('ContinuousMountainCar', 4, 'Beta-AC'): (2680, 344, 335, 2354, 'c0c9e33d91859340', '0000000000dea4c0', '607a10c5e1910e8d', 0, 'bbf7ad2295260091', '647bb3b2ce693e73'),
    ('ContinuousMountainCar', 5, 'Beta-AC'): (2680, 344, 335, 2354, 'c4ccb8f84fee9240', '0000000000dea4c0', '68d72400d6d608c0', 0, '429638c416b52e8d', '14673a21237b1a06'),
}


def context(domain, order, agent):
    return ra.Context(domain=DOMAINS[domain], order=order, n_envs=N, seed=SEED, max_episode_steps=CAP, gamma=0.95, **AGENTS[agent])


def start_states(domain, s):
    """the restart states s (D, N) -> (this module's start states, the episode steps they start with)"""
    s, ep = np.array(s, dtype=np.float32), np.zeros(N, dtype=np.uint32)
    k = np.arange(N)
    if domain in ("MountainCar", "ContinuousMountainCar"):
        s[0, k % 8 == 0], s[1, k % 8 == 0] = 0.56, 0.06
    elif domain == "CartPole":
        s[2] = np.linspace(-0.2, 0.2, N, dtype=np.float32)
        s[3] = 1.5 * np.sign(s[2])
        ep[np.abs(s[2]) < 0.03] = 5
    else:
        s[0, k % 8 == 0], s[2, k % 8 == 0] = 2.6, 2.0
        ep[k % 8 == 4] = 4
    return s, ep


def start(c, domain, agent):
    c.reset()
    s, ep = start_states(domain, c.states)
    c.states = s
    if ep.any():
        if agent in BATCH:
            c.episode_record = (np.broadcast_to(s, (CAP,) + s.shape).copy(), np.zeros((CAP, N), dtype=np.float32))
        c.episode_steps = ep
    return s


def learned(c, agent):
    """-> (everything the learners hold, the sum of singular_solves)"""
    out, sing = [], 0
    for i in range(N):
        out.append(c.get_weights(i))
        if agent in BATCH:
            theta, A, b, z, n = c.get_lstd_batch_state(i)
            out += [theta, A, b, np.uint32(n)] + ([] if z is None else [z])
            sing += n
        else:
            out += [x for x in c.get_lstd_state(i) if x is not None]
        if agent in ACTOR:
            out.append(c.get_policy_weights(i))
    if agent in BATCH:
        out += list(c.episode_record)
    return out, sing


def run(domain, order, agent, cuts):
    """-> (the statistics of every train() call, the end state, the sum of singular_solves)"""
    with context(domain, order, agent) as c:
        start(c, domain, agent)
        stats = [c.train(n) for n in cuts]
        end, sing = learned(c, agent)
        return stats, [c.states, c.actions, c.episode_steps] + end, sing


def handle_leg(domain, order, agent):
    """one Handler::handle on crafted transitions, some terminal, after train(7) -- every learner has ended an episode by then (LSTD / LSTDLambda have
    solved), so theta is not zero and the TD errors are each agent's own -> (digest of the TD errors' bytes, digest of what the learners hold afterwards)"""
    with context(domain, order, agent) as c:
        frm = start(c, domain, agent)
        c.train(CAP, want_stats=False)
        to = np.ascontiguousarray(frm[:, ::-1])
        rew = np.linspace(-1, 1, N, dtype=np.float32)
        term = (np.arange(N) % 3 == 0).astype(np.uint8)
        if agent in BATCH:
            td = c.handle_transitions(np.stack([frm, to]), np.stack([rew, -rew]), np.stack([to, frm]), np.stack([term, 1 - term]),
                                      (np.arange(N) % 3).astype(np.uint32), td=True)
        elif c.continuous:
            td = c.handle(frm, np.linspace(-1.5, 1.5, N, dtype=np.float32), rew, to, term)
        else:
            td = c.handle(frm, np.arange(N, dtype=np.int32) % c.A, rew, to, term)
        return digest([td.astype("<f4")]), digest(learned(c, agent)[0])


def same_bits(x, y):
    """np.array_equal, held to the bytes: a least-squares state can hold NaN, and the episode record shows NaN past each learner's rows"""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def bits(x):
    return struct.pack("<d", x).hex()


def digest(arrays):
    h = hashlib.sha256()
    for arr in arrays:
        h.update(np.ascontiguousarray(arr).tobytes())
    return h.hexdigest()[:16]


def row_of(whole, end, sing, domain, order, agent):
    return tuple(whole[k] for k in INTS) + (bits(whole["sum_abs_td_error"]), bits(whole["sum_reward"]), digest(end), sing) + handle_leg(domain, order, agent)


def record(domain, order, agent):
    (st,), end, sing = run(domain, order, agent, (STEPS,))
    return row_of(st, end, sing, domain, order, agent)


@pytest.mark.parametrize("domain,order,agent", ROWS, ids=["-".join(map(str, r)) for r in ROWS])
def test_frame_holds_the_parents_run(domain, order, agent):
    exp = EXPECTED[(domain, order, agent)]
    assert exp[1] > exp[2] > 0                                 # the row exercises what it is there for: both episode ends
    (whole,), end, sing = run(domain, order, agent, (STEPS,))
    got = row_of(whole, end, sing, domain, order, agent)
    print(domain, order, agent, got)
    assert got == exp
    for cut in CUTS:
        parts, end2, _ = run(domain, order, agent, (cut, STEPS - cut))
        for k in INTS:
            assert parts[0][k] + parts[1][k] == whole[k], (cut, k)
        if domain == "CartPole" and cut < CAP:                 # a terminal and a truncated episode on both sides of the launch boundary
            assert all(p["episodes"] > p["episodes_truncated"] > 0 for p in parts), (cut, parts)
        assert len(end) == len(end2)
        for x, y in zip(end, end2):
            assert same_bits(x, y), cut


if __name__ == "__main__":                               # re-record (against RSRL_HIP_LIB, when set): the rows of EXPECTED
    for row in ROWS:
        print(f"    {row!r}: {record(*row)!r},", flush=True)
