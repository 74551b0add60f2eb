"""What the wave-loop frame (csrc/wave_loop.hpp) owns, for the order-7 wave family's memory-sweep agents (k_wave_lambda, k_wave_aux, k_wave_qsigma): the
learner's state / action / episode-step load and store, the step cap, the five statistics, both episode-end conventions, the column sweep (f32 and
bf16) and Handler::handle's path through the same kernels.

Per row: 7 learners (two 256-thread blocks of four waves, the second holding three), max_episode_steps = 7, a fixed seed, train(40) with statistics;
then the same run in fresh contexts as train(13) + train(27) and as train(3) + train(37); then, in a fresh context, one handle() on 7 crafted
transitions.
  Acrobot    starts from reset(): no episode ends by itself in 7 steps, truncation only (35 of 35 episodes)
  CartPole   from the restart state no pole falls within 7 steps, and poles merely tilted to +-0.2 rad all fall within the first two; the poles
             start spread over (-0.2, 0.2) rad with an outward angular velocity of 1.5 rad/s: 6 terminal episodes (at steps 1, 1, 3, 3, 4, 6) and
             34 truncated ones, 4 + 0 / 2 + 34 across the cut at 3, 6 + 7 / 0 + 27 across the cut at 13 (the f32 oracle's wave-order loop gives
             these counts for all seven agent settings, f32 and bf16)
EXPECTED was recorded from the library as it stood BEFORE the frame existed (the parent commit's build, loaded through RSRL_HIP_LIB), with
`python tests/test_gpu_wave_frame.py`: the integers as they are, the two f32-per-launch sums by their f64 bit pattern, the end state -- states,
actions, episode steps, epsilons, every learner's weights and second matrix -- by a digest, handle()'s TD errors by their bytes and the weights
after it by a digest."""
import hashlib
import struct

import numpy as np
import pytest

import rsrl_amd as ra

pytestmark = pytest.mark.gpu

N, CAP, STEPS, CUTS, SEED = 7, 7, 40, (13, 3), 11
EG = dict(policy=ra.EPSILON_GREEDY, epsilon=0.1)
AGENTS = {
    "TD": dict(algo=ra.TD, policy=ra.RANDOM, lr=0.001),
    "TDLambda": dict(algo=ra.TD_LAMBDA, policy=ra.RANDOM, lam=0.5, lr=0.001),
    "GreedyGQ": dict(algo=ra.GREEDY_GQ, lr=0.0002, lr_td=0.001, **EG),
    "SARSALambda": dict(algo=ra.SARSA_LAMBDA, lam=0.5, alpha=0.0005, **EG),
    "SARSALambda-schedule": dict(algo=ra.SARSA_LAMBDA, lam=0.5, alpha=0.0005, epsilon_decay=0.9, epsilon_min=0.01, **EG),
    "QLambda": dict(algo=ra.Q_LAMBDA, lam=0.5, alpha=0.0005, **EG),
    "QSigma": dict(algo=ra.Q_SIGMA, sigma=0.5, n_steps=2, lr=0.0002, **EG),
}
SECOND = {"TDLambda": "get_traces", "SARSALambda": "get_traces", "SARSALambda-schedule": "get_traces", "QLambda": "get_traces", "GreedyGQ": "get_td_weights"}
DOMAINS = {"CartPole": ra.CART_POLE, "Acrobot": ra.ACROBOT}
DTYPES = {"f32": ra.W_F32, "bf16": ra.W_BF16}
ROWS = [(d, w, a) for d in DOMAINS for w in DTYPES for a in AGENTS]
INTS = ("env_steps", "episodes", "episodes_truncated", "sum_episode_steps")

# (domain, dtype, agent): (env_steps, episodes, episodes_truncated, sum_episode_steps, sum_abs_td_error bits, sum_reward bits, end-state digest,
#                          handle()'s TD errors, digest of the weights after handle())
EXPECTED = {
    ('CartPole', 'f32', 'TD'): (280, 40, 34, 256, '000000c47b5f2940', '00000000000018c0', '05d8c162b051d8f1', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '0298f201c15b68af'),
    ('CartPole', 'f32', 'TDLambda'): (280, 40, 34, 256, '000000000000f87f', '00000000000018c0', 'feda739664b8b76a', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '806216236585d8df'),
    ('CartPole', 'f32', 'GreedyGQ'): (280, 40, 34, 256, '00000018de361d40', '00000000000018c0', '3791a36f447246fd', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '01d2fc688d726ba4'),
    ('CartPole', 'f32', 'SARSALambda'): (280, 40, 34, 256, '0000006c5ed12340', '00000000000018c0', '951821c2f496c0f4', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '22c42633a46e94ac'),
    ('CartPole', 'f32', 'SARSALambda-schedule'): (280, 40, 34, 256, '000000f884a12340', '00000000000018c0', 'bb63d05abb8821cd', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '22c42633a46e94ac'),
    ('CartPole', 'f32', 'QLambda'): (280, 40, 34, 256, '0000004804b51c40', '00000000000018c0', '1d29950f09626a1a', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '22c42633a46e94ac'),
    ('CartPole', 'f32', 'QSigma'): (280, 40, 34, 256, '00000088b50a1940', '00000000000018c0', 'fcf7a6ff4f24ad22', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', 'd2a23a7de3af6bf7'),
    ('CartPole', 'bf16', 'TD'): (280, 40, 34, 256, '00000034675c2940', '00000000000018c0', 'fea036d7ba224c42', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '6334975f830aa1b2'),
    ('CartPole', 'bf16', 'TDLambda'): (280, 40, 34, 256, '000000000000f87f', '00000000000018c0', 'feda739664b8b76a', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '3a9381c8887a1863'),
    ('CartPole', 'bf16', 'GreedyGQ'): (280, 40, 34, 256, '000000d830a81c40', '00000000000018c0', '068ecadc6e589742', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '60769ab2c3a73e62'),
    ('CartPole', 'bf16', 'SARSALambda'): (280, 40, 34, 256, '00000080e8332340', '00000000000018c0', '01e89c7486039e31', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', 'c0baa829958a3490'),
    ('CartPole', 'bf16', 'SARSALambda-schedule'): (280, 40, 34, 256, '00000030ee242340', '00000000000018c0', 'ec80f2089dcff1fa', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', 'c0baa829958a3490'),
    ('CartPole', 'bf16', 'QLambda'): (280, 40, 34, 256, '000000b84aa81c40', '00000000000018c0', '03aa9e0d5cf7b974', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', 'c0baa829958a3490'),
    ('CartPole', 'bf16', 'QSigma'): (280, 40, 34, 256, '000000d01b4f1940', '00000000000018c0', 'fbe5c1cf21b370b7', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', 'd2a23a7de3af6bf7'),
    ('Acrobot', 'f32', 'TD'): (280, 35, 35, 245, '000000b4010d7340', '00000000008071c0', '49ec20c37beea1b7', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '1e96620fb29fa546'),
    ('Acrobot', 'f32', 'TDLambda'): (280, 35, 35, 245, '000000000000f87f', '00000000008071c0', 'cb6f520aa506085c', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', 'ecec6f7abffa0fcf'),
    ('Acrobot', 'f32', 'GreedyGQ'): (280, 35, 35, 245, '0000003c6a3c7140', '00000000008071c0', '7d1cd408feb23efc', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '7d87d1ab27790b80'),
    ('Acrobot', 'f32', 'SARSALambda'): (280, 35, 35, 245, '00000084e4496d40', '00000000008071c0', 'f805094f90801dc0', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', 'efd1255a20fdb4ae'),
    ('Acrobot', 'f32', 'SARSALambda-schedule'): (280, 35, 35, 245, '0000006051bf6d40', '00000000008071c0', '7da2ce8d3de3113f', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', 'efd1255a20fdb4ae'),
    ('Acrobot', 'f32', 'QLambda'): (280, 35, 35, 245, '0000008869026f40', '00000000008071c0', 'ddad1aded47a6c70', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', 'efd1255a20fdb4ae'),
    ('Acrobot', 'f32', 'QSigma'): (280, 35, 35, 245, '0000001013906a40', '00000000008071c0', 'ea11863cfbd0eda2', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '0cc5f11e4d6807ac'),
    ('Acrobot', 'bf16', 'TD'): (280, 35, 35, 245, '000000547e0c7340', '00000000008071c0', '1e3ac26ddc7caed0', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '1bf04f9addab1f81'),
    ('Acrobot', 'bf16', 'TDLambda'): (280, 35, 35, 245, '000000000000f87f', '00000000008071c0', 'cb6f520aa506085c', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '49b855c0c4e19059'),
    ('Acrobot', 'bf16', 'GreedyGQ'): (280, 35, 35, 245, '0000008428487140', '00000000008071c0', 'af7b389c81e982a9', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', 'de2ac9a33beda672'),
    ('Acrobot', 'bf16', 'SARSALambda'): (280, 35, 35, 245, '000000e4e8616d40', '00000000008071c0', 'cb72cdad1fb76096', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '03ec29da6dd85602'),
    ('Acrobot', 'bf16', 'SARSALambda-schedule'): (280, 35, 35, 245, '000000a0d4bf6d40', '00000000008071c0', 'cdf34e5dbc99d630', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '03ec29da6dd85602'),
    ('Acrobot', 'bf16', 'QLambda'): (280, 35, 35, 245, '000000b4be026f40', '00000000008071c0', 'a2f72abf68061cae', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '03ec29da6dd85602'),
    ('Acrobot', 'bf16', 'QSigma'): (280, 35, 35, 245, '000000cc85b96a40', '00000000008071c0', '3c74b705eee53887', '000080bfabaa2abfabaaaabe00000000abaaaa3eabaa2a3f0000803f', '0cc5f11e4d6807ac'),
}


def context(domain, dtype, agent):
    return ra.Context(domain=DOMAINS[domain], order=7, n_envs=N, seed=SEED, max_episode_steps=CAP, gamma=0.99, weight_dtype=DTYPES[dtype], **AGENTS[agent])


def start(c, domain):
    """reset(), and CartPole's own start -> the start states"""
    c.reset()
    if domain == "CartPole":
        s = c.states.copy()
        s[2] = np.linspace(-0.2, 0.2, N, dtype=np.float32)
        s[3] = 1.5 * np.sign(s[2])
        c.states = s
    return c.states.copy()


def matrices(c, agent):
    out = [c.get_weights(i) for i in range(N)]
    if agent in SECOND:
        out += [getattr(c, SECOND[agent])(i) for i in range(N)]
    return out


def run(domain, dtype, agent, cuts):
    """-> (the statistics of every train() call, the end state: states, actions, episode steps, epsilons, weights, second matrix)"""
    with context(domain, dtype, agent) as c:
        start(c, domain)
        stats = [c.train(n) for n in cuts]
        return stats, [c.states, c.actions, c.episode_steps, c.epsilons] + matrices(c, agent)


def handle_leg(domain, dtype, agent):
    """one Handler::handle on 7 crafted transitions -> (the TD errors' bytes, the digest of the matrices afterwards)"""
    with context(domain, dtype, agent) as c:
        frm = start(c, domain)
        to = np.ascontiguousarray(frm[:, ::-1])
        td = c.handle(frm, np.arange(N, dtype=np.int32) % c.A, np.linspace(-1, 1, N, dtype=np.float32), to,
                      np.array([1, 0, 0, 1, 0, 0, 0], dtype=np.uint8))
        return td.astype("<f4").tobytes().hex(), digest(matrices(c, agent))


def same_bits(x, y):
    """np.array_equal, held to the bytes: TDLambda's update has no learning rate (td_lambda.rs: w += td_error * z) and at these settings its weights
    overflow to NaN within the 40 steps, which array_equal calls unequal to itself"""
    return x.shape == y.shape and x.dtype == y.dtype and np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()


def bits(x):
    return struct.pack("<d", x).hex()


def digest(arrays):
    h = hashlib.sha256()
    for arr in arrays:
        h.update(np.ascontiguousarray(arr).tobytes())
    return h.hexdigest()[:16]


def row_of(whole, end, domain, dtype, agent):
    return tuple(whole[k] for k in INTS) + (bits(whole["sum_abs_td_error"]), bits(whole["sum_reward"]), digest(end)) + handle_leg(domain, dtype, agent)


def record(domain, dtype, agent):
    (st,), end = run(domain, dtype, agent, (STEPS,))
    return row_of(st, end, domain, dtype, agent)


@pytest.mark.parametrize("domain,dtype,agent", ROWS, ids=["-".join(r) for r in ROWS])
def test_frame_holds_the_parents_run(domain, dtype, agent):
    exp = EXPECTED[(domain, dtype, agent)]
    assert exp[2] > 0 and (domain != "CartPole" or exp[1] > exp[2])          # the row exercises what it is there for
    (whole,), end = run(domain, dtype, agent, (STEPS,))
    got = row_of(whole, end, domain, dtype, agent)
    print(domain, dtype, agent, got)
    assert got == exp
    for cut in CUTS:
        parts, end2 = run(domain, dtype, agent, (cut, STEPS - cut))
        for k in INTS:
            assert parts[0][k] + parts[1][k] == whole[k], (cut, k)
        if domain == "CartPole" and cut < CAP:                 # terminal episodes on both sides of the launch boundary
            assert all(p["episodes"] > p["episodes_truncated"] for p in parts), cut
        assert len(end) == len(end2)
        for x, y in zip(end, end2):
            assert same_bits(x, y), cut


if __name__ == "__main__":                               # re-record (against RSRL_HIP_LIB, when set): the rows of EXPECTED
    for row in ROWS:
        print(f"    {row!r}: {record(*row)!r},", flush=True)
