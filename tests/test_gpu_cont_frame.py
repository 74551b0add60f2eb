"""What the continuous-action kernels do around the agents' rules and the two policies, held to the library as it stood before they shared one
policy trait (cont_policy.hpp) and one loop per agent pair (kernels_cont.hpp): CACLA, the TD(0)-critic ActorCritic under Gaussian and under Beta, NAC under
Gaussian and under Beta (the actor's period n_steps = 3), and -- for its policy side and domain step only, its loop is in
tests/test_gpu_group_frame.py -- the iLSTD Beta ActorCritic.  Fourier orders 1, 2, 5: the packed F = 4, the unpacked F = 9, the largest F = 36.

Per row: 259 learners (one full 256-thread block, then three learners in a partial wave), max_episode_steps = 7, a fixed seed, crafted weights
(every learner its own columns and critic), train(40) with statistics; then the same run in fresh contexts as train(13) + train(27) and as
train(3) + train(37); then, in a fresh context after train(7), one f32 handle() on 131 crafted transitions (a partial batch, every third terminal;
the learners past 131 are in the digest of the state afterwards and are compared to their bytes before the call); NAC: nac_update under a mask
and q_evaluate_f32; every row: the policy side (sample on the ctx's own states and on explicit ones, mode, params, pdf), the domain step with
explicit and with the pending actions (NAC and the TD ActorCritic under Beta: the 2a - 1 rows) and the mode rollout at a step limit of 50.

The starts are tests/test_gpu_group_frame.py's ContinuousMountainCar starts -- every eighth learner (k % 8 == 0) stands at x = 0.56, v = 0.06: its
first step reaches the goal whatever the action (v >= 0.06 - 0.0015 - 0.0025) -- and two more groups, because those starts alone give no terminal
episode after step 1 and no truncated one before step 7:
  k % 8 == 4   x = 0.3, v = 0.065: the goal at step 5 or 6 whatever the action (|dv| <= 0.0015 + 0.0025 per step) -- a terminal episode AFTER the cut at 3
  k % 8 == 2   episode_steps = 5: the cap cuts the episode at its second step -- a truncated episode BEFORE the cut at 3
So the whole run and both sides of train(3) + train(37) see episodes > episodes_truncated > 0, and so does train(13).  train(27) after it CANNOT:
every episode open after step 7 began at the restart state (x = -0.5 at rest), from where 7 steps at |v| <= 0.07 end 0.6 short of the goal.  There
the assertion is episodes == episodes_truncated > 0.

EXPECTED was recorded from the library as it stood BEFORE the trait and the shared loops existed (the parent commit's build, loaded through RSRL_HIP_LIB),
with `python tests/test_gpu_cont_frame.py`: the integers as they are, the two f64 sums by their bit pattern, everything else by a digest of its
bytes.  No tolerance appears in this file: every comparison is equality."""
import hashlib
import struct

import numpy as np
import pytest

import rsrl_amd as ra

pytestmark = pytest.mark.gpu

N, M, CAP, STEPS, CUTS, SEED, LIMIT = 259, 131, 7, 40, (13, 3), 11, 50
COMMON = dict(domain=ra.CONTINUOUS_MOUNTAIN_CAR, n_envs=N, seed=SEED, max_episode_steps=CAP, gamma=0.95)
AGENTS = {
    "CACLA": dict(algo=ra.CACLA, policy=ra.GAUSSIAN, lr=0.05, alpha=0.02),
    "TDAC-Gaussian": dict(algo=ra.CONTINUOUS_TD_ACTOR_CRITIC, policy=ra.GAUSSIAN, lr=0.05, alpha=0.02),
    "TDAC-Beta": dict(algo=ra.CONTINUOUS_TD_ACTOR_CRITIC, policy=ra.BETA, lr=0.05, alpha=0.02),
    "NAC-Gaussian": dict(algo=ra.NAC, policy=ra.GAUSSIAN, lr=0.005, alpha=0.02, n_steps=3),      # (SCB's features carry the score: a TD rate would diverge)
    "NAC-Beta": dict(algo=ra.NAC, policy=ra.BETA, lr=0.005, alpha=0.02, n_steps=3),
    "Beta-AC": dict(algo=ra.ILSTD_ACTOR_CRITIC, policy=ra.BETA, lr=0.05, alpha=0.3, n_steps=2),
}
POLICY_SIDE_ONLY = ("Beta-AC",)
ROWS = [(a, o) for a in AGENTS for o in (1, 2, 5)]
INTS = ("env_steps", "episodes", "episodes_truncated", "sum_episode_steps")

# (agent, order): (env_steps, episodes, episodes_truncated, sum_episode_steps, sum_abs_td_error bits, sum_reward bits, end-state digest,
#                  digest of handle()'s TD errors, digest of the state after handle(), digest of NAC's legs, digest of the policy side)
# -- None where the row has no such leg (Beta-AC: no loop and no handle here; nac: NAC only)
EXPECTED = {
    ('CACLA', 1): (10360, 1390, 1325, 9471, '00004030e95dc240', '00000000801bc4c0', '77fca90f1a5c0e16', 'f6b8df614a675a5d', '419a810390762dff', None, '72a82eaa020ba5af'),
    ('CACLA', 2): (10360, 1391, 1326, 9477, '000050d21751c040', '00000000801bc4c0', '746518f0769137f7', '42740f6bd3757a81', '03c378864f314951', None, 'b1c8f9449ca2672e'),
    ('CACLA', 5): (10360, 1390, 1325, 9471, '000090073800b340', '00000000801bc4c0', '4c5697a3fe3f75a6', 'dd5b4275bf59fd44', 'bae8842856074c66', None, 'ae38bfb018a51129'),
    ('TDAC-Gaussian', 1): (10360, 1392, 1327, 9483, '000080a7565dc240', '00000000801bc4c0', 'f277cf3f1dc418b6', '98d745d9c46046a1', 'e592c196c878329b', None, 'b5ee7ae18176e274'),
    ('TDAC-Gaussian', 2): (10360, 1393, 1328, 9489, '000040509045c040', '00000000801bc4c0', '7ea80d5adb563385', '69496f3a3c99398c', '669c4cfc92594cf3', None, '45737d51f87bfcc6'),
    ('TDAC-Gaussian', 5): (10360, 1393, 1328, 9489, '0000b002d2b2b140', '00000000801bc4c0', '90ff616c653f7ffe', 'b9dd5a76c118a8c2', 'd5fad9a8a377e0c6', None, 'f628cee23ddd9817'),
    ('TDAC-Beta', 1): (10360, 1391, 1326, 9477, '0000400b275ec240', '00000000801bc4c0', '163262ebec554b1b', '58484da65a89e6e4', 'ae73f457b147ae30', None, '198ca2b0b0f8f1b0'),
    ('TDAC-Beta', 2): (10360, 1391, 1326, 9477, '000060ea7852c040', '00000000801bc4c0', '5e36a07ade5cee8a', '3dc8860f9ba78b56', 'd385c5388a18f81e', None, '84bd422763f2f6fd'),
    ('TDAC-Beta', 5): (10360, 1391, 1326, 9477, '00000074e10ab340', '00000000801bc4c0', '0f30f28580422980', 'aeeb99c95a7381d2', '04e250f38c322cd0', None, '1c4337de571b190e'),
    ('NAC-Gaussian', 1): (10360, 1390, 1325, 9471, '0000c0bc1ffdc340', '00000000801bc4c0', 'a6f5a2c7a95e1037', 'c8b78ea1cf6d2df4', 'e2aaf2c306a4b150', 'a1f9ed80652c1d60', 'd96c66f8ddf19540'),
    ('NAC-Gaussian', 2): (10360, 1391, 1326, 9477, '0000400308ffc340', '00000000801bc4c0', '9eb664f53b325d28', 'f35b3cfb2bf5dd87', 'd7199fd40a37d6b4', 'cfd867712950bb58', '2f304d3efcb2cc92'),
    ('NAC-Gaussian', 5): (10360, 1390, 1325, 9471, '0000a0a50340c540', '00000000801bc4c0', '023d591e4430c223', '04ddc2620af8cb73', '3c90f89915fa70d1', '149e65b13d746e7d', 'e0f7582143c93754'),
    ('NAC-Beta', 1): (10360, 1391, 1326, 9477, '000080645ff3c340', '00000000801bc4c0', '1d226d47f45d48e2', 'c8904f9c4fd12df0', '602ce7f552c26a2e', '1b277ea180d0bcb6', '80749e913d0b31b3'),
    ('NAC-Beta', 2): (10360, 1391, 1326, 9477, '000080161fb5c340', '00000000801bc4c0', 'c7de393a36af6b55', '4e04f3a1c81fda2d', 'dd84d4e5406fe449', '4e56306f13867322', 'b85ee02d150fb9e2'),
    ('NAC-Beta', 5): (10360, 1391, 1326, 9477, '0000b01b3c81c240', '00000000801bc4c0', '08d856b67f741f1e', '1abd7b72a1aab430', '0c1f0f7b02e4ec05', '73bbbf42e4ffad58', '8006d39ed3a1c683'),
    ('Beta-AC', 1): (None, None, None, None, None, None, None, None, None, None, 'aed86631e5edaca1'),
    ('Beta-AC', 2): (None, None, None, None, None, None, None, None, None, None, 'b891b5a093f54675'),
    ('Beta-AC', 5): (None, None, None, None, None, None, None, None, None, None, 'c5c0927ea807bfa0'),
}


def context(agent, order):
    return ra.Context(order=order, **COMMON, **AGENTS[agent])


def start(c, agent):
    """crafted weights, this module's start states and episode steps -> the start states (D, N)"""
    c.reset()
    rng = np.random.default_rng(SEED)
    pol = (rng.normal(size=(N, c.F, 2)) * 0.05).astype(np.float32)      # (small: the Gaussian's stddev stays near softplus(0), its score near 1)
    w = (rng.normal(size=(N, c.n_weight_rows, 1)) * 0.1).astype(np.float32)
    for i in range(N):
        c.set_policy_weights(pol[i], i)
        if agent not in POLICY_SIDE_ONLY:
            c.set_weights(w[i], i)
    s, ep, k = np.array(c.states, dtype=np.float32), np.zeros(N, dtype=np.uint32), np.arange(N)
    s[0, k % 8 == 0], s[1, k % 8 == 0] = 0.56, 0.06
    s[0, k % 8 == 4], s[1, k % 8 == 4] = 0.3, 0.065
    ep[k % 8 == 2] = 5
    c.states, c.episode_steps = s, ep
    return s


def learned(c):
    """-> (every learner's weights (N, rows, 1), every learner's policy columns (N, F, 2))"""
    return np.stack([c.get_weights(i) for i in range(N)]), np.stack([c.get_policy_weights(i) for i in range(N)])


def end_state(c):
    return [c.states, c.actions, c.episode_steps] + list(learned(c))


def run(agent, order, cuts):
    """-> (the statistics of every train() call, the end state)"""
    with context(agent, order) as c:
        start(c, agent)
        stats = [c.train(n) for n in cuts]
        return stats, end_state(c)


def crafted_batch(frm, agent):
    """131 transitions, every third terminal; the actions cross each policy's interval"""
    frm = np.ascontiguousarray(frm[:, :M])
    to = np.ascontiguousarray(frm[:, ::-1])
    rew = np.linspace(-1, 1, M, dtype=np.float32)
    term = (np.arange(M) % 3 == 0).astype(np.uint8)
    lo, hi = (-1.5, 1.5) if "Beta" not in agent else (-0.25, 1.25)
    return frm, np.linspace(lo, hi, M, dtype=np.float32), rew, to, term


def handle_leg(agent, order):
    """-> (digest of the TD errors' bytes, digest of the state afterwards)"""
    with context(agent, order) as c:
        frm = start(c, agent)
        c.train(CAP, want_stats=False)
        w0, pol0 = learned(c)
        td = c.handle(*crafted_batch(frm, agent))
        w1, pol1 = learned(c)
        assert same_bits(w0[M:], w1[M:]) and same_bits(pol0[M:], pol1[M:])         # the learners past the batch keep their bytes
        moved = np.array([pol0[i].tobytes() != pol1[i].tobytes() for i in range(M)])
        if agent == "CACLA":                                                       # some gates open, some stay shut
            assert 0 < moved.sum() < M, moved.sum()
        elif agent.startswith("NAC"):                                              # critic.handle: the columns stay
            assert not moved.any()
        return digest([td.astype("<f4")]), digest(end_state(c))


def nac_leg(agent, order):
    """NAC::handle(()) under a mask with every fifth learner out (norms, columns), then Q on crafted states and actions -> digest"""
    with context(agent, order) as c:
        frm = start(c, agent)
        c.train(CAP, want_stats=False)
        mask = (np.arange(N) % 5 != 0).astype(np.uint8)
        pol0 = learned(c)[1]
        norms = c.nac_update(mask)
        pol1 = learned(c)[1]
        assert same_bits(pol0[mask == 0], pol1[mask == 0]) and not norms[mask == 0].any() and norms[mask == 1].all()
        frm, act, _, to, _ = crafted_batch(frm, agent)
        return digest([norms, pol1, c.q_evaluate_f32(frm, act), c.q_evaluate_f32(to, act[::-1])])


def policy_leg(agent, order):
    """the policy side, the domain step and the mode rollout -> digest"""
    with context(agent, order) as c:
        s = start(c, agent)
        c.train(CAP, want_stats=False)
        here = c.states
        explicit = np.ascontiguousarray(s[:, ::-1][:, :M])
        act = np.linspace(-0.25, 1.25, M, dtype=np.float32)
        out = [c.policy_sample(), c.actions, c.policy_sample(explicit), c.policy_mode(explicit), *c.policy_params(explicit), c.policy_pdf(explicit, act)]
        out += [*c.domain_step(np.linspace(-1.5, 1.5, N, dtype=np.float32)), c.states]
        c.states = here
        pending = c.actions
        out += [*c.domain_step(), c.states]
        assert same_bits(c.actions, pending)
        out += list(c.rollout_greedy(LIMIT))
        return digest(out)


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def bits(x):
    return struct.pack("<d", x).hex()


def digest(arrays):
    h = hashlib.sha256()
    for arr in arrays:
        h.update(np.ascontiguousarray(arr).tobytes())
    return h.hexdigest()[:16]


def both_ends(st):
    return st["episodes"] > st["episodes_truncated"] > 0


def row_of(whole, end, agent, order):
    if agent in POLICY_SIDE_ONLY:
        return (None,) * 10 + (policy_leg(agent, order),)
    return (tuple(whole[k] for k in INTS) + (bits(whole["sum_abs_td_error"]), bits(whole["sum_reward"]), digest(end)) + handle_leg(agent, order)
            + (nac_leg(agent, order) if agent.startswith("NAC") else None, policy_leg(agent, order)))


def record(agent, order):
    if agent in POLICY_SIDE_ONLY:
        return row_of(None, None, agent, order)
    (st,), end = run(agent, order, (STEPS,))
    return row_of(st, end, agent, order)


@pytest.mark.parametrize("agent,order", ROWS, ids=["-".join(map(str, r)) for r in ROWS])
def test_frame_holds_the_parents_run(agent, order):
    exp = EXPECTED[(agent, order)]
    if agent in POLICY_SIDE_ONLY:
        got = row_of(None, None, agent, order)
        print(agent, order, got)
        assert got == exp
        return
    (whole,), end = run(agent, order, (STEPS,))
    assert both_ends(whole), whole                             # the row exercises what it is there for: both episode ends
    assert np.isfinite(whole["sum_abs_td_error"])              # ... on a run that has not diverged
    got = row_of(whole, end, agent, order)
    print(agent, order, got)
    assert got == exp
    for cut in CUTS:
        parts, end2 = run(agent, order, (cut, STEPS - cut))
        for k in INTS:
            assert parts[0][k] + parts[1][k] == whole[k], (cut, k)
        assert both_ends(parts[0]), (cut, parts)
        if cut < CAP:                                          # a terminal and a truncated episode on both sides of the launch boundary
            assert both_ends(parts[1]), (cut, parts)
        else:                                                  # (past step 7 every open episode began at the restart state: the cap cuts them all)
            assert parts[1]["episodes"] == parts[1]["episodes_truncated"] > 0, (cut, parts)
        assert len(end) == len(end2)
        for x, y in zip(end, end2):
            assert same_bits(x, y), cut


if __name__ == "__main__":                               # re-record (against RSRL_HIP_LIB, when set): the rows of EXPECTED
    for row in ROWS:
        print(f"    {row!r}: {record(*row)!r},", flush=True)
