"""Every kernel family's policy / Enumerable code (device_core.hpp find_max .. policy_probs) against the reference's f64 semantics on the crafted
table of tests/policy_edges.py: exact ties, near-tie chains around argmaxima's 1e-7 band in every order, +-FLT_MAX, subnormals, -inf / +inf / NaN in
every position, vectors without any maximum, saturated Softmax -- inputs learned weights never produce.  tests/test_policy_edges_cpu.py shows that on
this table f64 alone decides every discrete output, so the bars are:

  indices (find_max / find_min, mode, the support of the Greedy / EpsilonGreedy probabilities, Greedy / EpsilonGreedy / Random samples)   exact
  probabilities            within 3e-7 of f64 (the bar of test_gpu_parity_mc.py); exactly FLT_MAX where the reference saturates at f64::MAX
  find_max / find_min value, Softmax's Function<(S, A)>   the crafted entry, bit for bit as q_evaluate returns it
  expected_value           within 4 * 2^-24 * sum |p q| of the f64 fold, NaN exactly where that is NaN
  Softmax samples          exact unless u = (x.z >> 8) / 2^24 lies within 2e-6 of a cumulative f64 probability; at most 0.1 % left out per leg

Q is set through the weights: all rows zero except the Fourier bias row (the last feature, phi = 1) -- for tile coding one tiling's slice -- so that
Q(s, .) is the crafted vector for EVERY state; each leg first checks that q_evaluate on random states returns the table (NaN for NaN).  Per-learner
weights: learner i carries vector i.  Shared weights: a few dozen vectors, one after the other, on one ctx.  The Gibbs actor (TD ActorCritic) carries
the vectors as preferences theta; its Function<(S, A)> returns them.

Read-only legs (rsrl_hip_q_find_max / _min / _expected_value, rsrl_hip_policy_probs / _prob / _mode / _sample(states), two sample calls on the draws
orc.draw(seed, env_offset + i, call, BLK_API)) run per family row and policy, Softmax at each tau of the table.  Driver-loop legs reach the YZ and the
wave-uniform variants no read-only call does: lr = 0 (alpha = 0 for the actor), reset, train(1), train(2); the weights must come back bit-identical,
no episode may end, and c.actions after reset / step 0 / step 2 must be the f64 policy_sample of the crafted vector on the loop's own draw
(BLK_INIT at t, BLK_STEP at t and t + 2).  They use the finite, moderate rows (0 * delta must stay 0).

Measured on an MI355X: profiles/policy_edges.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_edges as pe  # noqa: E402
import rsrl_amd as ra  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, OFFSET = 77, 1000
DBL_MAX = np.finfo(np.float64).max


MC, CP, AB = ra.MOUNTAIN_CAR, ra.CART_POLE, ra.ACROBOT
TILE = dict(basis=ra.TILE_CODING, n_tilings=8, tiles_per_dim=4)
# row -> (Context arguments, bf16 sub-table, shared weights, Gibbs actor)
FAMILY = {
    "reg-trait-fast": (dict(domain=MC, order=3, steps_per_launch=1), False, False, False),          # launch_trait_sample; the driver loop: k_step_reg_lm and k_train_reg
    "reg-qop": (dict(domain=CP, order=1), False, False, False),                                     # k_qop<FourierModel>, A = 2
    "generic-fourier": (dict(domain=MC, order=6), False, False, False),                             # k_qop<FourierGenericModel>
    "tile": (dict(domain=MC, **TILE), False, False, False),                                         # k_qop<TileModel>
    "shared-tile": (dict(domain=MC, weight_mode=ra.W_SHARED, **TILE), False, True, False),
    "shared-dense": (dict(domain=MC, order=3, weight_mode=ra.W_SHARED), False, True, False),
    "wave-f32": (dict(domain=AB, order=7), False, False, False),                                    # k_wave_qop
    "wave-bf16": (dict(domain=AB, order=7, weight_dtype=ra.W_BF16), True, False, False),
    "hiv": (dict(domain=ra.HIV_TREATMENT, order=1), False, False, False),                           # launch_hiv_qop, A = 4: kth_set_bit's generic branch
    "gibbs-actor": (dict(domain=MC, order=3, algo=ra.TD_ACTOR_CRITIC), False, False, True),         # theta carries the vectors
}
ROWS = list(FAMILY)
POLICIES = [("greedy", pe.GREEDY, 1.0), ("egreedy", pe.EGREEDY, 1.0), ("random", pe.RANDOM, 1.0)] + [(f"softmax-{t:g}", pe.SOFTMAX, t) for t in pe.TAUS]
N_ACTIONS = {"reg-qop": 2, "hiv": 4}


def rand_states(c, M, seed):
    lo, hi = c.state_bounds()
    rng = np.random.default_rng(seed)
    return (lo[:, None] + (hi - lo)[:, None] * rng.random((c.D, M))).astype(np.float32)


def weights_of(c, v):
    """(F, A) weights with Q(s, .) = v for every s: the bias row of a Fourier basis, the last tiling's slice of a tile table"""
    W = np.zeros((c.F, len(v)), dtype=np.float32)
    if c.cfg.basis == 0:
        W[-1] = v
    else:
        W[c.F - c.F // c.cfg.n_tilings:] = v
    return W


def craft(c, Q, actor):
    for i, v in enumerate(Q):
        (c.set_policy_weights if actor else c.set_weights)(weights_of(c, v), i)


def shared_subset(Q, groups):
    """a few dozen rows of the table for the shared-weight legs: every 12th, every vector without a maximum, NaN / -inf in position 0"""
    with np.errstate(invalid="ignore"):
        pick = [i for i, q in enumerate(Q) if i % 12 == 0 or pe.no_maximum(q) or ((np.isnan(q[0]) or q[0] == -np.inf) and np.isfinite(q[1:]).all() and i % 3 == 0)]
    assert {"tie", "chain", "mag", "nonfinite", "spread"} <= set(groups[pick]) and 24 <= len(pick) <= 60, len(pick)
    return pick


def equal_nan(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def check_readonly(orc, c, Q, row, name, policy, tau, actor, calls_before=0):
    """the read-only calls of ctx c, whose learner / batch item i sees the crafted vector Q[i]; calls_before: the sample calls the ctx has already
    answered (the draws of the next two are addressed past them)"""
    M, A = Q.shape
    S = rand_states(c, M, 5)
    eps = pe.EPSILON
    stats = dict(worst=0.0, left_out=0, samples=0)
    # ---- the precondition: the device's Q(s, .) IS the crafted vector
    if actor:
        q = np.stack([c.policy_prob(S, np.full(M, a, np.int32)) for a in range(A)])         # Softmax's Function<(S, A)>: the raw preference
    else:
        q = c.q_evaluate(S)
    bad = [i for i in range(M) if not equal_nan(q[:, i], Q[i])]
    assert not bad, (row, "q_evaluate does not reproduce", [(Q[i], q[:, i]) for i in bad[:5]], len(bad))
    Q64 = Q.astype(np.float64)
    if not actor:
        # ---- Enumerable
        for fn, ref in ((c.q_find_max, pe.find_max), (c.q_find_min, pe.find_min)):
            idx, val = fn(S)
            for i in range(M):
                assert idx[i] == ref(Q64[i])[0], (row, fn.__name__, Q[i], idx[i])
            got, crafted = val.view(np.uint32), q[idx, np.arange(M)].view(np.uint32)          # the value: the crafted entry, bit for bit
            assert all(got[i] == crafted[i] or (np.isnan(val[i]) and np.isnan(q[idx[i], i])) for i in range(M)), (row, fn.__name__)
        for p in pe.prob_rows(A):
            ev = c.q_expected_value(S, np.repeat(p[:, None], M, axis=1))
            for i in range(M):
                want, mag = pe.expected_value(Q64[i], p)
                if np.isnan(want):
                    assert np.isnan(ev[i]), (row, Q[i], p, ev[i])
                elif np.isinf(want):
                    assert ev[i] == want, (row, Q[i], p, ev[i])
                else:
                    # a product below fp32's normal range is rounded to a multiple of 2^-149 whatever the kernel does: there the bar is that absolute step
                    # per term; everywhere else it is the relative one alone
                    with np.errstate(invalid="ignore"):
                        t = np.abs(Q64[i] * p)
                    floor = A * 2.0 ** -149 if np.any((t > 0) & (t < 2.0 ** -126)) else 0.0
                    assert abs(float(ev[i]) - want) <= 4 * 2.0 ** -24 * mag + floor, (row, Q[i], p, ev[i], want)
    # ---- the policy as a function
    probs = c.policy_probs(S)
    pa = [(np.arange(M) + k) % A for k in (0, 1)]
    psa = [c.policy_prob(S, a.astype(np.int32)) for a in pa]
    mode = c.policy_mode(S) if policy != pe.RANDOM else None
    for i in range(M):
        want = pe.ref_probs(orc, policy, Q64[i], eps, tau)
        sat = want == DBL_MAX
        assert np.all(probs[sat, i] == pe.FLT_MAX), (row, name, Q[i], probs[:, i], want)
        err = float(np.abs(probs[~sat, i] - want[~sat]).max()) if (~sat).any() else 0.0
        assert err <= 3e-7, (row, name, Q[i], probs[:, i], want)
        stats["worst"] = max(stats["worst"], err)
        if policy in (pe.GREEDY, pe.EGREEDY):                                               # the support: the set of maxima, exactly
            floor = 0.0 if policy == pe.GREEDY else eps / A + 1e-3
            assert np.array_equal(probs[:, i] > floor, want > floor), (row, name, Q[i], probs[:, i], want)
        for a, got in zip(pa, psa):
            if policy == pe.SOFTMAX:
                assert equal_nan(got[i], Q[i, a[i]]), (row, name, Q[i], a[i], got[i])
            else:
                assert abs(float(got[i]) - want[a[i]]) <= 3e-7, (row, name, Q[i], a[i], got[i], want)
        if mode is not None:
            assert mode[i] == pe.ref_mode(orc, policy, Q64[i], tau), (row, name, Q[i], mode[i], probs[:, i])
    # ---- samples: two calls
    for call in range(2):
        acts = c.policy_sample(S)
        for i in range(M):
            x = orc.draw(SEED, OFFSET + i, calls_before + call, orc.BLK_API)
            stats["samples"] += 1
            if policy == pe.SOFTMAX and pe.softmax_in_band(orc, Q64[i], x, tau):
                stats["left_out"] += 1
                continue
            assert acts[i] == pe.ref_sample(orc, policy, Q64[i], x, eps, tau), (row, name, call, Q[i], x, acts[i])
    return stats


def report(kind, row, name, stats):
    share = stats["left_out"] / max(1, stats["samples"])
    print(f"\nEDGE {kind} {row} {name}: worst |p - p64| = {stats.get('worst', 0.0):.3g}, left out {stats['left_out']} of {stats['samples']} samples")
    assert share <= 1e-3, (row, name, stats)


@pytest.mark.parametrize("name,policy,tau", POLICIES, ids=[p[0] for p in POLICIES])
@pytest.mark.parametrize("row", ROWS)
def test_read_only_calls(orc, row, name, policy, tau):
    kw, bf16, shared, actor = FAMILY[row]
    if actor and policy != pe.SOFTMAX:
        with pytest.raises(ra.RsrlHipError, match="policy = Softmax"):                      # the Gibbs actor IS a Softmax policy
            ra.Context(n_envs=4, policy=policy, **kw)
        return
    Q, groups = pe.table(N_ACTIONS.get(row, 3), bf16)
    base = dict(policy=policy, epsilon=pe.EPSILON, tau=tau, seed=SEED, env_offset=OFFSET, **kw)
    if not shared:
        with ra.Context(n_envs=len(Q), **base) as c:
            assert c.A == Q.shape[1]
            craft(c, Q, actor)
            stats = check_readonly(orc, c, Q, row, name, policy, tau, actor)
    else:
        stats = dict(worst=0.0, left_out=0, samples=0)
        M = 8
        with ra.Context(n_envs=M, **base) as c:
            for k, j in enumerate(shared_subset(Q, groups)):
                c.set_weights_all(weights_of(c, Q[j]))
                one = check_readonly(orc, c, np.repeat(Q[j][None], M, axis=0), row, name, policy, tau, False, calls_before=2 * k)
                stats = dict(worst=max(stats["worst"], one["worst"]), left_out=stats["left_out"] + one["left_out"], samples=stats["samples"] + one["samples"])
    report("read-only", row, name, stats)


# ------------------------------------------------------------------------------------------------------------------------- the driver loop
DRIVE = [("greedy", pe.GREEDY, 1.0), ("egreedy", pe.EGREEDY, 1.0), ("random", pe.RANDOM, 1.0), ("softmax-0.05", pe.SOFTMAX, 0.05), ("softmax-0.7", pe.SOFTMAX, 0.7)]


def drive(orc, c, Q, row, name, policy, tau, actor, stats):
    """reset, train(1), train(2) on a ctx whose learner i sees Q[i] (already crafted), lr = 0: the loop's samples against the f64 oracle on the loop's draws"""
    N = len(Q)
    getw = c.get_policy_weights if actor else c.get_weights
    probe = sorted({0, N // 2, N - 1}) if not c.shared else [0]
    before = [getw(i).copy() for i in probe]
    t0 = c.step_count
    c.reset()
    Q64 = Q.astype(np.float64)

    def compare(acts, t, blk, what):
        for i in range(N):
            x = orc.draw(SEED, OFFSET + i, t, blk)
            stats["samples"] += 1
            if policy == pe.SOFTMAX and pe.softmax_in_band(orc, Q64[i], x, tau):
                stats["left_out"] += 1
                continue
            assert acts[i] == pe.ref_sample(orc, policy, Q64[i], x, pe.EPSILON, tau), (row, name, what, Q[i], x, acts[i])

    compare(c.actions, t0, orc.BLK_INIT, "reset")
    c.train(1)
    compare(c.actions, t0, orc.BLK_STEP, "step 0")
    c.train(2)
    compare(c.actions, t0 + 2, orc.BLK_STEP, "step 2")
    assert c.step_count == t0 + 3 and np.all(c.episode_steps == 3), (row, name, "an episode ended")
    for i, w in zip(probe, before):                                                          # the condition for all of the above: nothing was learned
        assert np.array_equal(getw(i).view(np.uint32), w.view(np.uint32)), (row, name, "weights moved with lr = 0", i)


DRIVE_CASES = [(row, spl) + pol for row in ROWS for spl in (0, 1) for pol in DRIVE if pol[1] == pe.SOFTMAX or not FAMILY[row][3]]


@pytest.mark.parametrize("row,spl,name,policy,tau", DRIVE_CASES, ids=[f"{c[0]}-{'spl1' if c[1] else 'fused'}-{c[2]}" for c in DRIVE_CASES])
def test_driver_loop_samples(orc, row, spl, name, policy, tau):
    kw, bf16, shared, actor = FAMILY[row]
    Q, groups = pe.table(N_ACTIONS.get(row, 3), bf16)
    keep = pe.moderate(Q)
    Q, groups = Q[keep], groups[keep]
    base = dict(policy=policy, epsilon=pe.EPSILON, tau=tau, seed=SEED, env_offset=OFFSET, lr=0.0, max_episode_steps=100000, **dict(kw, steps_per_launch=spl))
    if actor:
        base["alpha"] = 0.0
    stats = dict(left_out=0, samples=0)
    if not shared:
        with ra.Context(n_envs=len(Q), **base) as c:
            craft(c, Q, actor)
            drive(orc, c, Q, row, name, policy, tau, actor, stats)
    else:
        N = 70                                                                              # more than one wave, a ragged last one
        with ra.Context(n_envs=N, **base) as c:
            for j in range(0, len(Q), len(Q) // 24):                                        # two dozen of the moderate rows, every group among them
                c.set_weights_all(weights_of(c, Q[j]))
                drive(orc, c, np.repeat(Q[j][None], N, axis=0), row, name, policy, tau, False, stats)
    report("driver-loop", row + ("/spl1" if spl else ""), name, stats)


# ------------------------------------------------------------------------------------------------------------------------- tau < 0 is refused
def test_negative_temperature_is_refused():
    """the max-shifted Softmax overflows fp32 for tau < 0 (tests/test_policy_edges_cpu.py): create and the policy rollout refuse it, with the reason"""
    why = "only positive Softmax temperatures are evaluated.*overflow fp32"
    for kw in (dict(policy=ra.SOFTMAX, tau=-1.0), dict(policy=ra.SOFTMAX, tau=-0.05), dict(algo=ra.SARSA, policy=ra.EPSILON_GREEDY, agent_policy=ra.SOFTMAX, agent_tau=-0.5),
               dict(domain=ra.MOUNTAIN_CAR, order=3, algo=ra.TD_ACTOR_CRITIC, policy=ra.SOFTMAX, tau=-2.0)):
        with pytest.raises(ra.RsrlHipError, match=why) as e:
            ra.Context(n_envs=4, **kw)
        assert e.value.code == -1
    with pytest.raises(ra.RsrlHipError, match="Tau parameter in Softmax must be non-zero") as e:        # (the reference's own rule keeps its message)
        ra.Context(n_envs=4, policy=ra.SOFTMAX, tau=-1e-8)
    assert e.value.code == -1
    with ra.Context(n_envs=4, policy=ra.GREEDY, tau=-1.0, max_episode_steps=20) as c:        # tau is not read by the other policies
        with pytest.raises(ra.RsrlHipError, match=why) as e:
            c.rollout_policy(ra.SOFTMAX, 10, tau=-1.0)
        assert e.value.code == -1
        c.rollout_policy(ra.SOFTMAX, 10, tau=1e-7)
        c.rollout_policy(ra.EPSILON_GREEDY, 10, tau=-1.0)
