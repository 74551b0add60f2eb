"""ContinuousMountainCar, the Beta policy and the iLSTD ActorCritic over them (train_tdac_beta.hip) on the device, against tests/beta_numpy.py:
the domain's f32 transition, the rule (the critic half bit for bit an RSRL_ILSTD ctx's), the policy side (params, mode, pdf), the sampler
(distribution, range, and draw for draw on the same Philox words), and the agent contract through tests/agent_contract.py: train against the host
trait loop / launch depths / shards, checkpoints (file version 10, aux_kind 11), the refusals and the C++ example.

The f32 chain of psi, ln and exp has no derivable bound: the bounds of MEASURED below are four times the maxima profiles/tdac_beta_rate.md records
(the factor covers inputs the measurement did not see); every test prints its figure before it asserts."""
import functools
import os

import numpy as np
import pytest
from scipy import stats

import rsrl_amd
from rsrl_amd import RsrlHipError, _abi
from tests import beta_numpy as bn
from tests.agent_contract import check_checkpoint_resume, check_foreign_checkpoints_refused, check_train_invariance, run_example

pytestmark = pytest.mark.gpu

CMC, AC, ILSTD, BETA = rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, rsrl_amd.ILSTD_ACTOR_CRITIC, rsrl_amd.ILSTD, rsrl_amd.BETA
ORDERS = [1, 3, 5]           # F = 4, 16, 36: groups of 4, 16 and 64 lanes -- the smallest group, the example's, a whole wave
N = 67                       # the last block holds a partial set of groups
ACTIONS = [-3.0, -1.0, -0.2, 0.0, 0.7, 1.0, 3.0]
SHAPES = [(1.3, 1.3), (2.5, 6.0), (12.0, 1.05)]
KS_C = 3.27                  # 2 exp(-2 c^2) = 2e-9
# a draw whose acceptance test lies within this of its boundary (in f64) may be decided the other way by the device's f32 test: the test's sides are
# sums of terms up to d v <= ~30, each within a few f32 ulps (2e-6 at 30) of its f64 value
MARGIN = 2e-5
ESTATE, EINVAL = -5, -1

# four times the measured maxima (profiles/tdac_beta_rate.md)
MEASURED = {
    ("rule", 1): 4 * 1.934e-7, ("rule", 3): 4 * 9.788e-7, ("rule", 5): 4 * 1.908e-6,      # max |dw| / max(1, |w|) over three rounds of handle
    "params": 4 * 1.301e-7,      # max |d alpha| / max(1, alpha), beta likewise
    "mode": 4 * 2.721e-7,        # max |d mode|
    "pdf": 4 * 5.177e-6,         # max |d pdf| / max(1, pdf)
    "sample": 4 * 4.649e-7,      # max |d x| over the draws of the three shape pairs that lie clear of an acceptance boundary
}

BASE = dict(domain=CMC, order=3, algo=AC, policy=BETA, n_envs=N, seed=5, gamma=0.95, lr=0.05, alpha=0.3, n_steps=3)


def ctx(**kw):
    return rsrl_amd.Context(**dict(BASE, **kw))


def hold(name, figure):
    print("measured %s: %.4g (bound %.4g)" % (name, figure, MEASURED[name]))
    assert figure <= MEASURED[name], (name, figure, MEASURED[name])


def crafted_states():
    """67 states on a grid over the state space -- both walls, the start, the goal's neighbourhood -- none of whose seven transitions lands within
    1e-4 of x = 0.6 before the clip (in the f64 restatement): the terminal flag is then the same in f32"""
    out = []
    for x in np.linspace(-1.2, 0.599, 13):
        for v in (-0.07, -0.03, 0.0, 0.011, 0.05, 0.07):
            s = np.array([x, v], dtype=np.float32)
            ok = True
            for a in ACTIONS:
                vv = bn.clip(-0.07, float(s[1]) + 0.0015 * bn.clip(-1.0, a, 1.0) - 0.0025 * np.cos(3.0 * float(s[0])), 0.07)
                ok &= abs(float(s[0]) + vv - 0.6) > 1e-4
            if ok:
                out.append(s)
    out += [np.array(s, dtype=np.float32) for s in ((-0.5, 0.0), (0.59, 0.06), (0.55, 0.07), (-1.2, -0.07))]
    assert len(out) >= N
    return np.array(out[-N:]).T.copy()


def test_domain_step_against_the_restatement():
    """DESIGN 6's bound for MountainCar's transition, 1e-5 on both components: the arithmetic is that kernel's with one term changed"""
    S = crafted_states()
    n_term = 0
    with ctx() as c:
        assert c.A == 0 and c.D == 2 and c.n_policy_out == 2 and c.action_bounds() == (-1.0, 1.0)
        lo, hi = c.state_bounds()
        assert lo.tolist() == [-1.2, -0.07] and hi.tolist() == [0.6, 0.07]
        for a in ACTIONS:
            c.states = S
            frm, nxt, rew, term = c.domain_step(np.full(N, a, dtype=np.float32))
            assert np.array_equal(frm, S) and np.array_equal(c.states, nxt)
            for i in range(N):
                (x, v), r, t = bn.cmc_step(S[:, i], a)
                assert abs(nxt[0, i] - x) <= 1e-5 and abs(nxt[1, i] - v) <= 1e-5, (a, i, nxt[:, i], x, v)
                assert bool(term[i]) == t and rew[i] == r, (a, i)
                n_term += t
        # the ctx's pending actions when none are given
        c.states = S
        c.actions = np.linspace(-1.0, 1.0, N).astype(np.float32)
        _, nxt2, _, _ = c.domain_step()
        for i in (0, 33, N - 1):
            (x, v), _, _ = bn.cmc_step(S[:, i], np.linspace(-1.0, 1.0, N).astype(np.float32)[i])
            assert abs(nxt2[0, i] - x) <= 1e-5 and abs(nxt2[1, i] - v) <= 1e-5
    assert n_term > 0


@functools.lru_cache(maxsize=None)
def _case(orc, order):
    return bn.handle_case(orc, order)


@pytest.mark.parametrize("order", ORDERS)
def test_rule_against_the_restatement_and_the_critic_half_is_ilstd_bit_for_bit(orc, order):
    case = _case(orc, order)
    F, p = case["F"], case["params"]
    kw = dict(order=order, n_envs=N, seed=17, gamma=p["gamma"], n_steps=p["n_steps"])
    with ctx(lr=p["lr"], alpha=p["alpha"], **kw) as c, rsrl_amd.Context(domain=rsrl_amd.MOUNTAIN_CAR, algo=ILSTD, policy=rsrl_amd.RANDOM, alpha=p["lr"], **kw) as v:
        assert c.n_out == 1 and c.F == F and c.n_policy_out == 2
        for i, (theta, A, mu, W) in enumerate(case["init"]):
            c.set_lstd_state(theta, A, mu, i)
            v.set_lstd_state(theta, A, mu, i)
            c.set_policy_weights(W, i)
        phi32, got = [], []
        for k, (frm, a, rew, nxt, term) in enumerate(case["rounds"]):
            phi32.append(c.project(frm))
            td = c.handle(frm, a, rew, nxt, term)
            td_v = v.handle(frm, np.zeros(N, dtype=np.int32), rew, nxt, term)
            assert np.array_equal(td.view(np.uint32), td_v.view(np.uint32)), k
            for i in range(N):
                for x, y in zip(c.get_lstd_state(i), v.get_lstd_state(i)):
                    assert x.tobytes() == y.tobytes(), (k, i)
                d = case["diag"][k, i]
                assert abs(float(td[i]) - d) <= 2.0 ** -22 * (1.0 + abs(d)), (k, i, td[i], d)
            got.append(np.stack([c.get_policy_weights(i) for i in range(N)]))
        assert c.step_count == len(case["rounds"])
    want = bn.actor_after(orc, case, order, phi32)
    keep = ~case["skipped"]
    assert (~keep).sum() <= 0.05 * N
    fig = max(float(np.max(np.abs(g[keep] - w[keep]) / np.maximum(1.0, np.abs(w[keep])))) for g, w in zip(got, want))
    moved = max(float(np.max(np.abs(w[keep] - np.stack([x[3] for x in case["init"]])[keep]))) for w in want)
    assert moved > 1e-3                                               # the columns moved far more than the bound
    hold(("rule", order), fig)


def test_policy_side_against_the_restatement(orc):
    order = 3
    rng = np.random.default_rng(11)
    special = [(10.0, 10.0), (12.5, 0.0), (0.0, 0.0), (-20.0, -20.0), (-25.0, 1.0), (2.0, -30.0), (10.0, -20.0), (9.999, 30.0)]
    with ctx(order=order, seed=3) as c:
        F = c.F
        W = np.zeros((N, F, 2), dtype=np.float32)
        for i in range(N):
            if i < len(special):
                W[i, F - 1] = special[i]                              # all weight on the constant feature: x is the weight itself
            elif i < 32:
                W[i, F - 1] = rng.uniform(-3.0, 3.0, size=2)
            else:
                w = rng.normal(size=(F, 2))
                W[i] = w * rng.uniform(0.5, 3.0, size=2) / np.abs(w).sum(axis=0)
            c.set_policy_weights(W[i], i)
            assert np.array_equal(c.get_policy_weights(i), W[i])
        S = rng.uniform([-1.2, -0.07], [0.6, 0.07], size=(N, 2)).T.astype(np.float32)
        phi = c.project(S).astype(np.float64)
        x = np.einsum("fn,nfk->nk", phi, W.astype(np.float64))
        assert np.array_equal(x[:len(special)], np.array(special, dtype=np.float32).astype(np.float64))
        al, be = bn.beta_params(x[:, 0], x[:, 1])
        assert abs(al[2] - 1.6931471805599454) < 1e-15 and 0.0 < al[3] - 1.0 < 3e-9 and al[3] == be[3] and al[0] == 11.0      # (f64: exp(-20) survives; f32: alpha = 1)
        ga, gb = c.policy_params(S)
        hold("params", max(float(np.max(np.abs(ga - al) / np.maximum(1.0, al))), float(np.max(np.abs(gb - be) / np.maximum(1.0, be)))))
        assert ga.min() >= 1.0 and gb.min() >= 1.0 and ga[3] == 1.0 and gb[3] == 1.0 and ga[0] == 11.0
        # the mode of the DEVICE's parameters decides the branch (alpha = 1 exactly: the mean); the value is held to the restatement's
        mode = c.policy_mode(S)
        want = bn.beta_mode(ga.astype(np.float64), gb.astype(np.float64))
        assert mode[3] == 0.5 and mode[4] == np.float32(1.0 / (1.0 + float(gb[4])))      # the mean branch
        hold("mode", float(np.max(np.abs(mode - want))))
        a = rng.uniform(0.0, 1.0, size=N).astype(np.float32)
        a[0], a[1], a[5] = 0.0, 1.0, 0.5
        pdf = c.policy_pdf(S, a)
        wantp = bn.beta_pdf(al, be, a.astype(np.float64))
        assert np.isfinite(pdf).all()
        hold("pdf", float(np.max(np.abs(pdf - wantp) / np.maximum(1.0, wantp))))
        # the value side: V from the f64 theta, as iLSTD's
        th = rng.normal(size=F)
        c.set_lstd_state(th, np.eye(F), np.zeros(F), 9)
        q = c.q_evaluate(S)
        vv = np.float32(orc.fourier_project(orc.MOUNTAIN_CAR, order, S[:, 9]) @ th)
        assert q.shape == (1, N) and abs(q[0, 9] - vv) <= abs(np.spacing(vv))


def test_policy_mode_of_parameters_a_few_ulps_above_one():
    """preferences in (-17, -10): alpha - 1 and beta - 1 are one to a few hundred f32 ulps of 1, both above 1, so the mode is their ratio.  Found by
    tests/fuzz_beta.py: with the denominator formed as alpha + beta - 2 the sum rounded to a multiple of 2^-22 first and the mode of
    (1 + 2^-23, 1 + 2^-22) came out as 1/4 or 1/2 for 1/3"""
    prefs = [(-15.9, -15.2), (-15.2, -14.5), (-14.0, -15.5), (-12.0, -13.0), (-16.5, -10.5), (-10.5, -16.5), (-15.9, -15.9), (-15.2, -15.9)]
    n = len(prefs)
    with ctx(order=1, n_envs=n) as c:
        for i, pr in enumerate(prefs):
            W = np.zeros((c.F, 2), dtype=np.float32)
            W[c.F - 1] = pr
            c.set_policy_weights(W, i)
        S = np.zeros((2, n), dtype=np.float32)
        S[0] = -0.5
        ga, gb = c.policy_params(S)
        assert ga.min() > 1.0 and gb.min() > 1.0 and max(ga.max(), gb.max()) < 1.0 + 1e-4
        assert ga[0] == np.float32(1.0 + 2.0 ** -23) and gb[0] == np.float32(1.0 + 2.0 ** -22)      # the pair of the docstring: the mode is 1/3
        mode = c.policy_mode(S)
        hold("mode", float(np.max(np.abs(mode - bn.beta_mode(ga.astype(np.float64), gb.astype(np.float64))))))


@pytest.mark.parametrize("alpha,beta", SHAPES)
def test_sampler_distribution_range_and_draws(alpha, beta):
    """4 096 learners with identical columns, 16 policy_sample calls on explicit states: 65 536 draws"""
    M, calls, seed = 4096, 16, 77
    with ctx(order=1, n_envs=M, seed=seed) as c:
        W = bn.columns_for(alpha, beta, c.F)
        for i in range(M):
            c.set_policy_weights(W, i)
        S = np.zeros((2, M), dtype=np.float32)
        S[0] = -0.5
        da, db = c.policy_params(S)
        assert np.all(da == da[0]) and np.all(db == db[0]) and abs(da[0] - alpha) < 1e-5 and abs(db[0] - beta) < 1e-5
        draws = np.stack([c.policy_sample(S) for _ in range(calls)])
    a64, b64 = float(da[0]), float(db[0])
    flat = draws.astype(np.float64).ravel()
    n = flat.size
    assert n == 65536 and flat.min() >= bn.LO and flat.max() <= bn.HI
    d = stats.kstest(flat, stats.beta(a64, b64).cdf).statistic
    print("KS distance %.4g (bound %.4g)" % (d, KS_C / np.sqrt(n)))
    assert d < KS_C / np.sqrt(n), (alpha, beta, d)
    ref, margin = zip(*(bn.beta_sample(seed, np.arange(M), t, bn.BLK_API, a64, b64) for t in range(calls)))
    ref, margin = np.stack(ref), np.stack(margin)
    close = margin < MARGIN                                           # the restatement alone decides which draws a rounded test may flip
    print("draws within %g of an acceptance boundary: %d" % (MARGIN, close.sum()))
    assert close.sum() <= 8, close.sum()
    err = np.abs(draws.astype(np.float64) - ref)
    hold("sample", float(err[~close].max()))


def _start_near_the_goal(c, off):
    """reset, then every fourth learner (by global id) at x = 0.59, v = 0.06: terminal ends occur as well as cut ones"""
    c.reset()
    s = c.states
    s[:, (np.arange(c.N) + off) % 4 == 0] = np.array([[0.59], [0.06]], dtype=np.float32)
    c.states = s


@pytest.mark.parametrize("order", ORDERS)
def test_train_is_the_trait_loop_launch_depth_and_shard_invariant(order):
    """(66 learners: the harness joins two shards of N / 2; the last block still holds a partial set of groups at every order)"""
    n, K, cap = 66, 40, 7
    kw = dict(order=order, n_envs=n, max_episode_steps=cap, lr=0.02, alpha=0.2, gamma=0.97, n_steps=2)
    st, ref = check_train_invariance(ctx, kw, K, cap, depths=(1, 3, 0), first_split=13, kernel="k_train_tdac_beta", setup=_start_near_the_goal)
    assert st["env_steps"] == n * K and st["episodes"] > st["episodes_truncated"] > 0 and st["sum_abs_td_error"] > 0
    assert np.isfinite(ref["lstd_theta"]).all() and np.abs(ref["lstd_theta"]).max() > 0 and np.abs(ref["theta"]).max() > 0
    assert ref["actions"].dtype == np.float32 and ref["actions"].min() >= bn.LO and ref["actions"].max() <= bn.HI and ref["theta"].shape == (n, (order + 1) ** 2, 2)


def test_checkpoint_resumes_bitwise_and_foreign_files_are_refused(tmp_path):
    kw = dict(n_envs=32, order=3, max_episode_steps=17, lr=0.02, alpha=0.2)
    path = os.path.join(str(tmp_path), "tdac_beta.ckpt")

    def the_f32_actions_and_the_columns_move_the_checksum(a, b):
        before = b.checksum()
        act = b.actions
        act[3] = np.nextafter(act[3], np.float32(0.5))
        b.actions = act
        moved = b.checksum()
        assert moved[1] != before[1] and moved[0] == before[0]
        pw = b.get_policy_weights(7)
        pw[2, 1] = np.nextafter(pw[2, 1], np.float32(np.inf))
        b.set_policy_weights(pw, 7)
        assert b.checksum()[0] != before[0]

    check_checkpoint_resume(ctx, kw, path, 25, 20, carry=("states", "actions", "episode_steps"), then=the_f32_actions_and_the_columns_move_the_checksum)
    with open(path, "rb") as f:
        head = f.read(72)
    F = 16
    assert int.from_bytes(head[8:12], "little") == 10 and int.from_bytes(head[12:16], "little") == CMC and int.from_bytes(head[52:56], "little") == 11
    assert os.path.getsize(path) == 72 + 32 * 8 * (F + F * F + F) + 32 * 4 * F * 2
    gibbs = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=AC, policy=rsrl_amd.SOFTMAX, n_envs=32, n_steps=3, lr=0.02, alpha=0.2)
    ilstd = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=ILSTD, policy=rsrl_amd.RANDOM, n_envs=32, n_steps=3, alpha=0.02)
    check_foreign_checkpoints_refused(ctx, kw, path, [gibbs, ilstd], tmp_path)


def test_refusals_in_both_directions():
    L = _abi.lib()
    S = np.zeros((2, N), dtype=np.float32)
    S[0] = -0.5
    ai, af = np.zeros(N, dtype=np.int32), np.full(N, 0.5, dtype=np.float32)
    r, t, out_i, out_f = np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.float32)
    p = lambda x: x.ctypes.data_as(_abi.C.c_void_p)      # noqa: E731

    def refused(call, code=ESTATE):
        rc = call()
        assert rc == code and L.rsrl_hip_last_error(), (rc, L.rsrl_hip_last_error())

    with ctx(max_episode_steps=20) as c:
        h, F = c._h, c.F
        before = c.checksum()
        # the int32 calls
        for call in (lambda: L.rsrl_hip_get_actions(h, p(out_i)), lambda: L.rsrl_hip_set_actions(h, p(ai)),
                     lambda: L.rsrl_hip_domain_step(h, p(ai), p(S.copy()), p(S.copy()), p(r), p(t)),
                     lambda: L.rsrl_hip_handle(h, p(S), p(ai), p(r), p(S), p(t), N, p(out_f)),
                     lambda: L.rsrl_hip_policy_sample(h, p(S), N, p(out_i)), lambda: L.rsrl_hip_policy_sample(h, None, N, p(out_i)),
                     lambda: L.rsrl_hip_policy_mode(h, p(S), N, p(out_i))):
            refused(call)
        # what needs an enumerable action set, an int32 trajectory, or state this agent does not have
        probs = np.zeros((3, N), dtype=np.float32)
        for k, call in enumerate((lambda: L.rsrl_hip_policy_probs(h, p(S), N, p(probs)), lambda: L.rsrl_hip_policy_prob(h, p(S), p(ai), N, p(out_f)), lambda: c.q_find_max(S),
                                  lambda: c.q_find_min(S), lambda: L.rsrl_hip_q_expected_value(h, p(S), N, p(probs), p(out_f)),
                                  lambda: c.get_traces(0), lambda: c.set_traces(np.zeros((F, 1)), 0), lambda: L.rsrl_hip_get_td_weights(h, 0, p(probs)),
                                  lambda: L.rsrl_hip_set_td_weights(h, 0, p(probs)), lambda: L.rsrl_hip_get_behaviour_weights(h, 0, p(probs)),
                                  lambda: c.handle_batch(np.zeros((1, 2, N)), np.zeros((1, N)), np.zeros((1, N)), np.zeros(N)),
                                  lambda: c.rollout_trajectory(5), lambda: c.rollout_policy(rsrl_amd.RANDOM, 5))):
            try:
                rc = call()
            except RsrlHipError as e:
                rc = e.code
            assert rc == ESTATE, (k, rc)
        # host actions are validated
        for bad in (np.nan, np.inf, 1.5, -1.0001):
            x = af.copy()
            x[5] = bad
            refused(lambda: L.rsrl_hip_set_actions_f32(h, p(x)), EINVAL)
        x = af.copy()
        x[5] = np.nan
        refused(lambda: L.rsrl_hip_domain_step_f32(h, p(x), p(S.copy()), p(S.copy()), p(r), p(t)), EINVAL)
        refused(lambda: L.rsrl_hip_handle_f32(h, p(S), p(x), p(r), p(S), p(t), N, p(out_f)), EINVAL)
        assert c.checksum() == before and c.step_count == 0
        # rollout_greedy runs policy.mode from the start state: with zero columns alpha = beta, the mode is 0.5
        n_states, tot = c.rollout_greedy(0)
        (x, v), steps = bn.cmc_start(), 0
        while steps < 20:
            (x, v), _, term = bn.cmc_step((x, v), 0.5)
            steps += 1
            if term:
                break
        assert np.all(n_states == steps + 1) and np.all(tot == -float(steps))
    with rsrl_amd.Context(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=AC, policy=rsrl_amd.SOFTMAX, n_envs=N, n_steps=2) as g:
        h = g._h
        assert g.n_policy_out == 3 and not g.continuous
        lo, hi = _abi.C.c_double(), _abi.C.c_double()
        refused(lambda: L.rsrl_hip_action_bounds(h, _abi.C.byref(lo), _abi.C.byref(hi)), EINVAL)
        for call in (lambda: L.rsrl_hip_get_actions_f32(h, p(out_f)), lambda: L.rsrl_hip_set_actions_f32(h, p(af)),
                     lambda: L.rsrl_hip_domain_step_f32(h, p(af), p(S.copy()), p(S.copy()), p(r), p(t)),
                     lambda: L.rsrl_hip_handle_f32(h, p(S), p(af), p(r), p(S), p(t), N, p(out_f)),
                     lambda: L.rsrl_hip_policy_sample_f32(h, p(S), N, p(out_f)), lambda: L.rsrl_hip_policy_sample_f32(h, None, N, p(out_f)),
                     lambda: L.rsrl_hip_policy_mode_f32(h, p(S), N, p(out_f)), lambda: L.rsrl_hip_policy_params(h, p(S), N, p(out_f), p(r)),
                     lambda: L.rsrl_hip_policy_pdf(h, p(S), p(af), N, p(out_f))):
            refused(call)
    with rsrl_amd.Context(n_envs=4) as q:
        assert q.n_policy_out == 0


def test_reset_samples_on_the_initial_stream_and_leaves_both_agents_alone():
    seed = 41
    with ctx(seed=seed, order=3, env_offset=100) as c:
        W = bn.columns_for(2.5, 6.0, c.F)
        for i in range(N):
            c.set_policy_weights(W, i)
        c.set_lstd_state(np.arange(c.F, dtype=np.float64), 2.0 * np.eye(c.F), np.ones(c.F), 3)
        c.reset()
        assert np.array_equal(c.states, np.tile(np.array([[-0.5], [0.0]], dtype=np.float32), (1, N))) and not c.episode_steps.any()
        al, be = c.policy_params(c.states)
        ref, margin = bn.beta_sample(seed, 100 + np.arange(N), 0, bn.BLK_INIT, float(al[0]), float(be[0]))
        keep = margin >= MARGIN
        assert np.max(np.abs(c.actions.astype(np.float64) - ref)[keep]) <= MEASURED["sample"] and keep.sum() >= N - 1
        th, m, u = c.get_lstd_state(3)
        assert np.array_equal(th, np.arange(c.F)) and np.array_equal(m, 2.0 * np.eye(c.F)) and np.array_equal(u, np.ones(c.F))
        assert np.array_equal(c.get_policy_weights(5), W)
        # policy_sample() before the first handle repeats the initial stream; after one, the step's
        assert np.array_equal(c.policy_sample(), c.actions)


def test_example_builds_and_runs_two_episodes(tmp_path):
    out = run_example(tmp_path, "tdac_beta", [8, 2, 1000])
    lines = out.strip().splitlines()
    assert len(lines) == 4 and lines[0].startswith("Batch 1:") and lines[1].startswith("Batch 2:") and "Beta:" in lines[2] and lines[3].startswith("OOS:")
    assert "nan" not in out.lower()
