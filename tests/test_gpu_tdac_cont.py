"""ActorCritic::tdac with a TD(0) critic over the Gaussian and the Beta policy (RSRL_CONTINUOUS_TD_ACTOR_CRITIC, train_cont.hip) on the
device, against tests/tdac_cont_numpy.py: the TD half bit for bit an RSRL_TD ctx's on RSRL_MOUNTAIN_CAR, the columns of all 67 learners against
the f64 restatement, alpha = 0, the agent contract through tests/agent_contract.py (train against the host trait loop / launch depths / shards,
the checkpoint, foreign files, the C++ examples), the refusals, reset, the pending-action step and the mode rollout, device-pointer calls against
a twin ctx, and a slice of the random campaign (tests/fuzz_tdac_cont.py).

The f32 chain of the policy step (ln, exp, digamma, the division by Sigma^2) has no derivable bound: the bounds of MEASURED below are four times
the maxima profiles/tdac_cont_rate.md records (scripts/tdac_cont_rate.py, on these very inputs; the factor covers inputs the measurement did not
see); the test prints its figure before it asserts.  What is compared against is the f64 restatement on the device's own projection, never a
second run of the device.  N = 67: one full wave and a partial one; orders 1, 2, 3, 5 give F = 4 / 9 / 16 / 36, the unpacked (9) and the packed
register path."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import rsrl_amd
from rsrl_amd import RsrlHipError, _abi
from rsrl_amd._devmem import DeviceBuffer
from tests import beta_numpy as bn
from tests import gaussian_numpy as gn
from tests import tdac_cont_numpy as tn
from tests.agent_contract import check_checkpoint_resume, check_foreign_checkpoints_refused, check_train_invariance, run_example
from tests.campaign import run_slice
from tests.fuzz_tdac_cont import trait_loop

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CMC, MC, TDAC, NAC, CACLA = rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, rsrl_amd.MOUNTAIN_CAR, 35, rsrl_amd.NAC, rsrl_amd.CACLA
GAUSSIAN, BETA = rsrl_amd.GAUSSIAN, rsrl_amd.BETA
POLICIES = [GAUSSIAN, BETA]
PID = {GAUSSIAN: "gaussian", BETA: "beta"}
ORDERS = [1, 2, 3, 5]        # F = 4, 9, 16, 36
N = 67                       # one full wave and a partial one
ESTATE, EINVAL = -5, -1

# four times the measured maxima (profiles/tdac_cont_rate.md): max |d column| / max(1, |column|) over all 67 learners after three rounds
MEASURED = {(GAUSSIAN, 1): 4 * 9.412e-8, (GAUSSIAN, 2): 4 * 1.443e-7, (GAUSSIAN, 3): 4 * 1.106e-7, (GAUSSIAN, 5): 4 * 1.032e-7,
            (BETA, 1): 4 * 1.162e-7, (BETA, 2): 4 * 1.335e-7, (BETA, 3): 4 * 1.210e-7, (BETA, 5): 4 * 1.160e-7}

BASE = dict(domain=CMC, order=3, algo=TDAC, n_envs=N, seed=5, gamma=0.95, lr=0.01, alpha=0.01)
both = pytest.mark.parametrize("policy", POLICIES, ids=[PID[p] for p in POLICIES])


class Ctx(rsrl_amd.Context):
    """tests/agent_contract.snapshot compares an agent's `weights`; it does not know this agent's policy columns.  Here get_weights shows all
    three columns of a learner, (F, 3): w, then the policy's two -- so the harness holds the policy to the same bits as the V learner"""

    def get_weights(self, env_index=0):
        return np.concatenate([super().get_weights(env_index), self.get_policy_weights(env_index)], axis=1)


def ctx(**kw):
    return Ctx(**dict(BASE, **kw))


def plain(**kw):
    return rsrl_amd.Context(**dict(BASE, **kw))


def td_ctx(order, p):
    return rsrl_amd.Context(domain=MC, order=order, algo=rsrl_amd.TD, policy=rsrl_amd.RANDOM, n_envs=N, seed=9, gamma=p["gamma"], lr=p["lr"])


# ---- 1. the rule: one pass over handle_case's inputs per order and policy, shared and left unchanged
@functools.lru_cache(maxsize=None)
def _run(order, policy):
    with plain(order=order, policy=policy) as probe:
        case = tn.handle_case(order, probe.project, policy)
    p = case["params"]
    with plain(order=order, policy=policy, gamma=p["gamma"], lr=p["lr"], alpha=p["alpha"]) as c, td_ctx(order, p) as t:
        fig, arr = tn.figures(c, t, case)
        arr["steps"] = c.step_count
    print("measured (%s, %d): %.4g" % (PID[policy], order, fig["cols"]))
    return case, fig, arr


@both
@pytest.mark.parametrize("order", ORDERS)
def test_td_half_is_rsrl_tds_bit_for_bit(order, policy):
    case, _, arr = _run(order, policy)
    assert arr["steps"] == len(case["rounds"]) == 3
    w0 = np.stack([w for w, _ in case["init"]])
    for k in range(3):
        assert arr["td"][k].shape == (N,) and arr["td"][k].tobytes() == arr["td_ref"][k].tobytes(), k
        assert arr["ws"][k].shape == (N, case["F"], 1) and arr["ws"][k].tobytes() == arr["ws_ref"][k].tobytes(), k
    assert np.max(np.abs(arr["ws"][2][:, :, 0] - w0)) > 1e-4 and np.isfinite(arr["ws"][2]).all()          # the V learner moved
    # ... and against the f64 restatement, loosely: the identity above is the test, this guards the reference ctx itself
    assert np.max(np.abs(arr["ws"][2][:, :, 0] - arr["want_w"])) < 1e-5
    assert np.max(np.abs(np.stack(arr["td"]) - np.stack(arr["tds"]))) < 1e-5


@both
@pytest.mark.parametrize("order", ORDERS)
def test_columns_against_the_f64_restatement(order, policy):
    case, fig, arr = _run(order, policy)
    assert tn.keeps_every_learner_in(case, arr["cs"], arr["xs"], arr["want_w"], arr["want_cols"]) == []      # every learner is in: none left out
    init = np.stack([W for _, W in case["init"]]).astype(np.float64)
    moved = np.abs(arr["want_cols"] - init).max(axis=(1, 2))
    assert moved.min() > 1e-7 and moved.max() > 1e-3 and np.isfinite(arr["cols"][2]).all()                  # the columns move by far more than any bound
    print("measured (%s, %d): %.4g (bound %.4g)" % (PID[policy], order, fig["cols"], MEASURED[(policy, order)]))
    assert fig["cols"] <= MEASURED[(policy, order)], (policy, order, fig["cols"], MEASURED[(policy, order)])


@both
@pytest.mark.parametrize("order", [2, 3])
def test_alpha_zero_leaves_the_columns_and_the_td_half_is_still_tds(order, policy):
    case = _run(order, policy)[0]
    p = case["params"]
    with plain(order=order, policy=policy, gamma=p["gamma"], lr=p["lr"], alpha=0.0) as c, td_ctx(order, p) as t:
        _, arr = tn.figures(c, t, dict(case, params=dict(p, alpha=0.0)))
    init = np.stack([W for _, W in case["init"]])
    for k in range(3):
        assert np.array_equal(arr["cols"][k], init), k                                                      # equal as values (fma(0, phi, w) is w)
        assert arr["td"][k].tobytes() == arr["td_ref"][k].tobytes() and arr["ws"][k].tobytes() == arr["ws_ref"][k].tobytes(), k
    assert np.max(np.abs(arr["ws"][2] - np.stack([w for w, _ in case["init"]])[:, :, None])) > 1e-4


# ---- 2. the agent contract
CAP, K = 7, 40


def _start_near_the_goal(c, off):
    """reset, then every fourth learner (by global id) at x = 0.59, v = 0.06: terminal ends occur as well as cut ones"""
    c.reset()
    s = c.states
    s[:, (np.arange(c.N) + off) % 4 == 0] = np.array([[0.59], [0.06]], dtype=np.float32)
    c.states = s


@both
@pytest.mark.parametrize("order", ORDERS)
def test_train_is_the_trait_loop_launch_depth_and_shard_invariant(order, policy):
    """(66 learners: the harness joins two shards of N / 2.)  The trait loop steps on the PENDING actions: domain_step_f32(NULL), handle_f32,
    domain_reset, policy_sample_f32(NULL)"""
    n = 66
    kw = dict(order=order, policy=policy, n_envs=n, max_episode_steps=CAP, lr=0.02, alpha=0.01, gamma=0.97)
    st, ref = check_train_invariance(ctx, kw, K, CAP, depths=(1, 3, 0), first_split=13, kernel="k_train_tdac_cont", setup=_start_near_the_goal, trait=trait_loop)
    F = (order + 1) ** 2
    assert st["env_steps"] == n * K and st["episodes"] > st["episodes_truncated"] > 0 and st["sum_abs_td_error"] > 0
    assert st["sum_episode_steps"] >= CAP * st["episodes_truncated"] + (st["episodes"] - st["episodes_truncated"])
    w = ref["weights"]
    assert w.shape == (n, F, 3) and np.isfinite(w).all()
    assert np.abs(w[:, :, 0]).max(axis=1).min() > 0 and np.abs(w[:, :, 1:]).max(axis=(1, 2)).min() > 0      # all three columns of every learner moved
    a = ref["actions"]
    assert a.dtype == np.float32 and np.isfinite(a).all()
    if policy == BETA:
        assert a.min() >= 0.0 and a.max() <= 1.0 and a.max() > 0.6 and a.min() < 0.4                        # the agent's action, not the domain's 2a - 1


@both
def test_checkpoint_resumes_bitwise_and_foreign_files_are_refused(tmp_path, policy):
    kw = dict(n_envs=32, order=3, policy=policy, max_episode_steps=17, lr=0.02)
    path = os.path.join(str(tmp_path), "tdac_cont.ckpt")
    check_checkpoint_resume(ctx, kw, path, 25, 20, carry=("states", "actions", "episode_steps"))
    with open(path, "rb") as f:
        head = f.read(72)
    F = 16
    assert int.from_bytes(head[8:12], "little") == 10 and int.from_bytes(head[12:16], "little") == CMC
    assert int.from_bytes(head[44:48], "little") == TDAC and int.from_bytes(head[52:56], "little") == (17 if policy == GAUSSIAN else 16)
    assert os.path.getsize(path) == 72 + 32 * 4 * F + 32 * 4 * F * 2
    other = dict(domain=CMC, order=3, n_envs=32, lr=0.02)
    tdac_beta = dict(other, algo=rsrl_amd.ILSTD_ACTOR_CRITIC, policy=BETA, n_steps=2, alpha=0.2)            # kind 11
    nac_beta = dict(other, algo=NAC, policy=BETA, n_steps=5)                                                # kind 12
    nac_gauss = dict(other, algo=NAC, policy=GAUSSIAN, n_steps=5)                                           # kind 14
    cacla = dict(other, algo=CACLA, policy=GAUSSIAN)                                                        # kind 15
    twin = dict(other, algo=TDAC, policy=BETA if policy == GAUSSIAN else GAUSSIAN)                          # kind 16 / 17: each other's
    td = dict(domain=MC, order=3, algo=rsrl_amd.TD, policy=rsrl_amd.RANDOM, n_envs=32, lr=0.02)
    check_foreign_checkpoints_refused(ctx, kw, path, [tdac_beta, nac_beta, nac_gauss, cacla, twin, td], tmp_path)


@pytest.mark.parametrize("name", ["tdac_gaussian", "tdac_beta_td"])
def test_example_builds_and_runs(tmp_path, name):
    out = run_example(tmp_path, name, [8, 2, 300])
    lines = out.strip().splitlines()
    assert lines[0].startswith("Batch 1:") and lines[1].startswith("Batch 2:") and lines[-1].startswith("OOS:") and len(lines) == (3 if name == "tdac_gaussian" else 4)


# ---- 3. the refusals
@both
def test_refusals(policy):
    L = _abi.lib()
    S = np.zeros((2, N), dtype=np.float32)
    S[0] = -0.5
    ai, af = np.zeros(N, dtype=np.int32), np.full(N, 0.5, dtype=np.float32)
    r, t, out_i, out_f = np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.float32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731

    def refused(call, code=ESTATE):
        try:
            rc = call()
        except RsrlHipError as e:
            rc = e.code
        assert rc == code and L.rsrl_hip_last_error(), (rc, L.rsrl_hip_last_error())
        assert c.checksum() == before and c.step_count == 0 and c.actions.tobytes() == acts.tobytes()      # after EACH refusal

    with plain(policy=policy, max_episode_steps=20) as c:
        h, F = c._h, c.F
        c.reset()
        before, acts = c.checksum(), c.actions
        for call in (lambda: L.rsrl_hip_get_actions(h, p(out_i)), lambda: L.rsrl_hip_set_actions(h, p(ai)),
                     lambda: L.rsrl_hip_domain_step(h, p(ai), p(S.copy()), p(S.copy()), p(r), p(t)),
                     lambda: L.rsrl_hip_handle(h, p(S), p(ai), p(r), p(S), p(t), N, p(out_f)),
                     lambda: L.rsrl_hip_policy_sample(h, p(S), N, p(out_i)), lambda: L.rsrl_hip_policy_sample(h, None, N, p(out_i)),
                     lambda: L.rsrl_hip_policy_mode(h, p(S), N, p(out_i))):
            refused(call)                                                                # the int32 calls
        for call in (lambda: c.q_find_max(S), lambda: c.q_find_min(S),
                     lambda: L.rsrl_hip_q_expected_value(h, p(S), N, p(np.zeros((3, N), dtype=np.float32)), p(out_f)),
                     lambda: c.q_evaluate_f32(S, af), lambda: c.nac_update(),
                     lambda: c.handle_batch(np.zeros((1, 2, N)), np.zeros((1, N)), np.zeros((1, N)), np.zeros(N)),
                     lambda: c.handle_transitions(np.zeros((1, 2, N)), np.zeros((1, N)), np.zeros((1, 2, N)), np.zeros((1, N)), np.zeros(N)),
                     lambda: c.rollout_trajectory(5), lambda: c.rollout_policy(rsrl_amd.RANDOM, 5),
                     lambda: c.get_traces(0), lambda: L.rsrl_hip_get_td_weights(h, 0, p(out_f)), lambda: c.get_lstd_state(0)):
            refused(call)                                                                # the ESTATE list
        for bad in (np.nan, np.inf, -np.inf):                                            # a host action that is not finite: EINVAL (under Beta a finite one is clamped)
            x = af.copy()
            x[5] = bad
            refused(lambda: L.rsrl_hip_handle_f32(h, p(S), p(x), p(r), p(S), p(t), N, p(out_f)), EINVAL)
            refused(lambda: L.rsrl_hip_set_actions_f32(h, p(x)), EINVAL)
            refused(lambda: L.rsrl_hip_domain_step_f32(h, p(x), None, None, None, None), EINVAL)
            refused(lambda: L.rsrl_hip_policy_pdf(h, p(S), p(x), N, p(out_f)), EINVAL)
        # the value side is V with one column, as RSRL_TD's
        assert c.n_weight_rows == F and c.n_out == 1 and c.n_policy_out == 2 and c.A == 0
        assert c.get_weights(0).shape == (F, 1) and not c.get_weights(0).any() and not c.get_policy_weights(0).any()
        w = np.linspace(-1.0, 1.0, F, dtype=np.float32).reshape(F, 1)
        c.set_weights(w, 3)
        X = np.random.default_rng(2).uniform([-1.2, -0.07], [0.6, 0.07], size=(N, 2)).T.astype(np.float32)
        v = c.q_evaluate(X)
        phi = c.project(X).astype(np.float64)
        assert v.shape == (1, N) and not v[0, :3].any() and abs(v[0, 3] - phi[:, 3] @ w[:, 0].astype(np.float64)) < 1e-5 and v[0, 3] != 0
        if policy == BETA:                                                               # Beta clamps a caller's finite action: 0 and 1 are taken
            x = af.copy()
            x[0], x[1] = 0.0, 1.0
            td = c.handle(S, x, r, S, t)
            assert np.isfinite(td).all() and all(np.isfinite(c.get_policy_weights(i)).all() for i in (0, 1))
    for kw in (dict(policy=rsrl_amd.RANDOM), dict(policy=rsrl_amd.SOFTMAX), dict(domain=MC), dict(order=6), dict(agent_policy=rsrl_amd.SOFTMAX)):
        with pytest.raises(RsrlHipError) as e:
            plain(**dict(dict(policy=policy), **kw))
        assert e.value.code == EINVAL and "RSRL_CONTINUOUS_TD_ACTOR_CRITIC" in str(e.value), kw
    for kw in (dict(algo=34), dict(algo=36)):
        with pytest.raises(RsrlHipError) as e:
            plain(policy=policy, **kw)
        assert e.value.code == EINVAL and "unknown algo" in str(e.value), kw


# ---- 4. reset
@both
def test_reset_samples_on_blk_init_and_leaves_the_learner_alone(policy):
    order = 3
    case = _run(order, policy)[0]
    with plain(order=order, policy=policy, seed=11) as c:
        for i, (w, W) in enumerate(case["init"]):
            c.set_weights(w.reshape(-1, 1), i)
            c.set_policy_weights(W, i)
        c.reset()
        S = c.states
        assert np.all(S[0] == np.float32(-0.5)) and np.all(S[1] == 0.0) and not c.episode_steps.any() and c.step_count == 0
        for i, (w, W) in enumerate(case["init"]):
            assert c.get_weights(i).tobytes() == w.reshape(-1, 1).tobytes() and c.get_policy_weights(i).tobytes() == W.tobytes(), i
        p0, p1 = c.policy_params(S)
        a = c.actions
        if policy == GAUSSIAN:
            # the sample is gauss_sample on BLK_INIT at the device's own parameters, one f32 fma behind them; not BLK_STEP's
            want = p0.astype(np.float64) + p1.astype(np.float64) * gn.gauss_normal(11, np.arange(N), 0, bn.BLK_INIT)
            other = p0.astype(np.float64) + p1.astype(np.float64) * gn.gauss_normal(11, np.arange(N), 0, bn.BLK_STEP)
            assert np.max(np.abs(a.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))) < 4e-6      # (tests/test_gpu_nac_gaussian.py's bound on the sample)
            assert np.max(np.abs(a.astype(np.float64) - other)) > 1e-2
        else:
            # beta_sample on BLK_INIT at the device's own parameters: the learners whose acceptance tests are not within MARGIN of their boundary
            from tests.nac_numpy import MARGIN
            want, margin = bn.beta_sample(11, np.arange(N), 0, bn.BLK_INIT, p0.astype(np.float64), p1.astype(np.float64))
            other, _ = bn.beta_sample(11, np.arange(N), 0, bn.BLK_STEP, p0.astype(np.float64), p1.astype(np.float64))
            keep = margin >= MARGIN
            assert keep.sum() >= N - 3 and np.max(np.abs(a.astype(np.float64)[keep] - want[keep])) <= 4 * 4.649e-7      # (tests/test_gpu_tdac_beta.py's bound on the sample)
            assert np.max(np.abs(a.astype(np.float64) - other)) > 1e-2 and a.min() >= bn.LO and a.max() <= bn.HI
        assert c.policy_sample().tobytes() == a.tobytes() and c.policy_sample().tobytes() == a.tobytes()


# ---- 5. the pending actions through each policy's loop convention; the rollout is each policy's mode loop
@both
def test_pending_actions_step_by_the_loops_convention_and_the_rollout_is_the_mode_loop(policy):
    rng = np.random.default_rng(31)
    S = rng.uniform([-1.2, -0.07], [0.6, 0.07], size=(N, 2)).T.astype(np.float32)
    S[:, 0], S[:, 1], S[:, 2] = (0.59, 0.06), (-1.2, -0.07), (-0.5, 0.0)
    if policy == GAUSSIAN:
        a = rng.uniform(-1.5, 1.5, size=N).astype(np.float32)
        a[0], a[1], a[2], a[3] = 1.0, -1.0, 0.0, 7.25
        to_domain = lambda x: x                                   # noqa: E731      the action itself
        not_it = lambda x: (2.0 * x - 1.0).astype(np.float32)     # noqa: E731
    else:
        a = rng.uniform(0.0, 1.0, size=N).astype(np.float32)
        a[0], a[1], a[2] = 1.0, 0.0, 0.5
        to_domain = lambda x: (2.0 * x - 1.0).astype(np.float32)  # noqa: E731      2a - 1 (exact in f32)
        not_it = lambda x: x                                      # noqa: E731
    limit = 40
    with plain(order=3, policy=policy, max_episode_steps=limit - 1) as c:
        c.states, c.actions = S, a
        assert c.actions.tobytes() == a.tobytes()
        r1 = c.domain_step()                                                             # the pending actions
        c.states = S
        r2 = c.domain_step(to_domain(a))                                                 # explicit actions: the domain's, literally
        for x, y in zip(r1, r2):
            assert x.tobytes() == y.tobytes()
        c.states = S
        assert c.domain_step(not_it(a))[1].tobytes() != r1[1].tobytes()                  # NOT the other policy's convention
        assert c.actions.tobytes() == a.tobytes()                                        # the pending actions are the agent's, unchanged
        for i in range(N):
            c.set_policy_weights((rng.normal(size=(c.F, 2)) * 0.5).astype(np.float32), i)
        for lim in (limit, 0):                                                           # (0: bounded by max_episode_steps, limit - 1 transitions)
            n_states, total = c.rollout_greedy(lim)
            c.reset()
            n_host, tot_host, live = np.ones(N, dtype=np.uint32), np.zeros(N, dtype=np.float32), np.ones(N, dtype=bool)
            for _ in range(limit - 1):
                m = c.policy_mode(c.states)
                _, _, rew, term = c.domain_step(to_domain(m))
                n_host[live] += 1
                tot_host[live] += rew[live]
                live &= term == 0
            assert np.array_equal(n_states, n_host) and total.tobytes() == tot_host.tobytes(), lim
        assert n_states.max() == limit and len(np.unique(c.policy_mode(c.states))) > N // 2


# ---- 6. device pointers
@both
def test_f32_entry_points_on_device_arrays_equal_a_twin_on_host_arrays(policy):
    F32, U8 = np.float32, np.uint8
    ptr = lambda b: C.c_void_p(b.ptr)      # noqa: E731
    rng = np.random.default_rng(15)
    kw = dict(order=3, policy=policy, n_envs=N, max_episode_steps=9, lr=0.02)
    with ctx(**kw) as h, ctx(**kw) as d:
        for c in (h, d):
            _start_near_the_goal(c, 0)
            c.train(12)
        L, D = d._L, d.D
        da = DeviceBuffer(N, F32)
        _abi.check(L.rsrl_hip_get_actions_f32(d._h, ptr(da)))
        act_h = h.actions
        frm_h, nxt_h, rew_h, term_h = h.domain_step()                                    # the pending actions
        dfrm, dnxt, drew, dterm = DeviceBuffer(D * N, F32), DeviceBuffer(D * N, F32), DeviceBuffer(N, F32), DeviceBuffer(N, U8)
        _abi.check(L.rsrl_hip_domain_step_f32(d._h, None, ptr(dfrm), ptr(dnxt), ptr(drew), ptr(dterm)))
        d.sync()
        assert np.array_equal(da.to_host(), act_h) and dfrm.to_host((D, N)).tobytes() == frm_h.tobytes() and dnxt.to_host((D, N)).tobytes() == nxt_h.tobytes()
        assert drew.to_host().tobytes() == rew_h.tobytes() and np.array_equal(dterm.to_host(), term_h)
        dtd = DeviceBuffer(N, F32)
        _abi.check(L.rsrl_hip_handle_f32(d._h, ptr(dfrm), ptr(da), ptr(drew), ptr(dnxt), ptr(dterm), N, ptr(dtd)))
        td_h = h.handle(frm_h, act_h, rew_h, nxt_h, term_h)
        d.sync()
        assert dtd.to_host().tobytes() == td_h.tobytes()
        X = rng.uniform([-1.2, -0.07], [0.6, 0.07], size=(N, 2)).T.astype(F32)
        dX, do0 = DeviceBuffer(D * N, F32), DeviceBuffer(N, F32)
        dX.from_host(X)
        _abi.check(L.rsrl_hip_policy_sample_f32(d._h, ptr(dX), N, ptr(do0)))
        d.sync()
        assert do0.to_host().tobytes() == h.policy_sample(X).tobytes()
        _abi.check(L.rsrl_hip_policy_sample_f32(d._h, None, N, ptr(do0)))
        d.sync()
        assert do0.to_host().tobytes() == h.policy_sample().tobytes() and d.actions.tobytes() == h.actions.tobytes()
        for i in range(N):
            assert d.get_weights(i).tobytes() == h.get_weights(i).tobytes(), i            # (all three columns: Ctx.get_weights)
        assert d.checksum() == h.checksum() and d.step_count == h.step_count


# ---- 7. the random campaign
def test_random_configurations():
    # tests/fuzz_tdac_cont.py: both policies, orders 1-5 at random learner counts, seeds, env offsets up to the top of the id range, caps from 0
    # (none) and 1 (every step ends an episode), launch depths and shards: the f64 leg and the self leg
    from tests.fuzz_tdac_cont import SUITE_CASES, SUITE_SEED
    d = run_slice("fuzz_tdac_cont.py", SUITE_CASES, SUITE_SEED)
    print(d["counts"], d["legs"])
    assert d["exit_code"] == 0 and not d["failures"], d["failures"][:3]
    assert SUITE_CASES == 24 and d["counts"] == {"ok": SUITE_CASES}, d["counts"]
    assert d["legs"]["f64"] == SUITE_CASES and d["legs"]["self"] == SUITE_CASES and d["legs"]["ckpt"] == SUITE_CASES // 3 and d["legs"].get("shard", 0) >= 2, d["legs"]
