"""CACLA over the Gaussian policy with a TD(0) critic (RSRL_CACLA, train_cont.hip) on the device, against tests/cacla_numpy.py: the TD half bit
for bit an RSRL_TD ctx's on RSRL_MOUNTAIN_CAR, the gate of every learner the restatement's, closed-gate learners' columns byte for byte their
inputs (one of them with a c_s that overflows f32), open-gate columns against the f64 restatement, the agent contract through
tests/agent_contract.py (train against the host trait loop / launch depths / shards, the checkpoint, foreign files, the C++ example), the
refusals, reset, the mode rollout, device-pointer calls against a twin ctx, and a slice of the random campaign (tests/fuzz_cacla.py).

The f32 chain of the open gate (ln, exp, the division by Sigma^2) has no derivable bound: the bounds of MEASURED below are four times the
maxima profiles/cacla_rate.md records (scripts/cacla_rate.py, on these very inputs; the factor covers inputs the measurement did not see);
the test prints its figure before it asserts.  N = 67: one full wave and a partial one; orders 1, 2, 3, 5 give F = 4 / 9 / 16 / 36, the unpacked
(9) and the packed register path."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import rsrl_amd
from rsrl_amd import RsrlHipError, _abi
from rsrl_amd._devmem import DeviceBuffer
from tests import beta_numpy as bn
from tests import cacla_numpy as cn
from tests import gaussian_numpy as gn
from tests.agent_contract import check_checkpoint_resume, check_foreign_checkpoints_refused, check_train_invariance, run_example
from tests.campaign import run_slice

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CMC, MC, CACLA, NAC, GAUSSIAN, BETA = rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, rsrl_amd.MOUNTAIN_CAR, 33, rsrl_amd.NAC, rsrl_amd.GAUSSIAN, rsrl_amd.BETA
ORDERS = [1, 2, 3, 5]        # F = 4, 9, 16, 36
N = 67                       # one full wave and a partial one
ESTATE, EINVAL = -5, -1

# four times the measured maxima (profiles/cacla_rate.md): max |d column| / max(1, |column|) over the open-gate learners after three rounds
MEASURED = {("cols", 1): 4 * 7.268e-8, ("cols", 2): 4 * 6.826e-8, ("cols", 3): 4 * 1.021e-7, ("cols", 5): 4 * 9.590e-8}

BASE = dict(domain=CMC, order=3, algo=CACLA, policy=GAUSSIAN, n_envs=N, seed=5, gamma=0.95, lr=0.01, alpha=0.01)


class Ctx(rsrl_amd.Context):
    """tests/agent_contract.snapshot compares an agent's `weights`; it does not know CACLA's policy columns.  Here get_weights shows all three
    columns of a learner, (F, 3): w, w_m, w_s -- so the harness holds the policy to the same bits as the V learner"""

    def get_weights(self, env_index=0):
        return np.concatenate([super().get_weights(env_index), self.get_policy_weights(env_index)], axis=1)


def ctx(**kw):
    return Ctx(**dict(BASE, **kw))


def plain(**kw):
    return rsrl_amd.Context(**dict(BASE, **kw))


# ---- 1. the rule: one pass over handle_case's inputs per order, shared and left unchanged
@functools.lru_cache(maxsize=None)
def _run(order):
    with plain(order=order) as probe:
        case = cn.handle_case(order, probe.project)
    p = case["params"]
    with plain(order=order, gamma=p["gamma"], lr=p["lr"], alpha=p["alpha"]) as c, \
            rsrl_amd.Context(domain=MC, order=order, algo=rsrl_amd.TD, policy=rsrl_amd.RANDOM, n_envs=N, seed=9, gamma=p["gamma"], lr=p["lr"]) as t:
        fig, arr = cn.figures(c, t, case)
        arr["steps"] = c.step_count
    print("measured (cols, %d): %.4g" % (order, fig["cols"]))
    return case, fig, arr


@pytest.mark.parametrize("order", ORDERS)
def test_td_half_is_rsrl_tds_bit_for_bit(order):
    case, _, arr = _run(order)
    assert arr["steps"] == len(case["rounds"]) == 3
    w0 = np.stack([w for w, _ in case["init"]])
    for k in range(3):
        assert arr["td"][k].shape == (N,) and arr["td"][k].tobytes() == arr["td_ref"][k].tobytes(), k
        assert arr["ws"][k].shape == (N, case["F"], 1) and arr["ws"][k].tobytes() == arr["ws_ref"][k].tobytes(), k
    assert np.max(np.abs(arr["ws"][2][:, :, 0] - w0)) > 1e-4 and np.isfinite(arr["ws"][2]).all()          # the V learner moved
    # ... and against the f64 restatement, loosely: the identity above is the test, this guards the reference ctx itself
    assert np.max(np.abs(arr["ws"][2][:, :, 0] - arr["want_w"])) < 1e-5


@pytest.mark.parametrize("order", ORDERS)
def test_gate_and_closed_columns(order):
    case, _, arr = _run(order)
    before = np.stack([W for _, W in case["init"]])
    for k in range(3):
        assert np.all(np.abs(arr["margins"][k]) >= cn.MARGIN)                                            # no learner is left out
        moved = np.array([arr["cols"][k][i].tobytes() != before[i].tobytes() for i in range(N)])
        assert np.array_equal(moved, arr["gates"][k]), (k, np.nonzero(moved != arr["gates"][k])[0])      # every learner's gate is the restatement's
        assert arr["gates"][k].sum() >= N / 4 and (~arr["gates"][k]).sum() >= N / 4
        before = arr["cols"][k]
    i = cn.OVERFLOW_LEARNER
    assert not any(g[i] for g in arr["gates"]) and arr["cols"][2][i].tobytes() == case["init"][i][1].tobytes()
    assert np.isfinite(arr["cols"][2]).all()


@pytest.mark.parametrize("order", ORDERS)
def test_open_gate_columns_against_the_f64_restatement(order):
    case, fig, arr = _run(order)
    init = np.stack([W for _, W in case["init"]]).astype(np.float64)
    assert arr["opened"].sum() > N / 2 and np.max(np.abs(arr["want_cols"][arr["opened"]] - init[arr["opened"]])) > 1e-3
    print("measured (cols, %d): %.4g (bound %.4g)" % (order, fig["cols"], MEASURED[("cols", order)]))
    assert fig["cols"] <= MEASURED[("cols", order)], (order, fig["cols"], MEASURED[("cols", order)])


# ---- 2. the agent contract
CAP, K = 7, 40


def _start_near_the_goal(c, off):
    """reset, then every fourth learner (by global id) at x = 0.59, v = 0.06: terminal ends occur as well as cut ones.  From w = 0 and rewards of
    -1 no gate opens within these K steps (V first sinks below every target), so every second learner starts with V = -40 everywhere (the constant feature is the last
    one): there r + gamma V(s') = -39.8 > V(s), and the gate stays open until V has risen past -1 / (1 - gamma)"""
    c.reset()
    s = c.states
    s[:, (np.arange(c.N) + off) % 4 == 0] = np.array([[0.59], [0.06]], dtype=np.float32)
    c.states = s
    w = np.zeros((c.F, 1), dtype=np.float32)
    w[c.F - 1] = -40.0
    for i in range(c.N):
        if (i + off) % 2 == 0:
            c.set_weights(w, i)


@pytest.mark.parametrize("order", ORDERS)
def test_train_is_the_trait_loop_launch_depth_and_shard_invariant(order):
    """(66 learners: the harness joins two shards of N / 2.)"""
    n = 66
    kw = dict(order=order, n_envs=n, max_episode_steps=CAP, lr=0.02, alpha=0.01, gamma=0.97)
    st, ref = check_train_invariance(ctx, kw, K, CAP, depths=(1, 3, 0), first_split=13, kernel="k_train_cacla", setup=_start_near_the_goal)
    F = (order + 1) ** 2
    assert st["env_steps"] == n * K and st["episodes"] > st["episodes_truncated"] > 0 and st["sum_abs_td_error"] > 0
    assert st["sum_episode_steps"] >= CAP * st["episodes_truncated"] + (st["episodes"] - st["episodes_truncated"])
    w = ref["weights"]
    assert w.shape == (n, F, 3) and np.isfinite(w).all()
    assert np.abs(w[:, :, 0]).max() > 0 and np.abs(w[:, :, 1]).max() > 0 and np.abs(w[:, :, 2]).max() > 0          # all three columns moved
    assert np.abs(w[0::2, :, 1:]).max(axis=(1, 2)).min() > 0                                                        # ... of every learner that began at V = -40
    assert ref["actions"].dtype == np.float32 and np.isfinite(ref["actions"]).all()


def test_checkpoint_resumes_bitwise_and_foreign_files_are_refused(tmp_path):
    kw = dict(n_envs=32, order=3, max_episode_steps=17, lr=0.02)
    path = os.path.join(str(tmp_path), "cacla.ckpt")
    check_checkpoint_resume(ctx, kw, path, 25, 20, carry=("states", "actions", "episode_steps"))
    with open(path, "rb") as f:
        head = f.read(72)
    F = 16
    assert int.from_bytes(head[8:12], "little") == 10 and int.from_bytes(head[12:16], "little") == CMC
    assert int.from_bytes(head[44:48], "little") == CACLA and int.from_bytes(head[52:56], "little") == 15
    assert os.path.getsize(path) == 72 + 32 * 4 * F + 32 * 4 * F * 2
    nac_gauss = dict(domain=CMC, order=3, algo=NAC, policy=GAUSSIAN, n_envs=32, n_steps=5, lr=0.02)
    nac_beta = dict(domain=CMC, order=3, algo=NAC, policy=BETA, n_envs=32, n_steps=5, lr=0.02)
    tdac_beta = dict(domain=CMC, order=3, algo=rsrl_amd.ILSTD_ACTOR_CRITIC, policy=BETA, n_envs=32, n_steps=2, lr=0.02, alpha=0.2)
    td = dict(domain=MC, order=3, algo=rsrl_amd.TD, policy=rsrl_amd.RANDOM, n_envs=32, lr=0.02)
    check_foreign_checkpoints_refused(ctx, kw, path, [nac_gauss, nac_beta, tdac_beta, td], tmp_path)


def test_example_builds_and_runs(tmp_path):
    out = run_example(tmp_path, "cacla", [8, 2, 300])
    lines = out.strip().splitlines()
    assert len(lines) == 3 and lines[0].startswith("Batch 1:") and lines[1].startswith("Batch 2:") and lines[2].startswith("OOS:")


# ---- 3. the refusals
def test_refusals():
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

    with plain(max_episode_steps=20) as c:
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
        for bad in (np.nan, np.inf, -np.inf):
            x = af.copy()
            x[5] = bad
            refused(lambda: L.rsrl_hip_handle_f32(h, p(S), p(x), p(r), p(S), p(t), N, p(out_f)), EINVAL)
            refused(lambda: L.rsrl_hip_set_actions_f32(h, p(x)), EINVAL)
            refused(lambda: L.rsrl_hip_domain_step_f32(h, p(x), None, None, None, None), EINVAL)
            refused(lambda: L.rsrl_hip_policy_pdf(h, p(S), p(x), N, p(out_f)), EINVAL)
        assert c.checksum() == before and c.step_count == 0 and c.actions.tobytes() == acts.tobytes()
        # the value side is V with one column, as RSRL_TD's
        assert c.n_weight_rows == F and c.n_out == 1 and c.n_policy_out == 2 and c.A == 0
        assert c.get_weights(0).shape == (F, 1) and not c.get_weights(0).any() and not c.get_policy_weights(0).any()
        w = np.linspace(-1.0, 1.0, F, dtype=np.float32).reshape(F, 1)
        c.set_weights(w, 3)
        X = np.random.default_rng(2).uniform([-1.2, -0.07], [0.6, 0.07], size=(N, 2)).T.astype(np.float32)
        v = c.q_evaluate(X)
        phi = c.project(X).astype(np.float64)
        assert v.shape == (1, N) and not v[0, :3].any() and abs(v[0, 3] - phi[:, 3] @ w[:, 0].astype(np.float64)) < 1e-5 and v[0, 3] != 0
    for kw in (dict(policy=BETA), dict(policy=rsrl_amd.RANDOM), dict(domain=MC), dict(order=6), dict(agent_policy=rsrl_amd.SOFTMAX)):
        with pytest.raises(RsrlHipError) as e:
            plain(**kw)
        assert e.value.code == EINVAL and "RSRL_CACLA" in str(e.value), kw
    for kw in (dict(algo=32), dict(algo=34)):
        with pytest.raises(RsrlHipError) as e:
            plain(**kw)
        assert e.value.code == EINVAL and "unknown algo" in str(e.value), kw


# ---- 4. reset
def test_reset_samples_on_blk_init_and_leaves_the_learner_alone():
    order = 3
    case = _run(order)[0]
    with plain(order=order, seed=11) as c:
        for i, (w, W) in enumerate(case["init"]):
            if i != cn.OVERFLOW_LEARNER:
                c.set_weights(w.reshape(-1, 1), i)
                c.set_policy_weights(W, i)
        c.reset()
        S = c.states
        assert np.all(S[0] == np.float32(-0.5)) and np.all(S[1] == 0.0) and not c.episode_steps.any() and c.step_count == 0
        for i, (w, W) in enumerate(case["init"]):
            if i != cn.OVERFLOW_LEARNER:
                assert c.get_weights(i).tobytes() == w.reshape(-1, 1).tobytes() and c.get_policy_weights(i).tobytes() == W.tobytes(), i
        dmu, dsd = c.policy_params(S)
        a = c.actions
        # the sample is gauss_sample on BLK_INIT at the device's own parameters, one f32 fma behind them; not BLK_STEP's
        z = gn.gauss_normal(11, np.arange(N), 0, bn.BLK_INIT)
        want = dmu.astype(np.float64) + dsd.astype(np.float64) * z
        assert np.max(np.abs(a.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))) < 4e-6      # (tests/test_gpu_nac_gaussian.py's bound on the sample)
        other = dmu.astype(np.float64) + dsd.astype(np.float64) * gn.gauss_normal(11, np.arange(N), 0, bn.BLK_STEP)
        assert np.max(np.abs(a.astype(np.float64) - other)) > 1e-2
        assert c.policy_sample().tobytes() == a.tobytes() and c.policy_sample().tobytes() == a.tobytes()


# ---- 5. the loop hands the domain the action itself; the rollout is the mode loop
def test_pending_actions_step_literally_and_the_rollout_is_the_mode_loop():
    rng = np.random.default_rng(31)
    S = rng.uniform([-1.2, -0.07], [0.6, 0.07], size=(N, 2)).T.astype(np.float32)
    S[:, 0], S[:, 1], S[:, 2] = (0.59, 0.06), (-1.2, -0.07), (-0.5, 0.0)
    a = rng.uniform(-1.5, 1.5, size=N).astype(np.float32)
    a[0], a[1], a[2], a[3] = 1.0, -1.0, 0.0, 7.25
    limit = 40
    with plain(order=3, max_episode_steps=limit - 1) as c:
        c.states, c.actions = S, a
        assert c.actions.tobytes() == a.tobytes()                                        # any finite f32, as it is: no clamp
        r1 = c.domain_step()
        c.states = S
        r2 = c.domain_step(a)
        c.states = S
        r3 = c.domain_step(np.clip(a, -1.0, 1.0))                                        # the domain clips (map_onto)
        for x, y, z in zip(r1, r2, r3):
            assert x.tobytes() == y.tobytes() == z.tobytes()
        c.states = S
        assert c.domain_step((2.0 * a - 1.0).astype(np.float32))[1].tobytes() != r1[1].tobytes()      # NOT the Beta loop's mapping
        for i in range(N):
            c.set_policy_weights((rng.normal(size=(c.F, 2)) * 0.5).astype(np.float32), i)
        for lim in (limit, 0):                                                           # (0: bounded by max_episode_steps, limit - 1 transitions)
            n_states, total = c.rollout_greedy(lim)
            c.reset()
            n_host, tot_host, live = np.ones(N, dtype=np.uint32), np.zeros(N, dtype=np.float32), np.ones(N, dtype=bool)
            for _ in range(limit - 1):
                m = c.policy_mode(c.states)
                _, _, rew, term = c.domain_step(m)
                n_host[live] += 1
                tot_host[live] += rew[live]
                live &= term == 0
            assert np.array_equal(n_states, n_host) and total.tobytes() == tot_host.tobytes(), lim
        assert n_states.max() == limit and len(np.unique(c.policy_mode(c.states))) > N // 2


# ---- 6. device pointers
def test_f32_entry_points_on_device_arrays_equal_a_twin_on_host_arrays():
    F32, U8 = np.float32, np.uint8
    ptr = lambda b: C.c_void_p(b.ptr)      # noqa: E731
    rng = np.random.default_rng(15)
    kw = dict(order=3, n_envs=N, max_episode_steps=9, lr=0.02)
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
    # tests/fuzz_cacla.py: orders 1-5 at random learner counts, seeds, env offsets up to the top of the id range, caps from 0 (none) and 1 (every
    # step ends an episode), launch depths and shards: train against the host trait loop bit for bit, a checkpoint leg and a handle leg
    from tests.fuzz_cacla import SUITE_CASES, SUITE_SEED
    d = run_slice("fuzz_cacla.py", SUITE_CASES, SUITE_SEED)
    print(d["counts"], d["legs"])
    assert d["exit_code"] == 0 and not d["failures"], d["failures"][:3]
    assert SUITE_CASES == 150 and d["counts"] == {"ok": SUITE_CASES}, d["counts"]
    assert d["legs"]["handle"] == SUITE_CASES and d["legs"]["trait"] == SUITE_CASES and d["legs"]["ckpt"] == SUITE_CASES // 3 and d["legs"].get("shard", 0) >= 10, d["legs"]
