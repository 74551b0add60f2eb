"""LSTD and LSTDLambda (RSRL_LSTD, RSRL_LSTD_LAMBDA; train_lstd_batch.hip) on the device: the solve bit for bit against its restatement
(tests/lstd_batch_numpy.py lu_solve) on crafted states, the accumulators against the f64 rules, train against the host trait loop / launch depths /
shards bit for bit with the f64 state and the episode record among what is compared, the environment side against RSRL_TD's, checkpoints, the
checksum, the refusals, the value side, the C++ example and a long horizon replayed in numpy."""
import os

import numpy as np
import pytest

import rsrl_amd as ra
from rsrl_amd import RsrlHipError
from rsrl_amd._devmem import DeviceBuffer
from tests.agent_contract import (assert_same, check_checkpoint_resume, check_foreign_checkpoints_refused, check_train_invariance, join_shards,
                                  lstd_batch_trait_loop, rand_states, record_bits, run_example, snapshot)
from tests.lstd_batch_numpy import handle, initial_state, lu_solve, residual, state_of

pytestmark = pytest.mark.gpu

ALGOS = [ra.LSTD, ra.LSTD_LAMBDA]
REG = [(ra.MOUNTAIN_CAR, o) for o in (1, 2, 3, 4, 5)] + [(ra.CART_POLE, 1), (ra.ACROBOT, 1)]
EPS = np.finfo(np.float64).eps
EINVAL, ESTATE = -1, -5
LAMBDA = 0.8
BASE = dict(domain=ra.MOUNTAIN_CAR, order=3, algo=ra.LSTD, policy=ra.RANDOM, n_envs=64, seed=5, gamma=0.95, max_episode_steps=7, lam=LAMBDA)


def ctx(**kw):
    return ra.Context(**dict(BASE, **kw))


def lam_of(algo):
    return LAMBDA if algo == ra.LSTD_LAMBDA else None


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def f64_state(c):
    """every learner's exact state, name -> array stacked on axis 0"""
    per = [c.get_lstd_batch_state(i) for i in range(c.N)]
    out = dict(lstd_theta=np.stack([p[0] for p in per]), lstd_A=np.stack([p[1] for p in per]), lstd_b=np.stack([p[2] for p in per]),
               singular_solves=np.array([p[4] for p in per], dtype=np.uint32))
    if per[0][3] is not None:
        out["lstd_z"] = np.stack([p[3] for p in per])
    return out


def full_snapshot(c):
    """the harness's snapshot (its weights are f32(theta)), the f64 state and the episode record -- the record as bit patterns (it shows NaN past
    each learner's rows, which the harness's comparison refuses) with the learner on axis 0, where every per-learner entry joins"""
    out = snapshot(c)
    out.update(f64_state(c))
    out.update(record_bits(c))
    return out


class Recording(ra.Context):
    """a Context that leaves its full snapshot behind when its `with` ends: the contract harness compares its own snapshot only"""
    log = []

    def __exit__(self, *exc):
        if exc[0] is None:
            Recording.log.append(full_snapshot(self))
        return super().__exit__(*exc)


def crafted(F, kind, rng):
    """(A, b) for the solve: 0 random and well conditioned; 1 a triangular matrix with its rows permuted, so that the pivots are not the rows in
    index order; 2 a first column of equal magnitudes (the first index wins); 3 two equal rows (singular)"""
    M = rng.normal(0.0, 1.0, size=(F, F))
    if kind == 1:
        A = np.triu(0.3 * M, 1) + np.diag(rng.choice([-1.0, 1.0], size=F) * rng.uniform(1.0, 2.0, size=F))
        A = A[rng.permutation(F)]
    else:
        A = np.eye(F) + 0.5 * M / np.sqrt(F)
        if kind == 2:
            A[:, 0] = 1.25 * rng.choice([-1.0, 1.0], size=F)
        if kind == 3 and F > 1:
            A[F - 1] = A[F // 2]
    return A, rng.normal(0.0, 1.0, size=F)


def set_state(c, i, theta, A, b, z, sing=0):
    c.set_lstd_batch_state(theta, A, b, z if c.cfg.algo == ra.LSTD_LAMBDA else None, sing, i)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("order", [1, 3, 5])
def test_solve_is_the_restated_elimination_bit_for_bit(order, algo):
    N = 64
    rng = np.random.default_rng(10 * order + algo)
    with ctx(order=order, algo=algo, n_envs=N) as c:
        F = c.F
        assert F == (order + 1) ** 2
        given = []
        for i in range(N):
            A, b = crafted(F, i % 4, rng)
            theta, z = rng.normal(0.0, 1.0, size=F), rng.normal(0.0, 1.0, size=F)
            set_state(c, i, theta, A, b, z)
            given.append((theta, A, b, z))
        t0 = c.step_count
        c.lstd_solve()
        assert c.step_count == t0
        singular = 0
        for i, (theta, A, b, z) in enumerate(given):
            g_theta, g_A, g_b, g_z, g_sing = c.get_lstd_batch_state(i)
            assert np.array_equal(g_A, A) and np.array_equal(g_b, b) and (g_z is None or np.array_equal(g_z, z)), i      # untouched
            want = lu_solve(A, b)
            if want is None:
                singular += 1
                assert i % 4 == 3 and np.array_equal(g_theta, theta) and g_sing == 1, (i, g_sing)
            else:
                assert g_sing == 0 and g_theta.tobytes() == np.array(want).tobytes(), (i, i % 4, np.max(np.abs(g_theta - want)))
                res = residual(A, b, g_theta)
                assert res <= F * EPS, (i, i % 4, res / EPS)
        assert singular == N // 4
        c.lstd_solve()                                             # the counter counts
        assert [c.get_lstd_batch_state(i)[4] for i in range(8)] == [0, 0, 0, 2] * 2


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("domain,order", REG)
def test_handle_transitions_against_the_f64_rule(orc, domain, order, algo):
    N, T, gamma = 64, 7, 0.95
    lam = lam_of(algo)
    rng = np.random.default_rng(domain * 100 + order * 10 + algo)
    with ctx(domain=domain, order=order, algo=algo, n_envs=N, gamma=gamma) as c:
        F, D = c.F, c.D
        S = np.stack([rand_states(orc, domain, N, rng) for _ in range(T)])
        S2 = np.stack([rand_states(orc, domain, N, rng) for _ in range(T)])
        R = rng.normal(0.0, 1.0, size=(T, N)).astype(np.float32)
        Tm = (rng.random((T, N)) < 0.3).astype(np.uint8)
        L = np.array([0, 1, 2, 7], dtype=np.uint32)[np.arange(N) % 4]
        init = []
        for i in range(N):
            init.append((rng.normal(0.0, 0.5, size=F), np.eye(F) + 0.1 * rng.normal(0.0, 1.0, size=(F, F)) / np.sqrt(F), rng.normal(0.0, 1.0, size=F),
                         rng.normal(0.0, 1.0, size=F)))

        def install():
            for i, (theta, A, b, z) in enumerate(init):
                set_state(c, i, theta, A, b, z)

        # ---- host arrays (actions given: not read)
        install()
        t0 = c.step_count
        td = c.handle_transitions(S, R, S2, Tm, L, td=True, actions=rng.integers(0, c.A, size=(T, N)).astype(np.int32))
        assert c.step_count == t0 + 1
        got = f64_state(c)
        # tolerance (tests/test_gpu_lstd.py's): every quantity is a sum of rounded products per step and the device's features differ from the
        # oracle's by a few ulps: 16 F eps per step relative to the state's magnitude
        tol = 16.0 * F * T * EPS
        for i in range(N):
            n = int(L[i])
            theta, A, b, z = init[i]
            if n == 0:                                             # no call: every byte stays, no solve
                assert np.array_equal(got["lstd_theta"][i], theta) and np.array_equal(got["lstd_A"][i], A) and np.array_equal(got["lstd_b"][i], b)
                assert (lam is None or np.array_equal(got["lstd_z"][i], z)) and got["singular_solves"][i] == 0 and np.isnan(td[:, i]).all()
                continue
            st = state_of(theta, A, b, z if lam is not None else None)
            batch = [(orc.fourier_project(domain, order, S[k, :, i]), orc.fourier_project(domain, order, S2[k, :, i]), float(R[k, i]), bool(Tm[k, i]))
                     for k in range(n)]
            want_td = handle(st, batch, gamma, lam)
            for name, key in (("lstd_A", "A"), ("lstd_b", "b")) + ((("lstd_z", "z"),) if lam is not None else ()):
                w = np.array(st[key])
                err = np.max(np.abs(got[name][i] - w))
                assert err <= tol * (1.0 + np.max(np.abs(w))), (i, name, err, tol * (1.0 + np.max(np.abs(w))))
            # theta: the solve of the device's own A and b, bit for bit
            x = lu_solve(got["lstd_A"][i], got["lstd_b"][i])
            assert x is not None and got["singular_solves"][i] == 0
            assert got["lstd_theta"][i].tobytes() == np.array(x).tobytes(), i
            for k in range(n):
                assert abs(float(td[k, i]) - want_td[k]) <= 2.0 ** -22 * (1.0 + abs(want_td[k])), (i, k, td[k, i], want_td[k])
            assert np.isnan(td[n:, i]).all()
        with pytest.raises(RsrlHipError) as e:                     # a host length above T is refused, nothing moves
            c.handle_transitions(S, R, S2, Tm, np.where(L == 7, 10, L).astype(np.uint32))
        assert e.value.code == EINVAL
        assert_same(f64_state(c), got, "after a refused call")

        # ---- device arrays, no actions, a length of 10 where the host's said 7: clamped to T.  The same bits as the host arrays gave
        install()
        bufs = [DeviceBuffer(T * D * N, np.float32), DeviceBuffer(T * N, np.float32), DeviceBuffer(T * D * N, np.float32), DeviceBuffer(T * N, np.uint8),
                DeviceBuffer(N, np.uint32), DeviceBuffer(T * N, np.float32)]
        for buf, arr in zip(bufs, (S, R, S2, Tm, np.where(L == 7, 10, L).astype(np.uint32))):
            buf.from_host(arr)
        c.handle_transitions(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, td=bufs[5].ptr, T=T)
        c.sync()
        assert np.array_equal(bits(bufs[5].to_host((T, N))), bits(td)), "td_out (device arrays)"
        assert_same(f64_state(c), got, "device arrays against host arrays")
        # the ctx's own open record and episode steps are not touched
        assert not c.episode_steps.any() and np.isnan(c.episode_record[1]).all()
        for buf in bufs:
            buf.free()


# every end a truncation, in a partly filled last block (16 learners per block: 4.5 blocks); ragged terminal and truncated ends among the groups
# of one wave; one learner per wave (F = 36), a partly filled block again
CASES = {"mountain-car-truncations": (dict(domain=ra.MOUNTAIN_CAR, order=3, max_episode_steps=7, n_envs=72), 50, 10),
         "cart-pole-ragged": (dict(domain=ra.CART_POLE, order=1, max_episode_steps=40, n_envs=64), 120, 33),
         "order-5-a-learner-per-wave": (dict(domain=ra.MOUNTAIN_CAR, order=5, max_episode_steps=11, n_envs=6), 40, 7)}


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("case", list(CASES))
def test_train_is_the_trait_loop_launch_depth_and_shard_invariant(case, algo):
    kw, K, first_split = CASES[case]
    cap = kw["max_episode_steps"]
    Recording.log = []
    st, ref = check_train_invariance(lambda **k: Recording(**dict(BASE, **k)), dict(kw, algo=algo), K, cap, depths=(1, 16), first_split=first_split,
                                     kernel="k_train_lstd_batch", trait=lstd_batch_trait_loop)
    print("statistics", st)
    assert st["env_steps"] == kw["n_envs"] * K and st["episodes"] > 0 and st["sum_abs_td_error"] > 0
    if case == "cart-pole-ragged":
        es = ref["episode_steps"].reshape(-1, 4)                 # (F = 16: four learners per wave)
        assert st["episodes"] - st["episodes_truncated"] > 0 and (es != es[:, :1]).any()      # ragged inside one wave
    elif case == "mountain-car-truncations":
        assert st["episodes"] == st["episodes_truncated"] and (ref["episode_steps"] == K % cap).all()
    # the same four-way comparison with the f64 state and the record in it
    train, trait, d1, d16, s0, s1 = Recording.log
    assert np.isfinite(train["lstd_theta"]).all() and np.abs(train["lstd_theta"]).max() > 0 and not train["singular_solves"].any()
    assert np.array_equal(train["weights"][:, :, 0], train["lstd_theta"].astype(np.float32))
    assert_same(trait, train, "the trait loop against train")
    assert_same(d1, train, "the split train at steps_per_launch 1")
    assert_same(d16, train, "the split train at steps_per_launch 16")
    assert_same(join_shards(s0, s1), train, "two shards joined")


@pytest.mark.parametrize("case,K", [("mountain-car-truncations", 50), ("cart-pole-ragged", 120)])
def test_environment_side_is_tds(case, K):
    kw = CASES[case][0]
    with ctx(algo=ra.LSTD_LAMBDA, **kw) as c, ctx(algo=ra.TD, lr=0.01, **kw) as t:
        c.reset()
        t.reset()
        sc, stt = c.train(K), t.train(K)
        for name in ("states", "actions", "episode_steps"):
            assert np.array_equal(getattr(c, name).view(np.uint32), getattr(t, name).view(np.uint32)), name
        for name in ("env_steps", "episodes", "episodes_truncated", "sum_episode_steps"):
            assert sc[name] == stt[name], (name, sc[name], stt[name])
        assert sc["episodes"] > 0 and sc["sum_reward"] == stt["sum_reward"]


@pytest.mark.parametrize("algo", ALGOS)
def test_checkpoint_resumes_bitwise_and_the_checksum_covers_the_f64_state(tmp_path, algo):
    N, F, cap = 32, 16, 7
    kw = dict(n_envs=N, order=3, algo=algo, max_episode_steps=cap)
    path = os.path.join(str(tmp_path), "lstd_batch.ckpt")

    def one_ulp_moves_the_checksum(a, b):
        for part in (1, 3) if algo == ra.LSTD_LAMBDA else (1,):      # A, z
            before = b.checksum()
            st = list(b.get_lstd_batch_state(5))
            flat = st[part].reshape(-1)
            flat[3] = np.nextafter(flat[3], np.inf)
            b.set_lstd_batch_state(*st, env_index=5)
            assert b.checksum()[0] != before[0] and b.checksum()[1] == before[1], part

    # the harness's part: saved where every record is empty (3 * cap steps: every end is a truncation), so that nothing but its own carry is needed
    check_checkpoint_resume(ctx, kw, path, 3 * cap, 20, carry=("states", "actions", "episode_steps"), then=one_ulp_moves_the_checksum)
    with open(path, "rb") as f:
        head = f.read(72)
    assert int.from_bytes(head[8:12], "little") == 10 and int.from_bytes(head[44:48], "little") == algo and int.from_bytes(head[52:56], "little") == 10
    assert os.path.getsize(path) == 72 + N * 8 * (F + F * F + F + (F if algo == ra.LSTD_LAMBDA else 0)) + N * 4
    # ... and with open episodes: the caller carries the record next to the states, actions and episode steps
    with ctx(**kw) as a, ctx(**kw) as b:
        a.reset()
        a.train(10)
        a.save_weights(path)
        b.load_weights(path)
        b.states, b.actions, b.episode_steps, b.episode_record = a.states, a.actions, a.episode_steps, a.episode_record
        assert (a.episode_steps == 3).all() and b.step_count == a.step_count == 10
        for when, k in (("after the load", 0), ("20 steps after the load", 20)):
            if k:
                a.train(k)
                b.train(k)
            assert_same(full_snapshot(b), full_snapshot(a), when)
            assert a.checksum() == b.checksum(), when
        assert np.abs(f64_state(a)["lstd_theta"]).max() > 0
    other = ra.LSTD if algo == ra.LSTD_LAMBDA else ra.LSTD_LAMBDA
    others = [dict(algo=other), dict(algo=ra.RECURSIVE_LSTD), dict(algo=ra.TD, lr=0.01), dict(algo=ra.GRADIENT_MC, lr=0.01)]
    check_foreign_checkpoints_refused(ctx, kw, path, [dict(BASE, **dict(kw, **o)) for o in others], tmp_path)


@pytest.mark.parametrize("algo", ALGOS)
def test_initial_state_value_side_and_refusals(orc, algo):
    N, domain, order, cap = 16, ra.MOUNTAIN_CAR, 3, 7
    rng = np.random.default_rng(3)
    with ctx(n_envs=N, algo=algo, order=order, max_episode_steps=cap) as c:
        F = c.F
        assert c.n_out == 1
        for i in (0, N - 1):
            th, A, b, z, sing = c.get_lstd_batch_state(i)
            assert not th.any() and np.array_equal(A, 1e-6 * np.eye(F)) and not b.any() and sing == 0
            assert (z is None) == (algo == ra.LSTD) and (z is None or not z.any())
        c.reset()
        c.train(30)
        before = f64_state(c)
        c.reset()                                                 # reset restarts the episodes only
        assert_same(f64_state(c), before, "the agent's state across a reset")
        assert np.isnan(c.episode_record[1]).all() and not c.episode_steps.any()
        # get_weights = f32(theta); q_evaluate = f32(phi . theta) evaluated in f64; set_weights widens exactly and leaves the rest alone
        S = rand_states(orc, domain, N, rng)
        for i in range(N):
            st = list(c.get_lstd_batch_state(i))
            st[0] = st[0] + rng.normal(0.0, 1.0, size=F) * (i + 1)
            c.set_lstd_batch_state(*st, env_index=i)
            assert np.array_equal(c.get_weights(i)[:, 0], st[0].astype(np.float32))
        q = c.q_evaluate(S)
        assert q.shape == (1, N)
        for i in range(N):
            v = np.float32(orc.fourier_project(domain, order, S[:, i]) @ c.get_lstd_batch_state(i)[0])
            assert abs(q[0, i] - v) <= abs(np.spacing(v)), (i, q[0, i], v)
        s0 = c.get_lstd_batch_state(2)
        w = rng.normal(0.0, 1.0, size=(F, 1)).astype(np.float32)
        c.set_weights(w, 2)
        s1 = c.get_lstd_batch_state(2)
        assert np.array_equal(s1[0], w[:, 0].astype(np.float64)) and np.array_equal(s1[1], s0[1]) and np.array_equal(s1[2], s0[2]) and s1[4] == s0[4]
        zN, zTN = np.zeros(N, np.float32), np.zeros((1, N), np.float32)
        calls = [lambda: c.handle(S, np.zeros(N, np.int32), zN, S, np.zeros(N, np.uint8)),
                 lambda: c.handle_batch(S[None], np.zeros((1, N), np.int32), zTN, np.ones(N, np.uint32)),
                 lambda: c.get_lstd_state(0), lambda: c.set_lstd_state(np.zeros(F), np.eye(F), None, 0),
                 lambda: c.q_find_max(S), lambda: c.q_find_min(S), lambda: c.q_expected_value(S, np.full((c.A, N), 1.0 / c.A, dtype=np.float32)),
                 lambda: c.get_traces(0), lambda: c.set_traces(np.zeros((F, 1)), 0), lambda: c.get_td_weights(0),
                 lambda: c.set_td_weights(np.zeros((F, c.A)), 0), lambda: c.get_policy_weights(0), lambda: c.set_policy_weights(np.zeros((F, c.A)), 0),
                 lambda: getattr(c, "return_carry"), lambda: setattr(c, "return_carry", np.zeros(N))]
        for k, call in enumerate(calls):
            with pytest.raises(RsrlHipError) as e:
                call()
            assert e.value.code == ESTATE, k
            if k < 2:
                assert "handle_transitions" in str(e.value)
        # set_episode_steps above the cap: EINVAL, nothing changes; the cap itself is a full record
        steps = c.episode_steps
        steps[N - 1] = cap + 1
        with pytest.raises(RsrlHipError) as e:
            c.episode_steps = steps
        assert e.value.code == EINVAL and not c.episode_steps.any()
        steps[N - 1] = cap
        c.episode_steps = steps
        assert c.episode_steps[N - 1] == cap
    for other in (dict(algo=ra.TD, lr=0.01), dict(algo=ra.RECURSIVE_LSTD), dict(algo=ra.GRADIENT_MC, lr=0.01)):      # the new entry points are these agents' only
        with ctx(n_envs=4, **other) as t:
            z = np.zeros((1, t.D, 4), np.float32)
            for call in (lambda: t.handle_transitions(z, np.zeros((1, 4)), z, np.zeros((1, 4), np.uint8), np.ones(4, np.uint32)), lambda: t.lstd_solve(),
                         lambda: t.get_lstd_batch_state(0), lambda: t.set_lstd_batch_state(np.zeros(t.F), np.eye(t.F), np.zeros(t.F))):
                with pytest.raises(RsrlHipError) as e:
                    call()
                assert e.value.code == ESTATE, other


def test_lstd_lambda_example_builds_and_runs(tmp_path):
    for mode in ("lambda", "lstd"):
        out = run_example(tmp_path, "lstd_lambda", [64, 2, 300, 3, 50, mode])
        assert "Batch 2:" in out and "(16 features)" in out and "20-transition batch handled" in out and "0 abandoned solves" in out
        tmax = float(out.split("max |theta| of learner 0:")[1].split()[0])
        moved = float(out.split("moved by")[1].split()[0].rstrip(","))
        assert np.isfinite(tmax) and tmax > 0.0 and moved > 0.0


@pytest.mark.parametrize("algo", ALGOS)
def test_long_horizon_replayed_in_numpy(orc, algo):
    """300 batch-steps of the driver loop at 256 MountainCar order-3 learners, cap 50; four learners replayed in numpy on the transitions an
    RSRL_RECURSIVE_LSTD ctx's trait loop records (the same environment side, draw for draw; its policy_sample is the driver loop's).  A, b and z within 16 F K eps (1 + max |x|) -- test_gpu_lstd.py's
    per-step bound over the K steps; theta by the residual of the device's own A and b"""
    N, K, cap, domain, order, gamma = 256, 300, 50, ra.MOUNTAIN_CAR, 3, 0.99
    lam = lam_of(algo)
    rng = np.random.default_rng(11)
    pick = np.sort(rng.choice(N, size=4, replace=False))
    kw = dict(domain=domain, order=order, n_envs=N, seed=9, gamma=gamma, max_episode_steps=cap)
    with ctx(algo=algo, **kw) as c, ctx(algo=ra.RECURSIVE_LSTD, **kw) as t:
        F = c.F
        c.reset()
        c.train(K)
        t.reset()
        ep = np.zeros(N, dtype=np.int64)
        rec = []
        for _ in range(K):
            frm, nxt, rew, term = t.domain_step(t.actions)
            t.handle(frm, t.actions, rew, nxt, term)
            ep += 1
            ended = term.astype(bool) | (ep >= cap)
            rec.append((frm[:, pick].copy(), nxt[:, pick].copy(), rew[pick].copy(), term[pick].copy(), ended[pick].copy()))
            t.domain_reset(ended.astype(np.uint8))
            ep[ended] = 0
            t.policy_sample()
        assert np.array_equal(t.states.view(np.uint32), c.states.view(np.uint32)) and np.array_equal(ep, c.episode_steps)
        tol = 16.0 * F * K * EPS
        for k, i in enumerate(pick):
            st, batch, handled = initial_state(F, lam), [], 0
            for frm, nxt, rew, term, ended in rec:
                batch.append((orc.fourier_project(domain, order, frm[:, k]), orc.fourier_project(domain, order, nxt[:, k]), float(rew[k]), bool(term[k])))
                if ended[k]:
                    handle(st, batch, gamma, lam)
                    batch, handled = [], handled + 1
            g_theta, g_A, g_b, g_z, g_sing = c.get_lstd_batch_state(int(i))
            assert handled >= K // cap and g_sing == 0 and st["singular"] == 0
            for g, w in ((g_A, np.array(st["A"])), (g_b, np.array(st["b"]))) + (((g_z, np.array(st["z"])),) if lam is not None else ()):
                assert np.max(np.abs(g - w)) <= tol * (1.0 + np.max(np.abs(w))), (i, np.max(np.abs(g - w)), tol * (1.0 + np.max(np.abs(w))))
            res = residual(g_A, g_b, g_theta)
            assert np.abs(g_theta).max() > 0 and res <= F * EPS, (i, res / EPS)
        assert not f64_state(c)["singular_solves"].any()
