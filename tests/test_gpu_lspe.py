"""LambdaLSPE (RSRL_LAMBDA_LSPE; train_lspe.hip) on the device: solve() bit for bit against its restatement (tests/lspe_numpy.py over
tests/lstd_batch_numpy.py lu_solve) on crafted states with full and short row counts, the walk against the f64 rule on the oracle's features,
train against the host trait loop / launch depths / shards bit for bit with the f64 state and the record among what is compared, a long horizon
replayed in numpy to the bits of every quantity, the checkpoint, the checksum, the initial state and the refusals.

THE DEVICE'S OWN FEATURES.  rsrl_hip_project writes the f32 basis; the agent's features are f64 (lstd_feature), so no f32 array can carry their bits.
device_features() reads them through the agent itself: on theta = A = b = delta = rows = 0 one non-terminal transition (s, s) with reward 1 gives
residual 1, delta 1 and b = 0 + (0 + 1) * phi(s) -- b IS phi(s), one row of F >= 4 is deferred, and get_lstd_batch_state returns it.  With those
features the restatement is held to the device's BITS.  (At F = 4 a 7-row batch fills the row count from any installed value, so its A and b
before the solve cannot be read back by deferring it; the walk test holds that learner's theta to the bits of the restatement on the device's
features instead, which performs the relaxed elimination on bit-identical A and b.)"""
import os

import numpy as np
import pytest

import rsrl_amd as ra
from rsrl_amd import RsrlHipError
from rsrl_amd._devmem import DeviceBuffer
from tests.agent_contract import (assert_same, check_checkpoint_resume, check_foreign_checkpoints_refused, check_train_invariance, join_shards,
                                  lstd_batch_trait_loop, rand_states, record_bits, run_example, snapshot)
from tests.lspe_numpy import accumulate, handle, initial_state, state_of
from tests.lstd_batch_numpy import lu_solve
from tests.test_gpu_lstd_batch import CASES, REG, crafted

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
EINVAL, ESTATE = -1, -5
ALPHA, GAMMA, LAMBDA = 0.3, 0.95, 0.8
BASE = dict(domain=ra.MOUNTAIN_CAR, order=3, algo=ra.LAMBDA_LSPE, policy=ra.RANDOM, n_envs=64, seed=5, gamma=GAMMA, alpha=ALPHA, lam=LAMBDA,
            max_episode_steps=7)


def ctx(**kw):
    return ra.Context(**dict(BASE, **kw))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def zvec(F, delta, rows):
    z = np.zeros(F)
    z[0], z[1] = delta, rows
    return z


def f64_state(c, learners=None):
    """the learners' exact state (all of them, or those listed), name -> array stacked on axis 0; z[2 ..] must read 0"""
    per = [c.get_lstd_batch_state(i) for i in (range(c.N) if learners is None else learners)]
    assert all(not p[3][2:].any() for p in per)
    return dict(lstd_theta=np.stack([p[0] for p in per]), lstd_A=np.stack([p[1] for p in per]), lstd_b=np.stack([p[2] for p in per]),
                lspe_delta=np.array([p[3][0] for p in per]), lspe_rows=np.array([p[3][1] for p in per]),
                singular_solves=np.array([p[4] for p in per], dtype=np.uint32))


def full_snapshot(c):
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


def device_features(c, states):
    """the kernel's own f64 phi(s) of states (D, M), M <= c.N, one per learner -> (M, F); see the module's docstring.  Leaves the learners' state
    overwritten"""
    F, M = c.F, states.shape[1]
    S = np.zeros((1, c.D, c.N), np.float32)
    S[0, :, :M] = states
    zero = np.zeros(F)
    for i in range(M):
        c.set_lstd_batch_state(zero, np.zeros((F, F)), zero, zero, 0, i)
    L = np.zeros(c.N, np.uint32)
    L[:M] = 1
    c.handle_transitions(S, np.ones((1, c.N), np.float32), S, np.zeros((1, c.N), np.uint8), L)
    out = np.empty((M, F))
    for i in range(M):
        theta, A, b, z, sing = c.get_lstd_batch_state(i)
        assert z[0] == 1.0 and z[1] == 1.0 and not theta.any() and sing == 0, (i, z[:2])
        out[i] = b
    return out


def relaxed(theta, x, alpha):
    keep = 1.0 - alpha
    return np.array([keep * float(t) + alpha * float(v) for t, v in zip(theta, x)])


@pytest.mark.parametrize("order", [1, 3, 5])
def test_solve_is_the_restated_relaxed_elimination_bit_for_bit(order):
    N = 64
    rng = np.random.default_rng(390 + order)
    with ctx(order=order, n_envs=N) as c:
        F = c.F
        assert F == (order + 1) ** 2
        given = []
        for i in range(N):                                         # (the kind changes every second learner: each kind meets both row counts)
            kind, rows = (i // 2) % 4, F if i % 2 == 0 else F - 1
            A, b = crafted(F, kind, rng)
            theta = rng.normal(0.0, 1.0, size=F)
            c.set_lstd_batch_state(theta, A, b, zvec(F, 0.25, rows), 0, i)
            given.append((kind, rows, theta, A, b))
        t0 = c.step_count
        c.lstd_solve()
        assert c.step_count == t0
        got = f64_state(c)
        solved = singular = 0
        for i, (kind, rows, theta, A, b) in enumerate(given):
            x = lu_solve(A, b)
            if rows == F and x is not None:
                solved += 1
                want = relaxed(theta, x, ALPHA)
                assert got["lstd_theta"][i].tobytes() == want.tobytes(), (i, kind, np.max(np.abs(got["lstd_theta"][i] - want)))
                assert not got["lstd_A"][i].any() and not got["lstd_b"][i].any() and got["lspe_delta"][i] == 0.0 and got["lspe_rows"][i] == 0.0, i
                assert got["singular_solves"][i] == 0
            else:                                                  # deferred, or abandoned: every byte stays
                assert got["lstd_theta"][i].tobytes() == theta.tobytes() and got["lstd_A"][i].tobytes() == A.tobytes(), (i, kind, rows)
                assert got["lstd_b"][i].tobytes() == b.tobytes() and got["lspe_delta"][i] == 0.25 and got["lspe_rows"][i] == rows, (i, kind, rows)
                abandoned = rows == F and x is None
                singular += abandoned
                assert abandoned == (rows == F and kind == 3) and got["singular_solves"][i] == (1 if abandoned else 0), (i, kind, rows)
        assert solved == 3 * N // 8 and singular == N // 8
        c.lstd_solve()                                             # the solved learners hold no rows now: deferred; the singular ones count again
        again = f64_state(c)
        assert np.array_equal(again["singular_solves"], 2 * got["singular_solves"])
        for name in ("lstd_theta", "lstd_A", "lstd_b", "lspe_delta", "lspe_rows"):
            assert again[name].tobytes() == got[name].tobytes(), name


@pytest.mark.parametrize("domain,order", REG)
def test_handle_transitions_against_the_f64_rule(orc, domain, order):
    N, T = 64, 7
    rng = np.random.default_rng(domain * 100 + order * 10 + 39)
    with ctx(domain=domain, order=order, n_envs=N) as c:
        F, D = c.F, c.D
        S = np.stack([rand_states(orc, domain, N, rng) for _ in range(T)])
        S2 = np.stack([rand_states(orc, domain, N, rng) for _ in range(T)])
        R = rng.normal(0.0, 1.0, size=(T, N)).astype(np.float32)
        Tm = (rng.random((T, N)) < 0.3).astype(np.uint8)
        L = np.array([0, 1, 2, 7], dtype=np.uint32)[np.arange(N) % 4]
        init = [(rng.normal(0.0, 0.5, size=F), np.eye(F) + 0.1 * rng.normal(0.0, 1.0, size=(F, F)) / np.sqrt(F), rng.normal(0.0, 1.0, size=F),
                 float(rng.normal(0.0, 1.0))) for _ in range(N)]

        def install():
            for i, (theta, A, b, delta) in enumerate(init):
                c.set_lstd_batch_state(theta, A, b, zvec(F, delta, 0), 0, i)      # no rows: no solve wherever F > T

        install()
        t0 = c.step_count
        td = c.handle_transitions(S, R, S2, Tm, L, td=True, actions=rng.integers(0, c.A, size=(T, N)).astype(np.int32))
        assert c.step_count == t0 + 1
        got = f64_state(c)
        tol = 16.0 * F * T * EPS                                   # the existing bar (tests/test_gpu_lstd_batch.py): 16 F T eps (1 + max |w|)
        solving = []
        for i in range(N):
            n = int(L[i])
            theta, A, b, delta = init[i]
            if n == 0:                                             # no call: every byte stays, no rows counted, no solve
                assert got["lstd_theta"][i].tobytes() == theta.tobytes() and got["lstd_A"][i].tobytes() == A.tobytes()
                assert got["lstd_b"][i].tobytes() == b.tobytes() and got["lspe_delta"][i] == delta and got["lspe_rows"][i] == 0.0
                assert got["singular_solves"][i] == 0 and np.isnan(td[:, i]).all()
                continue
            st = state_of(theta, A, b, delta, 0)
            batch = [(orc.fourier_project(domain, order, S[k, :, i]), orc.fourier_project(domain, order, S2[k, :, i]), float(R[k, i]), bool(Tm[k, i]))
                     for k in range(n)]
            want_td = accumulate(st, batch, GAMMA, LAMBDA)
            for k in range(n):
                assert abs(float(td[k, i]) - want_td[k]) <= 2.0 ** -22 * (1.0 + abs(want_td[k])), (i, k, td[k, i], want_td[k])
            assert np.isnan(td[n:, i]).all() and got["singular_solves"][i] == 0
            if st["rows"] == F:                                    # (F = 4, seven rows: solved -- below)
                assert F == 4 and n == 7
                solving.append(i)
                assert not got["lstd_A"][i].any() and not got["lstd_b"][i].any() and got["lspe_delta"][i] == 0.0 and got["lspe_rows"][i] == 0.0, i
                continue
            assert got["lspe_rows"][i] == n and got["lstd_theta"][i].tobytes() == theta.tobytes(), i      # deferred: theta does not move
            for name, w in (("lstd_A", np.array(st["A"])), ("lstd_b", np.array(st["b"])), ("lspe_delta", np.array(st["delta"]))):
                err = np.max(np.abs(got[name][i] - w))
                assert err <= tol * (1.0 + np.max(np.abs(w))), (i, name, err, tol * (1.0 + np.max(np.abs(w))))
        assert (F == 4) == bool(solving)
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
        assert not c.episode_steps.any() and np.isnan(c.episode_record[1]).all()      # the ctx's own open record is not touched
        for buf in bufs:
            buf.free()

        # ---- F = 4: the learners whose seven rows were solved hold the bits of the restatement on the device's own features
        if solving:
            phi = np.stack([device_features(c, S[k]) for k in range(T)])      # (T, N, F)
            phi2 = np.stack([device_features(c, S2[k]) for k in range(T)])
            for i in solving:
                theta, A, b, delta = init[i]
                st = state_of(theta, A, b, delta, 0)
                _, did = handle(st, [(phi[k, i], phi2[k, i], float(R[k, i]), bool(Tm[k, i])) for k in range(7)], ALPHA, GAMMA, LAMBDA)
                assert did == "solved" and got["lstd_theta"][i].tobytes() == np.array(st["theta"]).tobytes(), (i, np.max(np.abs(got["lstd_theta"][i] - st["theta"])))


@pytest.mark.parametrize("case", list(CASES))
def test_train_is_the_trait_loop_launch_depth_and_shard_invariant(case):
    kw, K, first_split = CASES[case]
    cap = kw["max_episode_steps"]
    Recording.log = []
    st, ref = check_train_invariance(lambda **k: Recording(**dict(BASE, **k)), dict(kw), K, cap, depths=(1, 7), first_split=first_split,
                                     kernel="k_train_lspe", trait=lstd_batch_trait_loop)
    print("statistics", st)
    assert st["env_steps"] == kw["n_envs"] * K and st["episodes"] > 0 and st["sum_abs_td_error"] > 0
    train, trait, d1, d7, s0, s1 = Recording.log
    assert np.isfinite(train["lstd_theta"]).all() and not train["singular_solves"].any()
    assert np.array_equal(train["weights"][:, :, 0], train["lstd_theta"].astype(np.float32))
    assert_same(trait, train, "the trait loop against train")
    assert_same(d1, train, "the split train at steps_per_launch 1")
    assert_same(d7, train, "the split train at steps_per_launch 7")
    assert_same(join_shards(s0, s1), train, "two shards joined")
    # a deferred and a performed solve, from rows and theta: theta leaves 0 only in a performed solve; a row count strictly between 0 and F was
    # left by a handled batch whose solve was deferred.  Looked for at the end and two caps in (the truncation case ends on a performed solve)
    with ctx(**kw) as c:
        c.reset()
        c.train(2 * cap)
        mid = f64_state(c)
        F = c.F
    deferred = sum(int(((s["lspe_rows"] > 0) & (s["lspe_rows"] < F)).sum()) for s in (mid, train))
    performed = int(train["lstd_theta"].any(axis=1).sum())
    print("learners seen between a deferred solve and the next batch: %d; learners with a performed solve: %d of %d" % (deferred, performed, kw["n_envs"]))
    assert deferred > 0 and performed > 0


def test_long_horizon_replayed_in_numpy_to_the_bit(orc):
    """285 batch-steps of the driver loop at 64 MountainCar order-3 learners, cap 10 (every end a truncation: 28 batches of 10 rows against F = 16,
    performed and deferred solves in turn, the last one deferred); four learners replayed in numpy on the transitions an RSRL_RECURSIVE_LSTD ctx's
    trait loop records (the same environment side, draw for draw) with the device's own f64 features: theta, A, b, delta, rows and the counter to
    the bit"""
    N, K, cap, domain, order = 64, 285, 10, ra.MOUNTAIN_CAR, 3
    rng = np.random.default_rng(11)
    pick = np.sort(rng.choice(N, size=4, replace=False))
    kw = dict(domain=domain, order=order, n_envs=N, seed=9, max_episode_steps=cap)
    with ctx(**kw) as c, ctx(**dict(kw, algo=ra.RECURSIVE_LSTD)) as t, ctx(**kw) as probe:
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
        # the device's features of every recorded state, 64 states a call
        flat = np.concatenate([np.concatenate([r[0] for r in rec], axis=1), np.concatenate([r[1] for r in rec], axis=1)], axis=1)      # (D, 2 K 4)
        phi = np.concatenate([device_features(probe, flat[:, j:j + N]) for j in range(0, flat.shape[1], N)]).reshape(2, K, len(pick), F)
        want_oracle = orc.fourier_project(domain, order, flat[:, 5])
        assert np.max(np.abs(phi.reshape(-1, F)[5] - want_oracle)) <= 64 * EPS      # (the probe reads features: a few ulps from the oracle's)
        seen = set()
        for k, i in enumerate(pick):
            st, batch = initial_state(F), []
            for j, (frm, nxt, rew, term, ended) in enumerate(rec):
                batch.append((phi[0, j, k], phi[1, j, k], float(rew[k]), bool(term[k])))
                if ended[k]:
                    seen.add(handle(st, batch, ALPHA, GAMMA, LAMBDA)[1])
                    batch = []
            g_theta, g_A, g_b, g_z, g_sing = c.get_lstd_batch_state(int(i))
            assert g_theta.tobytes() == np.array(st["theta"]).tobytes(), (i, np.max(np.abs(g_theta - st["theta"])))
            assert g_A.tobytes() == np.array(st["A"]).tobytes() and g_b.tobytes() == np.array(st["b"]).tobytes(), i
            assert g_z[0].tobytes() == np.float64(st["delta"]).tobytes() and g_z[1] == st["rows"] and g_sing == st["singular"] == 0, (i, g_z[:2], st["delta"], st["rows"])
            assert np.abs(g_theta).max() > 0 and g_z[1] == 10 and g_A.any() and g_z[0] != 0.0
        assert seen == {"solved", "deferred"}


def test_checkpoint_resumes_bitwise_and_the_checksum_covers_delta_and_rows(tmp_path):
    N, F, cap = 32, 16, 7
    kw = dict(n_envs=N, order=3, max_episode_steps=cap)
    path = os.path.join(str(tmp_path), "lspe.ckpt")

    def delta_and_rows_move_the_checksum(a, b):
        st = list(b.get_lstd_batch_state(5))
        assert st[3][0] != 0.0 and st[3][1] == 7                    # (41 steps, five 7-row episodes: solved, deferred, deferred, solved, deferred)
        for part, new in ((0, np.nextafter(st[3][0], np.inf)), (1, 6.0)):
            before = b.checksum()
            z = st[3].copy()
            z[part] = new
            b.set_lstd_batch_state(st[0], st[1], st[2], z, st[4], env_index=5)
            assert b.checksum()[0] != before[0] and b.checksum()[1] == before[1], part
            b.set_lstd_batch_state(*st, env_index=5)
            assert b.checksum() == before

    check_checkpoint_resume(ctx, kw, path, 3 * cap, 20, carry=("states", "actions", "episode_steps"), then=delta_and_rows_move_the_checksum)
    with open(path, "rb") as f:
        head = f.read(72)
    assert int.from_bytes(head[8:12], "little") == 10 and int.from_bytes(head[44:48], "little") == ra.LAMBDA_LSPE and int.from_bytes(head[52:56], "little") == 19
    assert os.path.getsize(path) == 72 + N * 8 * (F + F * F + F + 2) + N * 4
    # ... and with open episodes: the caller carries the record next to the states, actions and episode steps
    with ctx(**kw) as a, ctx(**kw) as b:
        a.reset()
        a.train(17)
        a.save_weights(path)
        b.load_weights(path)
        b.states, b.actions, b.episode_steps, b.episode_record = a.states, a.actions, a.episode_steps, a.episode_record
        assert (a.episode_steps == 3).all() and b.step_count == a.step_count == 17
        for when, k in (("after the load", 0), ("20 steps after the load", 20)):
            if k:
                a.train(k)
                b.train(k)
            assert_same(full_snapshot(b), full_snapshot(a), when)
            assert a.checksum() == b.checksum(), when
        assert np.abs(f64_state(a)["lstd_theta"]).max() > 0
    others = [dict(algo=ra.LSTD_LAMBDA), dict(algo=ra.LSTD), dict(algo=ra.RECURSIVE_LSTD)]
    check_foreign_checkpoints_refused(ctx, kw, path, [dict(BASE, **dict(kw, **o)) for o in others], tmp_path)
    # a row count that is no integer in 0 .. F is refused at load, and the ctx stays as it was
    blob = bytearray(open(path, "rb").read())
    at = 72 + N * 8 * (F + F * F + F) + 8 * (2 * 3 + 1)            # learner 3's rows
    for bad in (17.0, 2.5, -1.0):
        blob[at:at + 8] = np.float64(bad).tobytes()
        open(path, "wb").write(bytes(blob))
        with ctx(**kw) as b:
            before = b.checksum()
            with pytest.raises(RsrlHipError) as e:
                b.load_weights(path)
            assert e.value.code == EINVAL and b.checksum() == before, bad


def test_initial_state_and_refusals(orc):
    N, cap = 16, 7
    rng = np.random.default_rng(3)
    with ctx(n_envs=N, max_episode_steps=cap) as c:
        F = c.F
        assert c.n_out == 1
        for i in (0, N - 1):
            th, A, b, z, sing = c.get_lstd_batch_state(i)
            assert not th.any() and np.array_equal(A, 1e-6 * np.eye(F)) and not b.any() and sing == 0
            assert z[0] == 0.0 and z[1] == F and not z[2:].any()
        S = rand_states(orc, ra.MOUNTAIN_CAR, N, rng)
        zN, zTN = np.zeros(N, np.float32), np.zeros((1, N), np.float32)
        calls = [lambda: c.handle(S, np.zeros(N, np.int32), zN, S, np.zeros(N, np.uint8)),
                 lambda: c.handle_batch(S[None], np.zeros((1, N), np.int32), zTN, np.ones(N, np.uint32)),
                 lambda: c.get_lstd_state(0), lambda: c.set_lstd_state(np.zeros(F), np.eye(F), None, 0)]
        for k, call in enumerate(calls):
            with pytest.raises(RsrlHipError) as e:
                call()
            assert e.value.code == ESTATE, k
            if k < 2:
                assert "handle_transitions" in str(e.value)
        # the row count: an integer in 0 .. F, or EINVAL with nothing moved
        c.reset()
        c.train(2 * cap)
        before, cs = f64_state(c), c.checksum()
        st = c.get_lstd_batch_state(2)
        for bad in (F + 1.0, 0.5, -1.0, float("nan")):
            with pytest.raises(RsrlHipError) as e:
                c.set_lstd_batch_state(st[0] + 1.0, st[1] + 1.0, st[2] + 1.0, zvec(F, 3.0, bad), 9, 2)
            assert e.value.code == EINVAL, bad
            assert_same(f64_state(c), before, "after a refused set_lstd_batch_state (rows = %r)" % bad)
            assert c.checksum() == cs
        for good in (0.0, float(F)):
            c.set_lstd_batch_state(st[0], st[1], st[2], zvec(F, 3.0, good), st[4], 2)
            assert tuple(c.get_lstd_batch_state(2)[3][:2]) == (3.0, good)
        # z = NULL: neither delta nor rows is read
        c.set_lstd_batch_state(st[0] + 1.0, st[1], st[2], None, 4, 2)
        th, A, b, z, sing = c.get_lstd_batch_state(2)
        assert np.array_equal(th, st[0] + 1.0) and tuple(z[:2]) == (3.0, float(F)) and sing == 4
        # the value side is LSTD's: get_weights = f32(theta), q_evaluate = f32(phi . theta) evaluated in f64; a reset leaves the agent alone
        assert np.array_equal(c.get_weights(2)[:, 0], (st[0] + 1.0).astype(np.float32))
        q = c.q_evaluate(S)
        for i in range(N):
            v = np.float32(orc.fourier_project(ra.MOUNTAIN_CAR, 3, S[:, i]) @ c.get_lstd_batch_state(i)[0])
            assert abs(q[0, i] - v) <= abs(np.spacing(v)), (i, q[0, i], v)
        now = f64_state(c)
        c.reset()
        assert_same(f64_state(c), now, "the agent's state across a reset")


def test_lambda_lspe_example_builds_and_runs(tmp_path):
    out = run_example(tmp_path, "lambda_lspe", [64, 2, 300, 3, 50])
    lines = [ln for ln in out.splitlines() if ln.startswith("LambdaLSPE:")]
    assert "Batch 2:" in out and len(lines) == 3 and all("8-transition batch handled" in ln and "0 abandoned solves" in ln for ln in lines), out
    assert "(deferred)" in lines[0] and "(solved)" in lines[1] and "(deferred)" in lines[2], out
