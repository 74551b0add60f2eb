"""RecursiveLSTD and iLSTD (RSRL_RECURSIVE_LSTD, RSRL_ILSTD; train_lstd.hip) on the device: handle against the f64 restatement, train against the
trait-granular loop / launch depths / shards bit for bit, checkpoints and the checksum over the f64 state, a long horizon replayed in numpy, the value
side, the refusals and the C++ example."""
import os

import numpy as np
import pytest

import rsrl_amd
from rsrl_amd import RsrlHipError
from tests.agent_contract import (check_checkpoint_resume, check_foreign_checkpoints_refused, check_train_invariance, diff, learner_state, rand_states,
                                  run_example)
from tests.lstd_numpy import ilstd, near_tie_band, recursive_lstd, replay_trait_loop

pytestmark = pytest.mark.gpu

RLSTD, ILSTD = rsrl_amd.RECURSIVE_LSTD, rsrl_amd.ILSTD
ALGOS = [RLSTD, ILSTD]
REG = [(rsrl_amd.MOUNTAIN_CAR, o) for o in (1, 2, 3, 4, 5)] + [(rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]
LOOP = [(rsrl_amd.MOUNTAIN_CAR, 1), (rsrl_amd.MOUNTAIN_CAR, 3), (rsrl_amd.MOUNTAIN_CAR, 5), (rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]
EPS = np.finfo(np.float64).eps


BASE = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=RLSTD, policy=rsrl_amd.RANDOM, n_envs=32, seed=5, gamma=0.95, alpha=0.05, n_steps=3)


def ctx(**kw):
    return rsrl_amd.Context(**dict(BASE, **kw))


def randomise(c, algo, rng):
    """a well-conditioned random f64 state per learner: RecursiveLSTD's C small and symmetric (a = 1 + g . phi stays near 1), iLSTD's A near I"""
    F, out = c.F, []
    for i in range(c.N):
        theta = rng.normal(0.0, 0.5, size=F)
        M = rng.normal(0.0, 1.0, size=(F, F))
        if algo == RLSTD:
            mat, mu = 1e-3 * (np.eye(F) + (M + M.T) / (4.0 * F)), None
        else:
            mat, mu = np.eye(F) + 0.1 * M / np.sqrt(F), rng.normal(0.0, 1.0, size=F)
        c.set_lstd_state(theta, mat, mu, i)
        out.append((theta, mat, mu))
    return out


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("domain,order", REG)
def test_handle_against_the_f64_rule(orc, domain, order, algo):
    N, gamma, alpha, n_upd, rounds_of_handle = 64, 0.95, 0.05, 3, 3
    rng = np.random.default_rng(domain * 100 + order * 10 + algo)
    with ctx(domain=domain, order=order, algo=algo, n_envs=N, gamma=gamma, alpha=alpha, n_steps=n_upd) as c:
        F = c.F
        st = randomise(c, algo, rng)
        ref = [list(x) for x in st]
        skipped = np.zeros(N, dtype=bool)
        for _ in range(rounds_of_handle):
            c.states = rand_states(orc, domain, N, rng)
            a = rng.integers(0, c.A, size=N).astype(np.int32)
            frm, nxt, rew, term = c.domain_step(a)
            term = (term | (rng.random(N) < 0.25)).astype(np.uint8)
            td = c.handle(frm, a, rew, nxt, term)
            for i in range(N):
                phi_s, phi_n = orc.fourier_project(domain, order, frm[:, i]), orc.fourier_project(domain, order, nxt[:, i])
                theta, mat, mu = ref[i]
                if algo == RLSTD:
                    d, theta, mat = recursive_lstd(theta, mat, phi_s, phi_n, float(rew[i]), bool(term[i]), gamma)
                else:
                    rounds = []
                    d, theta, mat, mu = ilstd(theta, mat, mu, phi_s, phi_n, float(rew[i]), bool(term[i]), gamma, alpha, n_upd, rounds=rounds)
                    skipped[i] |= any(near_tie_band(m) for m in rounds)
                ref[i] = [theta, mat, mu]
                assert abs(float(td[i]) - d) <= 2.0 ** -22 * (1.0 + abs(d)), (i, td[i], d)
        # tolerance: every quantity is a sum of at most F rounded products per step, the features differ from the oracle's by a few ulps, and
        # iLSTD's mu update is phi_s * (pd . theta) against the literal (phi_s pd^T) theta: 16 F eps per step relative to the state's magnitude
        steps = rounds_of_handle * (1 + (n_upd if algo == ILSTD else 0))
        tol = 16.0 * F * steps * EPS
        for i in np.flatnonzero(~skipped):
            for j, (g, w) in enumerate(zip(c.get_lstd_state(int(i)), ref[i])):
                if w is None:
                    continue
                scale = 1.0 + np.max(np.abs(w))
                assert np.max(np.abs(g - w)) <= tol * scale, (i, j, np.max(np.abs(g - w)), tol * scale)
        assert skipped.sum() <= N // 4, skipped.sum()          # (counted: an |mu_j| within 1e-9 of the 1e-7 tie band)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("domain,order", LOOP)
def test_train_is_the_trait_loop_launch_depth_and_shard_invariant(domain, order, algo):
    N, K, cap = 64, 60, 23
    kw = dict(domain=domain, order=order, algo=algo, n_envs=N, max_episode_steps=cap, gamma=0.97, alpha=0.02, n_steps=2)
    st, ref = check_train_invariance(ctx, kw, K, cap, depths=(1, 64), first_split=20, kernel="k_train_lstd")
    assert st["episodes"] > 0 and st["env_steps"] == N * K
    assert np.isfinite(ref["lstd_theta"]).all() and np.abs(ref["lstd_theta"]).max() > 0


@pytest.mark.parametrize("algo", ALGOS)
def test_checkpoint_resumes_bitwise_and_the_checksum_covers_the_f64_state(tmp_path, algo):
    kw = dict(n_envs=32, order=3, algo=algo, max_episode_steps=17)
    path = os.path.join(str(tmp_path), "lstd.ckpt")

    def one_ulp_of_the_matrix_moves_the_checksum(a, b):
        before = b.checksum()
        th, m, u = b.get_lstd_state(5)
        m[3, 4] = np.nextafter(m[3, 4], np.inf)                # one ulp of one learner's matrix: the f64 state is in out[0]
        b.set_lstd_state(th, m, u, 5)
        assert b.checksum()[0] != before[0] and b.checksum()[1] == before[1]

    check_checkpoint_resume(ctx, kw, path, 25, 20, carry=("states", "actions", "episode_steps"), then=one_ulp_of_the_matrix_moves_the_checksum)
    with open(path, "rb") as f:
        head = f.read(72)
    F = 16
    assert int.from_bytes(head[8:12], "little") == 10 and int.from_bytes(head[52:56], "little") == 8
    assert os.path.getsize(path) == 72 + 32 * 8 * (F + F * F + (F if algo == ILSTD else 0))
    other = RLSTD if algo == ILSTD else ILSTD
    others = (dict(algo=other, policy=rsrl_amd.RANDOM), dict(algo=rsrl_amd.TD, policy=rsrl_amd.RANDOM))
    check_foreign_checkpoints_refused(ctx, kw, path, [dict(BASE, **dict(kw, **o_kw)) for o_kw in others], tmp_path)


@pytest.mark.parametrize("algo", ALGOS)
def test_long_horizon_replayed_in_numpy(orc, algo):
    """2 000 batch-steps at 4 096 MountainCar order-5 learners through the trait loop, 8 learners replayed in f64 numpy.  Bound: every step adds at
    most ~F eps of rounding per quantity and the device's features differ from the oracle's by a few ulps; the least-squares recursions do not
    amplify those by more than 1e4 over the run (C's and A's condition), so |device - numpy| <= 1e4 * F * K * eps * (1 + max |x|)"""
    N, K, domain, order, gamma, alpha, n_upd = 4096, 2000, rsrl_amd.MOUNTAIN_CAR, 5, 0.99, 0.01, 2
    rng = np.random.default_rng(11)
    pick = np.sort(rng.choice(N, size=8, replace=False))
    with ctx(domain=domain, order=order, algo=algo, n_envs=N, seed=9, gamma=gamma, alpha=alpha, n_steps=n_upd, max_episode_steps=400) as c:
        F = c.F
        c.reset()
        ep = np.zeros(N, dtype=np.int64)
        rec = []
        for _ in range(K):
            frm, nxt, rew, term = c.domain_step(c.actions)
            c.handle(frm, c.actions, rew, nxt, term)
            rec.append((frm[:, pick].copy(), nxt[:, pick].copy(), rew[pick].copy(), term[pick].copy()))
            ep += 1
            mask = (term.astype(bool) | (ep >= 400)).astype(np.uint8)
            c.domain_reset(mask)
            ep[mask == 1] = 0
            c.policy_sample()
        tol = 1e4 * F * K * EPS
        for k, i in enumerate(pick):
            theta, mat, mu = replay_trait_loop(orc, algo == RLSTD, domain, order, F, [(frm[:, k], nxt[:, k], r[k], t[k]) for frm, nxt, r, t in rec], gamma, alpha, n_upd)
            g_th, g_m, g_mu = c.get_lstd_state(int(i))
            for g, w in ((g_th, theta), (g_m, mat)) + (((g_mu, mu),) if algo == ILSTD else ()):
                assert np.max(np.abs(g - w)) <= tol * (1.0 + np.max(np.abs(w))), (i, np.max(np.abs(g - w)), tol * (1.0 + np.max(np.abs(w))))
            assert np.abs(theta).max() > 0


@pytest.mark.parametrize("algo", ALGOS)
def test_initial_state_value_side_and_refusals(orc, algo):
    N, domain, order = 16, rsrl_amd.MOUNTAIN_CAR, 3
    rng = np.random.default_rng(3)
    with ctx(n_envs=N, algo=algo, order=order, max_episode_steps=30) as c:
        F = c.F
        assert c.n_out == 1
        for i in (0, N - 1):
            th, m, u = c.get_lstd_state(i)
            assert not th.any() and np.array_equal(m, (1e-5 if algo == RLSTD else 1.0) * np.eye(F))
            assert (u is None) == (algo == RLSTD) and (u is None or not u.any())
        c.reset()
        c.train(40)
        st = [learner_state(c, i) for i in range(N)]
        c.reset()                                                 # reset restarts the episodes only
        assert all(diff(st[i], learner_state(c, i)) == [] for i in range(N))
        # get_weights = f32(theta); q_evaluate = f32(phi . theta) evaluated in f64
        S = rand_states(orc, domain, N, rng)
        for i in range(N):
            th, _, _ = c.get_lstd_state(i)
            th = th + rng.normal(0.0, 1.0, size=F) * (i + 1)
            c.set_lstd_state(th, c.get_lstd_state(i)[1], None, i)
            assert np.array_equal(c.get_weights(i)[:, 0], th.astype(np.float32))
        q = c.q_evaluate(S)
        assert q.shape == (1, N)
        for i in range(N):
            th = c.get_lstd_state(i)[0]
            v = np.float32(orc.fourier_project(domain, order, S[:, i]) @ th)
            assert abs(q[0, i] - v) <= abs(np.spacing(v)), (i, q[0, i], v)
        # set_weights widens exactly and leaves the matrix and mu alone
        th0, m0, u0 = c.get_lstd_state(2)
        w = rng.normal(0.0, 1.0, size=(F, 1)).astype(np.float32)
        c.set_weights(w, 2)
        th1, m1, u1 = c.get_lstd_state(2)
        assert np.array_equal(th1, w[:, 0].astype(np.float64)) and np.array_equal(m1, m0) and (u0 is None or np.array_equal(u1, u0))
        calls = [lambda: c.q_find_max(S), lambda: c.q_find_min(S), lambda: c.q_expected_value(S, np.full((c.A, N), 1.0 / c.A, dtype=np.float32)),
                 lambda: c.get_traces(0), lambda: c.set_traces(np.zeros((F, 1)), 0), lambda: c.get_td_weights(0),
                 lambda: c.set_td_weights(np.zeros((F, c.A)), 0), lambda: c.get_policy_weights(0),
                 lambda: c.set_policy_weights(np.zeros((F, c.A)), 0),
                 lambda: c.handle_batch(np.zeros((1, c.D, N)), np.zeros((1, N)), np.zeros((1, N)), np.zeros(N))]
        for k, call in enumerate(calls):
            with pytest.raises(RsrlHipError) as e:
                call()
            assert e.value.code == -5, k
    with rsrl_amd.Context(domain=domain, order=order, algo=rsrl_amd.TD, policy=rsrl_amd.RANDOM, n_envs=4) as t:
        with pytest.raises(RsrlHipError) as e:
            t.get_lstd_state(0)
        assert e.value.code == -5


def test_lstd_example_builds_and_runs(tmp_path):
    for mode in ("recursive", "ilstd"):
        out = run_example(tmp_path, "lstd", [64, 2, 200, 3, mode])
        assert "Batch 2:" in out and "(16 features)" in out
        tmax = float(out.split("max |theta| of learner 0:")[1].split()[0])
        assert np.isfinite(tmax) and tmax > 0.0
