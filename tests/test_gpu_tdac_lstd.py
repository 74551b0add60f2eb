"""ActorCritic::tdac with the iLSTD critic (RSRL_ILSTD_ACTOR_CRITIC, train_tdac_lstd.hip) on the device: handle against the restatement
(tests/tdac_lstd_numpy.py), the critic half bit for bit an iLSTD ctx's, train against the trait-granular loop / launch depths / shards bit for bit,
checkpoints (file version 10, aux_kind 9, the file's bytes pinned) and the checksum, the value side reading the f64 theta and the policy side the
actor, the refusals and the C++ example."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

import rsrl_amd
from rsrl_amd import RsrlHipError
from tests.ac_numpy import near_boundary
from tests.agent_contract import (check_checkpoint_resume, check_foreign_checkpoints_refused, check_train_invariance, diff, learner_state, rand_states,
                                  run_example)
from tests.tdac_lstd_numpy import handle_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AC, ILSTD = rsrl_amd.ILSTD_ACTOR_CRITIC, rsrl_amd.ILSTD
REG = [(rsrl_amd.MOUNTAIN_CAR, o) for o in (1, 2, 3, 4, 5)] + [(rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]
LOOP = [(rsrl_amd.MOUNTAIN_CAR, 1), (rsrl_amd.MOUNTAIN_CAR, 3), (rsrl_amd.MOUNTAIN_CAR, 5), (rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]
EPS = np.finfo(np.float64).eps


BASE = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=AC, policy=rsrl_amd.SOFTMAX, n_envs=32, seed=5, gamma=0.95, lr=0.05, alpha=0.3, tau=1.0, n_steps=3)


def ctx(**kw):
    return rsrl_amd.Context(**dict(BASE, **kw))


def randomise(c, rng, also=()):
    """a well-conditioned random iLSTD state per learner (tests/test_gpu_lstd.py's: A near I) and a random actor; the f64 state also goes into the
    ctxs of `also`"""
    F = c.F
    for i in range(c.N):
        theta, M, mu = rng.normal(0.0, 0.5, size=F), rng.normal(0.0, 1.0, size=(F, F)), rng.normal(0.0, 1.0, size=F)
        for x in (c,) + tuple(also):
            x.set_lstd_state(theta, np.eye(F) + 0.1 * M / np.sqrt(F), mu, i)
        c.set_policy_weights(rng.normal(0.0, 0.3, size=(F, c.A)).astype(np.float32), i)


def _transitions(c, orc, domain, rng):
    N = c.N
    c.states = rand_states(orc, domain, N, rng)
    a = rng.integers(0, c.A, size=N).astype(np.int32)
    frm, nxt, rew, term = c.domain_step(a)
    term = (term | (rng.random(N) < 0.25)).astype(np.uint8)          # the critic reads V(s') of these: s' as domain_step reported it
    return frm, a, rew, nxt, term


@functools.lru_cache(maxsize=None)
def _case(orc, domain, order):
    return handle_case(orc, domain, order)


@pytest.mark.parametrize("domain,order", REG)
def test_handle_against_the_restatement(orc, domain, order):
    """the f64 state: tests/test_gpu_lstd.py's bound (every quantity is a sum of at most F rounded products per step and the features differ from the
    oracle's by a few ulps: 16 F eps per step relative to the state's magnitude), learners within 1e-9 of argmaxima's tie band left out, at most N / 4
    of them (tests/test_tdac_lstd_cpu.py: none with this seed).  The actor: tests/test_gpu_tdac.py's bound after one handle -- the same f32
    arithmetic on the same f32 features"""
    case = _case(orc, domain, order)
    N, F, p = len(case["init"]), case["F"], case["params"]
    with ctx(domain=domain, order=order, n_envs=N, seed=17, **p) as c:
        assert c.n_out == 1 and c.F == F
        for i, (theta, A, mu, Th) in enumerate(case["init"]):
            c.set_lstd_state(theta, A, mu, i)
            c.set_policy_weights(Th, i)
        for k, (frm, a, rew, nxt, term) in enumerate(case["rounds"]):
            td = c.handle(frm, a, rew, nxt, term)
            for i in range(N):
                d = case["diag"][k, i]
                assert abs(float(td[i]) - d) <= 2.0 ** -22 * (1.0 + abs(d)), (k, i, td[i], d)
            if k == 0:
                for i in range(N):
                    old, want = case["init"][i][3].astype(np.float64), case["first"][i]
                    sphi = np.abs(orc.fourier_project(domain, order, frm[:, i])).sum()
                    x_scale = np.max(np.abs(want - old))
                    err = np.max(np.abs(c.get_policy_weights(i) - want))
                    assert err <= 3e-6 * (1 + x_scale) * sphi + 3e-6 * np.max(np.abs(old)), (i, err)
        steps = len(case["rounds"]) * (1 + p["n_steps"])
        tol = 16.0 * F * steps * EPS
        skipped = case["skipped"]
        for i in np.flatnonzero(~skipped):
            for j, (g, w) in enumerate(zip(c.get_lstd_state(i), case["final"][i][:3])):
                scale = 1.0 + np.max(np.abs(w))
                assert np.max(np.abs(g - w)) <= tol * scale, (i, j, np.max(np.abs(g - w)), tol * scale)
        assert skipped.sum() <= N // 4, skipped.sum()


@pytest.mark.parametrize("domain,order", LOOP)
def test_the_critic_half_is_ilstd_bit_for_bit(orc, domain, order):
    N = 64
    kw = dict(domain=domain, order=order, n_envs=N, seed=3, gamma=0.95, n_steps=2)
    rng = np.random.default_rng(order * 7 + domain)
    with ctx(lr=0.05, alpha=0.3, tau=0.7, **kw) as c, rsrl_amd.Context(algo=ILSTD, policy=rsrl_amd.RANDOM, alpha=0.05, **kw) as v:
        randomise(c, rng, also=(v,))
        for _ in range(3):                                            # three rounds: the actor moves, the critic must not notice
            frm, a, rew, nxt, term = _transitions(c, orc, domain, rng)
            assert 0 < term.sum() < N
            td_ac = c.handle(frm, a, rew, nxt, term)
            td_v = v.handle(frm, a, rew, nxt, term)
            assert np.array_equal(td_ac.view(np.uint32), td_v.view(np.uint32))
            for i in range(N):
                for x, y in zip(c.get_lstd_state(i), v.get_lstd_state(i)):
                    assert x.tobytes() == y.tobytes(), i
        assert np.array_equal(c.get_weights(5), v.get_weights(5))


@pytest.mark.parametrize("domain,order", LOOP)
def test_train_is_the_trait_loop_launch_depth_and_shard_invariant(domain, order):
    N, K, cap = 64, 60, 23
    kw = dict(domain=domain, order=order, n_envs=N, max_episode_steps=cap, tau=0.7, lr=0.02, alpha=0.2, gamma=0.97, n_steps=2)
    st, ref = check_train_invariance(ctx, kw, K, cap, depths=(1, 64), first_split=20, kernel="k_train_tdac_lstd")
    assert st["episodes"] > 0 and st["env_steps"] == N * K and st["sum_abs_td_error"] > 0
    assert np.isfinite(ref["lstd_theta"]).all() and np.abs(ref["lstd_theta"]).max() > 0 and np.abs(ref["theta"]).max() > 0


def _digest_recipe():
    spec = importlib.util.spec_from_file_location("make_checkpoint_digest_tdac_lstd", os.path.join(ROOT, "tests", "golden", "make_checkpoint_digest_tdac_lstd.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_checkpoint_resumes_bitwise_and_the_checksum_covers_both_agents(tmp_path):
    kw = dict(n_envs=32, order=3, max_episode_steps=17, lr=0.02, alpha=0.2, tau=0.5)
    path = os.path.join(str(tmp_path), "tdac_lstd.ckpt")

    def one_bit_of_either_agent_moves_the_checksum(a, b):
        before = b.checksum()
        th, m, u = b.get_lstd_state(5)
        m[3, 4] = np.nextafter(m[3, 4], np.inf)                # one bit of one learner's f64 matrix
        b.set_lstd_state(th, m, u, 5)
        flipped = b.checksum()
        assert flipped[0] != before[0] and flipped[1] == before[1]
        pw = b.get_policy_weights(7)
        pw[2, 1] = np.nextafter(pw[2, 1], np.float32(np.inf))  # one bit of one learner's actor
        b.set_policy_weights(pw, 7)
        assert b.checksum()[0] != flipped[0] and b.checksum()[0] != before[0] and b.checksum()[1] == before[1]

    check_checkpoint_resume(ctx, kw, path, 25, 20, carry=("states", "actions", "episode_steps"), then=one_bit_of_either_agent_moves_the_checksum)
    with open(path, "rb") as f:
        head = f.read(72)
    F, A = 16, 3
    assert int.from_bytes(head[8:12], "little") == 10 and int.from_bytes(head[40:44], "little") == 1 and int.from_bytes(head[52:56], "little") == 9
    assert os.path.getsize(path) == 72 + 32 * 8 * (F + F * F + F) + 32 * 4 * F * A
    others = [dict(algo=ILSTD, policy=rsrl_amd.RANDOM, alpha=0.02), dict(algo=rsrl_amd.TD_ACTOR_CRITIC), dict(algo=rsrl_amd.TD, policy=rsrl_amd.RANDOM)]
    check_foreign_checkpoints_refused(ctx, kw, path, [dict(BASE, **dict(kw, **other)) for other in others], tmp_path)
    # a truncated file is refused before anything is touched
    raw = open(path, "rb").read()
    open(path, "wb").write(raw[:-4])
    with ctx(**kw) as b:
        before = b.checksum()
        with pytest.raises(RsrlHipError, match="truncated"):
            b.load_weights(path)
        assert b.checksum() == before


def test_checkpoint_file_is_the_recorded_one(tmp_path):
    recipe = _digest_recipe()
    want = json.load(open(recipe.FIXTURE))[recipe.NAME]
    got, checksum = recipe.digest(str(tmp_path))
    print(got, "recorded:", want)
    assert (got["version"], got["aux_kind"]) == (10, 9) == (want["version"], want["aux_kind"])
    assert got["bytes"] == want["bytes"] == 72 + 32 * 8 * (16 + 256 + 16) + 32 * 4 * 48
    assert got["sha256"] == want["sha256"]
    kw, steps, _, _ = recipe.CASE
    with rsrl_amd.Context(**kw) as r:
        r.load_weights(os.path.join(str(tmp_path), recipe.NAME + ".ckpt"))
        assert r.step_count == steps and r.checksum()[0] == checksum[0]


def test_value_side_policy_side_reset_and_refusals(orc):
    N, seed, tau, domain, order = 64, 23, 0.5, rsrl_amd.MOUNTAIN_CAR, 3
    rng = np.random.default_rng(4)
    with ctx(n_envs=N, seed=seed, tau=tau, order=order, max_episode_steps=40) as c:
        F = c.F
        assert c.n_out == 1
        for i in (0, N - 1):                                          # theta = 0, A = I, mu = 0, actor = 0
            th, m, u = c.get_lstd_state(i)
            assert not th.any() and np.array_equal(m, np.eye(F)) and u is not None and not u.any() and not c.get_policy_weights(i).any()
        randomise(c, rng)
        Ts = [c.get_policy_weights(i) for i in range(N)]
        S = rand_states(orc, domain, N, rng)
        phis = [orc.fourier_project(domain, order, S[:, i]) for i in range(N)]
        # ---- the value side: V from the f64 theta, exactly as iLSTD's
        q = c.q_evaluate(S)
        assert q.shape == (1, N)
        for i in range(N):
            th = c.get_lstd_state(i)[0]
            v = np.float32(phis[i] @ th)
            assert abs(q[0, i] - v) <= abs(np.spacing(v)), (i, q[0, i], v)
            assert np.array_equal(c.get_weights(i)[:, 0], th.astype(np.float32))
        th0, m0, u0 = c.get_lstd_state(2)
        w = rng.normal(0.0, 1.0, size=(F, 1)).astype(np.float32)
        c.set_weights(w, 2)
        th1, m1, u1 = c.get_lstd_state(2)
        assert np.array_equal(th1, w[:, 0].astype(np.float64)) and np.array_equal(m1, m0) and np.array_equal(u1, u0)
        assert np.array_equal(c.get_policy_weights(2), Ts[2])
        # ---- the policy side: the actor, exactly as the TD ActorCritic's
        h = np.array([Ts[i].astype(np.float64).T @ phis[i] for i in range(N)]).T
        probs = c.policy_probs(S)
        want = np.array([orc.policy_probs(orc.SOFTMAX, h[:, i], tau=tau) for i in range(N)]).T
        assert np.max(np.abs(probs - want)) <= 1e-6
        assert np.array_equal(c.policy_mode(S), [orc.argmax_first(probs[:, i], prec="f32") for i in range(N)])
        a = rng.integers(0, c.A, size=N).astype(np.int32)
        assert np.allclose(c.policy_prob(S, a), h[a, np.arange(N)], atol=2e-5, rtol=1e-5)      # Softmax's Function<(S, A)> is the raw preference (softmax.rs:84-92)
        sample = c.policy_sample(S)                                  # the first API call: BLK_API, call 0
        for i in range(N):
            x = orc.draw(seed, i, 0, orc.BLK_API)
            if not near_boundary(want[:, i], x):
                assert sample[i] == orc.policy_sample(orc.SOFTMAX, h[:, i], x, tau=tau), i
        # ---- the refusals
        calls = [lambda: c.q_find_max(S), lambda: c.q_find_min(S), lambda: c.q_expected_value(S, probs),
                 lambda: c.get_traces(0), lambda: c.set_traces(np.zeros((F, 1)), 0), lambda: c.get_td_weights(0),
                 lambda: c.set_td_weights(np.zeros((F, c.A)), 0), lambda: c.get_behaviour_weights(0),
                 lambda: c.handle_batch(np.zeros((1, c.D, N)), np.zeros((1, N)), np.zeros((1, N)), np.zeros(N))]
        for k, call in enumerate(calls):
            with pytest.raises(RsrlHipError) as e:
                call()
            assert e.value.code == -5, k
        # ---- reset: the initial sample reads the actor, and neither agent's state moves
        before = [learner_state(c, i) for i in range(N)]
        c.reset()
        assert all(diff(before[i], learner_state(c, i)) == [] for i in range(N))
        phi0 = orc.fourier_project(domain, order, orc.domain_reset(domain, prec="f32"))
        acts = c.actions
        for i in range(N):
            h0 = Ts[i].astype(np.float64).T @ phi0
            x = orc.draw(seed, i, 0, orc.BLK_INIT)
            if not near_boundary(orc.policy_probs(orc.SOFTMAX, h0, tau=tau), x):
                assert acts[i] == orc.policy_sample(orc.SOFTMAX, h0, x, tau=tau), i
        # ---- rollout_greedy = Domain::rollout(|s| policy.mode(s)): a host loop of domain_step + policy_mode through the same ctx
        L = 30
        n_states, total = c.rollout_greedy(L)
        c.domain_reset()
        tot, steps, done = np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.int64), np.zeros(N, dtype=bool)
        for _ in range(L - 1):
            frm, nxt, rew, term = c.domain_step(c.policy_mode(c.states))
            live = ~done
            tot[live] = (tot[live] + rew[live]).astype(np.float32)
            steps[live] += 1
            done |= term.astype(bool)
        assert np.array_equal(n_states, steps + 1)
        assert np.array_equal(total, tot)
    bad = [dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(domain=rsrl_amd.CART_POLE, order=2), dict(weight_mode=rsrl_amd.W_SHARED),
           dict(domain=rsrl_amd.HIV_TREATMENT, order=1), dict(policy=rsrl_amd.RANDOM), dict(agent_policy=rsrl_amd.SOFTMAX), dict(epsilon_decay=0.99),
           dict(n_steps=0), dict(n_steps=33)]
    for b in bad:
        with pytest.raises(RsrlHipError) as e:
            ctx(**b)
        assert e.value.code == -1 and "RSRL_ILSTD_ACTOR_CRITIC" in str(e.value), b
    with pytest.raises(RsrlHipError, match="unknown algo 20"):
        ctx(algo=20)


def test_example_builds_and_runs(tmp_path):
    out = run_example(tmp_path, "tdac_ilstd", [64, 3, 200])
    assert "Batch 3:" in out and "OOS:" in out
    tail = out.split("iLSTD: max |theta| of learner 0:")[1]
    vmax, tmax = float(tail.split()[0]), float(tail.split("actor: max |theta| of learner 0:")[1].split()[0])
    assert np.isfinite(vmax) and vmax > 0.0 and np.isfinite(tmax) and tmax > 0.0
    assert "(16 features)" in tail and "(48 weights)" in tail           # MountainCar, order 3: F = 16; theta_a has three columns
