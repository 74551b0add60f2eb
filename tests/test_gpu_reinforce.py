"""REINFORCE and BaselineREINFORCE (RSRL_REINFORCE, RSRL_BASELINE_REINFORCE, train_reinforce.hip) on the device: handle_batch against the f64 rule
(the running return bit for bit), a zero baseline is REINFORCE and the baseline never moves, the driver loop against a restated episode loop,
train against the host trait loop / launch depths / shards bit for bit, checkpoints of an open episode, the policy side reading theta, the
refusals and the C++ example."""
import os

import numpy as np
import pytest

import rsrl_amd
from rsrl_amd import RsrlHipError
from tests.ac_numpy import near_boundary
from tests.agent_contract import check_checkpoint_resume, check_foreign_checkpoints_refused, check_train_invariance, rand_states, run_example, snapshot
from tests.reinforce_numpy import reinforce_batch, reinforce_restated_loop as _restated_loop

pytestmark = pytest.mark.gpu

ALGOS = [rsrl_amd.REINFORCE, rsrl_amd.BASELINE_REINFORCE]
REG = [(rsrl_amd.MOUNTAIN_CAR, o) for o in (1, 2, 3, 4, 5)] + [(rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]
LOOP = [(rsrl_amd.MOUNTAIN_CAR, 3), (rsrl_amd.MOUNTAIN_CAR, 5), (rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]
EINVAL, ESTATE = -1, -5


def ctx(**kw):
    base = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=rsrl_amd.REINFORCE, policy=rsrl_amd.SOFTMAX, n_envs=32, seed=5, gamma=0.95, alpha=0.05, tau=1.0)
    base.update(kw)
    return rsrl_amd.Context(**base)


def f32_returns(rewards, gamma):
    """g = r + gamma * g evaluated in numpy float32, as the device computes it"""
    g, gm, out = np.float32(0.0), np.float32(gamma), []
    for r in rewards:
        g = np.float32(np.float32(r) + np.float32(gm * g))
        out.append(g)
    return out


def _ragged_batch(c, orc, domain, T, rng):
    N = c.N
    S = np.stack([rand_states(orc, domain, N, rng) for _ in range(T)])
    A = rng.integers(0, c.A, size=(T, N)).astype(np.int32)
    R = rng.normal(0.0, 1.0, size=(T, N)).astype(np.float32)
    L = rng.integers(0, T + 1, size=N).astype(np.uint32)
    L[0], L[1], L[2] = 0, 1, T
    return S, A, R, L


@pytest.mark.parametrize("tau", [1.0, 0.5])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("domain,order", REG)
def test_handle_batch_against_the_f64_rule(orc, domain, order, algo, tau):
    N, T, gamma, alpha = 32, 40, 0.9, 0.05
    rng = np.random.default_rng(domain * 100 + order * 10 + int(tau * 4) + algo)
    with ctx(domain=domain, order=order, algo=algo, tau=tau, n_envs=N, seed=17, gamma=gamma, alpha=alpha) as c:
        Ts = [rng.normal(0.0, 0.3, size=(c.F, c.A)).astype(np.float32) for _ in range(N)]
        Bs = [rng.normal(0.0, 0.3, size=(c.F, c.A)).astype(np.float32) for _ in range(N)] if algo == rsrl_amd.BASELINE_REINFORCE else None
        for i in range(N):
            c.set_policy_weights(Ts[i], i)
            if Bs is not None:
                c.set_weights(Bs[i], i)
        thb0, g0 = [c.get_behaviour_weights(i) for i in range(N)], c.return_carry
        S, A, R, L = _ragged_batch(c, orc, domain, T, rng)
        t0 = c.step_count
        ret = c.handle_batch(S, A, R, L, returns=True)
        assert c.step_count == t0 + 1
        for i in range(N):
            n = int(L[i])
            want_g = f32_returns(R[:n, i], gamma)
            assert np.array_equal(ret[:n, i].view(np.uint32), np.array(want_g, dtype=np.float32).view(np.uint32)), i
            assert np.isnan(ret[n:, i]).all(), i
            phis = [orc.fourier_project(domain, order, S[t, :, i]) for t in range(n)]
            want, _ = reinforce_batch(Ts[i], phis, A[:n, i], R[:n, i].astype(np.float64), gamma, alpha, tau, None if Bs is None else Bs[i])
            got = c.get_policy_weights(i)
            if n == 0:
                assert np.array_equal(got, Ts[i]), i
                continue
            sphi = sum(np.abs(p).sum() for p in phis)
            x_scale = np.max(np.abs(want - Ts[i]))
            assert np.max(np.abs(got - want)) <= 3e-6 * (1 + x_scale) * sphi + 3e-6 * np.max(np.abs(Ts[i])), (i, np.max(np.abs(got - want)))
            assert np.array_equal(c.get_behaviour_weights(i), thb0[i]), i
        assert np.array_equal(c.return_carry, g0)


@pytest.mark.parametrize("domain,order", LOOP)
def test_zero_baseline_is_reinforce_and_the_baseline_never_moves(orc, domain, order):
    N, T = 32, 25
    kw = dict(domain=domain, order=order, n_envs=N, tau=0.7, max_episode_steps=19, gamma=0.97, alpha=0.02)
    rng = np.random.default_rng(order + 10 * domain)
    with ctx(algo=rsrl_amd.REINFORCE, **kw) as r, ctx(algo=rsrl_amd.BASELINE_REINFORCE, **kw) as b, \
            ctx(algo=rsrl_amd.BASELINE_REINFORCE, **kw) as bb:
        for c in (r, b, bb):
            c.reset()
            c.train(40)
        S, A, R, L = _ragged_batch(r, orc, domain, T, rng)
        for c in (r, b):
            c.handle_batch(S, A, R, L)
            c.train(30)
        for i in range(N):
            assert np.array_equal(r.get_policy_weights(i).view(np.uint32), b.get_policy_weights(i).view(np.uint32)), i
            assert np.array_equal(r.get_behaviour_weights(i).view(np.uint32), b.get_behaviour_weights(i).view(np.uint32)), i
        assert np.array_equal(r.return_carry.view(np.uint32), b.return_carry.view(np.uint32))
        Bs = [rng.normal(0.0, 0.5, size=(bb.F, bb.A)).astype(np.float32) for _ in range(N)]
        for i in range(N):
            bb.set_weights(Bs[i], i)
        bb.train(30)
        bb.handle_batch(S, A, R, L)
        bb.train(7)
        for i in range(N):
            assert np.array_equal(bb.get_weights(i).view(np.uint32), Bs[i].view(np.uint32)), i


@pytest.mark.parametrize("algo", ALGOS)
def test_driver_loop_against_a_restated_loop(orc, algo):
    N, K, cap, seed, gamma, alpha, tau, domain, order = 32, 50, 20, 31, 0.95, 0.002, 0.5, rsrl_amd.MOUNTAIN_CAR, 3
    rng = np.random.default_rng(8)
    with ctx(algo=algo, n_envs=N, seed=seed, gamma=gamma, alpha=alpha, tau=tau, max_episode_steps=cap) as c:
        B = None
        if algo == rsrl_amd.BASELINE_REINFORCE:
            B = [rng.normal(0.0, 0.5, size=(c.F, c.A)).astype(np.float32) for _ in range(N)]
            for i in range(N):
                c.set_weights(B[i], i)
        S0 = rand_states(orc, domain, N, rng)
        S0[0, : N // 2] = rng.uniform(0.40, 0.49, size=N // 2).astype(np.float32)     # half of them start next to the goal: terminals on the way
        S0[1, : N // 2] = rng.uniform(0.03, 0.07, size=N // 2).astype(np.float32)
        A0 = rng.integers(0, 3, size=N).astype(np.int32)
        c.states, c.actions = S0, A0
        dev_acts, episodes, truncated = [], 0, 0
        for _ in range(K):
            st = c.train(1)
            episodes += st["episodes"]; truncated += st["episodes_truncated"]
            dev_acts.append(c.actions)
        acts, Ts, Tbs, near = _restated_loop(orc, domain, order, N, K, cap, seed, gamma, alpha, tau, S0, A0,
                                             None if B is None else [b.astype(np.float64) for b in B])
        same = (np.array(dev_acts) == acts).all(axis=0)
        assert same.mean() >= 0.9, same
        assert (same & ~near).mean() >= 0.5
        for i in np.flatnonzero(same & ~near):
            for got, want in ((c.get_policy_weights(i), Ts[i]), (c.get_behaviour_weights(i), Tbs[i])):
                assert np.max(np.abs(got - want)) <= 3e-6 * (1 + np.max(np.abs(want))) * K * 16, i
        assert episodes > truncated > 0                               # terminals and caps both happened


def _host_trait_loop(c, K, cap):
    """domain_step -> append to host buffers -> handle_batch(the episodes that just ended) -> domain_reset(ended) -> policy_sample().  Returns
    the snapshot train is held to: theta at the loop's end is train's theta_b, theta after the still-open prefixes too is train's theta, and
    their g is train's return_carry"""
    N, D = c.N, c.D
    S, A, R = np.zeros((cap, D, N), np.float32), np.zeros((cap, N), np.int32), np.zeros((cap, N), np.float32)
    ep = c.episode_steps.astype(np.int64)
    cols = np.arange(N)
    for _ in range(K):
        acts = c.actions
        frm, nxt, rew, term = c.domain_step(acts)
        S[ep, :, cols] = frm.T
        A[ep, cols] = acts
        R[ep, cols] = rew
        ep += 1
        ended = term.astype(bool) | (ep >= cap)
        c.handle_batch(S, A, R, np.where(ended, ep, 0).astype(np.uint32))
        c.domain_reset(ended.astype(np.uint8))
        ep[ended] = 0
        c.policy_sample()
    c.episode_steps = ep.astype(np.uint32)
    theta_end = np.stack([c.get_policy_weights(i) for i in range(N)])
    ret = c.handle_batch(S, A, R, ep.astype(np.uint32), returns=True)
    g = np.where(ep > 0, ret[np.maximum(ep - 1, 0), cols], np.float32(0.0)).astype(np.float32)
    return dict(snapshot(c), theta_b=theta_end, return_carry=g)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("domain,order", LOOP)
def test_train_is_the_trait_loop_launch_depth_and_shard_invariant(domain, order, algo):
    N, K, cap = 64, 60, 23
    kw = dict(domain=domain, order=order, algo=algo, n_envs=N, max_episode_steps=cap, tau=0.7, alpha=0.02, gamma=0.97)
    rng = np.random.default_rng(3)
    Bs = [rng.normal(0.0, 0.5, size=((order + 1) ** (2 if domain == rsrl_amd.MOUNTAIN_CAR else 4), 2 if domain == rsrl_amd.CART_POLE else 3))
          .astype(np.float32) for _ in range(N)] if algo == rsrl_amd.BASELINE_REINFORCE else None

    def setup(c, off=0):
        if Bs is not None:
            for i in range(c.N):
                c.set_weights(Bs[off + i], i)
        c.reset()

    st, _ = check_train_invariance(ctx, kw, K, cap, depths=(1, 7), first_split=20, kernel="k_train_reinforce", setup=setup, trait=_host_trait_loop)
    assert st["episodes"] > 0


@pytest.mark.parametrize("algo", ALGOS)
def test_checkpoint_resumes_an_open_episode_bitwise(tmp_path, algo):
    kw = dict(algo=algo, n_envs=32, order=3, max_episode_steps=17, alpha=0.2, tau=0.5)
    path = os.path.join(str(tmp_path), "reinforce.ckpt")

    def an_episode_is_open(a):
        assert (a.return_carry != 0).any()

    check_checkpoint_resume(ctx, kw, path, 25, 20, carry=("states", "actions", "episode_steps"), at_save=an_episode_is_open)
    with open(path, "rb") as f:
        head = f.read(72)
    assert int.from_bytes(head[8:12], "little") == 9 and int.from_bytes(head[52:56], "little") == 7
    other_algo = rsrl_amd.BASELINE_REINFORCE if algo == rsrl_amd.REINFORCE else rsrl_amd.REINFORCE
    others = [dict(algo=other_algo, policy=rsrl_amd.SOFTMAX), dict(algo=rsrl_amd.ACTOR_CRITIC, policy=rsrl_amd.SOFTMAX),
              dict(algo=rsrl_amd.TD_ACTOR_CRITIC, policy=rsrl_amd.SOFTMAX)]
    others = [dict(kw, domain=rsrl_amd.MOUNTAIN_CAR, **other) for other in others]
    check_foreign_checkpoints_refused(ctx, kw, path, others, tmp_path)


def test_checksum_covers_theta():
    with ctx(n_envs=8) as c:
        c.reset()
        c.train(5)
        before = c.checksum()
        th = c.get_policy_weights(3)
        th[2, 1] += 0.25
        c.set_policy_weights(th, 3)
        assert c.checksum()[0] != before[0]
        assert c.checksum()[1] == before[1]


@pytest.mark.parametrize("algo", ALGOS)
def test_policy_side_reads_theta_and_reset_restarts(orc, algo):
    N, seed, tau, domain, order = 64, 23, 0.5, rsrl_amd.MOUNTAIN_CAR, 3
    rng = np.random.default_rng(4)
    with ctx(algo=algo, n_envs=N, seed=seed, tau=tau, order=order, max_episode_steps=40) as c:
        Ts = [rng.normal(0.0, 1.0, size=(c.F, c.A)).astype(np.float32) for _ in range(N)]
        for i in range(N):
            c.set_policy_weights(Ts[i], i)
        S = rand_states(orc, domain, N, rng)
        h = np.array([Ts[i].astype(np.float64).T @ orc.fourier_project(domain, order, S[:, i]) for i in range(N)]).T
        probs = c.policy_probs(S)
        want = np.array([orc.policy_probs(orc.SOFTMAX, h[:, i], tau=tau) for i in range(N)]).T
        assert np.max(np.abs(probs - want)) <= 2e-6                  # (preferences of up to ~5 at tau 0.5: fp32 exp)
        assert np.array_equal(c.policy_mode(S), [orc.argmax_first(probs[:, i], prec="f32") for i in range(N)])
        if algo == rsrl_amd.BASELINE_REINFORCE:
            Bs = [rng.normal(0.0, 1.0, size=(c.F, c.A)).astype(np.float32) for _ in range(N)]
            for i in range(N):
                c.set_weights(Bs[i], i)
            q = c.q_evaluate(S)
            qw = np.array([Bs[i].astype(np.float64).T @ orc.fourier_project(domain, order, S[:, i]) for i in range(N)]).T
            assert q.shape == (c.A, N) and np.allclose(q, qw, atol=2e-5, rtol=1e-5)
        c.return_carry = np.full(N, 3.0, np.float32)
        c.reset()                                                    # new episodes: theta_b <- theta, g <- 0, the initial sample from theta
        assert np.array_equal(c.return_carry, np.zeros(N, np.float32))
        phi0 = orc.fourier_project(domain, order, orc.domain_reset(domain, prec="f32"))
        acts = c.actions
        for i in range(N):
            assert np.array_equal(c.get_behaviour_weights(i), Ts[i]), i
            h0 = Ts[i].astype(np.float64).T @ phi0
            x = orc.draw(seed, i, 0, orc.BLK_INIT)
            if not near_boundary(orc.policy_probs(orc.SOFTMAX, h0, tau=tau), x):
                assert acts[i] == orc.policy_sample(orc.SOFTMAX, h0, x, tau=tau), i
        # domain_reset(mask) restarts exactly the masked learners' episodes
        th1 = c.get_policy_weights(1)
        c.set_policy_weights(th1 + 1.0, 1); c.set_policy_weights(th1 + 1.0, 0)
        c.return_carry = np.full(N, 2.0, np.float32)
        mask = np.zeros(N, np.uint8); mask[1] = 1
        c.domain_reset(mask)
        g = c.return_carry
        assert g[1] == 0.0 and (np.delete(g, 1) == 2.0).all()
        assert np.array_equal(c.get_behaviour_weights(1), th1 + 1.0) and np.array_equal(c.get_behaviour_weights(0), Ts[0])


def test_refusals():
    bad = [dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(order=7), dict(domain=rsrl_amd.CART_POLE, order=2),
           dict(weight_mode=rsrl_amd.W_SHARED), dict(domain=rsrl_amd.HIV_TREATMENT, order=1), dict(policy=rsrl_amd.EPSILON_GREEDY),
           dict(agent_policy=rsrl_amd.SOFTMAX), dict(epsilon_decay=0.99)]
    for algo, name in ((rsrl_amd.REINFORCE, "RSRL_REINFORCE"), (rsrl_amd.BASELINE_REINFORCE, "RSRL_BASELINE_REINFORCE")):
        for b in bad:
            with pytest.raises(RsrlHipError) as e:
                ctx(algo=algo, **b)
            assert e.value.code == EINVAL and name in str(e.value), b
    S = np.zeros((2, 4), np.float32)
    for algo in ALGOS:
        with ctx(algo=algo, n_envs=4) as c:
            calls = [lambda: c.handle(S, np.zeros(4, np.int32), np.zeros(4, np.float32), S, np.zeros(4, np.uint8)),
                     lambda: c.get_traces(0), lambda: c.get_td_weights(0)]
            if algo == rsrl_amd.REINFORCE:
                calls += [lambda: c.get_weights(0), lambda: c.set_weights(np.zeros((c.F, c.A)), 0), lambda: c.q_evaluate(S), lambda: c.q_find_max(S)]
            else:
                assert c.get_weights(0).shape == (c.F, c.A)
            for call in calls:
                with pytest.raises(RsrlHipError) as e:
                    call()
                assert e.value.code == ESTATE
            with pytest.raises(RsrlHipError) as e:
                c.handle_batch(np.zeros((2, 2, 4)), np.zeros((2, 4)), np.zeros((2, 4)), np.array([3, 0, 0, 0]))     # a length beyond T
            assert e.value.code == EINVAL
    for other in (dict(algo=rsrl_amd.ACTOR_CRITIC), dict(algo=rsrl_amd.TD_ACTOR_CRITIC), dict(algo=rsrl_amd.QLEARNING, policy=rsrl_amd.GREEDY)):
        with ctx(n_envs=4, **other) as c:
            for call in (lambda: c.handle_batch(np.zeros((1, 2, 4)), np.zeros((1, 4)), np.zeros((1, 4)), np.ones(4)), lambda: c.get_behaviour_weights(0),
                         lambda: c.set_behaviour_weights(np.zeros((c.F, c.A)), 0), lambda: c.return_carry):
                with pytest.raises(RsrlHipError) as e:
                    call()
                assert e.value.code == ESTATE


def test_reinforce_example_builds_and_runs(tmp_path):
    for baseline in ("0", "1"):
        out = run_example(tmp_path, "reinforce", [64, 3, 200, baseline])
        assert "Batch 3:" in out and "OOS:" in out
        tmax = float(out.split("max |theta| of learner 0:")[1].split()[0])
        assert np.isfinite(tmax) and tmax > 0.0
        assert "(48 weights)" in out
