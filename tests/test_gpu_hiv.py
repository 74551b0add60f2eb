"""HIVTreatment on the device (train_hiv.hip): the f64 hidden state bit for bit against the numpy restatement of hiv.rs / ode.rs
(tests/hiv_numpy.py), the one-step agents against an f64 rule, the driver loop against the trait-granular loop, shards, checkpoints,
rollouts, the checksum and the configurations HIV refuses.  The numpy integration costs ~0.15 s per env-step: its horizons stay short."""
import os

import numpy as np
import pytest

import rsrl_amd
from rsrl_amd import RsrlHipError
from tests import hiv_numpy as hv
from tests.agent_contract import check_checkpoint_resume, check_train_invariance

pytestmark = pytest.mark.gpu

HIV = rsrl_amd.HIV_TREATMENT
LO, HI = [-5.0] * 6, [8.0] * 6


def ctx(**kw):
    base = dict(domain=HIV, order=1, n_envs=32, seed=7, gamma=0.9, lr=0.01, epsilon=0.1)
    base.update(kw)
    return rsrl_amd.Context(**base)


def ulps_f32(a, b):
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float64).astype(np.float32).astype(np.float64)
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
    return np.abs(a - b) / sp


def test_domain_step_is_the_reference_bitwise():
    N = 256
    rng = np.random.default_rng(3)
    y0 = np.tile(hv.DEFAULT.reshape(6, 1), (1, N))
    y0[:, N // 2:] = 10.0 ** rng.uniform(-7.0, 10.0, size=(6, N // 2))       # both clip limits
    with ctx(n_envs=N) as c:
        c.set_hidden_states(y0)
        assert hv.bits_equal(c.get_hidden_states(), y0)
        assert np.all(ulps_f32(c.states, hv.observe(y0)) <= 1)
        assert (c.states == 8.0).any() and (c.states == -5.0).any()
        y = y0
        for _ in range(20):
            a = rng.integers(0, 4, size=N).astype(np.int32)
            frm, nxt, rew, term = c.domain_step(a)
            y, obs, r = hv.step(y, a)
            assert hv.bits_equal(c.get_hidden_states(), y)
            assert np.all(ulps_f32(nxt, obs) <= 1) and np.array_equal(nxt, c.states)
            assert np.all(ulps_f32(rew, r) <= 1)
            assert not term.any()


def test_fourier_convention_pinned_on_cart_pole(orc):
    rng = np.random.default_rng(5)
    lo, hi = orc.domain_bounds(1)
    for order in (1, 2, 3):
        s = rng.uniform(lo, hi).astype(np.float32)
        assert np.allclose(hv.fourier(s.reshape(-1, 1), order, lo, hi)[:, 0], orc.fourier_project(1, order, s), atol=1e-12)


def _rule(orc, algo, W, phi_s, phi_n, a, r, gamma, alpha, eps, x_inner):
    """one-step agents' TD error and the error sent on, f64 (q_learning.rs, sarsa.rs, expected_sarsa.rs, pal.rs; never terminal)"""
    qs, qn = W.T @ phi_s, W.T @ phi_n
    if algo == rsrl_amd.QLEARNING:
        d = r + gamma * qn.max() - qs[a]
        return d, d
    if algo == rsrl_amd.SARSA:
        na = orc.policy_sample(orc.EGREEDY, qn, x_inner, eps=eps)
        d = r + gamma * qn[na] - qs[a]
        return d, d
    if algo == rsrl_amd.EXPECTED_SARSA:
        p = orc.policy_probs(orc.EGREEDY, qn, eps=eps)
        d = r + gamma * float(np.dot(qn, p)) - qs[a]
        return d, alpha * d
    ast, nast = orc.argmax_first(qs), orc.argmax_first(qn)
    td = r + gamma * qn[ast] - qs[a]
    d = max(td - alpha * (qs[ast] - qs[a]), td - alpha * (qn[nast] - qn[a]))
    return d, alpha * d


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("algo", [rsrl_amd.QLEARNING, rsrl_amd.SARSA, rsrl_amd.EXPECTED_SARSA, rsrl_amd.PAL])
def test_handle_against_the_f64_rule(orc, order, algo):
    N, lr, gamma, alpha, eps, seed = 8, 0.05, 0.9, 0.7, 0.2, 11
    rng = np.random.default_rng(order * 10 + algo)
    with ctx(n_envs=N, order=order, algo=algo, policy=rsrl_amd.EPSILON_GREEDY, epsilon=eps, lr=lr, gamma=gamma, alpha=alpha, seed=seed) as c:
        Ws = [rng.normal(0.0, 0.1, size=(c.F, 4)).astype(np.float32) for _ in range(N)]
        for i in range(N):
            c.set_weights(Ws[i], i)
        a = rng.integers(0, 4, size=N).astype(np.int32)
        frm, nxt, rew, term = c.domain_step(a)
        t = c.step_count
        td = c.handle(frm, a, rew, nxt, term)
        phi_s, phi_n = hv.fourier(frm, order, LO, HI), hv.fourier(nxt, order, LO, HI)
        assert np.allclose(c.project(frm), phi_s, atol=2e-5)
        for i in range(N):
            W = Ws[i].astype(np.float64)
            d, e = _rule(orc, algo, W, phi_s[:, i], phi_n[:, i], int(a[i]), float(rew[i]), gamma, alpha, eps, orc.draw(seed, i, t, orc.BLK_INNER))
            assert abs(td[i] - d) <= 2e-5 * (1 + abs(d)), (i, td[i], d)
            want = W[:, a[i]] + lr * e * phi_s[:, i]
            got = c.get_weights(i)[:, a[i]]
            assert np.max(np.abs(got - want)) <= 3e-6 * (1 + abs(d)) * max(1.0, np.abs(phi_s[:, i]).sum())


def test_driver_loop_against_a_restated_loop(orc):
    N, K, cap, seed, lr, gamma = 32, 30, 12, 21, 0.01, 0.9
    with ctx(n_envs=N, policy=rsrl_amd.RANDOM, max_episode_steps=cap, seed=seed, lr=lr, gamma=gamma) as c:
        c.reset()
        first, a, y, obs32, ep, W, n_trunc = hv.q_learning_random_loop(orc, LO, HI, 1, c.F, N, K, cap, seed, lr, gamma)
        assert np.array_equal(c.actions, first)
        st = c.train(K)
        assert np.array_equal(c.actions, a)
        assert hv.bits_equal(c.get_hidden_states(), y)
        assert np.all(ulps_f32(c.states, obs32) <= 1)
        assert np.array_equal(c.episode_steps, ep)
        for i in range(N):
            assert np.allclose(c.get_weights(i), W[i], atol=2e-5, rtol=1e-4), i
        assert st["episodes"] == n_trunc == st["episodes_truncated"] and st["env_steps"] == N * K


@pytest.mark.parametrize("policy", [rsrl_amd.EPSILON_GREEDY, rsrl_amd.SOFTMAX])
@pytest.mark.parametrize("algo", [rsrl_amd.SARSA, rsrl_amd.EXPECTED_SARSA])
def test_train_is_the_trait_loop_and_split_invariant(policy, algo):
    N, K, cap = 64, 200, 45
    kw = dict(n_envs=N, order=2, algo=algo, policy=policy, max_episode_steps=cap, epsilon=0.2, tau=0.5, lr=1e-3)
    check_train_invariance(ctx, kw, K, cap, depths=(7,), first_split=50)


def test_checkpoint_resumes_bitwise(tmp_path):
    kw = dict(n_envs=32, order=3, algo=rsrl_amd.QLEARNING, policy=rsrl_amd.EPSILON_GREEDY, max_episode_steps=17, lr=1e-4)
    path = os.path.join(str(tmp_path), "hiv.ckpt")
    check_checkpoint_resume(ctx, kw, path, 25, 20, carry=("states", "hidden", "actions", "episode_steps"))


def test_rollouts_from_a_fresh_default_env():
    L = 6
    with ctx(n_envs=16, order=2, policy=rsrl_amd.GREEDY, max_episode_steps=L - 1) as c:
        rng = np.random.default_rng(9)
        for i in range(c.N):
            c.set_weights(rng.normal(0.0, 0.1, size=(c.F, 4)).astype(np.float32), i)
        c.reset()
        c.train(3)
        tr = c.rollout_trajectory(0)             # step_limit 0: bounded by max_episode_steps
        ns, tot = c.rollout_greedy(L)
        assert np.array_equal(ns, tr["n_states"]) and np.array_equal(tot, tr["total_reward"])
        assert np.all(tr["n_states"] == L) and not tr["terminal"].any()
        c.domain_reset()
        assert np.array_equal(tr["states"][0], c.states)
        for k in range(L - 1):
            act = c.policy_mode(c.states)
            _, nxt, rew, _ = c.domain_step(act)
            assert np.array_equal(tr["actions"][k], act) and np.array_equal(tr["rewards"][k], rew)
            assert np.array_equal(tr["states"][k + 1], nxt)
        pol = c.rollout_policy(rsrl_amd.RANDOM, L)
        assert np.all(pol["n_states"] == L)


def test_checksum_covers_the_hidden_state():
    with ctx() as c:
        w0, s0 = c.checksum()
        y = c.get_hidden_states()
        y[5, 3] = np.nextafter(y[5, 3], np.inf)
        c.set_hidden_states(y)
        w1, s1 = c.checksum()
        assert w1 == w0 and s1 != s0
        assert c.state_bounds() is not None


@pytest.mark.parametrize("kw", [
    dict(basis=rsrl_amd.TILE_CODING), dict(order=4), dict(order=7),
    dict(algo=rsrl_amd.SARSA_LAMBDA), dict(algo=rsrl_amd.Q_LAMBDA), dict(algo=rsrl_amd.GREEDY_GQ), dict(algo=rsrl_amd.Q_SIGMA),
    dict(algo=rsrl_amd.TD, policy=rsrl_amd.RANDOM), dict(algo=rsrl_amd.TD_LAMBDA, policy=rsrl_amd.RANDOM),
    dict(weight_mode=rsrl_amd.W_SHARED), dict(weight_dtype=rsrl_amd.W_BF16), dict(policy=rsrl_amd.EPSILON_GREEDY, epsilon_decay=0.99),
])
def test_unsupported_combinations_are_einval(kw):
    with pytest.raises(RsrlHipError) as e:
        ctx(**kw)
    assert e.value.code == -1 and "HIVTreatment" in str(e.value)


def test_exchange_and_hidden_state_errors():
    with ctx() as c:
        for call in (lambda: c.peer_export(1), lambda: rsrl_amd.Context.group_create([c])):
            with pytest.raises(RsrlHipError) as e:
                call()
            assert e.value.code == -1
        lo, hi = c.state_bounds()
        assert np.all(np.asarray(lo) == -5.0) and np.all(np.asarray(hi) == 8.0)
        with pytest.raises(RsrlHipError) as e:
            c.states = np.full((6, c.N), 8.5, dtype=np.float32)
        assert e.value.code == -1
    with rsrl_amd.Context(n_envs=4) as mc:
        with pytest.raises(RsrlHipError) as e:
            mc.get_hidden_states()
        assert e.value.code == -1 and "hidden state" in str(e.value)
