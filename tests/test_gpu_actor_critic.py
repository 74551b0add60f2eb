"""ActorCritic (control/ac.rs) with the Gibbs actor and the SARSA critic of examples/a2c.rs on the device (train_ac.hip): handle against an f64
restatement of the rule, the policy side reading theta and the value side reading W, the driver loop against a restated loop, train against the
trait-granular loop / launch depths / shards bit for bit, checkpoints, the checksum, the refusals and the C++ example."""
import os

import numpy as np
import pytest

import rsrl_amd
from rsrl_amd import RsrlHipError
from tests.ac_numpy import ac_restated_loop as _restated_loop, ac_rule, near_boundary
from tests.agent_contract import check_checkpoint_resume, check_foreign_checkpoints_refused, check_train_invariance, rand_states, run_example

pytestmark = pytest.mark.gpu

AC, QAC = rsrl_amd.ACTOR_CRITIC, rsrl_amd.Q_ACTOR_CRITIC
REG = [(rsrl_amd.MOUNTAIN_CAR, o) for o in (1, 2, 3, 4, 5)] + [(rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]


def ctx(**kw):
    base = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=AC, policy=rsrl_amd.SOFTMAX, n_envs=32, seed=5, gamma=0.95, lr=0.05, alpha=0.3, tau=1.0)
    base.update(kw)
    return rsrl_amd.Context(**base)


def randomise(c, rng, scale=0.3):
    Ws = [rng.normal(0.0, scale, size=(c.F, c.A)).astype(np.float32) for _ in range(c.N)]
    Ts = [rng.normal(0.0, scale, size=(c.F, c.A)).astype(np.float32) for _ in range(c.N)]
    for i in range(c.N):
        c.set_weights(Ws[i], i)
        c.set_policy_weights(Ts[i], i)
    return Ws, Ts


@pytest.mark.parametrize("tau", [1.0, 0.5])
@pytest.mark.parametrize("algo", [AC, QAC])
@pytest.mark.parametrize("domain,order", REG)
def test_handle_against_the_f64_rule(orc, domain, order, algo, tau):
    N, seed, lr, gamma, alpha = 64, 17, 0.05, 0.95, 0.3
    rng = np.random.default_rng(domain * 100 + order * 10 + algo + int(tau * 4))
    with ctx(domain=domain, order=order, algo=algo, tau=tau, n_envs=N, seed=seed, lr=lr, gamma=gamma, alpha=alpha) as c:
        Ws, Ts = randomise(c, rng)
        c.states = rand_states(orc, domain, N, rng)
        a = rng.integers(0, c.A, size=N).astype(np.int32)
        frm, nxt, rew, term = c.domain_step(a)
        term = (term | (rng.random(N) < 0.25)).astype(np.uint8)        # terminal transitions take no inner draw
        t = c.step_count
        td = c.handle(frm, a, rew, nxt, term)
        checked = 0
        for i in range(N):
            phi_s = orc.fourier_project(domain, order, frm[:, i])
            phi_n = orc.fourier_project(domain, order, nxt[:, i])
            x = orc.draw(seed, i, t, orc.BLK_INNER)
            W, Th = Ws[i].astype(np.float64), Ts[i].astype(np.float64)
            if not term[i] and near_boundary(orc.policy_probs(orc.SOFTMAX, Th.T @ phi_n, tau=tau), x):
                continue
            d, W2, T2 = ac_rule(orc, algo == QAC, W, Th, phi_s, phi_n, int(a[i]), float(rew[i]), bool(term[i]), gamma, lr, alpha, tau, x)
            assert abs(td[i] - d) <= 2e-5 * (1 + abs(d)), (i, td[i], d)
            sphi = np.abs(phi_s).sum()
            for got, want, old in ((c.get_weights(i), W2, W), (c.get_policy_weights(i), T2, Th)):
                x_scale = np.max(np.abs(want - old))
                assert np.max(np.abs(got - want)) <= 3e-6 * (1 + x_scale) * sphi + 3e-6 * np.max(np.abs(old)), i
            checked += 1
        assert checked >= N * 3 // 4


def test_policy_side_reads_theta_value_side_reads_w(orc):
    N, seed, tau, domain, order = 64, 23, 0.5, rsrl_amd.MOUNTAIN_CAR, 3
    rng = np.random.default_rng(4)
    with ctx(n_envs=N, seed=seed, tau=tau, order=order, max_episode_steps=40) as c:
        Ws, Ts = randomise(c, rng, scale=1.0)
        S = rand_states(orc, domain, N, rng)
        phis = [orc.fourier_project(domain, order, S[:, i]) for i in range(N)]
        h = np.array([Ts[i].astype(np.float64).T @ phis[i] for i in range(N)]).T
        q = np.array([Ws[i].astype(np.float64).T @ phis[i] for i in range(N)]).T
        probs = c.policy_probs(S)
        want = np.array([orc.policy_probs(orc.SOFTMAX, h[:, i], tau=tau) for i in range(N)]).T
        assert np.max(np.abs(probs - want)) <= 1e-6
        mode = c.policy_mode(S)
        assert np.array_equal(mode, [orc.argmax_first(probs[:, i], prec="f32") for i in range(N)])
        assert (mode != q.argmax(axis=0)).any()                     # the actor's mode is not Q's greedy action
        assert np.allclose(c.q_evaluate(S), q, atol=2e-5, rtol=1e-5)
        sample = c.policy_sample(S)                                  # the first API call: BLK_API, call 0
        for i in range(N):
            x = orc.draw(seed, i, 0, orc.BLK_API)
            if not near_boundary(want[:, i], x):
                assert sample[i] == orc.policy_sample(orc.SOFTMAX, h[:, i], x, tau=tau), i
        c.reset()
        s0 = orc.domain_reset(domain, prec="f32")
        phi0 = orc.fourier_project(domain, order, s0)
        acts = c.actions
        for i in range(N):
            h0 = Ts[i].astype(np.float64).T @ phi0
            x = orc.draw(seed, i, 0, orc.BLK_INIT)
            if not near_boundary(orc.policy_probs(orc.SOFTMAX, h0, tau=tau), x):
                assert acts[i] == orc.policy_sample(orc.SOFTMAX, h0, x, tau=tau), i
        # rollout_greedy = Domain::rollout(|s| policy.mode(s)): a host loop of domain_step + policy_mode through the same ctx
        L = 30
        n_states, total = c.rollout_greedy(L)
        c.domain_reset()
        tot = np.zeros(N, dtype=np.float32)
        steps = np.zeros(N, dtype=np.int64)
        done = np.zeros(N, dtype=bool)
        for _ in range(L - 1):
            frm, nxt, rew, term = c.domain_step(c.policy_mode(c.states))
            live = ~done
            tot[live] = (tot[live] + rew[live]).astype(np.float32)
            steps[live] += 1
            done |= term.astype(bool)
        assert np.array_equal(n_states, steps + 1)
        assert np.array_equal(total, tot)


@pytest.mark.parametrize("algo", [AC, QAC])
def test_driver_loop_against_a_restated_loop(orc, algo):
    # alpha stays small (a2c.rs uses 0.001): QCritic's actor feeds theta's rounding back through p with a gain of about alpha |Q| |phi|^2 / tau
    # per step, and above 1 the f32 and f64 runs part geometrically whatever the kernel does
    N, K, cap, seed, gamma, lr, alpha, tau, domain, order = 32, 50, 20, 31, 0.95, 0.05, 0.002, 0.5, rsrl_amd.MOUNTAIN_CAR, 3
    rng = np.random.default_rng(8)
    with ctx(n_envs=N, algo=algo, seed=seed, gamma=gamma, lr=lr, alpha=alpha, tau=tau, max_episode_steps=cap) as c:
        S0 = rand_states(orc, domain, N, rng)
        S0[0, : N // 2] = rng.uniform(0.40, 0.49, size=N // 2).astype(np.float32)     # half of them start next to the goal: terminals on the way
        S0[1, : N // 2] = rng.uniform(0.03, 0.07, size=N // 2).astype(np.float32)
        A0 = rng.integers(0, 3, size=N).astype(np.int32)
        c.states, c.actions = S0, A0
        dev_acts, episodes, truncated = [], 0, 0
        for _ in range(K):                                            # one batch-step per call: the same bits as train(K), every action seen
            st = c.train(1)
            episodes += st["episodes"]; truncated += st["episodes_truncated"]
            dev_acts.append(c.actions)
        acts, Ws, Ts, near = _restated_loop(orc, algo == QAC, domain, order, N, K, cap, seed, gamma, lr, alpha, tau, S0, A0)
        same = (np.array(dev_acts) == acts).all(axis=0)               # an fp32 rounding may flip a softmax draw: that learner leaves the comparison
        assert same.mean() >= 0.9, same
        assert (same & ~near).mean() >= 0.5
        for i in np.flatnonzero(same & ~near):
            for got, want in ((c.get_weights(i), Ws[i]), (c.get_policy_weights(i), Ts[i])):
                assert np.max(np.abs(got - want)) <= 3e-6 * (1 + np.max(np.abs(want))) * K * 16, i
        assert episodes > truncated > 0                               # terminals and caps both happened


@pytest.mark.parametrize("algo", [AC, QAC])
@pytest.mark.parametrize("domain,order", [(rsrl_amd.MOUNTAIN_CAR, 3), (rsrl_amd.MOUNTAIN_CAR, 5), (rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)])
def test_train_is_the_trait_loop_launch_depth_and_shard_invariant(domain, order, algo):
    N, K, cap = 64, 60, 23
    kw = dict(domain=domain, order=order, algo=algo, n_envs=N, max_episode_steps=cap, tau=0.7, lr=0.02, alpha=0.2, gamma=0.97)
    st, _ = check_train_invariance(ctx, kw, K, cap, depths=(1, 7), first_split=20)
    assert st["episodes"] > 0


def test_checkpoint_resumes_bitwise_and_refuses_other_agents(tmp_path):
    kw = dict(n_envs=32, order=3, max_episode_steps=17, lr=0.02, alpha=0.2, tau=0.5)
    path = os.path.join(str(tmp_path), "ac.ckpt")
    check_checkpoint_resume(ctx, kw, path, 25, 20, carry=("states", "actions", "episode_steps"))
    others = [dict(algo=rsrl_amd.SARSA), dict(algo=rsrl_amd.GREEDY_GQ, lr_td=0.01), dict(algo=QAC)]
    others = [dict(kw, domain=rsrl_amd.MOUNTAIN_CAR, policy=rsrl_amd.SOFTMAX, **other) for other in others]
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


def test_refusals():
    bad = [dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(order=7), dict(domain=rsrl_amd.CART_POLE, order=7), dict(domain=rsrl_amd.CART_POLE, order=2),
           dict(weight_mode=rsrl_amd.W_SHARED), dict(domain=rsrl_amd.CART_POLE, order=7, weight_dtype=rsrl_amd.W_BF16),
           dict(domain=rsrl_amd.HIV_TREATMENT, order=1), dict(policy=rsrl_amd.EPSILON_GREEDY), dict(policy=rsrl_amd.GREEDY),
           dict(agent_policy=rsrl_amd.SOFTMAX), dict(epsilon_decay=0.99)]
    for algo in (AC, QAC):
        for b in bad:
            with pytest.raises(RsrlHipError) as e:
                ctx(algo=algo, **b)
            assert e.value.code == -1 and "ActorCritic supports" in str(e.value), b
    with ctx(n_envs=4) as c:
        for call in (lambda: c.get_traces(0), lambda: c.set_traces(np.zeros((c.F, c.A)), 0), lambda: c.get_td_weights(0),
                     lambda: c.set_td_weights(np.zeros((c.F, c.A)), 0)):
            with pytest.raises(RsrlHipError) as e:
                call()
            assert e.value.code == -5
    for algo in (rsrl_amd.SARSA, rsrl_amd.GREEDY_GQ, rsrl_amd.SARSA_LAMBDA):
        with ctx(algo=algo, n_envs=4) as c:
            for call in (lambda: c.get_policy_weights(0), lambda: c.set_policy_weights(np.zeros((c.F, c.A)), 0)):
                with pytest.raises(RsrlHipError) as e:
                    call()
                assert e.value.code == -5


def test_a2c_example_builds_and_runs(tmp_path):
    out = run_example(tmp_path, "a2c", [64, 3, 200])
    assert "Batch 3:" in out and "OOS:" in out
    tmax = float(out.split("max |theta| of learner 0:")[1].split()[0])
    assert np.isfinite(tmax) and tmax > 0.0
