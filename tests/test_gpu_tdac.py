"""ActorCritic with the TD(0) state-value critic (RSRL_TD_ACTOR_CRITIC, train_tdac.hip) on the device: handle against the f64 rule, the critic half
bit for bit a TD ctx's, the policy side reading theta and the value side reading w, the driver loop against a restated loop, train against the
trait-granular loop / launch depths / shards bit for bit, checkpoints, the checksum, the refusals and the C++ example."""
import os

import numpy as np
import pytest

import rsrl_amd
from rsrl_amd import RsrlHipError
from tests.ac_numpy import near_boundary
from tests.agent_contract import check_checkpoint_resume, check_foreign_checkpoints_refused, check_train_invariance, rand_states, run_example
from tests.tdac_numpy import tdac_restated_loop as _restated_loop, tdac_rule

pytestmark = pytest.mark.gpu

TDAC = rsrl_amd.TD_ACTOR_CRITIC
REG = [(rsrl_amd.MOUNTAIN_CAR, o) for o in (1, 2, 3, 4, 5)] + [(rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]
LOOP = [(rsrl_amd.MOUNTAIN_CAR, 3), (rsrl_amd.MOUNTAIN_CAR, 5), (rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]


def ctx(**kw):
    base = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=TDAC, policy=rsrl_amd.SOFTMAX, n_envs=32, seed=5, gamma=0.95, lr=0.05, alpha=0.3, tau=1.0)
    base.update(kw)
    return rsrl_amd.Context(**base)


def randomise(c, rng, scale=0.3):
    Ws = [rng.normal(0.0, scale, size=(c.F, 1)).astype(np.float32) for _ in range(c.N)]
    Ts = [rng.normal(0.0, scale, size=(c.F, c.A)).astype(np.float32) for _ in range(c.N)]
    for i in range(c.N):
        c.set_weights(Ws[i], i)
        c.set_policy_weights(Ts[i], i)
    return Ws, Ts


def _transitions(c, orc, domain, rng):
    N = c.N
    c.states = rand_states(orc, domain, N, rng)
    a = rng.integers(0, c.A, size=N).astype(np.int32)
    frm, nxt, rew, term = c.domain_step(a)
    term = (term | (rng.random(N) < 0.25)).astype(np.uint8)          # the critic reads V(s') of these: s' as domain_step reported it
    return frm, a, rew, nxt, term


@pytest.mark.parametrize("tau", [1.0, 0.5])
@pytest.mark.parametrize("domain,order", REG)
def test_handle_against_the_f64_rule(orc, domain, order, tau):
    N, lr, gamma, alpha = 64, 0.05, 0.95, 0.3
    rng = np.random.default_rng(domain * 100 + order * 10 + int(tau * 4))
    with ctx(domain=domain, order=order, tau=tau, n_envs=N, seed=17, lr=lr, gamma=gamma, alpha=alpha) as c:
        assert c.n_out == 1
        Ws, Ts = randomise(c, rng)
        frm, a, rew, nxt, term = _transitions(c, orc, domain, rng)
        assert 0 < term.sum() < N
        td = c.handle(frm, a, rew, nxt, term)
        for i in range(N):
            phi_s = orc.fourier_project(domain, order, frm[:, i])
            phi_n = orc.fourier_project(domain, order, nxt[:, i])
            w, Th = Ws[i].astype(np.float64), Ts[i].astype(np.float64)
            d, w2, T2 = tdac_rule(w, Th, phi_s, phi_n, int(a[i]), float(rew[i]), bool(term[i]), gamma, lr, alpha, tau)
            assert abs(td[i] - d) <= 2e-5 * (1 + abs(d)), (i, td[i], d)
            sphi = np.abs(phi_s).sum()
            for got, want, old in ((c.get_weights(i)[:, 0], w2, w[:, 0]), (c.get_policy_weights(i), T2, Th)):
                x_scale = np.max(np.abs(want - old))
                assert np.max(np.abs(got - want)) <= 3e-6 * (1 + x_scale) * sphi + 3e-6 * np.max(np.abs(old)), i


@pytest.mark.parametrize("domain,order", LOOP)
def test_the_critic_half_is_td0_bit_for_bit(orc, domain, order):
    N = 64
    kw = dict(domain=domain, order=order, n_envs=N, seed=3, lr=0.05, gamma=0.95)
    rng = np.random.default_rng(order * 7 + domain)
    with ctx(alpha=0.3, tau=0.7, **kw) as c, rsrl_amd.Context(algo=rsrl_amd.TD, policy=rsrl_amd.RANDOM, **kw) as v:
        Ws, _ = randomise(c, rng, scale=1.0)
        for i in range(N):
            v.set_weights(Ws[i], i)
        for _ in range(3):                                            # three rounds: theta moves, w must not notice
            frm, a, rew, nxt, term = _transitions(c, orc, domain, rng)
            td_ac = c.handle(frm, a, rew, nxt, term)
            td_v = v.handle(frm, a, rew, nxt, term)
            assert np.array_equal(td_ac.view(np.uint32), td_v.view(np.uint32))
            for i in range(N):
                assert np.array_equal(c.get_weights(i).view(np.uint32), v.get_weights(i).view(np.uint32)), i


def test_policy_side_reads_theta_value_side_reads_w(orc):
    N, seed, tau, domain, order = 64, 23, 0.5, rsrl_amd.MOUNTAIN_CAR, 3
    rng = np.random.default_rng(4)
    with ctx(n_envs=N, seed=seed, tau=tau, order=order, max_episode_steps=40) as c:
        Ws, Ts = randomise(c, rng, scale=1.0)
        S = rand_states(orc, domain, N, rng)
        phis = [orc.fourier_project(domain, order, S[:, i]) for i in range(N)]
        h = np.array([Ts[i].astype(np.float64).T @ phis[i] for i in range(N)]).T
        v = np.array([Ws[i].astype(np.float64)[:, 0] @ phis[i] for i in range(N)])
        probs = c.policy_probs(S)
        want = np.array([orc.policy_probs(orc.SOFTMAX, h[:, i], tau=tau) for i in range(N)]).T
        assert np.max(np.abs(probs - want)) <= 1e-6
        assert np.array_equal(c.policy_mode(S), [orc.argmax_first(probs[:, i], prec="f32") for i in range(N)])
        q = c.q_evaluate(S)
        assert q.shape == (1, N) and np.allclose(q[0], v, atol=2e-5, rtol=1e-5)
        for call in (lambda: c.q_find_max(S), lambda: c.q_find_min(S), lambda: c.q_expected_value(S, probs)):
            with pytest.raises(RsrlHipError) as e:
                call()
            assert e.value.code == -5
        sample = c.policy_sample(S)                                  # the first API call: BLK_API, call 0
        for i in range(N):
            x = orc.draw(seed, i, 0, orc.BLK_API)
            if not near_boundary(want[:, i], x):
                assert sample[i] == orc.policy_sample(orc.SOFTMAX, h[:, i], x, tau=tau), i
        c.reset()
        phi0 = orc.fourier_project(domain, order, orc.domain_reset(domain, prec="f32"))
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


def test_driver_loop_against_a_restated_loop(orc):
    N, K, cap, seed, gamma, lr, alpha, tau, domain, order = 32, 50, 20, 31, 0.95, 0.05, 0.002, 0.5, rsrl_amd.MOUNTAIN_CAR, 3
    rng = np.random.default_rng(8)
    with ctx(n_envs=N, seed=seed, gamma=gamma, lr=lr, alpha=alpha, tau=tau, max_episode_steps=cap) as c:
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
        acts, ws, Ts, near = _restated_loop(orc, domain, order, N, K, cap, seed, gamma, lr, alpha, tau, S0, A0)
        same = (np.array(dev_acts) == acts).all(axis=0)               # an fp32 rounding may flip a softmax draw: that learner leaves the comparison
        assert same.mean() >= 0.9, same
        assert (same & ~near).mean() >= 0.5
        for i in np.flatnonzero(same & ~near):
            for got, want in ((c.get_weights(i)[:, 0], ws[i]), (c.get_policy_weights(i), Ts[i])):
                assert np.max(np.abs(got - want)) <= 3e-6 * (1 + np.max(np.abs(want))) * K * 16, i
        assert episodes > truncated > 0                               # terminals and caps both happened


@pytest.mark.parametrize("domain,order", LOOP)
def test_train_is_the_trait_loop_launch_depth_and_shard_invariant(domain, order):
    N, K, cap = 64, 60, 23
    kw = dict(domain=domain, order=order, n_envs=N, max_episode_steps=cap, tau=0.7, lr=0.02, alpha=0.2, gamma=0.97)
    st, _ = check_train_invariance(ctx, kw, K, cap, depths=(1, 7), first_split=20, kernel="k_train_tdac")
    assert st["episodes"] > 0


def test_checkpoint_resumes_bitwise_and_refuses_other_agents(tmp_path):
    kw = dict(n_envs=32, order=3, max_episode_steps=17, lr=0.02, alpha=0.2, tau=0.5)
    path = os.path.join(str(tmp_path), "tdac.ckpt")
    check_checkpoint_resume(ctx, kw, path, 25, 20, carry=("states", "actions", "episode_steps"))
    with open(path, "rb") as f:
        head = f.read(72)
    assert int.from_bytes(head[8:12], "little") == 8 and int.from_bytes(head[40:44], "little") == 1 and int.from_bytes(head[52:56], "little") == 6
    others = [dict(algo=rsrl_amd.ACTOR_CRITIC, policy=rsrl_amd.SOFTMAX), dict(algo=rsrl_amd.Q_ACTOR_CRITIC, policy=rsrl_amd.SOFTMAX),
              dict(algo=rsrl_amd.TD, policy=rsrl_amd.RANDOM)]
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


def test_refusals():
    bad = [dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(order=7), dict(domain=rsrl_amd.CART_POLE, order=7), dict(domain=rsrl_amd.CART_POLE, order=2),
           dict(weight_mode=rsrl_amd.W_SHARED), dict(domain=rsrl_amd.CART_POLE, order=7, weight_dtype=rsrl_amd.W_BF16),
           dict(domain=rsrl_amd.HIV_TREATMENT, order=1), dict(policy=rsrl_amd.EPSILON_GREEDY), dict(policy=rsrl_amd.GREEDY),
           dict(agent_policy=rsrl_amd.SOFTMAX), dict(epsilon_decay=0.99)]
    for b in bad:
        with pytest.raises(RsrlHipError) as e:
            ctx(**b)
        assert e.value.code == -1 and "RSRL_TD_ACTOR_CRITIC" in str(e.value), b
    with ctx(n_envs=4) as c:
        for call in (lambda: c.get_traces(0), lambda: c.set_traces(np.zeros((c.F, 1)), 0), lambda: c.get_td_weights(0),
                     lambda: c.set_td_weights(np.zeros((c.F, c.A)), 0)):
            with pytest.raises(RsrlHipError) as e:
                call()
            assert e.value.code == -5


def test_tdac_example_builds_and_runs(tmp_path):
    out = run_example(tmp_path, "tdac", [64, 3, 200])
    assert "Batch 3:" in out and "OOS:" in out
    tail = out.split("max |w| of learner 0:")[1]
    wmax, tmax = float(tail.split()[0]), float(tail.split("max |theta| of learner 0:")[1].split()[0])
    assert np.isfinite(wmax) and wmax > 0.0 and np.isfinite(tmax) and tmax > 0.0
    assert "(16 weights)" in tail and "(48 weights)" in tail           # MountainCar, order 3: F = 16; V has one column, theta three
