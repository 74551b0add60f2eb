"""GTD2 and TDC (RSRL_GTD2, RSRL_TDC; train_gtd.hip) on the device: handle bit for bit against the f32 restatement and within the teacher-forcing
bounds of the f64 rule, TDC without its estimator against a TD ctx, the environment side against TD's, train against the trait-granular loop /
launch depths / shards bit for bit (the second column included), checkpoints, the value side reading theta, the refusals, the checksum, the C++
example and a slice of the random campaign (tests/fuzz_gtd.py)."""
import os

import numpy as np
import pytest

import rsrl_amd
from rsrl_amd import RsrlHipError
from tests import gtd_numpy as gn
from tests.agent_contract import check_checkpoint_resume, check_foreign_checkpoints_refused, check_train_invariance, rand_states, run_example
from tests.campaign import run_slice

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGENTS = [rsrl_amd.GTD2, rsrl_amd.TDC]
REG = [(rsrl_amd.MOUNTAIN_CAR, o) for o in (1, 2, 3, 4, 5)] + [(rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]
CONTRACT = [(rsrl_amd.MOUNTAIN_CAR, 5, 17), (rsrl_amd.CART_POLE, 1, 25), (rsrl_amd.ACROBOT, 1, 23)]
ESTATE = -5


def ctx(**kw):
    base = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=rsrl_amd.GTD2, policy=rsrl_amd.RANDOM, n_envs=32, seed=5, gamma=0.95, lr=0.02, lr_td=0.05)
    base.update(kw)
    return rsrl_amd.Context(**base)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def randomise(c, rng):
    """random non-zero theta and w, |.| <= 0.5, installed through set_weights / set_td_weights -> (theta, w), each (N, F)"""
    th = rng.uniform(-0.5, 0.5, size=(c.N, c.F)).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, size=(c.N, c.F)).astype(np.float32)
    for i in range(c.N):
        c.set_weights(th[i].reshape(c.F, 1), i)
        c.set_td_weights(w[i].reshape(c.F, 1), i)
    return th, w


def columns(c):
    return (np.stack([c.get_weights(i)[:, 0] for i in range(c.N)]), np.stack([c.get_td_weights(i)[:, 0] for i in range(c.N)]))


def _transitions(c, orc, domain, rng):
    c.states = rand_states(orc, domain, c.N, rng)
    frm, nxt, rew, term = c.domain_step(rng.integers(0, c.A, size=c.N).astype(np.int32))
    term = (term | (rng.random(c.N) < 0.25)).astype(np.uint8)          # s' as domain_step reported it, terminal and live rows mixed
    term[0], term[1] = 1, 0                                            # (both kinds among the first rows of the smallest batch)
    return frm, nxt, rew, term


@pytest.mark.parametrize("M", [67, 5])
@pytest.mark.parametrize("domain,order", REG)
@pytest.mark.parametrize("algo", AGENTS)
def test_handle_is_the_f32_restatement_bit_for_bit(orc, algo, domain, order, M):
    N, gamma, lr, lr_td = 67, 0.95, 0.02, 0.05
    rng = np.random.default_rng(1000 * algo + 100 * domain + 10 * order + M)
    with ctx(algo=algo, domain=domain, order=order, n_envs=N, seed=17, gamma=gamma, lr=lr, lr_td=lr_td) as c:
        assert c.n_out == 1 and c.get_td_weights(0).shape == (c.F, 1)
        th, w = randomise(c, rng)
        for call in range(3):
            frm, nxt, rew, term = _transitions(c, orc, domain, rng)
            assert 0 < term[:M].sum() < M
            td = c.handle(frm[:, :M], np.zeros(M, np.int32), rew[:M], nxt[:, :M], term[:M])
            want_td, th[:M], w[:M] = gn.rule_f32(algo, th[:M], w[:M], gn.project(orc, domain, order, frm[:, :M]), gn.project(orc, domain, order, nxt[:, :M]),
                                                 rew[:M], term[:M] != 0, gamma, lr, lr_td)
            g_th, g_w = columns(c)
            assert np.array_equal(bits(td), bits(want_td)), call
            assert np.array_equal(bits(g_th), bits(th)) and np.array_equal(bits(g_w), bits(w)), call      # (learners M .. N-1: untouched)
        assert np.isfinite(th).all() and np.isfinite(w).all()


@pytest.mark.parametrize("domain,order", REG)
@pytest.mark.parametrize("algo", AGENTS)
def test_handle_against_the_f64_rule_teacher_forced(orc, algo, domain, order):
    """64 transitions in a row, the device and the f64 rule each free-running on the same transitions from the same start: the project's
    teacher-forcing bounds -- TD error 2e-4, weights 1.4e-5 of max(1, |.|).  (The f32 numpy restatement stayed within 1.1e-5 and
    8.6e-7 of the f64 one at orders 3 and 5, |.| <= 5.5 throughout; tests/test_gtd_cpu.py repeats that at order 3.)"""
    N, K, gamma = 8, 64, 0.95
    lr, lr_td = (0.01, 0.02) if order >= 4 else (0.02, 0.05)
    rng = np.random.default_rng(2000 * algo + 100 * domain + 10 * order)
    with ctx(algo=algo, domain=domain, order=order, n_envs=N, seed=3, gamma=gamma, lr=lr, lr_td=lr_td) as c:
        th0, w0 = randomise(c, rng)
        th, w = th0.astype(np.float64), w0.astype(np.float64)
        worst_td = worst_w = biggest = 0.0
        for k in range(K):
            S, S2 = rand_states(orc, domain, N, rng), rand_states(orc, domain, N, rng)
            rew = np.full(N, -1.0, dtype=np.float32)
            term = (rng.random(N) < 0.1).astype(np.uint8)
            td = c.handle(S, np.zeros(N, np.int32), rew, S2, term)
            p_s, p_n = gn.project(orc, domain, order, S, "f64"), gn.project(orc, domain, order, S2, "f64")
            for i in range(N):
                d, th[i], w[i] = gn.rule_f64(algo, th[i], w[i], p_s[i], p_n[i], -1.0, bool(term[i]), gamma, lr, lr_td)
                worst_td = max(worst_td, abs(float(td[i]) - d))
        g_th, g_w = columns(c)
        for i in range(N):
            for got, want in ((g_th[i], th[i]), (g_w[i], w[i])):
                worst_w = max(worst_w, float(np.max(np.abs(got - want))) / max(1.0, float(np.max(np.abs(want)))))
                biggest = max(biggest, float(np.max(np.abs(want))))
        print("algo %d domain %d order %d: td %.3g, weights %.3g of max(1, |.|), max |.| %.3g" % (algo, domain, order, worst_td, worst_w, biggest))
        assert np.isfinite(biggest)
        assert worst_td <= 2e-4, worst_td
        assert worst_w <= 1.4e-5, worst_w


LOOP = [(rsrl_amd.MOUNTAIN_CAR, 3), (rsrl_amd.CART_POLE, 1)]      # (random actions end CartPole episodes often: the terminal path runs)


@pytest.mark.parametrize("domain,order", LOOP)
def test_tdc_without_its_estimator_is_td(domain, order):
    kw = dict(domain=domain, order=order, n_envs=64, seed=11, gamma=0.95, lr=0.02, max_episode_steps=37)
    with ctx(algo=rsrl_amd.TDC, lr_td=0.0, **kw) as c, rsrl_amd.Context(algo=rsrl_amd.TD, policy=rsrl_amd.RANDOM, **kw) as t:
        c.reset()
        t.reset()
        sc, st = c.train(200), t.train(200)
        th, w = columns(c)
        tw = np.stack([t.get_weights(i)[:, 0] for i in range(t.N)])
        assert np.isfinite(tw).all() and np.max(np.abs(tw)) > 0
        assert np.array_equal(th, tw)                                 # as values: a zero's sign is the second axpy's
        assert not w.any()
        for name in ("states", "actions", "episode_steps"):
            assert np.array_equal(getattr(c, name).view(np.uint32), getattr(t, name).view(np.uint32)), name
        assert sc == st, (sc, st)
        if domain == rsrl_amd.CART_POLE:
            assert sc["episodes"] > sc["episodes_truncated"]           # terminal transitions happened
        else:
            assert sc["episodes_truncated"] > 0


@pytest.mark.parametrize("domain,order", LOOP)
@pytest.mark.parametrize("algo", AGENTS)
def test_environment_side_is_tds(algo, domain, order):
    kw = dict(domain=domain, order=order, n_envs=64, seed=11, gamma=0.95, lr=0.02, max_episode_steps=37)
    with ctx(algo=algo, lr_td=0.05, **kw) as c, rsrl_amd.Context(algo=rsrl_amd.TD, policy=rsrl_amd.RANDOM, **kw) as t:
        c.reset()
        t.reset()
        sc, st = c.train(200), t.train(200)
        for name in ("states", "actions", "episode_steps"):
            assert np.array_equal(getattr(c, name).view(np.uint32), getattr(t, name).view(np.uint32)), name
        for name in ("env_steps", "episodes", "episodes_truncated", "sum_episode_steps", "sum_reward"):
            assert sc[name] == st[name], name
        th, w = columns(c)
        assert np.isfinite(th).all() and np.isfinite(w).all() and np.max(np.abs(th)) > 0 and np.max(np.abs(w)) > 0


class _Recording:
    """a ctx factory that keeps every ctx's second column (all learners, (N, F, 1)) as it stood when the ctx was closed: the contract harness's
    snapshot does not read fa_w, so each of its comparisons is repeated on these"""

    def __init__(self):
        self.w = []

    def __call__(self, **kw):
        c = ctx(**kw)
        close = c.close

        def recording_close():
            if getattr(c, "_h", None):
                self.w.append(np.stack([c.get_td_weights(i) for i in range(c.N)]))
            close()
        c.close = recording_close
        return c


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes() and bool(np.array_equal(a, b))


@pytest.mark.parametrize("domain,order,cap", CONTRACT)
@pytest.mark.parametrize("algo", AGENTS)
def test_train_is_the_trait_loop_launch_depth_and_shard_invariant(algo, domain, order, cap):
    N, K, depths = 80, 90, (1, 7, 0)
    kw = dict(algo=algo, domain=domain, order=order, n_envs=N, max_episode_steps=cap, lr=0.01, lr_td=0.02, gamma=0.97)
    make = _Recording()
    st, ref = check_train_invariance(make, kw, K, cap, depths=depths, first_split=30, kernel="k_train_gtd")
    assert st["episodes"] > 0 and st["env_steps"] == N * K and np.isfinite(ref["weights"]).all() and np.max(np.abs(ref["weights"])) > 0
    # the harness's ctxs in its order: train(K), the trait loop, one per depth, two shards
    assert len(make.w) == 2 + len(depths) + 2
    w_ref = make.w[0]
    assert np.isfinite(w_ref).all() and np.max(np.abs(w_ref)) > 0
    assert _same_bits(make.w[1], w_ref), "w: the host trait loop against train(%d)" % K
    for spl, w in zip(depths, make.w[2:2 + len(depths)]):
        assert _same_bits(w, w_ref), "w: the three-way split at steps_per_launch %d" % spl
    assert _same_bits(np.concatenate(make.w[-2:], axis=0), w_ref), "w: two env_offset shards joined"


@pytest.mark.parametrize("algo", AGENTS)
def test_checkpoint_resumes_bitwise_and_refuses_other_agents(algo, tmp_path):
    kw = dict(algo=algo, n_envs=32, order=3, max_episode_steps=17, lr=0.02, lr_td=0.05)
    path = os.path.join(str(tmp_path), "gtd.ckpt")

    def second_columns_equal(a, b):
        assert _same_bits(np.stack(columns(a)), np.stack(columns(b)))
    check_checkpoint_resume(ctx, kw, path, 25, 20, carry=("states", "actions", "episode_steps"), then=second_columns_equal)
    with open(path, "rb") as f:
        head = f.read(72)
    assert int.from_bytes(head[8:12], "little") == 10 and int.from_bytes(head[40:44], "little") == 1 and int.from_bytes(head[52:56], "little") == 13
    assert os.path.getsize(path) == 72 + 2 * 32 * 16 * 4                # theta, then w: f32[F][1] per learner each
    sibling = rsrl_amd.TDC if algo == rsrl_amd.GTD2 else rsrl_amd.GTD2
    others = [dict(algo=rsrl_amd.TD, policy=rsrl_amd.RANDOM), dict(algo=rsrl_amd.TD_LAMBDA, policy=rsrl_amd.RANDOM, lam=0.5),
              dict(algo=rsrl_amd.GREEDY_GQ, policy=rsrl_amd.EPSILON_GREEDY), dict(algo=sibling, policy=rsrl_amd.RANDOM)]
    others = [dict(kw, domain=rsrl_amd.MOUNTAIN_CAR, **other) for other in others]
    check_foreign_checkpoints_refused(ctx, kw, path, others, tmp_path)


@pytest.mark.parametrize("algo", AGENTS)
def test_value_side_reads_theta_and_the_other_sides_are_refused(orc, algo):
    N, domain, order = 16, rsrl_amd.MOUNTAIN_CAR, 3
    rng = np.random.default_rng(40 + algo)
    with ctx(algo=algo, n_envs=N, order=order) as c:
        th, w = randomise(c, rng)
        S = rand_states(orc, domain, N, rng)
        phi = gn.project(orc, domain, order, S, "f64")
        v_th, v_w = np.sum(th.astype(np.float64) * phi, axis=1), np.sum(w.astype(np.float64) * phi, axis=1)
        q = c.q_evaluate(S)
        assert q.shape == (1, N) and np.allclose(q[0], v_th, atol=2e-5, rtol=1e-5)
        assert np.min(np.abs(v_th - v_w)) > 1e-3                        # distinct columns: V is not read from w
        probs = np.full((c.A, N), 1.0 / c.A, dtype=np.float32)
        for call in (lambda: c.q_find_max(S), lambda: c.q_find_min(S), lambda: c.q_expected_value(S, probs), lambda: c.get_traces(0),
                     lambda: c.set_traces(np.zeros((c.F, 1)), 0), lambda: c.get_policy_weights(0), lambda: c.get_lstd_state(0),
                     lambda: c.handle_batch(np.zeros((1, c.D, N), np.float32), None, np.zeros((1, N), np.float32), np.ones(N, np.uint32)),
                     lambda: c.handle_transitions(np.zeros((1, c.D, N), np.float32), np.zeros((1, N), np.float32), np.zeros((1, c.D, N), np.float32),
                                                  np.zeros((1, N), np.uint8), np.ones(N, np.uint32))):
            with pytest.raises(RsrlHipError) as e:
                call()
            assert e.value.code == ESTATE
        g_th, g_w = columns(c)
        assert np.array_equal(bits(g_th), bits(th)) and np.array_equal(bits(g_w), bits(w))      # reset leaves both columns alone, and so did the refusals
        c.reset()
        g_th, g_w = columns(c)
        assert np.array_equal(bits(g_th), bits(th)) and np.array_equal(bits(g_w), bits(w))
    with rsrl_amd.Context(algo=rsrl_amd.TD, policy=rsrl_amd.RANDOM, order=3, n_envs=4) as t:
        for call in (lambda: t.get_td_weights(0), lambda: t.set_td_weights(np.zeros((t.F, t.A)), 0)):
            with pytest.raises(RsrlHipError) as e:
                call()
            assert e.value.code == ESTATE and "only GreedyGQ has a second approximator (fa_td)" in str(e.value)


def test_checksum_moves_when_only_w_changes():
    with ctx(algo=rsrl_amd.TDC, n_envs=8) as c:
        c.reset()
        c.train(5)
        before = c.checksum()
        w = c.get_td_weights(3)
        w[2, 0] += 0.25
        c.set_td_weights(w, 3)
        assert c.checksum()[0] != before[0]
        assert c.checksum()[1] == before[1]


def test_gtd2_example_builds_and_runs(tmp_path):
    for args, name in (([64, 3, 200], "GTD2"), ([64, 2, 150, 3, 50, 1], "TDC")):
        out = run_example(tmp_path, "gtd2", args)
        assert "Batch %d:" % args[1] in out and name + ": one transition handled" in out
        tail = out.split("max |theta| of learner 0:")[1]
        tmax, wmax = float(tail.split()[0]), float(tail.split("max |w| of learner 0:")[1].split()[0])
        assert np.isfinite(tmax) and tmax > 0.0 and np.isfinite(wmax) and wmax > 0.0
        assert tail.count("(16 weights)") == 2                          # MountainCar, order 3: F = 16, one column each


def test_random_configurations_of_the_gradient_td_agents():
    # tests/fuzz_gtd.py: GTD2 and TDC on every register-family order at random learner counts, env offsets up to the top of the id range, rates in
    # [0, 0.05], caps from 0 (none) and 1 (every step ends an episode) to 200, launch depths and horizons up to 60: handle on partial batches
    # against the f32 numpy rule bit for bit, train against its splits with read-only calls between them and against shards, the TD identity and the
    # environment side against RSRL_TD's.
    from tests.fuzz_gtd import SUITE_CASES, SUITE_SEED
    d = run_slice("fuzz_gtd.py", SUITE_CASES, SUITE_SEED)
    print(d["counts"], d["legs"])
    assert d["exit_code"] == 0 and not d["failures"], d["failures"][:3]
    assert d["counts"].get("refused", 0) == 0 and d["counts"].get("diverged", 0) == 0, d["counts"]
    for name in ("GTD2", "TDC"):
        assert d["per_agent"].get(name, {}).get("ok", 0) == SUITE_CASES // 2, d["per_agent"]
    assert d["legs"]["handle"] == SUITE_CASES and d["legs"]["identity"] == SUITE_CASES and d["legs"]["env"] == SUITE_CASES and d["legs"].get("shard", 0) >= 3, d["legs"]
