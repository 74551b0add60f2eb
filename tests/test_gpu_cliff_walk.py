"""CliffWalk over the tabular Q on the device (train_table.hip) against its float32 restatement (tests/table_numpy.py) bit for bit -- the domain
step on every (cell, action) pair, handle for the four one-step agents, the driver loop under every policy from zero and from random tables, with
the statistics --, against the f64 rule within the project's bars, the LDS loop against the memory loop (RSRL_TABLE_MEM), the driver loop against
the trait loop / split calls / shards, rollouts, the value and policy queries, checkpoints and the C++ example.

N = 131 unless said otherwise: two full waves and three lanes of a third.

test_handle_bitwise_and_against_the_f64_rule: the bar on the moved entry, 1e-6 (1 + lr |delta|), is held against the f64 rule applied to the float32
table; the test prints the worst ratio of each case before it asserts (run with -s).  Measured on an MI355X over the eight cases: the TD error
within 0.019 of its bar, the moved entry within 0.50 of its bar, no case skipped."""
import os

import numpy as np
import pytest

import rsrl_amd
from tests import table_numpy as tn
from tests.ac_numpy import near_boundary
from tests.agent_contract import check_checkpoint_resume, check_foreign_checkpoints_refused, check_train_invariance, run_example

pytestmark = pytest.mark.gpu

N = 131
ALGOS = [rsrl_amd.QLEARNING, rsrl_amd.SARSA, rsrl_amd.EXPECTED_SARSA, rsrl_amd.PAL]
POLICIES = [rsrl_amd.GREEDY, rsrl_amd.EPSILON_GREEDY, rsrl_amd.SOFTMAX, rsrl_amd.RANDOM]
SEED, GAMMA, LR, ALPHA, EPS, TAU = 7, 0.9, 0.5, 0.7, 0.2, 4.0


def ctx(**kw):
    base = dict(domain=rsrl_amd.CLIFF_WALK, basis=rsrl_amd.TABLE, n_envs=N, seed=SEED, gamma=GAMMA, lr=LR, alpha=ALPHA, epsilon=EPS, tau=TAU)
    base.update(kw)
    return rsrl_amd.Context(**base)


def random_tables(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.normal(0.0, 10.0, size=(tn.CELLS, tn.A)).astype(np.float32) for _ in range(n)]


def install(c, tables):
    for i, q in enumerate(tables):
        c.set_weights(q, i)


def tables_of(c):
    return [c.get_weights(i) for i in range(c.N)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def test_domain_step_on_every_cell_and_action():
    cells = [(x, y) for x in range(tn.WIDTH) for y in range(tn.HEIGHT)]
    pairs = [(x, y, a) for (x, y) in cells for a in range(4)]
    with ctx(n_envs=len(pairs)) as c:
        assert c.D == 2 and c.A == 4 and c.F == 60 and c.get_weights(0).shape == (60, 4) and not c.get_weights(5).any()
        lo, hi = c.state_bounds()
        assert list(lo) == [0.0, 0.0] and list(hi) == [11.0, 4.0]
        assert not c.states.any() and not c.episode_steps.any()
        s = np.array([[p[0] for p in pairs], [p[1] for p in pairs]], dtype=np.float32)
        a = np.array([p[2] for p in pairs], dtype=np.int32)
        c.states = s
        frm, nxt, rew, term = c.domain_step(a)
        want = [tn.step(*p) for p in pairs]
        assert np.array_equal(frm, s) and np.array_equal(nxt, c.states)
        assert np.array_equal(nxt, np.array([[w[0] for w in want], [w[1] for w in want]], dtype=np.float32))
        assert same_bits(rew, np.array([w[2] for w in want], dtype=np.float32)) and np.array_equal(term, np.array([w[3] for w in want], dtype=np.uint8))
        assert term.sum() == sum(w[3] for w in want) > 0 and (rew == 50.0).any() and (rew == -50.0).any()
        c.reset()
        assert not c.states.any() and not c.episode_steps.any()
        # garbage through the query calls reads the documented row: row r of the table holds 4 r + a
        c.set_weights_all(np.arange(240, dtype=np.float32).reshape(60, 4))
        g = np.array([[np.nan, 2.75, -5.0, 100.0, 1e30, np.inf, -np.inf, 11.0, 10.999, 0.5, -0.0, 3.0],
                      [1.0, np.nan, 4.5, -1.0, 3.999, 2.0, np.inf, 4.0, 1e-30, -np.inf, 7.0, np.nan]], dtype=np.float32)
        q = c.q_evaluate(g)
        for j in range(g.shape[1]):
            r = tn.row_of_state(g[:, j])
            assert list(q[:, j]) == [4.0 * r + b for b in range(4)], (j, g[:, j], r, q[:, j])
        assert tn.row_of_state(g[:, 0]) == 1 and tn.row_of_state(g[:, 3]) == 55 and tn.row_of_state(g[:, 7]) == 59


@pytest.mark.parametrize("policy", [rsrl_amd.EPSILON_GREEDY, rsrl_amd.SOFTMAX])
@pytest.mark.parametrize("algo", ALGOS)
def test_handle_bitwise_and_against_the_f64_rule(orc, algo, policy):
    rng = np.random.default_rng(100 + 10 * algo + policy)
    Q0 = random_tables(N, 200 + 10 * algo + policy)
    frm = np.stack([rng.integers(0, 12, N), rng.integers(0, 5, N)]).astype(np.float32)
    to = np.stack([rng.integers(0, 12, N), rng.integers(0, 5, N)]).astype(np.float32)
    a = rng.integers(0, 4, N).astype(np.int32)
    rew = rng.choice(np.array([-50.0, 0.0, 0.0, 50.0], dtype=np.float32), N)      # the domain's rewards
    term = (rng.random(N) < 0.25).astype(np.uint8)                                # a quarter forced terminal
    apol = tn.Pol(policy, EPS, TAU)
    with ctx(algo=algo, policy=policy) as c:
        install(c, Q0)
        t = c.step_count
        td = c.handle(frm, a, rew, to, term)
        got = tables_of(c)
    checked, worst_d, worst_w = 0, 0.0, 0.0
    for i in range(N):
        rs, rn = tn.row_of_state(frm[:, i]), tn.row_of_state(to[:, i])
        xin = orc.draw(SEED, i, t, orc.BLK_INNER)
        Q = Q0[i].copy()
        d32 = tn.handle32(orc, algo, apol, Q, rs, int(a[i]), rn, rew[i], bool(term[i]), GAMMA, LR, ALPHA, xin)
        assert same_bits(td[i], d32) and same_bits(got[i], Q), (i, td[i], d32)
        moved = np.argwhere(bits(Q) != bits(Q0[i]))
        assert all(tuple(m) == (rs, int(a[i])) for m in moved)
        # against the f64 rule; a SARSA / Softmax inner draw next to a cumulative-probability boundary may pick the neighbour in float32
        if algo == rsrl_amd.SARSA and policy == rsrl_amd.SOFTMAX and not term[i] and near_boundary(orc.policy_probs(orc.SOFTMAX, Q0[i][rn], tau=TAU), xin):
            continue
        checked += 1
        d64, e64 = tn.rule64(orc, algo, apol, Q0[i][rs], Q0[i][rn], int(a[i]), float(rew[i]), bool(term[i]), GAMMA, ALPHA, xin)
        qmax = float(np.abs(Q0[i]).max())
        worst_d = max(worst_d, abs(float(td[i]) - d64) / (1e-5 * (1.0 + qmax)))
        worst_w = max(worst_w, abs(float(got[i][rs, a[i]]) - (float(Q0[i][rs, a[i]]) + LR * e64)) / (1e-6 * (1.0 + LR * abs(d64))))
    print("algo %d policy %d: checked %d of %d; |d delta| / bar <= %.3f, |d entry| / bar <= %.3f" % (algo, policy, checked, N, worst_d, worst_w))
    assert 4 * checked >= 3 * N
    assert worst_d <= 1.0 and worst_w <= 1.0, (worst_d, worst_w)


_REF = {}


def restated(orc, algo, policy, init, K=60, cap=20):
    """the float32 loop of one case, computed once and shared (never modified)"""
    key = (algo, policy, init, K, cap)
    if key not in _REF:
        Q0 = None if init == "zero" else random_tables(N, 300 + 10 * algo + policy)
        pol = tn.Pol(policy, EPS, TAU)
        _REF[key] = (Q0, tn.loop32(orc, algo, pol, pol, N, K, cap, SEED, GAMMA, LR, ALPHA, Q0=Q0))
    return _REF[key]


def run_train(algo, policy, Q0, K=60, cap=20):
    with ctx(algo=algo, policy=policy, max_episode_steps=cap) as c:
        if Q0 is not None:
            install(c, Q0)
        c.reset()
        first = c.actions
        st = c.train(K)
        return dict(first=first, stats=st, states=c.states, actions=c.actions, episode_steps=c.episode_steps, tables=tables_of(c), checksum=c.checksum())


@pytest.mark.parametrize("init", ["zero", "random"])
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("algo", ALGOS)
def test_driver_loop_is_the_restated_loop_bitwise(orc, algo, policy, init):
    Q0, want = restated(orc, algo, policy, init)
    got = run_train(algo, policy, Q0)
    assert np.array_equal(got["first"], want["first"])
    assert np.array_equal(got["states"], want["states"]) and np.array_equal(got["actions"], want["actions"])
    assert np.array_equal(got["episode_steps"], want["episode_steps"])
    for i in range(N):
        assert same_bits(got["tables"][i], want["tables"][i]), i
    for name, v in want["stats"].items():
        assert got["stats"][name] == v, (name, got["stats"][name], v)
    assert got["stats"]["episodes"] > 0 and got["stats"]["episodes_truncated"] > 0


@pytest.mark.parametrize("algo", [rsrl_amd.SARSA, rsrl_amd.EXPECTED_SARSA])
def test_an_agent_policy_of_its_own(orc, algo):
    # the agent's Softmax(2) next to the behaviour's EpsilonGreedy: SARSA's inner draw and ExpectedSARSA's expectation read the agent's
    Q0 = random_tables(N, 77)
    want = tn.loop32(orc, algo, tn.Pol(rsrl_amd.EPSILON_GREEDY, EPS, TAU), tn.Pol(rsrl_amd.SOFTMAX, EPS, 2.0), N, 45, 20, SEED, GAMMA, LR, ALPHA, Q0=Q0)
    with ctx(algo=algo, policy=rsrl_amd.EPSILON_GREEDY, agent_policy=rsrl_amd.SOFTMAX, agent_tau=2.0, max_episode_steps=20) as c:
        install(c, Q0)
        c.reset()
        c.train(13)                      # (the memory loop: fewer than 16 batch-steps in the launch)
        c.train(32)                      # (the LDS loop)
        assert np.array_equal(c.states, want["states"]) and np.array_equal(c.actions, want["actions"])
        assert all(same_bits(c.get_weights(i), want["tables"][i]) for i in range(N))


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("algo", ALGOS)
def test_the_lds_loop_and_the_memory_loop_leave_the_same_bits(monkeypatch, algo, policy):
    for init in ("zero", "random"):
        Q0 = None if init == "zero" else random_tables(N, 300 + 10 * algo + policy)
        runs, names = [], []
        for mem in ("1", "0"):
            monkeypatch.setenv("RSRL_TABLE_MEM", mem)
            with ctx(algo=algo, policy=policy, max_episode_steps=20) as c:
                if Q0 is not None:
                    install(c, Q0)
                c.reset()
                c.timing_enable(True)
                c.train(60)
                names.append(c.timing_read()[2])
                runs.append(dict(checksum=c.checksum(), states=c.states, actions=c.actions, tables=tables_of(c)))
        assert names == ["k_table_train_mem", "k_table_train_lds"], names
        assert runs[0]["checksum"] == runs[1]["checksum"] and np.array_equal(runs[0]["states"], runs[1]["states"])
        assert np.array_equal(runs[0]["actions"], runs[1]["actions"])
        assert all(same_bits(x, y) for x, y in zip(runs[0]["tables"], runs[1]["tables"]))


@pytest.mark.parametrize("policy", [rsrl_amd.EPSILON_GREEDY, rsrl_amd.SOFTMAX])
@pytest.mark.parametrize("algo", ALGOS)
def test_train_is_the_trait_loop_split_and_shard_invariant(algo, policy):
    # N even for the two shards: 130 = two full waves and two lanes
    kw = dict(n_envs=130, algo=algo, policy=policy, max_episode_steps=11)
    check_train_invariance(ctx, kw, 40, 11, depths=(1, 7, 0), first_split=13)


def test_rollouts(orc):
    L = 30
    Q0 = random_tables(N, 41)
    # some learners walk the 13-step path along the edge: North at the start, East along row 1, South at the last column
    for i in range(0, N, 3):
        Q0[i][tn.row(0, 0), 0] = 100.0
        for x in range(11):
            Q0[i][tn.row(x, 1), 1] = 100.0
        Q0[i][tn.row(11, 1), 2] = 100.0
    with ctx(policy=rsrl_amd.GREEDY, max_episode_steps=L - 1) as c:
        install(c, Q0)
        ns, tot = c.rollout_greedy(L)
        tr = c.rollout_trajectory(L)
        assert np.array_equal(ns, tr["n_states"]) and same_bits(tot, tr["total_reward"])
        for i in range(N):
            n, t32, cells = tn.rollout32(orc, tn.Pol(orc.GREEDY), Q0[i], L)
            assert ns[i] == n and same_bits(tot[i], t32), (i, ns[i], n)
            assert [tuple(int(v) for v in tr["states"][k, :, i]) for k in range(n)] == cells
        assert (ns[::3] == 14).all() and (tot[::3] == 50.0).all() and tr["terminal"][::3].all()
        # the same trajectory as a host loop of domain_step + policy_mode through the same ctx
        c.domain_reset()
        alive = np.ones(N, dtype=bool)
        steps = np.zeros(N, dtype=np.int64)
        for k in range(L - 1):
            act = c.policy_mode(c.states)
            _, nxt, rew, term = c.domain_step(act)
            assert np.array_equal(tr["actions"][k][alive], act[alive]) and np.array_equal(tr["rewards"][k][alive], rew[alive])
            assert np.array_equal(tr["states"][k + 1][:, alive], nxt[:, alive])
            steps[alive] += 1
            alive &= ~term.astype(bool)
        assert np.array_equal(steps + 1, ns) and np.array_equal(~alive, tr["terminal"].astype(bool))
        pol = c.rollout_policy(rsrl_amd.RANDOM, L)
        assert (pol["n_states"] >= 2).all() and (pol["n_states"] <= L).all()


@pytest.mark.parametrize("policy", POLICIES)
def test_value_and_policy_queries_against_the_oracle(orc, policy):
    Q0 = random_tables(N, 51)
    for i in range(0, N, 5):
        Q0[i][:, 1] = Q0[i][:, 3]          # ties between two actions
    rng = np.random.default_rng(52)
    s = np.stack([rng.uniform(-1.0, 13.0, N), rng.uniform(-1.0, 6.0, N)]).astype(np.float32)
    with ctx(policy=policy) as c:
        install(c, Q0)
        rows = [Q0[i][tn.row_of_state(s[:, i])] for i in range(N)]
        assert same_bits(c.q_evaluate(s), np.stack(rows, axis=1))
        idx, val = c.q_find_max(s)
        idn, vmin = c.q_find_min(s)
        probs = c.policy_probs(s)
        ev = c.q_expected_value(s, probs)
        call = 0
        smp = c.policy_sample(s)
        mode = c.policy_mode(s) if policy != rsrl_amd.RANDOM else None
        for i in range(N):
            q = rows[i]
            wi, wv = orc.find_max(q, prec="f32d")
            assert idx[i] == wi and same_bits(val[i], np.float32(wv))
            assert same_bits(vmin[i], q.min()) and q[idn[i]] == q.min()
            p = orc.policy_probs(policy, q, eps=EPS, tau=TAU, prec="f32d")
            assert same_bits(probs[:, i], p), (i, probs[:, i], p)
            e = np.float32(0.0)
            for b in range(4):
                e = np.float32(e + np.float32(q[b] * p[b]))
            assert same_bits(ev[i], e)
            assert smp[i] == orc.policy_sample(policy, q, orc.draw(SEED, i, call, orc.BLK_API), eps=EPS, tau=TAU, prec="f32d")
            if mode is not None:
                assert mode[i] == orc.policy_mode(policy, q, tau=TAU, prec="f32d")


def test_checkpoints(tmp_path):
    kw = dict(n_envs=N, algo=rsrl_amd.SARSA, policy=rsrl_amd.EPSILON_GREEDY, max_episode_steps=17)
    path = os.path.join(str(tmp_path), "cliff.ckpt")
    check_checkpoint_resume(ctx, kw, path, 25, 20, carry=("states", "actions", "episode_steps"))
    others = [dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, n_envs=N, algo=rsrl_amd.SARSA, policy=rsrl_amd.EPSILON_GREEDY),
              dict(domain=rsrl_amd.HIV_TREATMENT, order=1, n_envs=N, algo=rsrl_amd.SARSA, policy=rsrl_amd.EPSILON_GREEDY)]
    check_foreign_checkpoints_refused(ctx, kw, path, others, tmp_path)


def test_calls_that_make_no_sense_here():
    with ctx() as c:
        for call in (lambda: c.get_traces(0), lambda: c.get_td_weights(0), lambda: c.get_policy_weights(0), lambda: c.get_hidden_states(),
                     lambda: c.peer_export(1), lambda: rsrl_amd.Context.group_create([c]), lambda: c.project(c.states), lambda: c.tile_indices(c.states)):
            with pytest.raises(rsrl_amd.RsrlHipError):
                call()
        c.set_epsilon(0.5)
        c.train(3)
        with pytest.raises(rsrl_amd.RsrlHipError) as e:
            c.states = np.full((2, N), np.nan, dtype=np.float32)
        assert e.value.code == -1


def test_example_runs(tmp_path):
    out = run_example(tmp_path, "cliff_walk", [192, 3000])
    lines = out.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("QLearning") and lines[1].startswith("SARSA") and "13-step path" in lines[0]
