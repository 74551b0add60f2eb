"""ActorCritic::tdac with a TD(0) critic over the Gaussian or the Beta policy (RSRL_CONTINUOUS_TD_ACTOR_CRITIC = 35) without a GPU: the
restatement the GPU tests compare against (tests/tdac_cont_numpy.py) on hand-worked single transitions with F = 4 -- a terminal row reads V(s'),
the critic reads the UPDATED w, under Gaussian with c < 0 and a > mu the mean's preference decreases (what separates this rule from CACLA's), the
Beta step by hand --, the GPU rule test's inputs (every learner stays in, everything finite), the header / binding constants / Rust block on the
new name, admission (the supported configurations reach the device query, every other one is refused with a message naming
RSRL_CONTINUOUS_TD_ACTOR_CRITIC, 34 and 36 are no algos, the grid equals its fixture) and both examples compile."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest
from scipy.special import digamma

import rsrl_amd
from tests import cacla_numpy as cn
from tests import gaussian_numpy as gn
from tests import tdac_cont_numpy as tn
from tests.agent_contract import compile_example, create_rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EHIP = -1, -2
ALGO = 35
CMC, GAUSSIAN, BETA = rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, rsrl_amd.GAUSSIAN, rsrl_amd.BETA
BASE = dict(domain=CMC, order=3, algo=ALGO, policy=GAUSSIAN, n_envs=4)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def matrix():
    return _load("admission_matrix")


# ---- the rule, by hand: F = 4 (tests/test_cacla_cpu.py's vectors: exact binary fractions where it matters)
PHI = np.array([1.0, -0.5, 0.25, 1.0])
PHI_N = np.array([1.0, 0.5, -0.25, 1.0])
W = np.array([[0.4, -0.2], [0.1, 0.3], [-0.6, 0.5], [0.2, 0.1]])
V = np.array([0.5, -0.25, 0.75, 0.125])
GAMMA, LR, ALPHA = 0.5, 0.125, 0.01
A32 = float(np.float32(ALPHA))                 # alpha is rounded to f32 once


def test_the_critic_reads_the_updated_w_and_a_terminal_row_reads_v_of_s_prime():
    v_s, v_n = V @ PHI, V @ PHI_N                                                                  # 0.9375, 0.3125
    n2, cross = PHI @ PHI, PHI @ PHI_N                                                             # 2.3125, 1.6875
    assert v_s == 0.9375 and v_n == 0.3125 and n2 == 2.3125 and cross == 1.6875
    for r in (2.0, -1.0, 0.0):
        td, w2, c = tn.critic(V, PHI, PHI_N, r, False, GAMMA, LR)
        assert td == r + GAMMA * v_n - v_s and np.array_equal(w2, V + LR * td * PHI)
        assert abs(c - (r + GAMMA * (v_n + LR * td * cross) - (v_s + LR * td * n2))) < 1e-15      # V after TD's move, at both states
        assert abs(c - td * (1.0 - LR * (n2 - GAMMA * cross))) < 1e-15
    # terminal: TD's error does not read s', TDCritic's target reads V(s') of the terminal state itself -- r - V'(s'), not r - V'(s)
    for phi_n in (PHI_N, 40.0 * PHI_N, -40.0 * PHI_N):
        td, w2, c = tn.critic(V, PHI, phi_n, 1.0, True, GAMMA, LR)
        assert td == 1.0 - v_s and np.array_equal(w2, V + LR * td * PHI)
        assert abs(c - (1.0 - w2 @ phi_n)) < 1e-13
    c_small, c_big = tn.critic(V, PHI, PHI_N, 1.0, True, GAMMA, LR)[2], tn.critic(V, PHI, 40.0 * PHI_N, 1.0, True, GAMMA, LR)[2]
    assert c_small > 0 > c_big and abs(c_small - (1.0 - V @ PHI)) > 0.1                            # ... so V(s') decides its sign


def _gauss_by_hand(a):
    xm, xs = PHI @ W[:, 0], PHI @ W[:, 1]
    sd = np.log1p(np.exp(xs)) + 0.01
    var = sd * sd
    return xm, sd, (a - xm) / var, ((a - xm) ** 2 - var) / (2.0 * var ** 2) / (1.0 + np.exp(-xs))


def test_gaussian_step_by_hand_and_what_separates_it_from_cacla():
    mu = PHI @ W[:, 0]
    for r, a in ((2.0, mu + 0.7), (2.0, mu - 0.7), (-1.0, mu + 0.7), (-1.0, mu - 0.7)):
        td, w2, W2, c = tn.handle(GAUSSIAN, V, W, PHI, PHI_N, a, r, False, GAMMA, LR, ALPHA)
        _, _, cm, cs = _gauss_by_hand(a)
        e = A32 * c
        assert np.sign(c) == np.sign(td) == (1 if r > 0 else -1)
        assert np.allclose(W2[:, 0], W[:, 0] + e * cm * PHI, rtol=1e-14, atol=0) and np.allclose(W2[:, 1], W[:, 1] + e * cs * PHI, rtol=1e-13, atol=0)
        # the mean's preference moves by e c_m |phi|^2 = alpha c (a - mu) / Sigma |phi|^2: towards the action iff c > 0
        d_mu = PHI @ W2[:, 0] - mu
        assert abs(d_mu - e * cm * (PHI @ PHI)) < 1e-14 and np.sign(d_mu) == np.sign(c) * np.sign(a - mu)
    # THE case: c < 0 and a > mu -- <w_m, phi(s)> DECREASES.  CACLA's literal rule never lowers it: its gate is closed here, and where it is open the
    # mean's step alpha (a - mu)^2 / Sigma is >= 0 on either side
    a = mu + 0.7
    _, _, W2, c = tn.handle(GAUSSIAN, V, W, PHI, PHI_N, a, -1.0, False, GAMMA, LR, ALPHA)
    assert c < 0 and a > mu and PHI @ W2[:, 0] < mu - 1e-4
    _, _, Wc, gate, _ = cn.handle(V, W, PHI, PHI_N, a, -1.0, False, GAMMA, LR, ALPHA)
    assert not gate and Wc.tobytes() == W.tobytes() and cn.mean_step(W, PHI, mu - 0.7, ALPHA) > 0
    # alpha = 0: the columns keep their values, w and td are TD's
    td0, w0, W0, _ = tn.handle(GAUSSIAN, V, W, PHI, PHI_N, a, -1.0, False, GAMMA, LR, 0.0)
    td1, w1, _ = tn.critic(V, PHI, PHI_N, -1.0, False, GAMMA, LR)
    assert np.array_equal(W0, W) and td0 == td1 and np.array_equal(w0, w1)


def test_beta_step_by_hand():
    xa, xb = PHI @ W[:, 0], PHI @ W[:, 1]
    al, be = np.log1p(np.exp(xa)) + 1.0, np.log1p(np.exp(xb)) + 1.0
    for r, a in ((2.0, 0.3), (-1.0, 0.3), (2.0, 0.9), (-1.0, 0.02)):
        td, w2, W2, c = tn.handle(BETA, V, W, PHI, PHI_N, a, r, False, GAMMA, LR, ALPHA)
        e = A32 * c
        ga = np.log(a) - digamma(al) + digamma(al + be)
        gb = np.log1p(-a) - digamma(be) + digamma(al + be)
        assert np.allclose(W2[:, 0], W[:, 0] + e * ga / (1.0 + np.exp(-xa)) * PHI, rtol=1e-13, atol=0)
        assert np.allclose(W2[:, 1], W[:, 1] + e * gb / (1.0 + np.exp(-xb)) * PHI, rtol=1e-13, atol=0)
        assert td == r + GAMMA * (V @ PHI_N) - V @ PHI and np.array_equal(w2, V + LR * td * PHI)
    # an action above the mean alpha / (alpha + beta) with c > 0 raises alpha's preference and lowers beta's
    mean = al / (al + be)
    _, _, W2, c = tn.handle(BETA, V, W, PHI, PHI_N, min(0.98, mean + 0.3), 2.0, False, GAMMA, LR, ALPHA)
    assert c > 0 and PHI @ W2[:, 0] > xa and PHI @ W2[:, 1] < xb


@pytest.mark.parametrize("policy", [GAUSSIAN, BETA], ids=["gaussian", "beta"])
@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_the_gpu_rule_case_keeps_every_learner_in(orc, order, policy):
    proj = lambda S: np.stack([orc.fourier_project(orc.MOUNTAIN_CAR, order, S[:, i]) for i in range(S.shape[1])], axis=1)      # noqa: E731
    case = tn.handle_case(order, proj, policy)
    N, F = len(case["init"]), case["F"]
    assert N == 67 and F == (order + 1) ** 2 and len(case["rounds"]) == 3 and case["policy"] == policy
    phi_s, phi_n = [proj(r[0]) for r in case["rounds"]], [proj(r[3]) for r in case["rounds"]]
    w, cols, cs, tds, xs = tn.after(case, phi_s, phi_n)
    assert tn.keeps_every_learner_in(case, cs, xs, w, cols) == []
    for frm, a, rew, nxt, term in case["rounds"]:
        assert np.isfinite(a).all() and np.isfinite(rew).all() and a.dtype == rew.dtype == np.float32
        if policy == GAUSSIAN:
            mu = np.array([gn.prefs(W, phi_s[0][:, i])[0] for i, (_, W) in enumerate(case["init"])])
            assert np.abs(mu).max() <= 1.5
    init = np.stack([W for _, W in case["init"]]).astype(np.float64)
    moved = np.abs(cols - init).max(axis=(1, 2))
    assert moved.min() > 1e-7 and moved.max() > 1e-3 and np.isfinite(cols).all()                  # every learner's columns move, by far more than any bound
    # the same case again: the generator is deterministic, so the GPU tests and the rate script read these very inputs (up to the projection)
    again = tn.handle_case(order, proj, policy)
    assert all(x.tobytes() == y.tobytes() for r1, r2 in zip(case["rounds"], again["rounds"]) for x, y in zip(r1, r2))


# ---- the interface
def test_header_binding_constants_and_rust_block_agree():
    gen = _load("gen_rust_sys")
    h = open(os.path.join(ROOT, "include", "rsrl_hip.h")).read()
    assert re.search(r"RSRL_CONTINUOUS_TD_ACTOR_CRITIC\s*=\s*35\s*,", h) and "(34 is no algo.)" in h
    assert re.search(r"RSRL_CACLA\s*=\s*33\s*\}\s*rsrl_algo", h)                                  # CACLA is still the enum's last enumerator
    assert h.index("RSRL_CONTINUOUS_TD_ACTOR_CRITIC = 35") < h.index("(32 is no algo.)")          # ... and the new one stands before its comment
    assert rsrl_amd.CONTINUOUS_TD_ACTOR_CRITIC == 35 and rsrl_amd.context.CONTINUOUS_TD_ACTOR_CRITIC == 35 and tn.TDAC_CONT == 35
    assert rsrl_amd.CACLA == 33 and tn.GAUSSIAN == GAUSSIAN == 6 and tn.BETA == BETA == 4
    assert re.search(r"#define\s+RSRL_HIP_ABI_VERSION\s+9\b", h)
    block = gen.doc_block()
    assert "pub const RSRL_CONTINUOUS_TD_ACTOR_CRITIC: i32 = 35;" in block and "pub const RSRL_CACLA: i32 = 33;" in block and block == gen.generate()
    assert len(gen.parse_header()[0]) == len(dict(gen.declared_functions(block))) == 96          # no new entry point
    # the step's order is stated where a caller reads it, and in the kernel file's head comment
    k = open(os.path.join(ROOT, "rsrl_amd", "csrc", "kernels_cont.hpp")).read()
    for text in (h, k):
        assert "TDCritic::target" in text and "before any move" in text and "no gate" in text
    mirror = open(os.path.join(ROOT, "rsrl_amd", "host", "rsrl.hpp")).read()
    assert "tdac(const prediction::td::TD& eval, const policies::Gaussian&" in mirror and "tdac(const prediction::td::TD& eval, const policies::Beta&" in mirror
    assert "RSRL_CONTINUOUS_TD_ACTOR_CRITIC" in mirror


def test_34_and_36_are_no_algos():
    for algo in (34, 36, 1000):
        for kw in (dict(), dict(domain=rsrl_amd.MOUNTAIN_CAR, policy=rsrl_amd.RANDOM), dict(policy=BETA)):
            rc, msg = create_rc(BASE, algo=algo, **kw)
            assert rc == EINVAL and "unknown algo %d" % algo in msg, (algo, kw, rc, msg)
    for policy in (5, 7):
        rc, msg = create_rc(BASE, policy=policy)
        assert rc == EINVAL and "unknown policy %d" % policy in msg, (policy, rc, msg)


def test_supported_configurations_reach_the_device_query():
    for policy in (GAUSSIAN, BETA):
        for order in (1, 2, 3, 4, 5):
            for extra in (dict(), dict(steps_per_launch=1), dict(max_episode_steps=1000, lr=0.01, alpha=0.001, gamma=0.999), dict(n_steps=0), dict(n_steps=-7),
                          dict(n_steps=1 << 20)):
                rc, msg = create_rc(BASE, policy=policy, order=order, **extra)
                assert rc == 0 or (rc == EHIP and "device" in msg), (policy, order, extra, rc, msg)


def test_other_configurations_are_refused_with_a_message():
    bad = [dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(order=7), dict(weight_mode=rsrl_amd.W_SHARED), dict(weight_dtype=rsrl_amd.W_BF16),
           dict(agent_policy=rsrl_amd.SOFTMAX), dict(epsilon_decay=0.99), dict(domain=rsrl_amd.MOUNTAIN_CAR), dict(domain=rsrl_amd.CART_POLE, order=1),
           dict(domain=rsrl_amd.HIV_TREATMENT, order=1)]
    bad += [dict(b, policy=BETA) for b in bad]
    bad += [dict(policy=p) for p in (rsrl_amd.RANDOM, rsrl_amd.GREEDY, rsrl_amd.SOFTMAX, rsrl_amd.EPSILON_GREEDY)]
    bad += [dict(policy=rsrl_amd.SOFTMAX, domain=rsrl_amd.MOUNTAIN_CAR), dict(policy=rsrl_amd.RANDOM, domain=rsrl_amd.MOUNTAIN_CAR)]
    for b in bad:
        rc, msg = create_rc(BASE, **dict(dict(max_episode_steps=10), **b))
        assert rc == EINVAL and "RSRL_CONTINUOUS_TD_ACTOR_CRITIC" in msg and "RSRL_GAUSSIAN" in msg and "RSRL_BETA" in msg and \
            "RSRL_CONTINUOUS_MOUNTAIN_CAR" in msg and "orders 1-5" in msg, (b, rc, msg)
    rc, msg = create_rc(BASE, order=0)
    assert rc == EINVAL and "order" in msg
    rc, msg = create_rc(BASE, agent_policy=6)
    assert rc == EINVAL and "unknown agent policy 6" in msg
    # the pairings that stay refused: the discrete TD ActorCritic on this domain or with these policies, CACLA with Beta
    for kw in (dict(algo=rsrl_amd.TD_ACTOR_CRITIC), dict(algo=rsrl_amd.TD_ACTOR_CRITIC, policy=BETA), dict(algo=rsrl_amd.CACLA, policy=BETA),
               dict(algo=rsrl_amd.ILSTD_ACTOR_CRITIC, n_steps=2)):
        rc, msg = create_rc(BASE, **kw)
        assert rc == EINVAL and "RSRL_CONTINUOUS_TD_ACTOR_CRITIC" in msg, (kw, rc, msg)


def test_tdac_cont_grid_and_its_fixture(matrix):
    doc = json.load(open(matrix.TDAC_CONT_FIXTURE))
    assert doc["grid"] == [[n, v] for n, v in matrix.GRID_TDAC_CONT], "GRID_TDAC_CONT and its fixture drifted apart"
    assert dict(matrix.GRID_TDAC_CONT) == dict(algo=[33, 34, 35, 36], policy=[2, 3, 4, 6], domain=[0, 4], agent_policy=[-1, 6], order=[0, 1, 2, 3, 4, 5, 6])
    assert matrix.GRIDS[-1][0] is matrix.GRID_TDAC_CONT and len(matrix.GRIDS) == 10                # appended: the other grids stand as they stood
    names = [n for n, _ in matrix.GRID_TDAC_CONT]
    vals = dict(matrix.GRID_TDAC_CONT)
    rows = [{n: vals[n][int(ch, 16)] for n, ch in zip(names, key)} for key in doc["admitted"]]
    mine = [r for r in rows if r["algo"] == 35]
    # exactly: 2 policies x 5 orders on ContinuousMountainCar, agent_policy -1
    assert len(mine) == 10 and all(r["domain"] == 4 and r["agent_policy"] == -1 for r in mine)
    assert sorted((r["policy"], r["order"]) for r in mine) == [(p, o) for p in (4, 6) for o in (1, 2, 3, 4, 5)]
    assert not any(r["algo"] in (34, 36) for r in rows)
    cacla = [r for r in rows if r["algo"] == 33]
    assert len(cacla) == 5 and all(r["policy"] == 6 and r["domain"] == 4 and r["agent_policy"] == -1 for r in cacla) and len(rows) == 15


def test_create_admits_exactly_the_fixture_where_no_ctx_would_be_created(matrix):
    """every REFUSED configuration of the grid is refused on any machine (EINVAL needs no device); the admitted ones are asked only on a machine
    without a GPU, where they end at the device query"""
    from rsrl_amd import _build
    _build.build()
    want = set(json.load(open(matrix.TDAC_CONT_FIXTURE))["admitted"])
    names = [n for n, _ in matrix.GRID_TDAC_CONT]
    vals = dict(matrix.GRID_TDAC_CONT)
    n_refused = 0
    import itertools
    for idx in itertools.product(*(range(len(v)) for _, v in matrix.GRID_TDAC_CONT)):
        key = "".join("%x" % i for i in idx)
        kw = {n: vals[n][i] for n, i in zip(names, idx)}
        rc, msg = create_rc(dict(n_envs=4), **kw)
        if key in want:
            assert rc == 0 or (rc == EHIP and "device" in msg), (kw, rc, msg)
        else:
            assert rc == EINVAL and msg, (kw, rc, msg)
            n_refused += 1
    assert n_refused == 448 - 15


def test_examples_compile(tmp_path):
    compile_example(tmp_path, "tdac_gaussian")
    compile_example(tmp_path, "tdac_beta_td")
