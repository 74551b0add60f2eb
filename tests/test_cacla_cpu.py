"""CACLA over the Gaussian policy with a TD(0) critic (RSRL_CACLA = 33, control/cacla.rs) without a GPU: the restatement the GPU tests compare
against (tests/cacla_numpy.py) on hand-worked cases with F = 4 -- an open and a closed gate, a terminal transition (the target is r alone),
target == v exactly (closed), the mean's coefficient non-negative on either side of the mean --, the float32 restatement of the TD half and the
gate against the f64 one, the GPU rule test's inputs, the header / binding constants / Rust block on the new name, admission (the supported
configurations reach the device query, every other one is refused with a message naming RSRL_CACLA, 32 and 34 are no algos, the grid equals its
fixture) and examples/cacla.cpp compiles."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import rsrl_amd
from tests import cacla_numpy as cn
from tests import gaussian_numpy as gn
from tests.agent_contract import compile_example, create_rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EHIP = -1, -2
BASE = dict(domain=rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, order=3, algo=33, policy=rsrl_amd.GAUSSIAN, n_envs=4)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def matrix():
    return _load("admission_matrix")


# ---- the rule, by hand: F = 4
PHI = np.array([1.0, -0.5, 0.25, 1.0])
PHI_N = np.array([1.0, 0.5, -0.25, 1.0])
W = np.array([[0.4, -0.2], [0.1, 0.3], [-0.6, 0.5], [0.2, 0.1]])      # column 0 the mean's, column 1 the stddev's
V = np.array([0.5, -0.25, 0.75, 0.125])                                # the TD learner's weights: exact binary fractions
GAMMA, LR, ALPHA = 0.5, 0.125, 0.01


def _by_hand(a):
    """(mu, sd, c_m, c_s) at PHI"""
    xm, xs = PHI @ W[:, 0], PHI @ W[:, 1]
    sd = np.log1p(np.exp(xs)) + 0.01
    var = sd * sd
    return xm, sd, (a - xm) / var, ((a - xm) ** 2 - var) / (2.0 * var ** 2) / (1.0 + np.exp(-xs))


def test_open_and_closed_gate_by_hand():
    v_s, v_n = V @ PHI, V @ PHI_N
    assert v_s == 0.5 + 0.125 + 0.1875 + 0.125 and v_n == 0.5 - 0.125 - 0.1875 + 0.125           # 0.9375, 0.3125
    n2, cross = PHI @ PHI, PHI @ PHI_N                                                            # 2.3125, 1.6875
    for r, a, want_open in ((2.0, 0.3, True), (-1.0, 0.3, False), (2.0, -1.5, True), (0.0, 1.5, False)):
        td, w2, W2, gate, margin = cn.handle(V, W, PHI, PHI_N, a, r, False, GAMMA, LR, ALPHA)
        assert td == r + GAMMA * v_n - v_s                                                        # TD's error with the weights as they were
        assert np.array_equal(w2, V + LR * td * PHI)
        # the critic closure reads the UPDATED weights
        v2, vn2 = v_s + LR * td * n2, v_n + LR * td * cross
        assert abs(margin - (r + GAMMA * vn2 - v2)) < 1e-15 and gate == want_open == (margin > 0)
        if gate:
            mu, sd, cm, cs = _by_hand(a)
            e = (a - mu) * ALPHA
            assert np.allclose(W2[:, 0], W[:, 0] + e * cm * PHI, rtol=1e-14, atol=0) and np.allclose(W2[:, 1], W[:, 1] + e * cs * PHI, rtol=1e-13, atol=0)
            assert not np.array_equal(W2, W)
        else:
            assert W2.tobytes() == W.tobytes()                                                    # a closed gate moves nothing
    # the gate reads the updated V, not the one TD read: r = 0.8 is above v_s - gamma v_n = 0.78125 (td > 0) ...
    td, _, _, gate, margin = cn.handle(V, W, PHI, PHI_N, 0.3, 0.8, False, GAMMA, LR, ALPHA)
    assert td > 0 and gate and abs(margin - td * (1 - LR * (n2 - GAMMA * cross))) < 1e-15
    # ... and with a large rate the update overshoots: target - v has the sign of td (1 - lr (|phi|^2 - gamma <phi, phi'>)), here td * (1 - 1.46875)
    td, _, W2, gate, margin = cn.handle(V, W, PHI, PHI_N, 0.3, 0.8, False, GAMMA, 1.0, ALPHA)
    assert td > 0 and not gate and margin < 0 and W2.tobytes() == W.tobytes()


def test_terminal_target_is_the_reward_alone():
    v_s = V @ PHI
    # r = 1.0 > v_s = 0.9375: open, whatever V(s') is -- r - V(s') = 1 - 0.3125 would be open too, so take phi' with a large V(s')
    big = 40.0 * PHI_N
    for phi_n in (PHI_N, big, -big):
        td, w2, W2, gate, margin = cn.handle(V, W, PHI, phi_n, 0.3, 1.0, True, GAMMA, LR, ALPHA)
        assert td == 1.0 - v_s and np.array_equal(w2, V + LR * td * PHI)
        assert gate and abs(margin - (1.0 - w2 @ PHI)) < 1e-15 and margin == cn.handle(V, W, PHI, PHI_N, 0.3, 1.0, True, GAMMA, LR, ALPHA)[4]
    # ac.rs's TDCritic would read r - V(s') on a terminal transition; CACLA does not: with V(s') = -12.5 that form is far above v, the reward alone
    # (0.5 < 0.9375) is below it
    td, _, W2, gate, margin = cn.handle(V, W, PHI, -big, 0.3, 0.5, True, GAMMA, LR, ALPHA)
    assert V @ -big == -12.5 and 0.5 - V @ -big > v_s and not gate and margin < 0 and W2.tobytes() == W.tobytes()


def test_target_equal_to_v_is_closed():
    # lr = 0: V stays; r = v_s - gamma v_n = 0.78125 exactly, so target == v (every value a binary fraction)
    r = V @ PHI - GAMMA * (V @ PHI_N)
    td, w2, W2, gate, margin = cn.handle(V, W, PHI, PHI_N, 0.3, r, False, GAMMA, 0.0, ALPHA)
    assert r == 0.78125 and td == 0.0 and margin == 0.0 and not gate and W2.tobytes() == W.tobytes() and np.array_equal(w2, V)
    td, _, W2, gate, margin = cn.handle(V, W, PHI, PHI_N, 0.3, V @ PHI, True, GAMMA, 0.0, ALPHA)
    assert margin == 0.0 and not gate and W2.tobytes() == W.tobytes()
    assert cn.handle(V, W, PHI, PHI_N, 0.3, np.nextafter(r, 1.0), False, GAMMA, 0.0, ALPHA)[3]    # one ulp above: open
    # the float32 restatement decides the same, and a NaN closes the gate
    f = lambda x: np.asarray(x, dtype=np.float32)[None]      # noqa: E731
    for rr, want in ((r, False), (np.nextafter(np.float32(r), np.float32(1.0)), True), (np.nan, False)):
        _, _, v, target, g32 = cn.td_gate_f32(f(V), f(PHI), f(PHI_N), f(rr)[0:1].ravel(), np.array([False]), GAMMA, 0.0)
        assert bool(g32[0]) == want, (rr, v, target)


def test_the_means_coefficient_is_non_negative_on_either_side():
    mu = PHI @ W[:, 0]
    for a in (mu - 1.0, mu - 0.25, mu + 0.25, mu + 1.0, -1.5, 1.5):
        step = cn.mean_step(W, PHI, a, ALPHA)
        _, sd, cm, _ = _by_hand(a)
        assert step > 0 and abs(step - ALPHA * (a - mu) ** 2 / sd ** 2) <= 1e-15 * step and np.sign(cm) == np.sign(a - mu)
        # the mean at s moves UP by step * |phi|^2 whichever side the action lay on: not van Hasselt's mu += alpha (a - mu)
        _, _, W2, gate, _ = cn.handle(V, W, PHI, PHI_N, a, 2.0, False, GAMMA, LR, ALPHA)
        assert gate and abs((PHI @ W2[:, 0] - mu) - step * (PHI @ PHI)) < 1e-14
    assert cn.mean_step(W, PHI, mu, ALPHA) == 0.0


def test_float32_restatement_of_the_td_half_and_the_gate(orc):
    rng = np.random.default_rng(33)
    for order in (1, 3, 5):
        F, N = (order + 1) ** 2, 41
        lo, hi = orc.domain_bounds(orc.MOUNTAIN_CAR)
        S, S2 = (rng.uniform(lo, hi, size=(N, 2)).astype(np.float32) for _ in range(2))
        ps = np.stack([orc.fourier_project(orc.MOUNTAIN_CAR, order, s, "f32d") for s in S]).astype(np.float32)
        pn = np.stack([orc.fourier_project(orc.MOUNTAIN_CAR, order, s, "f32d") for s in S2]).astype(np.float32)
        w = (rng.normal(size=(N, F)) * 0.2).astype(np.float32)
        r, term = rng.uniform(-1.0, 1.0, size=N).astype(np.float32), rng.random(N) < 0.3
        td, w2, v, target, gate = cn.td_gate_f32(w, ps, pn, r, term, 0.95, 0.01)
        assert td.dtype == w2.dtype == v.dtype == target.dtype == np.float32 and 0 < gate.sum() < N
        for i in range(N):
            d, w64, _, g, m = cn.handle(w[i], np.zeros((F, 2)), ps[i], pn[i], 0.0, float(r[i]), bool(term[i]), float(np.float32(0.95)), float(np.float32(0.01)), 0.0)
            assert abs(td[i] - d) <= 2e-6 * max(1.0, abs(d)) and np.max(np.abs(w2[i] - w64)) <= 1e-6
            assert abs(float(target[i]) - float(v[i]) - m) <= 1e-5
            if abs(m) >= cn.MARGIN:
                assert bool(gate[i]) == g, (order, i, m)
            if term[i]:
                assert target[i] == r[i]                                                          # r alone, bit for bit
        # the TD half is the oracle's own f32d TD handle, bit for bit
        ag = orc.make_agent(domain=orc.MOUNTAIN_CAR, order=order, algo=orc.TD, policy=orc.RANDOM, gamma=0.95, lr=0.01)
        for i in range(N):
            wi = w[i].copy()
            d = orc.handle_td(ag, wi, None, S[i].astype(np.float32), r[i], S2[i].astype(np.float32), bool(term[i]), "f32d")
            assert np.float32(d).tobytes() == td[i].tobytes() and wi.tobytes() == w2[i].tobytes(), (order, i)


@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_the_gpu_rule_case(orc, order):
    """handle_case: no learner is left out, every margin is at least MARGIN, each gate outcome covers at least a quarter of the learners in every
    round, the overflow learner's gate is closed in every round and its c_s is not finite in f32, both kinds of transition occur"""
    proj = lambda S: np.stack([orc.fourier_project(orc.MOUNTAIN_CAR, order, S[:, i]) for i in range(S.shape[1])], axis=1)      # noqa: E731
    case = cn.handle_case(order, proj)
    N, F = len(case["init"]), case["F"]
    assert N == 67 and F == (order + 1) ** 2 and len(case["rounds"]) == 3
    phi_s, phi_n = [proj(r[0]) for r in case["rounds"]], [proj(r[3]) for r in case["rounds"]]
    w, cols, gates, tds, margins = cn.after(case, phi_s, phi_n)
    p = case["params"]
    for k, (frm, a, rew, nxt, term) in enumerate(case["rounds"]):
        assert np.all(np.abs(margins[k]) >= cn.MARGIN) and np.array_equal(margins[k], case["margins"][k])      # every learner, none left out
        assert gates[k].shape == (N,) and gates[k].sum() >= N / 4 and (~gates[k]).sum() >= N / 4
        assert 0 < term.sum() < N and not gates[k][cn.OVERFLOW_LEARNER] and a[cn.OVERFLOW_LEARNER] == np.float32(cn.OVERFLOW_ACTION)
        assert np.isfinite(rew).all() and np.isfinite(a).all()
        # the f32 decision on these inputs is the f64 one
        w_now = np.stack([x for x, _ in case["init"]]) if k == 0 else w32
        _, w32, _, _, g32 = cn.td_gate_f32(w_now, phi_s[k].T.astype(np.float32), phi_n[k].T.astype(np.float32), rew, term.astype(bool), p["gamma"], p["lr"])
        assert np.array_equal(g32, gates[k]), k
    i = cn.OVERFLOW_LEARNER
    assert cols[i].tobytes() == case["init"][i][1].astype(np.float64).tobytes()                  # closed throughout: as it was
    with np.errstate(over="ignore", invalid="ignore"):
        Wi, a32 = case["init"][i][1], np.float32(cn.OVERFLOW_ACTION)
        xs = np.float32(phi_s[0][:, i].astype(np.float32) @ Wi[:, 1])
        sd = np.float32(np.log1p(np.exp(xs)) + np.float32(0.01))
        var, d = np.float32(sd * sd), np.float32(a32 - np.float32(phi_s[0][:, i].astype(np.float32) @ Wi[:, 0]))
        assert xs == -50.0 and not np.isfinite(np.float32(np.float32(d * d) - var) / np.float32(np.float32(2.0) * np.float32(var * var)))
    opened = np.any(np.stack(gates), axis=0)
    assert opened.sum() > N / 2 and np.isfinite(cols).all() and np.isfinite(w).all()
    assert np.max(np.abs(cols[opened] - np.stack([W for _, W in case["init"]])[opened])) > 1e-3  # the columns move by far more than any bound


# ---- the interface
def test_header_binding_constants_and_rust_block_agree():
    gen = _load("gen_rust_sys")
    h = open(os.path.join(ROOT, "include", "rsrl_hip.h")).read()
    assert re.search(r"RSRL_TDC\s*=\s*31\s*,", h) and re.search(r"RSRL_CACLA\s*=\s*33\s*\}\s*rsrl_algo", h) and "(32 is no algo.)" in h
    assert rsrl_amd.CACLA == 33 and rsrl_amd.context.CACLA == 33 and cn.CACLA == 33 and rsrl_amd.GAUSSIAN == 6 and rsrl_amd.NAC == 28
    assert re.search(r"#define\s+RSRL_HIP_ABI_VERSION\s+9\b", h)
    block = gen.doc_block()
    assert "pub const RSRL_CACLA: i32 = 33;" in block and block == gen.generate()
    assert len(gen.parse_header()[0]) == len(dict(gen.declared_functions(block))) == 96          # no new entry point
    # the literal rule is stated where a caller reads it
    assert "cacla.rs" in h and "(a - mu)^2 / Sigma" in h and "van Hasselt" in h
    mirror = open(os.path.join(ROOT, "rsrl_amd", "host", "rsrl.hpp")).read()
    assert "namespace control { namespace cacla {" in mirror and "struct CACLA" in mirror


def test_32_and_34_are_no_algos():
    for algo in (32, 34, 1000):
        for kw in (dict(), dict(domain=rsrl_amd.MOUNTAIN_CAR, policy=rsrl_amd.RANDOM), dict(policy=rsrl_amd.BETA)):
            rc, msg = create_rc(BASE, algo=algo, **kw)
            assert rc == EINVAL and "unknown algo %d" % algo in msg, (algo, kw, rc, msg)


def test_supported_configurations_reach_the_device_query():
    for order in (1, 2, 3, 4, 5):
        for extra in (dict(), dict(steps_per_launch=1), dict(max_episode_steps=1000, lr=0.01, alpha=0.01, gamma=0.999), dict(n_steps=0), dict(n_steps=-7),
                      dict(n_steps=1 << 20)):
            rc, msg = create_rc(BASE, order=order, **extra)
            assert rc == 0 or (rc == EHIP and "device" in msg), (order, extra, rc, msg)


def test_other_configurations_are_refused_with_a_message():
    bad = [dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(order=7), dict(weight_mode=rsrl_amd.W_SHARED), dict(weight_dtype=rsrl_amd.W_BF16),
           dict(agent_policy=rsrl_amd.SOFTMAX), dict(epsilon_decay=0.99), dict(domain=rsrl_amd.MOUNTAIN_CAR), dict(domain=rsrl_amd.CART_POLE, order=1),
           dict(domain=rsrl_amd.HIV_TREATMENT, order=1)]
    # CACLA under any other policy: Beta (no reference loop says whether the domain sees a or 2a - 1) and the discrete ones
    bad += [dict(policy=p) for p in (rsrl_amd.BETA, rsrl_amd.RANDOM, rsrl_amd.GREEDY, rsrl_amd.SOFTMAX, rsrl_amd.EPSILON_GREEDY)]
    bad += [dict(policy=rsrl_amd.RANDOM, domain=rsrl_amd.MOUNTAIN_CAR), dict(policy=rsrl_amd.BETA, n_steps=2)]
    for b in bad:
        rc, msg = create_rc(BASE, **dict(dict(max_episode_steps=10), **b))
        assert rc == EINVAL and "RSRL_CACLA" in msg and "RSRL_NAC" in msg and "RSRL_GAUSSIAN" in msg and "RSRL_BETA" in msg and \
            "RSRL_CONTINUOUS_MOUNTAIN_CAR" in msg and "orders 1-5" in msg, (b, rc, msg)
    rc, msg = create_rc(BASE, order=0)
    assert rc == EINVAL and "order" in msg
    rc, msg = create_rc(BASE, agent_policy=6)
    assert rc == EINVAL and "unknown agent policy 6" in msg


def test_cacla_grid_and_its_fixture(matrix):
    doc = json.load(open(matrix.CACLA_FIXTURE))
    assert doc["grid"] == [[n, v] for n, v in matrix.GRID_CACLA], "GRID_CACLA and its fixture drifted apart"
    assert dict(matrix.GRID_CACLA) == dict(algo=[28, 32, 33, 34], policy=[3, 4, 6], domain=[0, 4], agent_policy=[-1, 6], order=[0, 1, 2, 3, 4, 5, 6])
    names = [n for n, _ in matrix.GRID_CACLA]
    vals = dict(matrix.GRID_CACLA)
    rows = [{n: vals[n][int(ch, 16)] for n, ch in zip(names, key)} for key in doc["admitted"]]
    cacla = [r for r in rows if r["algo"] == 33]
    # exactly: the Gaussian policy, ContinuousMountainCar, agent_policy -1, orders 1-5
    assert len(cacla) == 5 and all(r["policy"] == 6 and r["domain"] == 4 and r["agent_policy"] == -1 for r in cacla)
    assert sorted(r["order"] for r in cacla) == [1, 2, 3, 4, 5]
    assert not any(r["algo"] in (32, 34) for r in rows)
    # NAC's rows are what they were: Beta and Gaussian, orders 1-5 (the grid leaves n_steps at its default, 1)
    nac = [r for r in rows if r["algo"] == 28]
    assert len(nac) == 10 and all(r["domain"] == 4 and r["agent_policy"] == -1 and r["policy"] in (4, 6) for r in nac) and len(rows) == 15


def _gfx950_visible():
    import subprocess
    try:
        return subprocess.run(["/opt/rocm/bin/rocminfo"], capture_output=True, text=True).stdout.count("gfx950") > 0
    except Exception:
        return False


def test_create_admits_exactly_the_cacla_fixture(matrix):
    if _gfx950_visible():
        pytest.skip("GPU present: an admitted configuration would create a real ctx")
    from rsrl_amd import _build
    _build.build()
    res = matrix.sweep(matrix.GRID_CACLA)
    assert matrix.admitted(res) == json.load(open(matrix.CACLA_FIXTURE))["admitted"]
    for key, (rc, msg) in res.items():
        if rc != matrix.EHIP:
            assert rc == matrix.EINVAL and msg, (key, rc, msg)


def test_example_compiles(tmp_path):
    compile_example(tmp_path, "cacla")
