"""NAC with the Beta policy and the SCB SARSA critic (RSRL_NAC, examples/nac_beta.rs) without a GPU: the restatement the GPU tests compare against
(tests/nac_numpy.py) on hand-computed cases with F = 4, its float32 NAC::handle against the f64 one, the header / binding table / Rust block on the
new names, admission (the supported configurations reach the device query, every other one is refused with a message that names what is
supported, the sixth grid equals its fixture, 27 is still no algo), and examples/nac_beta.cpp compiles."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest
from scipy.special import digamma

import rsrl_amd
from rsrl_amd import _abi
from tests import beta_numpy as bn
from tests import nac_numpy as nn
from tests.agent_contract import compile_example, create_rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EHIP = -1, -2
BASE = dict(domain=rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, order=3, algo=28, policy=rsrl_amd.BETA, n_envs=4, n_steps=100)
NEW_CALLS = {"rsrl_hip_n_weight_rows": 1, "rsrl_hip_q_evaluate_f32": 5, "rsrl_hip_nac_update": 3}


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def matrix():
    return _load("admission_matrix")


# ---- the restatement, by hand: F = 4
PHI = np.array([1.0, -0.5, 0.25, 1.0])
W = np.array([[0.4, -0.2], [0.1, 0.3], [-0.6, 0.5], [0.2, 0.1]])
W3 = np.arange(1.0, 13.0) / 10.0                         # the critic's 3F = 12 weights


def _by_hand(phi, a):
    xa, xb = phi @ W[:, 0], phi @ W[:, 1]
    al, be = np.log1p(np.exp(xa)) + 1.0, np.log1p(np.exp(xb)) + 1.0
    ac = min(max(a, 2.0 ** -24), 1.0 - 2.0 ** -24)
    ga = np.log(ac) - digamma(al) + digamma(al + be)
    gb = np.log1p(-ac) - digamma(be) + digamma(al + be)
    return ga / (1.0 + np.exp(-xa)), gb / (1.0 + np.exp(-xb))


def test_psi_and_q_by_hand():
    for a in (0.3, 0.0, 1.0):
        ca, cb = _by_hand(PHI, a)
        p = nn.psi(W, PHI, a)
        assert p.shape == (12,) and np.allclose(p[:4], ca * PHI, rtol=1e-14, atol=0) and np.allclose(p[4:8], cb * PHI, rtol=1e-14, atol=0)
        assert np.array_equal(p[8:], PHI) and np.isfinite(p).all()
        q = ca * (W3[:4] @ PHI) + cb * (W3[4:8] @ PHI) + W3[8:] @ PHI
        assert abs(nn.q_value(W3, W, PHI, a) - q) <= 1e-13 * max(1.0, abs(q))
    assert nn.q_value(np.zeros(12), W, PHI, 0.3) == 0.0                       # w starts at zero: Q = 0


def test_sarsa_handle_terminal_and_non_terminal_by_hand():
    phi_n, a, na, r, gamma, lr = np.array([1.0, 0.5, -0.25, 1.0]), 0.3, 0.7, -1.0, 0.9, 0.01
    q, qn = nn.q_value(W3, W, PHI, a), nn.q_value(W3, W, phi_n, na)
    d, w2 = nn.sarsa_handle(W3, W, PHI, a, r, phi_n, na, True, gamma, lr)
    assert d == r - q and np.allclose(w2, W3 + lr * (r - q) * nn.psi(W, PHI, a), rtol=1e-15, atol=0)
    d, w2 = nn.sarsa_handle(W3, W, PHI, a, r, phi_n, na, False, gamma, lr)
    assert abs(d - (r + gamma * qn - q)) <= 1e-15 * abs(d) and np.allclose(w2, W3 + lr * d * nn.psi(W, PHI, a), rtol=1e-15, atol=0)
    # the terminal rule reads neither s' nor the draw
    assert nn.sarsa_handle(W3, W, PHI, a, r, 7.0 * phi_n, 0.01, True, gamma, lr)[0] == r - q
    # only the last F weights move by lr delta phi: the basis block's own feature is phi itself
    assert np.allclose(w2[8:] - W3[8:], lr * d * PHI, rtol=1e-12, atol=0)


def test_nac_handle_by_hand():
    alpha = 0.1
    # norm above 1e-3
    W2, norm = nn.nac_handle(W3, W, alpha)
    want = np.sqrt(sum((k / 10.0) ** 2 for k in range(1, 9)))
    assert abs(norm - want) <= 1e-15 and np.allclose(W2[:, 0], W[:, 0] + alpha / want * W3[:4], rtol=1e-15, atol=0)
    assert np.allclose(W2[:, 1], W[:, 1] + alpha / want * W3[4:8], rtol=1e-15, atol=0)
    # norm below 1e-3: the floor divides
    tiny = np.concatenate([np.full(8, 1e-5), W3[8:]])
    W2, norm = nn.nac_handle(tiny, W, alpha)
    assert norm == 1e-3 and np.allclose(W2, W + alpha / 1e-3 * 1e-5, rtol=1e-14, atol=0)
    # g = 0: norm = 1e-3 and nothing moves, whatever the basis block holds
    W2, norm = nn.nac_handle(np.concatenate([np.zeros(8), W3[8:]]), W, alpha)
    assert norm == 1e-3 and np.array_equal(W2, W)
    # the critic's last F weights are never read
    assert np.array_equal(nn.nac_handle(np.concatenate([W3[:8], 9.0 * W3[8:]]), W, alpha)[0], nn.nac_handle(W3, W, alpha)[0])


def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a, b = rng.normal(size=4000).astype(np.float32), rng.normal(size=4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1.0 + rng.normal(size=4000) * 1e-4)).astype(np.float32)      # heavy cancellation
    c[:2000] = rng.normal(size=2000).astype(np.float32)
    # a tie of the f64 sum that the product's low bits break: 1 + 2^-24 + 2^-60
    a[0], b[0], c[0] = np.float32(1.0 + 2.0 ** -12), np.float32(2.0 ** -12 + 2.0 ** -23), np.float32(1.0)
    got = nn.fma32(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                                           # a float32 neighbour (possibly double-rounded): pick the nearer by exact distance
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        best = min(cands, key=lambda x: (abs(Fraction(float(x)) - exact), int(x.view(np.uint32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i], got[i], best)


def test_float32_nac_handle_is_the_f64_one_to_a_few_ulps():
    rng = np.random.default_rng(9)
    for F in (4, 16, 36):
        for scale in (0.0, 1e-5, 3e-4, 1.0, 1e3):
            w = (rng.normal(size=3 * F) * scale).astype(np.float32)
            Wp = rng.normal(size=(F, 2)).astype(np.float32)
            got, norm = nn.nac_handle_f32(w, Wp, 0.1)
            want, norm64 = nn.nac_handle(w, Wp, float(np.float32(0.1)))
            assert got.dtype == np.float32 and abs(float(norm) - norm64) <= 4 * np.spacing(np.float32(norm64)), (F, scale)
            # per element: the scale carries (2F + 2) roundings of the norm's chain, the fma one more
            tol = (2 * F + 4) * 2.0 ** -24 * np.abs(want - Wp) + np.spacing(np.abs(want).astype(np.float32))
            assert np.all(np.abs(got.astype(np.float64) - want) <= tol), (F, scale)
            if scale == 0.0:
                assert norm == np.float32(1e-3) and np.array_equal(got, Wp)


@pytest.mark.parametrize("order", [1, 3, 5])
def test_the_gpu_rule_case_names_few_learners(orc, order):
    """the GPU rule test may leave out the learners whose inner draw evaluates an acceptance test within MARGIN of its boundary, 5 % at the most: with the
    oracle's f64 features the restatement names no more than that at the seed the GPU test uses; the actions 0 and 1 and both kinds of transition
    occur in every round"""
    case = nn.handle_case(order)
    N = len(case["init"])
    proj = lambda S: np.stack([orc.fourier_project(orc.MOUNTAIN_CAR, order, S[:, i]) for i in range(N)], axis=1)      # noqa: E731
    w, deltas, skipped = nn.critic_after(case, nn.RULE_SEED,[proj(r[0]) for r in case["rounds"]], [proj(r[3]) for r in case["rounds"]])
    assert N == 67 and skipped.sum() <= 3, skipped.sum()
    for frm, a, rew, nxt, term in case["rounds"]:
        assert 0 < term.sum() < N and a[0] == 0.0 and a[1] == 1.0 and a.min() >= 0.0 and a.max() <= 1.0
    w0 = np.stack([x for x, _ in case["init"]]).astype(np.float64)
    assert np.abs(w0).sum(axis=1).max() <= 3.0 + 1e-5 and np.max(np.abs(w - w0)) > 1e-3 and np.isfinite(w).all()
    for _, Wp in case["init"]:
        assert np.abs(Wp.astype(np.float64)).sum(axis=0).max() <= 3.0 + 1e-6


# ---- the interface
def test_header_binding_table_python_constants_and_rust_block_agree():
    gen = _load("gen_rust_sys")
    h = open(os.path.join(ROOT, "include", "rsrl_hip.h")).read()
    assert re.search(r"RSRL_NAC\s*=\s*28\b", h) and rsrl_amd.NAC == 28 and rsrl_amd.context.NAC == 28
    assert re.search(r"#define\s+RSRL_HIP_ABI_VERSION\s+9\b", h)
    funcs = {name: len(params) for name, params, _ in gen.parse_header()[0]}
    block = gen.doc_block()
    rust = dict(gen.declared_functions(block))
    for name, n in NEW_CALLS.items():
        assert funcs.get(name) == n, (name, funcs.get(name))
        assert len(_abi.SYMBOLS[name][1]) == n, name
        assert rust.get(name) == n, (name, rust.get(name))
        assert hasattr(_abi.lib(), name)
    assert "pub const RSRL_NAC: i32 = 28;" in block and block == gen.generate()


def test_supported_configurations_reach_the_device_query():
    for order in (1, 2, 3, 4, 5):
        for extra in (dict(), dict(steps_per_launch=1), dict(max_episode_steps=1000, lr=0.01, alpha=0.1, gamma=0.999), dict(n_steps=1), dict(n_steps=65536)):
            rc, msg = create_rc(BASE, order=order, **extra)
            assert rc == 0 or (rc == EHIP and "device" in msg), (order, extra, rc, msg)


def test_other_configurations_are_refused_with_a_message():
    bad = [dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(order=7), dict(weight_mode=rsrl_amd.W_SHARED), dict(weight_dtype=rsrl_amd.W_BF16),
           dict(policy=rsrl_amd.SOFTMAX), dict(policy=rsrl_amd.RANDOM), dict(policy=rsrl_amd.GREEDY), dict(agent_policy=rsrl_amd.SOFTMAX),
           dict(epsilon_decay=0.99), dict(domain=rsrl_amd.MOUNTAIN_CAR), dict(domain=rsrl_amd.MOUNTAIN_CAR, policy=rsrl_amd.SOFTMAX),
           dict(domain=rsrl_amd.CART_POLE, order=1, policy=rsrl_amd.SOFTMAX), dict(domain=rsrl_amd.HIV_TREATMENT, order=1, policy=rsrl_amd.GREEDY)]
    for b in bad:
        rc, msg = create_rc(BASE, **b)
        assert rc == EINVAL and "RSRL_NAC" in msg and "RSRL_BETA" in msg and "RSRL_CONTINUOUS_MOUNTAIN_CAR" in msg and "orders 1-5" in msg, (b, rc, msg)
    rc, msg = create_rc(BASE, agent_policy=rsrl_amd.BETA)
    assert rc == EINVAL and "unknown agent policy 4" in msg
    for n in (0, -1, 65537):
        rc, msg = create_rc(BASE, n_steps=n)
        assert rc == EINVAL and "RSRL_NAC" in msg and "n_steps" in msg and "65536" in msg, (n, rc, msg)
    rc, msg = create_rc(BASE, order=0)
    assert rc == EINVAL and "order" in msg


def test_twenty_seven_is_still_no_algo_and_nothing_follows_twenty_eight():
    for algo in (27, 29):
        for kw in (dict(), dict(domain=rsrl_amd.MOUNTAIN_CAR, policy=rsrl_amd.SOFTMAX)):
            rc, msg = create_rc(BASE, algo=algo, **kw)
            assert rc == EINVAL and "unknown algo %d" % algo in msg, (algo, kw, rc, msg)


def test_sixth_grid_and_its_fixture(matrix):
    doc = json.load(open(matrix.NAC_FIXTURE))
    assert doc["grid"] == [[n, v] for n, v in matrix.GRID_NAC], "GRID_NAC and its fixture drifted apart"
    names = [n for n, _ in matrix.GRID_NAC]
    vals = dict(matrix.GRID_NAC)
    rows = [{n: vals[n][int(ch, 16)] for n, ch in zip(names, key)} for key in doc["admitted"]]
    nac = [r for r in rows if r["algo"] == 28]
    # exactly: ContinuousMountainCar, Beta, agent_policy -1, orders 1-5, the period in [1, 65 536]
    assert len(nac) == 15 and all(r["domain"] == 4 and r["policy"] == 4 and r["agent_policy"] == -1 for r in nac)
    assert sorted({r["order"] for r in nac}) == [1, 2, 3, 4, 5] and sorted({r["n_steps"] for r in nac}) == [1, 100, 65536]
    assert not any(r["algo"] == 27 for r in rows)
    # the iLSTD ActorCritic's rows: its own range of n_steps (n_updates), on either domain with its own policy
    assert all(r["n_steps"] == 1 and (r["domain"], r["policy"]) in ((4, 4), (0, 2)) for r in rows if r["algo"] == 21)


def _gfx950_visible():
    import subprocess
    try:
        return subprocess.run(["/opt/rocm/bin/rocminfo"], capture_output=True, text=True).stdout.count("gfx950") > 0
    except Exception:
        return False


def test_create_admits_exactly_the_sixth_fixture(matrix):
    if _gfx950_visible():
        pytest.skip("GPU present: an admitted configuration would create a real ctx")
    from rsrl_amd import _build
    _build.build()
    res = matrix.sweep(matrix.GRID_NAC)
    assert matrix.admitted(res) == json.load(open(matrix.NAC_FIXTURE))["admitted"]
    for key, (rc, msg) in res.items():
        if rc != matrix.EHIP:
            assert rc == matrix.EINVAL and msg, (key, rc, msg)


def test_example_compiles(tmp_path):
    compile_example(tmp_path, "nac_beta")
