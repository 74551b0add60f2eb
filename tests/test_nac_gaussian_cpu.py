"""The Gaussian policy and NAC over it (RSRL_GAUSSIAN = 6 with RSRL_NAC, examples/nac.rs) without a GPU: the restatement the GPU tests compare
against (tests/gaussian_numpy.py) on hand-computed cases with F = 4 -- the score against a central difference of the log density in the mean and
in the VARIANCE, the density's integral --, the GPU rule test's inputs, the header / binding constants / Rust block on the new name, admission
(the supported configurations reach the device query, every other one is refused with a message that names what is supported, 5 and 7 are no
policies, the Gaussian grid equals its fixture) and examples/nac.cpp compiles."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import rsrl_amd
from tests import beta_numpy as bn
from tests import gaussian_numpy as gn
from tests import nac_numpy as nn
from tests.agent_contract import compile_example, create_rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EHIP = -1, -2
BASE = dict(domain=rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, order=3, algo=rsrl_amd.NAC, policy=6, n_envs=4, n_steps=100)


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
W = np.array([[0.4, -0.2], [0.1, 0.3], [-0.6, 0.5], [0.2, 0.1]])      # column 0 the mean's, column 1 the stddev's
W3 = np.arange(1.0, 13.0) / 10.0                                       # the critic's 3F = 12 weights


def _by_hand(phi, a):
    xm, xs = phi @ W[:, 0], phi @ W[:, 1]
    sd = np.log1p(np.exp(xs)) + 0.01
    var = sd * sd
    return (a - xm) / var, ((a - xm) ** 2 - var) / (2.0 * var ** 2) / (1.0 + np.exp(-xs)), xm, sd


def test_params_pdf_and_score_by_hand():
    xm, xs = gn.prefs(W, PHI)
    assert xm == 0.4 - 0.05 - 0.15 + 0.2 and abs(xs - (-0.2 - 0.15 + 0.125 + 0.1)) < 1e-16
    mu, sd = gn.gauss_params(xm, xs)
    assert mu == xm and abs(sd - (np.log(1.0 + np.exp(xs)) + 0.01)) < 1e-15 and gn.MIN_TOL == 0.01
    assert gn.gauss_params(0.0, -50.0)[1] >= 0.01 and gn.gauss_params(0.0, 12.0)[1] == 12.01         # MIN_TOL floors sd; Softplus is the identity from 10 on
    # the score is the derivative of the log density in the builder's two arguments, the mean and the variance
    for a in (-2.5, -1.0, 0.3, 1.0, 1.5):
        var, h = sd * sd, 1e-6
        gm, gv = gn.gauss_score(mu, sd, a)
        d_mu = (gn.gauss_logpdf(mu + h, var, a) - gn.gauss_logpdf(mu - h, var, a)) / (2 * h)
        d_var = (gn.gauss_logpdf(mu, var + h, a) - gn.gauss_logpdf(mu, var - h, a)) / (2 * h)
        assert abs(gm - d_mu) <= 1e-8 * max(1.0, abs(gm)) and abs(gv - d_var) <= 1e-8 * max(1.0, abs(gv)), (a, gm, d_mu, gv, d_var)
        assert abs(np.log(gn.gauss_pdf(mu, sd, a)) - gn.gauss_logpdf(mu, var, a)) < 1e-13
        # NOT the derivative in sd: that one carries the factor d Sigma / d sd = 2 sd, which grad_log leaves out
        d_sd = (gn.gauss_logpdf(mu, (sd + h) ** 2, a) - gn.gauss_logpdf(mu, (sd - h) ** 2, a)) / (2 * h)
        assert abs(d_sd - 2.0 * sd * gv) <= 1e-7 * max(1.0, abs(d_sd))
    # the density integrates to 1 (trapezoid over mu +- 12 sd) and peaks at the mode, mu
    x = np.linspace(mu - 12 * sd, mu + 12 * sd, 200001)
    p = gn.gauss_pdf(mu, sd, x)
    assert abs(float(np.sum((p[1:] + p[:-1]) * np.diff(x)) / 2.0) - 1.0) < 1e-9 and abs(x[np.argmax(p)] - mu) <= x[1] - x[0]


def test_psi_q_and_sarsa_handle_by_hand():
    for a in (0.3, -1.0, 1.0, 1.5):
        cm, cs, _, _ = _by_hand(PHI, a)
        p = gn.psi(W, PHI, a)
        assert p.shape == (12,) and np.allclose(p[:4], cm * PHI, rtol=1e-14, atol=0) and np.allclose(p[4:8], cs * PHI, rtol=1e-13, atol=0)
        assert np.array_equal(p[8:], PHI) and np.isfinite(p).all()
        q = cm * (W3[:4] @ PHI) + cs * (W3[4:8] @ PHI) + W3[8:] @ PHI
        assert abs(gn.q_value(W3, W, PHI, a) - q) <= 1e-13 * max(1.0, abs(q))
    assert gn.q_value(np.zeros(12), W, PHI, 0.3) == 0.0
    # the action is NOT clamped: 1.5 and 1 give different features
    assert not np.allclose(gn.psi(W, PHI, 1.5)[:8], gn.psi(W, PHI, 1.0)[:8])
    phi_n, a, na, r, gamma, lr = np.array([1.0, 0.5, -0.25, 1.0]), 0.3, -0.7, -1.0, 0.9, 0.01
    q, qn = gn.q_value(W3, W, PHI, a), gn.q_value(W3, W, phi_n, na)
    d, w2 = gn.sarsa_handle(W3, W, PHI, a, r, phi_n, na, True, gamma, lr)
    assert d == r - q and np.allclose(w2, W3 + lr * (r - q) * gn.psi(W, PHI, a), rtol=1e-15, atol=0)
    d, w2 = gn.sarsa_handle(W3, W, PHI, a, r, phi_n, na, False, gamma, lr)
    assert abs(d - (r + gamma * qn - q)) <= 1e-15 * abs(d) and np.allclose(w2, W3 + lr * d * gn.psi(W, PHI, a), rtol=1e-15, atol=0)
    assert gn.sarsa_handle(W3, W, PHI, a, r, 7.0 * phi_n, 0.01, True, gamma, lr)[0] == r - q      # the terminal rule reads neither s' nor the draw
    assert np.allclose(w2[8:] - W3[8:], lr * d * PHI, rtol=1e-12, atol=0)
    # NAC::handle(()) does not read the policy: tests/nac_numpy.py's, with the columns the mean's and the stddev's
    W2, norm = nn.nac_handle(W3, W, 0.01)
    want = np.sqrt(sum((k / 10.0) ** 2 for k in range(1, 9)))
    assert abs(norm - want) <= 1e-15 and np.allclose(W2[:, 0], W[:, 0] + 0.01 / want * W3[:4], rtol=1e-15, atol=0)
    assert np.allclose(W2[:, 1], W[:, 1] + 0.01 / want * W3[4:8], rtol=1e-15, atol=0)


def test_the_sample_is_box_mullers_cosine_normal_on_one_philox_block(orc):
    ids = np.arange(5)
    for purpose, t in ((bn.BLK_STEP, 0), (gn.BLK_INNER, 3), (bn.BLK_INIT, 0), (bn.BLK_API, 2 ** 33 + 1)):
        z = gn.gauss_normal(7, ids, t, purpose)
        for i in ids:
            wx, wy = orc.draw(7, int(i), t, purpose + 256)[:2]
            u1, u2 = ((wx >> 8) + 1) / 2.0 ** 24, (wy >> 8) / 2.0 ** 24
            assert z[i] == np.sqrt(-2.0 * np.log(u1)) * np.cos(float(np.float32(6.2831854820251465)) * u2), (purpose, i)
    # a function of (seed, id, t, purpose) only; the streams differ
    assert np.array_equal(gn.gauss_normal(7, ids, 3, 2), gn.gauss_normal(7, ids, 3, 2)) and not np.array_equal(gn.gauss_normal(7, ids, 3, 2), gn.gauss_normal(7, ids, 3, 0))
    z = np.concatenate([gn.gauss_normal(5, np.arange(4096), t, bn.BLK_API) for t in range(16)])      # n = 65 536
    n = z.size
    assert abs(z.mean()) < 5.0 / np.sqrt(n) and abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / n) and np.abs(z).max() <= gn.Z_MAX < 5.77
    assert np.array_equal(gn.gauss_sample(5, ids, 0, 4, 0.25, 2.0), 0.25 + 2.0 * gn.gauss_normal(5, ids, 0, 4))


@pytest.mark.parametrize("order", [1, 3, 5])
def test_the_gpu_rule_case(orc, order):
    """handle_case: |x_m| <= 1 and x_s in [-1, 3] at every state of the case (so sd >= 0.32), actions in [-1.5, 1.5] with -1 and 1 exactly, both
    kinds of transition in every round, and w moves by more than 1e-3 under the f64 rule"""
    case = gn.handle_case(order)
    N = len(case["init"])
    proj = lambda S: np.stack([orc.fourier_project(orc.MOUNTAIN_CAR, order, S[:, i]) for i in range(N)], axis=1)      # noqa: E731
    phi_s, phi_n = [proj(r[0]) for r in case["rounds"]], [proj(r[3]) for r in case["rounds"]]
    assert N == 67 and case["F"] == (order + 1) ** 2
    for ph in phi_s + phi_n:
        assert np.abs(ph).max() <= 1.0 + 1e-12 and np.allclose(ph[-1], 1.0)                 # the constant feature is the last one
        xm = np.array([ph[:, i] @ case["init"][i][1][:, 0].astype(np.float64) for i in range(N)])
        xs = np.array([ph[:, i] @ case["init"][i][1][:, 1].astype(np.float64) for i in range(N)])
        assert np.abs(xm).max() <= 1.0 + 1e-6 and xs.min() >= -1.0 - 1e-6 and xs.max() <= 3.0 + 1e-6
        assert gn.gauss_params(xm, xs)[1].min() >= 0.32
    for frm, a, rew, nxt, term in case["rounds"]:
        assert 0 < term.sum() < N and a[0] == -1.0 and a[1] == 1.0 and a.min() >= -1.5 and a.max() <= 1.5 and (np.abs(a) > 1.0).sum() > 5
    w, deltas = gn.critic_after(case, gn.RULE_SEED, phi_s, phi_n)
    w0 = np.stack([x for x, _ in case["init"]]).astype(np.float64)
    assert np.abs(w0).sum(axis=1).max() <= 3.0 + 1e-5 and np.max(np.abs(w - w0)) > 1e-3 and np.isfinite(w).all()
    assert all(np.isfinite(d).all() for d in deltas)


# ---- the interface
def test_header_binding_constants_and_rust_block_agree():
    gen = _load("gen_rust_sys")
    h = open(os.path.join(ROOT, "include", "rsrl_hip.h")).read()
    assert re.search(r"RSRL_BETA\s*=\s*4\s*,\s*RSRL_GAUSSIAN\s*=\s*6\b", h) and "(5 is no policy.)" in h
    assert rsrl_amd.GAUSSIAN == 6 and rsrl_amd.context.GAUSSIAN == 6 and rsrl_amd.BETA == 4 and rsrl_amd.NAC == 28
    assert re.search(r"#define\s+RSRL_HIP_ABI_VERSION\s+9\b", h)
    block = gen.doc_block()
    assert "pub const RSRL_GAUSSIAN: i32 = 6;" in block and "pub const RSRL_NAC: i32 = 28;" in block and block == gen.generate()
    # no new entry point: the exports are the parent's
    assert len(gen.parse_header()[0]) == len(dict(gen.declared_functions(block))) == 96


def test_supported_configurations_reach_the_device_query():
    for order in (1, 2, 3, 4, 5):
        for extra in (dict(), dict(steps_per_launch=1), dict(max_episode_steps=1000, lr=0.01, alpha=0.01, gamma=0.999), dict(n_steps=1), dict(n_steps=65536)):
            rc, msg = create_rc(BASE, order=order, **extra)
            assert rc == 0 or (rc == EHIP and "device" in msg), (order, extra, rc, msg)


def test_other_configurations_are_refused_with_a_message():
    bad = [dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(order=7), dict(weight_mode=rsrl_amd.W_SHARED), dict(weight_dtype=rsrl_amd.W_BF16),
           dict(agent_policy=rsrl_amd.SOFTMAX), dict(epsilon_decay=0.99), dict(domain=rsrl_amd.MOUNTAIN_CAR), dict(domain=rsrl_amd.CART_POLE, order=1),
           dict(domain=rsrl_amd.HIV_TREATMENT, order=1)]
    # the Gaussian policy under any other algo, the iLSTD ActorCritic included
    bad += [dict(algo=a) for a in (rsrl_amd.ILSTD_ACTOR_CRITIC, rsrl_amd.QLEARNING, rsrl_amd.SARSA, rsrl_amd.TD, rsrl_amd.TD_ACTOR_CRITIC, rsrl_amd.REINFORCE,
                                   rsrl_amd.ILSTD, rsrl_amd.GRADIENT_MC, rsrl_amd.LSTD, rsrl_amd.GTD2)]
    bad += [dict(algo=rsrl_amd.ILSTD_ACTOR_CRITIC, n_steps=2), dict(algo=rsrl_amd.QLEARNING, domain=rsrl_amd.MOUNTAIN_CAR)]
    for b in bad:
        rc, msg = create_rc(BASE, **dict(dict(max_episode_steps=10), **b))
        assert rc == EINVAL and "RSRL_NAC" in msg and "RSRL_GAUSSIAN" in msg and "RSRL_BETA" in msg and "RSRL_CONTINUOUS_MOUNTAIN_CAR" in msg and \
            "orders 1-5" in msg, (b, rc, msg)
    for n in (0, -1, 65537):
        rc, msg = create_rc(BASE, n_steps=n)
        assert rc == EINVAL and "RSRL_NAC" in msg and "n_steps" in msg and "65536" in msg, (n, rc, msg)
    rc, msg = create_rc(BASE, order=0)
    assert rc == EINVAL and "order" in msg


def test_five_and_seven_are_no_policies_and_six_is_no_agent_policy():
    for pol in (5, 7, -1):
        for kw in (dict(), dict(domain=rsrl_amd.MOUNTAIN_CAR, algo=rsrl_amd.QLEARNING), dict(algo=rsrl_amd.ILSTD_ACTOR_CRITIC, n_steps=2)):
            rc, msg = create_rc(BASE, policy=pol, **kw)
            assert rc == EINVAL and "unknown policy %d" % pol in msg, (pol, kw, rc, msg)
    for kw in (dict(), dict(policy=rsrl_amd.BETA), dict(domain=rsrl_amd.MOUNTAIN_CAR, algo=rsrl_amd.SARSA, policy=rsrl_amd.GREEDY)):
        rc, msg = create_rc(BASE, agent_policy=6, **kw)
        assert rc == EINVAL and "unknown agent policy 6" in msg, (kw, rc, msg)


def test_gaussian_grid_and_its_fixture(matrix):
    doc = json.load(open(matrix.GAUSS_FIXTURE))
    assert doc["grid"] == [[n, v] for n, v in matrix.GRID_GAUSS], "GRID_GAUSS and its fixture drifted apart"
    assert dict(matrix.GRID_GAUSS) == dict(policy=[4, 5, 6, 7], algo=[21, 28], domain=[0, 4], agent_policy=[-1, 6], order=[0, 1, 2, 3, 4, 5, 6],
                                           n_steps=[0, 1, 100, 65536, 65537])
    names = [n for n, _ in matrix.GRID_GAUSS]
    vals = dict(matrix.GRID_GAUSS)
    rows = [{n: vals[n][int(ch, 16)] for n, ch in zip(names, key)} for key in doc["admitted"]]
    gauss = [r for r in rows if r["policy"] == 6]
    # exactly: NAC, ContinuousMountainCar, agent_policy -1, orders 1-5, the period in [1, 65 536]
    assert len(gauss) == 15 and all(r["algo"] == 28 and r["domain"] == 4 and r["agent_policy"] == -1 for r in gauss)
    assert sorted({r["order"] for r in gauss}) == [1, 2, 3, 4, 5] and sorted({r["n_steps"] for r in gauss}) == [1, 100, 65536]
    assert not any(r["policy"] in (5, 7) for r in rows)
    # Beta's rows are what they were: NAC's fifteen and the iLSTD ActorCritic's five (n_steps = 1 is the one value inside its own range)
    beta = [r for r in rows if r["policy"] == 4]
    assert len(beta) == 20 and all(r["domain"] == 4 and r["agent_policy"] == -1 for r in beta) and sum(r["algo"] == 21 for r in beta) == 5


def _gfx950_visible():
    import subprocess
    try:
        return subprocess.run(["/opt/rocm/bin/rocminfo"], capture_output=True, text=True).stdout.count("gfx950") > 0
    except Exception:
        return False


def test_create_admits_exactly_the_gaussian_fixture(matrix):
    if _gfx950_visible():
        pytest.skip("GPU present: an admitted configuration would create a real ctx")
    from rsrl_amd import _build
    _build.build()
    res = matrix.sweep(matrix.GRID_GAUSS)
    assert matrix.admitted(res) == json.load(open(matrix.GAUSS_FIXTURE))["admitted"]
    for key, (rc, msg) in res.items():
        if rc != matrix.EHIP:
            assert rc == matrix.EINVAL and msg, (key, rc, msg)


def test_example_compiles(tmp_path):
    compile_example(tmp_path, "nac")
