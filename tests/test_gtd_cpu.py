"""GTD2 and TDC (RSRL_GTD2 = 30, RSRL_TDC = 31) without a GPU: the three restatements of tests/gtd_numpy.py agree where they must (the scaled f64
rule at lr = lr_td = 1 is the reference's text; the f32 device-order rule of TDC without its estimator is the oracle's TD handle), the header, the
Python constants and the Rust block agree, every supported configuration passes admission and reaches the device query while every other one is
refused with a message naming the agent, 29 and 32 are no algos, the admission grid equals its fixture, and examples/gtd2.cpp compiles."""
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import rsrl_amd
from tests import gtd_numpy as gn
from tests.agent_contract import compile_example, create_rc, rand_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EHIP = -1, -2
SUPPORTED = [(rsrl_amd.MOUNTAIN_CAR, o) for o in (1, 2, 3, 4, 5)] + [(rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]
AGENTS = [(rsrl_amd.GTD2, "RSRL_GTD2"), (rsrl_amd.TDC, "RSRL_TDC")]
BASE = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, policy=rsrl_amd.RANDOM, n_envs=4, lr=0.02, lr_td=0.05)


def _gfx950_visible():
    try:
        return subprocess.run(["/opt/rocm/bin/rocminfo"], capture_output=True, text=True).stdout.count("gfx950") > 0
    except Exception:
        return False


@pytest.fixture(scope="module")
def matrix():
    spec = importlib.util.spec_from_file_location("admission_matrix", os.path.join(ROOT, "scripts", "admission_matrix.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _transitions(orc, domain, order, n, rng, prec):
    S, S2 = rand_states(orc, domain, n, rng), rand_states(orc, domain, n, rng)
    return gn.project(orc, domain, order, S, prec), gn.project(orc, domain, order, S2, prec), S, S2


@pytest.mark.parametrize("algo", [gn.GTD2, gn.TDC])
@pytest.mark.parametrize("domain,order", [(rsrl_amd.MOUNTAIN_CAR, 1), (rsrl_amd.MOUNTAIN_CAR, 3), (rsrl_amd.CART_POLE, 1)])
def test_scaled_rule_at_unit_rates_is_the_references_text(orc, algo, domain, order):
    """three transitions in a row (the second terminal), each side free-running: 1e-12 of max(1, |.|).  Unit steps grow the weights, which is the
    departure's reason; three transitions stay finite"""
    rng = np.random.default_rng(10 * domain + order + algo)
    phi_s, phi_n, _, _ = _transitions(orc, domain, order, 3, rng, "f64")
    F = phi_s.shape[1]
    th_a = th_b = rng.normal(0.0, 0.3, size=F)
    w_a = w_b = rng.normal(0.0, 0.3, size=F)
    gamma = 0.95
    for k in range(3):
        r, term = float(rng.normal()), k == 1
        td_a, th_a, w_a = gn.rule_f64(algo, th_a, w_a, phi_s[k], phi_n[k], r, term, gamma, 1.0, 1.0)
        td_b, th_b, w_b = gn.literal(algo, th_b, w_b, phi_s[k], phi_n[k], r, term, gamma, sgd_rate=1.0)
        for got, want in ((td_a, td_b), (th_a, th_b), (w_a, w_b)):
            assert np.max(np.abs(np.asarray(got) - np.asarray(want))) <= 1e-12 * max(1.0, np.max(np.abs(want))), k
    assert np.isfinite(th_a).all() and np.isfinite(w_a).all()
    # TDC's td_est goes through its SGD: the scaled rule's lr_td is that rate
    td_a, th_a, w_a = gn.rule_f64(gn.TDC, th_b, w_b, phi_s[0], phi_n[0], 0.5, False, gamma, 1.0, 0.25)
    td_b, th_c, w_c = gn.literal(gn.TDC, th_b, w_b, phi_s[0], phi_n[0], 0.5, False, gamma, sgd_rate=0.25)
    assert td_a == td_b and np.max(np.abs(w_a - w_c)) <= 1e-12 * max(1.0, np.max(np.abs(w_c))) and np.max(np.abs(th_a - th_c)) <= 1e-12 * max(1.0, np.max(np.abs(th_c)))


def test_literal_rules_on_hand_worked_numbers():
    # phi = (1, 0), phi' = (0, 1), theta = (2, 3), w = (0.5, 7), r = 1, gamma = 0.5: w_s = 0.5, th_s = 2, th_n = 3, td = 1 + 1.5 - 2 = 0.5
    th, w, ps, pn = [2.0, 3.0], [0.5, 7.0], [1.0, 0.0], [0.0, 1.0]
    td, th2, w2 = gn.literal(gn.GTD2, th, w, ps, pn, 1.0, False, 0.5)
    assert td == 0.5 and w2.tolist() == [0.5, 7.0] and th2.tolist() == [2.5, 3.0 - 0.5 * 0.5]      # w += (td - w_s) phi = 0; theta += w_s (phi - gamma phi')
    td, th2, w2 = gn.literal(gn.TDC, th, w, ps, pn, 1.0, False, 0.5, sgd_rate=0.1)
    assert td == 0.5 and w2.tolist() == [0.5, 7.0] and th2.tolist() == [2.5, 2.5]                   # theta += td phi - w_s phi': no gamma on the correction
    # terminal: td = r - th_s = -1; phi' is subtracted all the same
    td, th2, w2 = gn.literal(gn.GTD2, th, w, ps, pn, 1.0, True, 0.5)
    assert td == -1.0 and w2.tolist() == [0.5 - 1.5, 7.0] and th2.tolist() == [2.5, 2.75]
    td, th2, w2 = gn.literal(gn.TDC, th, w, ps, pn, 1.0, True, 0.5, sgd_rate=0.1)
    assert td == -1.0 and np.allclose(w2, [0.5 - 0.15, 7.0], rtol=1e-15, atol=0) and th2.tolist() == [1.0, 2.5]


@pytest.mark.parametrize("domain,order", SUPPORTED)
def test_f32_tdc_without_its_estimator_is_the_oracles_td_handle(orc, domain, order):
    """w = 0 and lr_td = 0: the first axpy is TD's, the second adds a zero.  Compared as values (a zero's sign is the second axpy's)"""
    rng = np.random.default_rng(7 * domain + order)
    n, gamma, lr = 9, 0.95, 0.05
    phi_s, phi_n, S, S2 = _transitions(orc, domain, order, n, rng, "f32d")
    F = phi_s.shape[1]
    th0 = rng.normal(0.0, 0.3, size=(n, F)).astype(np.float32)
    r = rng.normal(0.0, 1.0, size=n).astype(np.float32)
    term = rng.random(n) < 0.4
    td, th2, w2 = gn.rule_f32(gn.TDC, th0, np.zeros((n, F), np.float32), phi_s, phi_n, r, term, gamma, lr, 0.0)
    assert td.dtype == np.float32 and th2.dtype == np.float32 and not w2.any()
    ag = orc.make_agent(domain=domain, order=order, algo=orc.TD, policy=orc.RANDOM, gamma=gamma, lr=lr)
    for i in range(n):
        w = th0[i].copy()
        d = orc.handle_td(ag, w, None, S[:, i], r[i], S2[:, i], bool(term[i]), "f32d")
        assert np.float32(d) == td[i] and np.array_equal(w, th2[i]), i
    assert term.any() and not term.all() and np.max(np.abs(th2 - th0)) > 0


@pytest.mark.parametrize("algo", [gn.GTD2, gn.TDC])
def test_f32_rule_stays_within_the_teacher_forcing_bounds_of_the_f64_rule(orc, algo):
    """the bit-exact reference of the GPU tests against the f64 rule, both free-running over 64 transitions from one start: TD error 2e-4,
    weights 1.4e-5 of max(1, |.|), at MountainCar order 3"""
    domain, order, gamma, lr, lr_td, n = rsrl_amd.MOUNTAIN_CAR, 3, 0.95, 0.02, 0.05, 64
    rng = np.random.default_rng(algo)
    S, S2 = rand_states(orc, domain, n, rng), rand_states(orc, domain, n, rng)
    p32, n32 = gn.project(orc, domain, order, S, "f32d"), gn.project(orc, domain, order, S2, "f32d")
    p64, n64 = gn.project(orc, domain, order, S, "f64"), gn.project(orc, domain, order, S2, "f64")
    F = p32.shape[1]
    th32, w32 = rng.uniform(-0.5, 0.5, size=(1, F)).astype(np.float32), rng.uniform(-0.5, 0.5, size=(1, F)).astype(np.float32)
    th64, w64 = th32[0].astype(np.float64), w32[0].astype(np.float64)
    worst_td = worst_w = 0.0
    for k in range(n):
        r, term = np.float32(-1.0), bool(rng.random() < 0.1)
        td32, th32, w32 = gn.rule_f32(algo, th32, w32, p32[k:k + 1], n32[k:k + 1], [r], [term], gamma, lr, lr_td)
        td64, th64, w64 = gn.rule_f64(algo, th64, w64, p64[k], n64[k], float(r), term, gamma, lr, lr_td)
        worst_td = max(worst_td, abs(float(td32[0]) - td64))
        for a, b in ((th32[0], th64), (w32[0], w64)):
            worst_w = max(worst_w, np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))
    print("f32 against f64 over %d transitions: td %.3g, weights %.3g of max(1, |.|)" % (n, worst_td, worst_w))
    assert worst_td <= 2e-4 and worst_w <= 1.4e-5, (worst_td, worst_w)


def test_header_python_constants_and_rust_block_agree():
    h = open(os.path.join(ROOT, "include", "rsrl_hip.h")).read()
    rust = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for value, name in AGENTS:
        assert re.search(name + r"\s*=\s*%d\b" % value, h)
        assert "pub const %s: i32 = %d;" % (name, value) in rust
    assert (rsrl_amd.GTD2, rsrl_amd.TDC) == (30, 31) and (rsrl_amd.context.GTD2, rsrl_amd.context.TDC) == (30, 31) and (gn.GTD2, gn.TDC) == (30, 31)
    enum = h.split("rsrl_algo;")[0].split("typedef enum { RSRL_QLEARNING")[1]
    assert not re.search(r"=\s*29\b\s*[,}]", enum) and "(29 is no algo.)" in enum
    assert re.search(r"#define\s+RSRL_HIP_ABI_VERSION\s+9\b", h)


def test_supported_configurations_reach_the_device_query():
    for algo, _ in AGENTS:
        for domain, order in SUPPORTED:
            for extra in (dict(), dict(steps_per_launch=1), dict(max_episode_steps=37), dict(lr=1.0, lr_td=1.0, gamma=0.99), dict(lr=0.0, lr_td=0.0)):
                rc, msg = create_rc(BASE, algo=algo, domain=domain, order=order, **extra)
                # no GPU: every admission rule has passed and the device query answers "no device"; with one, the ctx is created
                assert rc == 0 or (rc == EHIP and "device" in msg), (algo, domain, order, extra, rc, msg)


def test_other_configurations_are_refused_with_the_agents_name():
    bad = [dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(order=7), dict(domain=rsrl_amd.CART_POLE, order=2),
           dict(domain=rsrl_amd.CART_POLE, order=7), dict(domain=rsrl_amd.ACROBOT, order=3), dict(weight_mode=rsrl_amd.W_SHARED),
           dict(domain=rsrl_amd.CART_POLE, order=7, weight_dtype=rsrl_amd.W_BF16), dict(weight_dtype=rsrl_amd.W_BF16),
           dict(domain=rsrl_amd.HIV_TREATMENT, order=1), dict(policy=rsrl_amd.EPSILON_GREEDY), dict(policy=rsrl_amd.GREEDY),
           dict(policy=rsrl_amd.SOFTMAX), dict(agent_policy=rsrl_amd.RANDOM), dict(agent_policy=rsrl_amd.SOFTMAX), dict(epsilon_decay=0.99)]
    for algo, name in AGENTS:
        for b in bad:
            rc, msg = create_rc(BASE, algo=algo, **b)
            assert rc == EINVAL and name in msg and "register-family Fourier" in msg, (b, rc, msg)
        for lr_td in (-1.0, -1e-9, float("nan")):
            rc, msg = create_rc(BASE, algo=algo, lr_td=lr_td)
            assert rc == EINVAL and "lr_td must be >= 0" in msg, (lr_td, rc, msg)


def test_twenty_nine_and_thirty_two_are_no_algos():
    for algo in (29, 32, 1000):
        for kw in (dict(), dict(policy=rsrl_amd.SOFTMAX), dict(lr_td=-1.0)):
            rc, msg = create_rc(BASE, algo=algo, **kw)
            assert rc == EINVAL and "unknown algo %d" % algo in msg, (algo, kw, rc, msg)


def test_gtd_grid_is_the_first_on_algos_29_to_32_with_an_lr_td_axis(matrix):
    assert dict(matrix.GRID_GTD)["algo"] == [29, 30, 31, 32] and dict(matrix.GRID_GTD)["lr_td"] == [0.0, -1.0]
    assert [n for n, _ in matrix.GRID] + ["lr_td"] == [n for n, _ in matrix.GRID_GTD]
    assert all(v == w for (n, v), (_, w) in zip(matrix.GRID, matrix.GRID_GTD) if n != "algo"), "the grid's other axes are the first's"
    doc = json.load(open(matrix.GTD_FIXTURE))
    assert doc["grid"] == [[n, v] for n, v in matrix.GRID_GTD] and "fixed" not in doc, "GRID_GTD and its fixture drifted apart"
    # admission is exactly RecursiveLSTD's (18) for both agents, at lr_td = 0 only
    ia = [n for n, _ in matrix.GRID].index("algo")
    second = json.load(open(matrix.AGENTS_FIXTURE))
    i18 = "%x" % dict(matrix.GRID_AGENTS)["algo"].index(18)
    of18 = sorted(k[:ia] + "_" + k[ia + 1:] for k in second["admitted"] if k[ia] == i18)
    for digit in ("1", "2"):
        assert of18 and of18 == sorted(k[:ia] + "_" + k[ia + 1:-1] for k in doc["admitted"] if k[ia] == digit)
    assert {k[ia] for k in doc["admitted"]} == {"1", "2"} and {k[-1] for k in doc["admitted"]} == {"0"}


def test_create_admits_exactly_the_gtd_fixture(matrix):
    if _gfx950_visible():
        pytest.skip("GPU present: an admitted configuration would create a real ctx")
    from rsrl_amd import _build
    _build.build()
    res = matrix.sweep(matrix.GRID_GTD)
    assert matrix.admitted(res) == json.load(open(matrix.GTD_FIXTURE))["admitted"]
    ia = [n for n, _ in matrix.GRID_GTD].index("algo")
    for key, (rc, msg) in res.items():
        if rc != matrix.EHIP:
            assert rc == matrix.EINVAL and msg, (key, rc, msg)
        if key[ia] in "03":
            assert rc == matrix.EINVAL and "unknown algo %d" % (29 if key[ia] == "0" else 32) in msg, (key, rc, msg)


def test_example_compiles(tmp_path):
    compile_example(tmp_path, "gtd2")
