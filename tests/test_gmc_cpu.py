"""GradientMC (RSRL_GRADIENT_MC, 23) without a GPU: the header, the binding table and the Python constant agree, a hand-worked trajectory pins the
literal rule (tests/gmc_numpy.py), the rule equals the backward chain of the oracle's TD terminal update the GPU tests compare against bit for bit,
every supported configuration passes admission and reaches the device query while every other one is refused with a message naming the agent, 22 is
no algo, the admission grid of 22 and 23 equals its fixture, and examples/gradient_mc.cpp compiles."""
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import rsrl_amd
from rsrl_amd import _abi
from tests.agent_contract import compile_example, create_rc, rand_states
from tests.gmc_numpy import f32_returns, gradient_mc, td_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EHIP = -1, -2
SUPPORTED = [(rsrl_amd.MOUNTAIN_CAR, o) for o in (1, 2, 3, 4, 5)] + [(rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]
CHAIN = [(rsrl_amd.MOUNTAIN_CAR, 1), (rsrl_amd.MOUNTAIN_CAR, 2), (rsrl_amd.MOUNTAIN_CAR, 3), (rsrl_amd.MOUNTAIN_CAR, 5), (rsrl_amd.CART_POLE, 1),
         (rsrl_amd.ACROBOT, 1)]
NAME = "RSRL_GRADIENT_MC"

BASE = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=rsrl_amd.GRADIENT_MC, policy=rsrl_amd.RANDOM, n_envs=4, max_episode_steps=50)


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


def test_header_binding_table_and_python_constant_agree():
    h = open(os.path.join(ROOT, "include", "rsrl_hip.h")).read()
    assert re.search(NAME + r"\s*=\s*23\b", h)
    enum = h.split("rsrl_algo;")[0].split("typedef enum { RSRL_QLEARNING")[1]
    assert not re.search(r"=\s*22\b\s*[,}]", enum) and "(22 is no algo.)" in enum
    assert rsrl_amd.GRADIENT_MC == 23 and rsrl_amd.context.GRADIENT_MC == 23
    assert "pub const %s: i32 = 23;" % NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"#define\s+RSRL_HIP_ABI_VERSION\s+9\b", h)
    for sym in ("rsrl_hip_get_episode_record", "rsrl_hip_set_episode_record"):
        assert "int %s(" % sym in h and len(_abi.SYMBOLS[sym][1]) == 3


def test_rule_on_a_hand_worked_trajectory():
    # visited last to first: sum = 2, pred = -1, error 3, w1 = -1 + 0.3; then sum = 1 + 0.5 * 2 = 2, pred = 0.5, error 1.5, w0 = 0.5 + 0.15
    w, errors, returns = gradient_mc([0.5, -1.0], [[1.0, 0.0], [0.0, 1.0]], [1.0, 2.0], 0.5, 0.1)
    assert errors == [3.0, 1.5] and list(returns) == [2.0, 2.0]
    assert np.allclose(w, [0.65, -0.7], rtol=1e-15, atol=0)
    # the second visit reads the w the first one left: on a shared feature the order matters
    w2, errors2, _ = gradient_mc([0.5], [[1.0], [1.0]], [1.0, 2.0], 0.5, 0.1)
    assert errors2 == [1.5, 2.0 - (0.5 + 0.15)] and np.allclose(w2, [0.65 + 0.1 * 1.35], rtol=1e-15, atol=0)
    # no trajectory, no update; the f32 return is a multiply followed by an add
    assert gradient_mc([0.5], [], [], 0.5, 0.1)[0].tolist() == [0.5]
    assert list(f32_returns([1.0, 2.0], 0.5)) == [2.0, 2.0] and f32_returns([], 0.5).shape == (0,)
    g = f32_returns([0.1, 0.3, 0.7], 0.9)
    assert g[1] == np.float32(np.float32(0.3) + np.float32(np.float32(0.9) * np.float32(0.7)))


def _case(orc, domain, order, T=9, lr=0.01, gamma=0.95):
    rng = np.random.default_rng(100 * domain + order)
    S = rand_states(orc, domain, T, rng).T.copy()                   # (T, D)
    R = rng.normal(0.0, 1.0, size=T).astype(np.float32)
    ag = orc.make_agent(domain=domain, order=order, algo=orc.TD, policy=orc.RANDOM, gamma=gamma, lr=lr)
    F = (order + 1) ** S.shape[1]
    w0 = rng.normal(0.0, 0.3, size=F).astype(np.float32)
    return ag, S, R, w0, lr, gamma


@pytest.mark.parametrize("domain,order", CHAIN)
def test_literal_rule_is_the_backward_chain_of_td_terminal_updates(orc, domain, order):
    ag, S, R, w0, lr, gamma = _case(orc, domain, order)
    phis = [orc.fourier_project(domain, order, s) for s in S]
    want, errors, returns = gradient_mc(w0.astype(np.float64), phis, R.astype(np.float64), gamma, lr)
    w = w0.astype(np.float64)
    got_errors, got_returns = td_chain(orc, ag, w, S, R.astype(np.float64), gamma, "f64")
    assert np.max(np.abs(w - want)) <= 1e-12 and np.max(np.abs(np.array(got_errors) - np.array(errors))) <= 1e-12
    assert np.array_equal(got_returns, returns)
    assert np.max(np.abs(want - w0)) > 0


@pytest.mark.parametrize("domain,order", CHAIN)
def test_f32_device_order_chain_stays_within_the_f64_campaigns_bound(orc, domain, order):
    """the bit-exact reference of the GPU tests (prec "f32d", the return formed in f32) against the f64 chain: within the bound the f64 campaign
    holds TD's weights to, 1.4e-5 of max(1, |w|), at T = 9"""
    ag, S, R, w0, lr, gamma = _case(orc, domain, order)
    w64, w32 = w0.astype(np.float64), w0.copy()
    td_chain(orc, ag, w64, S, R.astype(np.float64), gamma, "f64")
    _, rets = td_chain(orc, ag, w32, S, R, gamma, "f32d")
    assert rets.dtype == np.float32 and w32.dtype == np.float32
    gap = np.max(np.abs(w32.astype(np.float64) - w64)) / max(1.0, np.max(np.abs(w64)))
    print("f32d against f64: %.3g of max(1, |w|)" % gap)
    assert gap <= 1.4e-5, gap


def test_supported_configurations_reach_the_device_query():
    for domain, order in SUPPORTED:
        for extra in (dict(), dict(steps_per_launch=1), dict(max_episode_steps=1), dict(max_episode_steps=1000, lr=0.01, gamma=0.99)):
            rc, msg = create_rc(BASE, domain=domain, order=order, **extra)
            # no GPU: every admission rule has passed and the device query answers "no device"; with one, the ctx is created
            assert rc == 0 or (rc == EHIP and "device" in msg), (domain, order, extra, rc, msg)


def test_other_configurations_are_refused_with_a_message():
    bad = [dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(order=7), dict(domain=rsrl_amd.CART_POLE, order=2),
           dict(domain=rsrl_amd.CART_POLE, order=7), dict(domain=rsrl_amd.ACROBOT, order=3), dict(weight_mode=rsrl_amd.W_SHARED),
           dict(domain=rsrl_amd.CART_POLE, order=7, weight_dtype=rsrl_amd.W_BF16), dict(weight_dtype=rsrl_amd.W_BF16),
           dict(domain=rsrl_amd.HIV_TREATMENT, order=1), dict(policy=rsrl_amd.EPSILON_GREEDY), dict(policy=rsrl_amd.GREEDY),
           dict(policy=rsrl_amd.SOFTMAX), dict(agent_policy=rsrl_amd.RANDOM), dict(agent_policy=rsrl_amd.SOFTMAX), dict(epsilon_decay=0.99)]
    for b in bad:
        rc, msg = create_rc(BASE, **b)
        assert rc == EINVAL and NAME in msg and "register-family Fourier" in msg, (b, rc, msg)
    rc, msg = create_rc(BASE, max_episode_steps=0)
    assert rc == EINVAL and NAME in msg and "max_episode_steps" in msg and "no record size" in msg, (rc, msg)


def test_twenty_two_and_a_far_value_are_no_algos():
    for algo in (22, 1000):
        for kw in (dict(), dict(policy=rsrl_amd.SOFTMAX), dict(max_episode_steps=0)):
            rc, msg = create_rc(BASE, algo=algo, **kw)
            assert rc == EINVAL and "unknown algo %d" % algo in msg, (algo, kw, rc, msg)


def test_fourth_grid_is_the_first_on_algos_22_and_23(matrix):
    assert dict(matrix.GRID_AGENTS3)["algo"] == [22, 23] and matrix.FIXED_AGENTS3 == {"max_episode_steps": 200}
    assert [n for n, _ in matrix.GRID] == [n for n, _ in matrix.GRID_AGENTS3]
    assert all(v == w for (n, v), (_, w) in zip(matrix.GRID, matrix.GRID_AGENTS3) if n != "algo"), "the grid's other axes are the first's"
    doc = json.load(open(matrix.AGENTS3_FIXTURE))
    assert doc["grid"] == [[n, v] for n, v in matrix.GRID_AGENTS3] and doc["fixed"] == matrix.FIXED_AGENTS3, "GRID_AGENTS3 and its fixture drifted apart"
    # admission is exactly RecursiveLSTD's (18): the fixture's keys with the algo digit replaced are the second fixture's keys of 18
    ia = [n for n, _ in matrix.GRID].index("algo")
    second = json.load(open(matrix.AGENTS_FIXTURE))
    i18 = "%x" % dict(matrix.GRID_AGENTS)["algo"].index(18)
    of18 = sorted(k[:ia] + "_" + k[ia + 1:] for k in second["admitted"] if k[ia] == i18)
    assert of18 and of18 == sorted(k[:ia] + "_" + k[ia + 1:] for k in doc["admitted"])
    assert {k[ia] for k in doc["admitted"]} == {"1"}                      # 23 only: 22 is admitted nowhere


def test_create_admits_exactly_the_fourth_fixture(matrix):
    if _gfx950_visible():
        pytest.skip("GPU present: an admitted configuration would create a real ctx")
    from rsrl_amd import _build
    _build.build()
    res = matrix.sweep(matrix.GRID_AGENTS3, matrix.FIXED_AGENTS3)
    assert matrix.admitted(res) == json.load(open(matrix.AGENTS3_FIXTURE))["admitted"]
    ia = [n for n, _ in matrix.GRID_AGENTS3].index("algo")
    for key, (rc, msg) in res.items():
        if rc != matrix.EHIP:
            assert rc == matrix.EINVAL and msg, (key, rc, msg)
        if key[ia] == "0":
            assert rc == matrix.EINVAL and "unknown algo 22" in msg, (key, rc, msg)
    # without the fixed cap nothing of the grid is admitted: GradientMC refuses max_episode_steps = 0 wherever it is otherwise admitted
    assert matrix.admitted(matrix.sweep(matrix.GRID_AGENTS3)) == []


def test_example_compiles(tmp_path):
    compile_example(tmp_path, "gradient_mc")
