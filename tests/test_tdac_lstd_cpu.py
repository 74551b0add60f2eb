"""ActorCritic::tdac with the iLSTD critic (RSRL_ILSTD_ACTOR_CRITIC, 21) without a GPU: the header, the Rust block and the Python constant agree,
every configuration the TD ActorCritic (13) runs on passes admission and reaches the device query while every other one is refused with a message,
20 is no algo, the third admission grid equals its fixture, examples/tdac_ilstd.cpp compiles, and hand-worked cases pin the restatement the GPU
tests compare against (tests/tdac_lstd_numpy.py)."""
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import rsrl_amd
from tests.ac_numpy import softmax
from tests.agent_contract import compile_example, create_rc
from tests.lstd_numpy import ilstd, ilstd_init
from tests.tdac_lstd_numpy import critic_target, handle_case, tdac_lstd_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EHIP = -1, -2
SUPPORTED = [(rsrl_amd.MOUNTAIN_CAR, o) for o in (1, 2, 3, 4, 5)] + [(rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]
NAME = "RSRL_ILSTD_ACTOR_CRITIC"


BASE = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=rsrl_amd.ILSTD_ACTOR_CRITIC, policy=rsrl_amd.SOFTMAX, n_envs=4, n_steps=2)


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


def test_header_rust_block_and_python_constant_agree():
    h = open(os.path.join(ROOT, "include", "rsrl_hip.h")).read()
    assert re.search(NAME + r"\s*=\s*21\b", h)
    enum = h.split("rsrl_algo;")[0].split("typedef enum { RSRL_QLEARNING")[1]
    for n in (12, 14, 17, 20):
        assert not re.search(r"=\s*%d\b\s*[,}]" % n, enum), n
    assert "(20 is no algo.)" in enum
    assert rsrl_amd.ILSTD_ACTOR_CRITIC == 21 and rsrl_amd.context.ILSTD_ACTOR_CRITIC == 21
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pub const %s: i32 = 21;" % NAME in doc
    assert re.search(r"#define\s+RSRL_HIP_ABI_VERSION\s+9\b", h)          # no new entry point: the version stays


def test_supported_configurations_reach_the_device_query():
    for domain, order in SUPPORTED:
        for extra in (dict(), dict(steps_per_launch=1), dict(tau=0.5, max_episode_steps=100, lr=1e-4, alpha=0.002, gamma=0.99), dict(n_steps=1), dict(n_steps=32)):
            rc, msg = create_rc(BASE, domain=domain, order=order, **extra)
            # no GPU: every admission rule has passed and the device query answers "no device"; with one, the ctx is created
            assert rc == 0 or (rc == EHIP and "device" in msg), (domain, order, extra, rc, msg)


def test_other_configurations_are_refused_with_a_message():
    bad = [dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(order=7), dict(domain=rsrl_amd.CART_POLE, order=2),
           dict(domain=rsrl_amd.CART_POLE, order=7), dict(domain=rsrl_amd.ACROBOT, order=3), dict(weight_mode=rsrl_amd.W_SHARED),
           dict(domain=rsrl_amd.CART_POLE, order=7, weight_dtype=rsrl_amd.W_BF16), dict(weight_dtype=rsrl_amd.W_BF16),
           dict(domain=rsrl_amd.HIV_TREATMENT, order=1), dict(policy=rsrl_amd.EPSILON_GREEDY), dict(policy=rsrl_amd.GREEDY),
           dict(policy=rsrl_amd.RANDOM), dict(agent_policy=rsrl_amd.SOFTMAX), dict(epsilon_decay=0.99)]
    for b in bad:
        rc, msg = create_rc(BASE, **b)
        assert rc == EINVAL and NAME in msg and "register-family Fourier" in msg, (b, rc, msg)
    for n in (0, -1, 33, 1000):
        rc, msg = create_rc(BASE, n_steps=n)
        assert rc == EINVAL and NAME in msg and "n_steps" in msg, (n, rc, msg)
    rc, msg = create_rc(BASE, tau=0.0)
    assert rc == EINVAL and "Tau" in msg


def test_twenty_is_no_algo():
    for kw in (dict(), dict(policy=rsrl_amd.RANDOM), dict(policy=rsrl_amd.EPSILON_GREEDY, order=5)):
        rc, msg = create_rc(BASE, algo=20, **kw)
        assert rc == EINVAL and "unknown algo 20" in msg, (kw, rc, msg)
    rc, msg = create_rc(BASE, algo=22)
    assert rc == EINVAL and "unknown algo 22" in msg


def test_third_grid_is_the_first_on_algos_20_and_21(matrix):
    assert dict(matrix.GRID_AGENTS2)["algo"] == [20, 21]
    assert [n for n, _ in matrix.GRID] == [n for n, _ in matrix.GRID_AGENTS2]
    assert all(v == w for (n, v), (_, w) in zip(matrix.GRID, matrix.GRID_AGENTS2) if n != "algo"), "the third grid's other axes are the first's"
    doc = json.load(open(matrix.AGENTS2_FIXTURE))
    assert doc["grid"] == [[n, v] for n, v in matrix.GRID_AGENTS2], "GRID_AGENTS2 and its fixture drifted apart"
    # admission is exactly algo 13's: the fixture's keys with the algo digest replaced are the second fixture's keys of 13
    ia = [n for n, _ in matrix.GRID].index("algo")
    second = json.load(open(matrix.AGENTS_FIXTURE))
    i13 = "%x" % dict(matrix.GRID_AGENTS)["algo"].index(13)
    of13 = sorted(k[:ia] + "_" + k[ia + 1:] for k in second["admitted"] if k[ia] == i13)
    assert of13 and of13 == sorted(k[:ia] + "_" + k[ia + 1:] for k in doc["admitted"])
    assert {k[ia] for k in doc["admitted"]} == {"1"}                      # 21 only: 20 is admitted nowhere


def test_create_admits_exactly_the_third_fixture(matrix):
    if _gfx950_visible():
        pytest.skip("GPU present: an admitted configuration would create a real ctx")
    from rsrl_amd import _build
    _build.build()
    res = matrix.sweep(matrix.GRID_AGENTS2)
    assert matrix.admitted(res) == json.load(open(matrix.AGENTS2_FIXTURE))["admitted"]
    ia = [n for n, _ in matrix.GRID_AGENTS2].index("algo")
    for key, (rc, msg) in res.items():
        if rc != matrix.EHIP:
            assert rc == matrix.EINVAL and msg, (key, rc, msg)
        if key[ia] == "0":
            assert rc == matrix.EINVAL and "unknown algo 20" in msg, (key, rc, msg)


def test_example_compiles(tmp_path):
    compile_example(tmp_path, "tdac_ilstd")


def test_rule_on_a_hand_worked_non_terminal_transition():
    # tests/test_lstd_cpu.py's non-terminal iLSTD case: theta = [0.5, -1], A = I, mu = 0, phi_s = [1, 0], phi_n = [0, 1], r = 2, gamma = 0.5, iLSTD's
    # alpha (lr) = 0.1, two rounds -> diagnostic 1, theta' = [0.68, -1], A' = [[2, -0.5], [0, 1]], mu' = [0.64, 0]
    th0, (_, A0, mu0) = np.array([0.5, -1.0]), ilstd_init(2)
    Th = np.zeros((2, 2))
    d, th, A, mu, T2 = tdac_lstd_rule(th0, A0, mu0, Th, [1.0, 0.0], [0.0, 1.0], 1, 2.0, False, 0.5, 0.1, 2, 0.25, 1.0)
    assert d == 2.0 + 0.5 * (-1.0) - 0.5
    assert np.allclose(th, [0.68, -1.0], rtol=1e-15, atol=0) and np.array_equal(A, [[2.0, -0.5], [0.0, 1.0]]) and np.allclose(mu, [0.64, 0.0], rtol=1e-15, atol=0)
    # the critic reads the UPDATED theta: c = 2 + 0.5 V'(s') - V'(s) = 2 - 0.5 - 0.68 = 0.82 (with the old theta it would be 1)
    c = 2.0 + 0.5 * th[1] - th[0]
    assert critic_target(th, [1.0, 0.0], [0.0, 1.0], 2.0, False, 0.5) == c and abs(c - 0.82) < 1e-15
    # e = f32(0.25 c), ONE rounding; theta_a = 0 so p = [0.5, 0.5]; a = 1: column 1 moves by +e/2 phi(s), column 0 by -e/2 phi(s)
    e = float(np.float32(0.25 * c))
    assert e != 0.25 * c
    assert np.array_equal(T2, [[-0.5 * e, 0.5 * e], [0.0, 0.0]])


def test_rule_on_a_hand_worked_terminal_transition():
    # the same state, terminal: pd = phi_s, A' = [[2, 0], [0, 1]]; diagnostic r - V(s) = 1.5; mu = [2, 0] - [1, 0] * 0.5 = [1.5, 0]; round 1:
    # u = 0.15, theta_0 = 0.65, mu_0 = 1.5 - 0.3 = 1.2; round 2: u = 0.12, theta_0 = 0.77, mu_0 = 0.96
    th0, (_, A0, mu0) = np.array([0.5, -1.0]), ilstd_init(2)
    Th = np.array([[0.2, -0.4], [1.0, 3.0]])
    d, th, A, mu, T2 = tdac_lstd_rule(th0, A0, mu0, Th, [1.0, 0.0], [0.0, 1.0], 0, 2.0, True, 0.5, 0.1, 2, 0.25, 0.5)
    assert d == 1.5 and np.array_equal(A, [[2.0, 0.0], [0.0, 1.0]])
    assert np.allclose(th, [0.77, -1.0], rtol=1e-15, atol=0) and np.allclose(mu, [0.96, 0.0], rtol=1e-15, atol=0)
    # the critic reads V' of the TERMINAL STATE s' itself: c = r - V'(s') = 2 - (-1) = 3, whatever V'(s) is; e = f32(0.75) = 0.75 exactly
    assert critic_target(th, [1.0, 0.0], [0.0, 1.0], 2.0, True, 0.5) == 3.0
    # p from the pre-update theta_a at tau = 0.5: preferences theta_a^T phi(s) = [0.2, -0.4] -> softmax([0.4, -0.8]); grad_log has no 1/tau
    p = softmax(np.array([0.2, -0.4]), 0.5)
    assert np.allclose(p, np.exp([0.4, -0.8]) / np.exp([0.4, -0.8]).sum(), rtol=1e-15, atol=0)
    want = Th + 0.75 * np.outer([1.0, 0.0], [1.0 - p[0], -p[1]])
    assert np.allclose(T2, want, rtol=1e-15, atol=0) and np.array_equal(T2[1], Th[1])


def test_with_alpha_zero_the_critic_is_ilstd_exactly():
    rng = np.random.default_rng(5)
    F, A = 6, 3
    th, M, mu = ilstd_init(F)
    th2, M2, mu2, Th = th.copy(), M.copy(), mu.copy(), rng.normal(size=(F, A))
    Th0 = Th.copy()
    for k in range(12):
        phi_s, phi_n, a, r, term = rng.uniform(-1, 1, size=F), rng.uniform(-1, 1, size=F), int(rng.integers(A)), float(rng.normal()), bool(k % 4 == 3)
        d1, th, M, mu = ilstd(th, M, mu, phi_s, phi_n, r, term, 0.9, 0.05, 3, literal=False)
        d2, th2, M2, mu2, Th = tdac_lstd_rule(th2, M2, mu2, Th, phi_s, phi_n, a, r, term, 0.9, 0.05, 3, 0.0, 0.7)
        assert d1 == d2 and th.tobytes() == th2.tobytes() and M.tobytes() == M2.tobytes() and mu.tobytes() == mu2.tobytes(), k
    assert np.array_equal(Th, Th0) and np.abs(th).max() > 0
    # ... and with alpha != 0 the critic still is (it does not read the actor), while the actor moves
    _, th3, M3, mu3, Th3 = tdac_lstd_rule(th2, M2, mu2, Th, phi_s, phi_n, a, r, False, 0.9, 0.05, 3, 0.5, 0.7)
    _, th4, M4, mu4 = ilstd(th, M, mu, phi_s, phi_n, r, False, 0.9, 0.05, 3, literal=False)
    assert th3.tobytes() == th4.tobytes() and M3.tobytes() == M4.tobytes() and mu3.tobytes() == mu4.tobytes() and not np.array_equal(Th3, Th)


@pytest.mark.parametrize("domain,order", SUPPORTED)
def test_the_gpu_handle_case_stays_clear_of_the_tie_band(orc, domain, order):
    """tests/test_gpu_tdac_lstd.py leaves a learner out of the f64 comparison when a solve round's |mu| lies within 1e-9 of argmaxima's 1e-7 band, and
    allows N / 4 of them: with the case's seed the numpy rule alone stays under that cap, terminal and non-terminal transitions both occur in every
    round, and the state stays finite"""
    case = handle_case(orc, domain, order)
    N = len(case["init"])
    assert case["skipped"].sum() <= N // 4, case["skipped"].sum()
    for frm, a, rew, nxt, term in case["rounds"]:
        assert 0 < term.sum() < N
    for theta, A, mu, Th in case["final"]:
        assert np.isfinite(theta).all() and np.isfinite(A).all() and np.isfinite(mu).all() and np.isfinite(Th).all()
    assert any(not np.array_equal(f, i[3].astype(np.float64)) for f, i in zip(case["first"], case["init"]))


def test_the_campaign_sampler_draws_only_admitted_configurations():
    """300 draws of tests/fuzz_tdac_lstd.py's sampler: rsrl_hip_create admits every one (EHIP -- no device -- here, a ctx with a GPU)"""
    from tests import fuzz_tdac_lstd as fz
    rng = np.random.default_rng(0)
    seen = set()
    for _ in range(300):
        kw = fz.draw_config(rng)
        assert kw["algo"] == rsrl_amd.ILSTD_ACTOR_CRITIC
        rc, msg = create_rc(BASE, **dict(kw, n_envs=min(kw["n_envs"], 4)))
        assert rc == 0 or (rc == EHIP and "device" in msg), (kw, rc, msg)
        seen.add((kw["domain"], kw["order"]))
    assert seen == set(SUPPORTED)
