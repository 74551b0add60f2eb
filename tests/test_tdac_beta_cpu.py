"""ContinuousMountainCar, the Beta policy and the iLSTD ActorCritic over them (examples/tdac_beta.rs) without a GPU: the header, the binding table,
the Python constants and the Rust block agree on the new names and argument counts; the supported configurations pass admission and reach the
device query while every other one with the new domain or policy is refused with a message that names what is supported; 27 is no algo; the
fifth admission grid equals its fixture; examples/tdac_beta.cpp compiles; and the restatement the GPU tests compare against
(tests/beta_numpy.py) reproduces the reference's two domain tests, the words of the oracle's Philox, hand-worked values of the policy, and a
Kolmogorov-Smirnov condition on its sampler."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest
from scipy import stats
from scipy.special import digamma

import rsrl_amd
from rsrl_amd import _abi
from tests import beta_numpy as bn
from tests.agent_contract import compile_example, create_rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EHIP = -1, -2
BASE = dict(domain=rsrl_amd.CONTINUOUS_MOUNTAIN_CAR, order=3, algo=rsrl_amd.ILSTD_ACTOR_CRITIC, policy=rsrl_amd.BETA, n_envs=4, n_steps=2)
# name -> argument count (the ctx included)
NEW_CALLS = {"rsrl_hip_n_policy_outputs": 1, "rsrl_hip_action_bounds": 3, "rsrl_hip_get_actions_f32": 2, "rsrl_hip_set_actions_f32": 2,
             "rsrl_hip_domain_step_f32": 6, "rsrl_hip_handle_f32": 8, "rsrl_hip_policy_sample_f32": 4, "rsrl_hip_policy_mode_f32": 4,
             "rsrl_hip_policy_params": 5, "rsrl_hip_policy_pdf": 5}
SHAPES = [(1.3, 1.3), (2.5, 6.0), (12.0, 1.05)]
KS_C = 3.27          # the two-sided Kolmogorov bound at 2e-9: 2 exp(-2 c^2) = 2e-9 at c = 3.27


@pytest.fixture(scope="module")
def matrix():
    spec = importlib.util.spec_from_file_location("admission_matrix", os.path.join(ROOT, "scripts", "admission_matrix.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_rust_sys", os.path.join(ROOT, "scripts", "gen_rust_sys.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_header_binding_table_python_constants_and_rust_block_agree(gen):
    h = open(os.path.join(ROOT, "include", "rsrl_hip.h")).read()
    assert re.search(r"RSRL_CONTINUOUS_MOUNTAIN_CAR\s*=\s*4\b", h) and re.search(r"RSRL_BETA\s*=\s*4\b", h)
    assert rsrl_amd.CONTINUOUS_MOUNTAIN_CAR == 4 and rsrl_amd.BETA == 4 and rsrl_amd.context.BETA == 4
    assert re.search(r"#define\s+RSRL_HIP_ABI_VERSION\s+9\b", h)
    funcs = {name: len(params) for name, params, _ in gen.parse_header()[0]}
    block = gen.doc_block()
    rust = dict(gen.declared_functions(block))
    for name, n in NEW_CALLS.items():
        assert funcs.get(name) == n, (name, funcs.get(name))
        assert len(_abi.SYMBOLS[name][1]) == n, name
        assert rust.get(name) == n, (name, rust.get(name))
    assert "pub const RSRL_CONTINUOUS_MOUNTAIN_CAR: i32 = 4;" in block and "pub const RSRL_BETA: i32 = 4;" in block
    assert block == gen.generate()


def test_supported_configurations_reach_the_device_query():
    for order in (1, 2, 3, 4, 5):
        for extra in (dict(), dict(steps_per_launch=1), dict(max_episode_steps=1000, lr=1e-5, alpha=0.001, gamma=0.999), dict(n_steps=1), dict(n_steps=32)):
            rc, msg = create_rc(BASE, order=order, **extra)
            assert rc == 0 or (rc == EHIP and "device" in msg), (order, extra, rc, msg)


def test_other_configurations_are_refused_with_a_message():
    bad = [dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(order=7), dict(weight_mode=rsrl_amd.W_SHARED), dict(weight_dtype=rsrl_amd.W_BF16),
           dict(policy=rsrl_amd.SOFTMAX), dict(policy=rsrl_amd.RANDOM), dict(policy=rsrl_amd.GREEDY), dict(agent_policy=rsrl_amd.SOFTMAX),
           dict(epsilon_decay=0.99), dict(domain=rsrl_amd.MOUNTAIN_CAR), dict(domain=rsrl_amd.CART_POLE, order=1), dict(domain=rsrl_amd.HIV_TREATMENT, order=1)]
    bad += [dict(algo=a, policy=p) for a in (rsrl_amd.QLEARNING, rsrl_amd.SARSA_LAMBDA, rsrl_amd.TD, rsrl_amd.TD_ACTOR_CRITIC, rsrl_amd.REINFORCE, rsrl_amd.ILSTD,
                                             rsrl_amd.GRADIENT_MC, rsrl_amd.LSTD) for p in (rsrl_amd.BETA, rsrl_amd.RANDOM, rsrl_amd.SOFTMAX)]
    for b in bad:
        rc, msg = create_rc(BASE, **dict(dict(max_episode_steps=10), **b))
        assert rc == EINVAL and "RSRL_ILSTD_ACTOR_CRITIC" in msg and "RSRL_BETA" in msg and "RSRL_CONTINUOUS_MOUNTAIN_CAR" in msg and "orders 1-5" in msg, (b, rc, msg)
    rc, msg = create_rc(BASE, agent_policy=rsrl_amd.BETA)
    assert rc == EINVAL and "unknown agent policy 4" in msg
    for n in (0, -1, 33):
        rc, msg = create_rc(BASE, n_steps=n)
        assert rc == EINVAL and "RSRL_ILSTD_ACTOR_CRITIC" in msg and "n_steps" in msg, (n, rc, msg)
    for kw in (dict(domain=5), dict(policy=5), dict(domain=-1)):
        rc, msg = create_rc(BASE, **kw)
        assert rc == EINVAL and "unknown" in msg, (kw, rc, msg)


def test_twenty_seven_is_no_algo():
    for kw in (dict(), dict(domain=rsrl_amd.MOUNTAIN_CAR, policy=rsrl_amd.SOFTMAX), dict(policy=rsrl_amd.RANDOM)):
        rc, msg = create_rc(BASE, algo=27, **kw)
        assert rc == EINVAL and "unknown algo 27" in msg, (kw, rc, msg)


def test_fifth_grid_and_its_fixture(matrix):
    doc = json.load(open(matrix.BETA_FIXTURE))
    assert doc["grid"] == [[n, v] for n, v in matrix.GRID_BETA], "GRID_BETA and its fixture drifted apart"
    names = [n for n, _ in matrix.GRID_BETA]
    vals = dict(matrix.GRID_BETA)
    rows = [{n: vals[n][int(ch, 16)] for n, ch in zip(names, key)} for key in doc["admitted"]]
    cont = [r for r in rows if r["domain"] == 4 or r["policy"] == 4]
    # exactly: algo 21, Beta, domain 4, Fourier 1-5, per-learner f32, agent_policy -1, no schedule, n_steps in range; both launch depths
    assert len(cont) == 10 and all(r["domain"] == 4 and r["policy"] == 4 and r["algo"] == 21 and r["basis"] == 0 and r["weight_mode"] == 0 and
                                   r["weight_dtype"] == 0 and r["agent_policy"] == -1 and r["epsilon_decay"] == 1.0 and r["n_steps"] == 2 for r in cont)
    assert sorted({r["order"] for r in cont}) == [1, 2, 3, 4, 5]
    assert not any(r["algo"] == 27 for r in rows)


def _gfx950_visible():
    import subprocess
    try:
        return subprocess.run(["/opt/rocm/bin/rocminfo"], capture_output=True, text=True).stdout.count("gfx950") > 0
    except Exception:
        return False


def test_create_admits_exactly_the_fifth_fixture(matrix):
    if _gfx950_visible():
        pytest.skip("GPU present: an admitted configuration would create a real ctx")
    from rsrl_amd import _build
    _build.build()
    res = matrix.sweep(matrix.GRID_BETA)
    assert matrix.admitted(res) == json.load(open(matrix.BETA_FIXTURE))["admitted"]
    for key, (rc, msg) in res.items():
        if rc != matrix.EHIP:
            assert rc == matrix.EINVAL and msg, (key, rc, msg)


def test_example_compiles(tmp_path):
    compile_example(tmp_path, "tdac_beta")


# ---- the restatement
def test_reference_domain_tests():
    """continuous.rs's two tests: the start state, and the terminal predicate at 0.6 and 0.6 (1 +- 1e-4)"""
    assert bn.cmc_start() == (-0.5, 0.0)
    assert not bn.cmc_is_terminal(-0.5)
    assert bn.cmc_is_terminal(0.6) and bn.cmc_is_terminal(0.6 * (1 + 1e-4)) and not bn.cmc_is_terminal(0.6 * (1 - 1e-4))
    # one step from the start with full throttle either way, by hand
    (x, v), r, t = bn.cmc_step((-0.5, 0.0), 3.0)            # clipped to 1
    assert v == 0.0015 - 0.0025 * np.cos(-1.5) and x == -0.5 + v and r == -1.0 and not t
    (x, v), r, t = bn.cmc_step((-0.5, 0.0), -1.0)
    assert v == -0.0015 - 0.0025 * np.cos(-1.5) and x == -0.5 + v
    (x, v), r, t = bn.cmc_step((0.59, 0.06), 1.0)
    assert x == 0.6 and t and r == 0.0
    (x, v), r, t = bn.cmc_step((-1.19, -0.07), -1.0)
    assert x == -1.2 and v == -0.07 - 0.0015 - 0.0025 * np.cos(3.0 * -1.19) and not t      # the left wall: no velocity reset


def test_policy_values_by_hand():
    assert bn.softplus(10.0) == 10.0 and bn.softplus(25.0) == 25.0 and abs(bn.softplus(0.0) - np.log(2.0)) < 1e-16
    assert bn.softplus_grad(10.0) == 1.0 and bn.softplus_grad(0.0) == 0.5
    a, b = bn.beta_params(0.0, 0.0)
    assert abs(a - 1.6931471805599454) < 1e-15 and a == b
    assert abs(bn.beta_mode(a, b) - 0.5) < 1e-15
    a1, b1 = bn.beta_params(-40.0, 2.0)                     # alpha -> 1 exactly: no mode, the mean
    assert a1 == 1.0 and bn.beta_mode(a1, b1) == 1.0 / (1.0 + b1)
    assert abs(bn.beta_mode(3.0, 2.0) - 2.0 / 3.0) < 1e-15
    # the density integrates to one and equals scipy's; the score is the derivative of its logarithm
    for al, be in SHAPES:
        x = np.linspace(0.01, 0.99, 99)
        assert np.allclose(bn.beta_pdf(al, be, x), stats.beta.pdf(x, al, be), rtol=1e-12, atol=0)
        h = 1e-6
        ga, gb = bn.beta_score(al, be, 0.3)
        assert abs((np.log(bn.beta_pdf(al + h, be, 0.3)) - np.log(bn.beta_pdf(al - h, be, 0.3))) / (2 * h) - ga) < 1e-8
        assert abs((np.log(bn.beta_pdf(al, be + h, 0.3)) - np.log(bn.beta_pdf(al, be - h, 0.3))) / (2 * h) - gb) < 1e-8
    ga0, _ = bn.beta_score(2.0, 3.0, 0.0)                   # clamped: finite
    assert ga0 == np.log(2.0 ** -24) - digamma(2.0) + digamma(5.0)
    # the step: both parameters are read before either column moves
    phi, W = np.array([0.5, -1.0, 1.0]), np.array([[0.2, 0.1], [0.0, -0.3], [0.4, 0.7]])
    W2 = bn.beta_step(W, phi, 0.25, 0.5)
    xa, xb = phi @ W[:, 0], phi @ W[:, 1]
    al, be = bn.beta_params(xa, xb)
    ga, gb = bn.beta_score(al, be, 0.25)
    assert np.allclose(W2[:, 0], W[:, 0] + 0.5 * ga / (1 + np.exp(-xa)) * phi, rtol=1e-15, atol=0)
    assert np.allclose(W2[:, 1], W[:, 1] + 0.5 * gb / (1 + np.exp(-xb)) * phi, rtol=1e-15, atol=0)


def test_with_alpha_zero_the_critic_is_ilstd_exactly():
    from tests.lstd_numpy import ilstd, ilstd_init
    rng = np.random.default_rng(7)
    F = 6
    th, M, mu = ilstd_init(F)
    th2, M2, mu2, W = th.copy(), M.copy(), mu.copy(), rng.normal(size=(F, 2)) * 0.3
    W0 = W.copy()
    for k in range(10):
        phi_s, phi_n, a, r, term = rng.uniform(-1, 1, size=F), rng.uniform(-1, 1, size=F), float(rng.uniform()), float(rng.normal()), bool(k % 4 == 3)
        d1, th, M, mu = ilstd(th, M, mu, phi_s, phi_n, r, term, 0.9, 0.05, 3, literal=False)
        d2, th2, M2, mu2, W = bn.tdac_beta_rule(th2, M2, mu2, W, phi_s, phi_n, a, r, term, 0.9, 0.05, 3, 0.0)
        assert d1 == d2 and th.tobytes() == th2.tobytes() and M.tobytes() == M2.tobytes() and mu.tobytes() == mu2.tobytes(), k
    assert np.array_equal(W, W0)
    _, th3, M3, mu3, W3 = bn.tdac_beta_rule(th2, M2, mu2, W, phi_s, phi_n, a, r, False, 0.9, 0.05, 3, 0.5)
    _, th4, M4, mu4 = ilstd(th, M, mu, phi_s, phi_n, r, False, 0.9, 0.05, 3, literal=False)
    assert th3.tobytes() == th4.tobytes() and M3.tobytes() == M4.tobytes() and mu3.tobytes() == mu4.tobytes() and not np.array_equal(W3, W)


def test_philox_words_are_the_oracles(orc):
    rng = np.random.default_rng(3)
    for _ in range(40):
        seed, gid, t = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 40))
        block = int(rng.choice([bn.BLK_INIT, bn.BLK_API, 256, 259, 260, 256 * 8 + 4, 256 * 8]))
        assert bn.philox_block(seed, np.array([gid]), t, block)[0].tolist() == orc.draw(seed, gid, t, block).tolist(), (seed, gid, t, block)


@pytest.mark.parametrize("alpha,beta", SHAPES)
def test_restated_sampler_is_beta_distributed(alpha, beta):
    """16 384 draws: the Kolmogorov-Smirnov distance to scipy.stats.beta is below 3.27 / sqrt(n), every draw lies in the clamp's interval, and the
    bounded loop ran out for none (at most a handful of learners reach round 5)"""
    n = 16384
    x, margin = bn.beta_sample(1234, np.arange(n), 5, bn.BLK_API, alpha, beta)
    assert x.min() >= bn.LO and x.max() <= bn.HI and np.isfinite(margin).all()
    d = stats.kstest(x, stats.beta(alpha, beta).cdf).statistic
    assert d < KS_C / np.sqrt(n), (alpha, beta, d)


def test_sample_is_a_function_of_seed_learner_step_and_purpose():
    gid = np.arange(64)
    x0, _ = bn.beta_sample(9, gid, 3, bn.BLK_STEP, 2.0, 3.0)
    assert np.array_equal(x0[5:9], bn.beta_sample(9, gid[5:9], 3, bn.BLK_STEP, 2.0, 3.0)[0])
    for other in (bn.beta_sample(10, gid, 3, bn.BLK_STEP, 2.0, 3.0)[0], bn.beta_sample(9, gid, 4, bn.BLK_STEP, 2.0, 3.0)[0],
                  bn.beta_sample(9, gid, 3, bn.BLK_INIT, 2.0, 3.0)[0], bn.beta_sample(9, gid + 64, 3, bn.BLK_STEP, 2.0, 3.0)[0]):
        assert not np.array_equal(x0, other)


@pytest.mark.parametrize("order", [1, 3, 5])
def test_the_gpu_rule_case_stays_clear_of_the_tie_band(orc, order):
    """the GPU rule test leaves out the learners tests/lstd_numpy.near_tie_band flags and caps their share at 5 %: the numpy rule alone stays under
    it, actions 0 and 1 occur, terminal and non-terminal transitions occur in every round, and |x| <= 3 holds for the initial columns"""
    case = bn.handle_case(orc, order)
    N = len(case["init"])
    assert N == 67 and case["skipped"].sum() <= 0.05 * N, case["skipped"].sum()
    for frm, a, rew, nxt, term in case["rounds"]:
        assert 0 < term.sum() < N and a[0] == 0.0 and a[1] == 1.0 and a.min() >= 0.0 and a.max() <= 1.0
    for _, _, _, W in case["init"]:
        assert np.abs(W.astype(np.float64)).sum(axis=0).max() <= 3.0 + 1e-6
