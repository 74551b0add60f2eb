"""RecursiveLSTD and iLSTD (RSRL_RECURSIVE_LSTD, RSRL_ILSTD) without a GPU: the header declares them, every supported configuration passes admission
and reaches the device query while every other one is refused with a message naming the algo, examples/lstd.cpp compiles, and hand-worked cases pin
the f64 restatement the GPU tests compare against (tests/lstd_numpy.py)."""
import os
import re

import numpy as np

import rsrl_amd
from rsrl_amd import _abi
from tests.agent_contract import compile_example, create_rc
from tests.lstd_numpy import argmaxima, ilstd, ilstd_init, ilstd_solve, near_tie_band, recursive_lstd, recursive_lstd_init

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EHIP = -1, -2
SUPPORTED = [(rsrl_amd.MOUNTAIN_CAR, o) for o in (1, 2, 3, 4, 5)] + [(rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]
ALGOS = [(rsrl_amd.RECURSIVE_LSTD, "RSRL_RECURSIVE_LSTD"), (rsrl_amd.ILSTD, "RSRL_ILSTD")]


BASE = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=rsrl_amd.RECURSIVE_LSTD, policy=rsrl_amd.RANDOM, n_envs=4)


def test_header_declares_the_algos_and_exports():
    h = open(os.path.join(ROOT, "include", "rsrl_hip.h")).read()
    assert re.search(r"RSRL_RECURSIVE_LSTD\s*=\s*18\b", h) and re.search(r"RSRL_ILSTD\s*=\s*19\b", h)
    enum = h.split("rsrl_algo;")[0].split("typedef enum { RSRL_QLEARNING")[1]
    for n in (12, 14, 17):
        assert not re.search(r"=\s*%d\b\s*[,}]" % n, enum), n
    assert (rsrl_amd.RECURSIVE_LSTD, rsrl_amd.ILSTD) == (18, 19)
    assert "int rsrl_hip_get_lstd_state(" in h and "int rsrl_hip_set_lstd_state(" in h
    assert "rsrl_hip_get_lstd_state" in _abi.SYMBOLS and "rsrl_hip_set_lstd_state" in _abi.SYMBOLS


def test_supported_configurations_reach_the_device_query():
    for algo, _ in ALGOS:
        for domain, order in SUPPORTED:
            for extra in (dict(), dict(steps_per_launch=1), dict(max_episode_steps=100, gamma=0.9, alpha=0.01), dict(n_steps=32), dict(n_steps=1)):
                rc, msg = create_rc(BASE, algo=algo, domain=domain, order=order, **extra)
                # no GPU: every admission rule has passed and the device query answers "no device"; with one, the ctx is created
                assert rc == 0 or (rc == EHIP and "device" in msg), (algo, domain, order, extra, rc, msg)


def test_other_configurations_are_refused_with_a_message():
    bad = [dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(order=7), dict(domain=rsrl_amd.CART_POLE, order=2),
           dict(domain=rsrl_amd.CART_POLE, order=7), dict(domain=rsrl_amd.ACROBOT, order=3), dict(weight_mode=rsrl_amd.W_SHARED),
           dict(domain=rsrl_amd.CART_POLE, order=7, weight_dtype=rsrl_amd.W_BF16), dict(weight_dtype=rsrl_amd.W_BF16),
           dict(domain=rsrl_amd.HIV_TREATMENT, order=1), dict(policy=rsrl_amd.EPSILON_GREEDY), dict(policy=rsrl_amd.GREEDY),
           dict(policy=rsrl_amd.SOFTMAX), dict(agent_policy=rsrl_amd.RANDOM), dict(epsilon_decay=0.99)]
    for algo, name in ALGOS:
        for b in bad:
            rc, msg = create_rc(BASE, algo=algo, **b)
            assert rc == EINVAL and name in msg and "register-family Fourier" in msg, (algo, b, rc, msg)
    for n in (0, -1, 33, 1000):
        rc, msg = create_rc(BASE, algo=rsrl_amd.ILSTD, n_steps=n)
        assert rc == EINVAL and "RSRL_ILSTD" in msg and "n_steps" in msg, (n, rc, msg)
    rc, msg = create_rc(BASE, algo=rsrl_amd.RECURSIVE_LSTD, n_steps=0)      # RecursiveLSTD has no n_updates: n_steps is not its field
    assert rc == 0 or (rc == EHIP and "device" in msg), (rc, msg)
    for n in (12, 14, 17, 20):
        rc, msg = create_rc(BASE, algo=n)
        assert rc == EINVAL and "unknown algo %d" % n in msg, (n, msg)


def test_lstd_example_compiles(tmp_path):
    compile_example(tmp_path, "lstd")


def test_argmaxima_ties_come_first():
    # exact ties: every index
    assert argmaxima([1.0, 3.0, 3.0, 2.0]) == ([1, 2], 3.0)
    # within 1e-7 of the max: appended, the max is NOT raised -- a later, larger value within the band joins without moving it
    ixs, mx = argmaxima([1.0, 1.0 + 5e-8, 1.0 + 9e-8])
    assert ixs == [0, 1, 2] and mx == 1.0
    # a value beyond 1e-7 of the (unraised) max restarts the list
    ixs, mx = argmaxima([1.0, 1.0 + 9e-8, 1.0 + 2e-7])
    assert ixs == [2] and mx == 1.0 + 2e-7
    # the first value against f64::MIN, and values below the max are skipped
    assert argmaxima([0.0, 0.0]) == ([0, 1], 0.0)
    assert argmaxima([5.0, 4.0, 5.0 + 1e-8]) == ([0, 2], 5.0)
    # NaN never enters the set
    assert argmaxima([float("nan"), 2.0]) == ([1], 2.0)
    assert near_tie_band([1.0, 1.0 + 1e-7]) and not near_tie_band([1.0, 1.0 + 5e-8])


def test_recursive_lstd_hand_worked():
    theta, C = recursive_lstd_init(2)
    assert np.array_equal(C, 1e-5 * np.eye(2)) and not theta.any()
    phi_s, phi_n = np.array([1.0, 0.0]), np.array([0.0, 1.0])
    # non-terminal, gamma = 0.5: pd = [1, -0.5]; g = C pd = 1e-5 [1, -0.5]; a = 1 + 1e-5; v = C phi_s = [1e-5, 0]; residual = 2
    res, th, C2 = recursive_lstd(theta, C, phi_s, phi_n, 2.0, False, 0.5)
    a = 1.0 + 1e-5
    assert res == 2.0
    assert np.allclose(th, [2.0 * 1e-5 / a, 0.0], rtol=1e-15, atol=0)
    assert np.allclose(C2, 1e-5 * np.eye(2) - np.outer([1e-5, 0.0], [1e-5, -0.5e-5]) / a, rtol=1e-15, atol=0)
    # terminal: theta moves by ((r - theta.phi_s) / a) v computed with C, then C is zero ...
    res, th2, C3 = recursive_lstd(th, C2, phi_s, phi_n, 1.0, True, 0.5)
    assert not C3.any() and res == 1.0 - th[0]
    v = C2 @ phi_s
    assert np.allclose(th2, th + (res / (1.0 + v @ phi_s)) * v, rtol=1e-15, atol=0)
    # ... and from then on no transition moves theta (v = 0), terminal or not
    th3, C4 = th2, C3
    rng = np.random.default_rng(0)
    for k in range(5):
        _, th3, C4 = recursive_lstd(th3, C4, rng.normal(size=2), rng.normal(size=2), float(rng.normal()), bool(k % 2), 0.9)
        assert np.array_equal(th3, th2) and not C4.any()


def test_ilstd_hand_worked():
    theta, A, mu = ilstd_init(2)
    assert np.array_equal(A, np.eye(2)) and not theta.any() and not mu.any()
    # terminal, r = 1, phi_s = [1, 1]: mu = [1, 1]; A = I + ones; theta = 0 so mu stays; one round with alpha = 0.5: idx = [0, 1] (a tie);
    # j = 0: u = 0.5, theta_0 = 0.5, mu -= 0.5 A[:,0] = [1, 1] - 0.5 [2, 1] = [0, 0.5];  j = 1 reads the UPDATED mu_1 = 0.5: u = 0.25,
    # theta_1 = 0.25, mu -= 0.25 A[:,1] = [0, 0.5] - 0.25 [1, 2] = [-0.25, 0]
    d, th, A2, mu2 = ilstd(theta, A, mu, [1.0, 1.0], [0.0, 0.0], 1.0, True, 0.9, 0.5, 1)
    assert d == 1.0
    assert np.array_equal(A2, [[2.0, 1.0], [1.0, 2.0]])
    assert np.array_equal(th, [0.5, 0.25]) and np.array_equal(mu2, [-0.25, 0.0])
    # had j = 1 read the mu of the round's start (1.0), theta_1 would be 0.5: the order matters
    assert th[1] != 0.5
    # the same case through the solve alone, and the device's form of mu -= (phi_s pd^T) theta agrees here (theta = 0)
    th_s, mu_s = ilstd_solve(np.zeros(2), A2, np.array([1.0, 1.0]), 0.5, 1)
    assert np.array_equal(th_s, th) and np.array_equal(mu_s, mu2)
    d2, th2, A3, mu3 = ilstd(theta, A, mu, [1.0, 1.0], [0.0, 0.0], 1.0, True, 0.9, 0.5, 1, literal=False)
    assert d2 == d and np.array_equal(th2, th) and np.array_equal(A3, A2) and np.array_equal(mu3, mu2)
    # non-terminal: pd = phi_s - gamma phi_n; the diagnostic reads theta from before the update
    th0 = np.array([0.5, -1.0])
    d, th4, A4, mu4 = ilstd(th0, np.eye(2), np.zeros(2), [1.0, 0.0], [0.0, 1.0], 2.0, False, 0.5, 0.1, 2)
    assert d == 2.0 + 0.5 * (-1.0) - 0.5
    assert np.array_equal(A4, [[2.0, -0.5], [0.0, 1.0]])
    # mu = r phi_s - phi_s (pd . theta) = [2, 0] - [1, 0] (0.5 + 0.5) = [1, 0]; round 1: j = 0, u = 0.1, mu = [1, 0] - 0.1 [2, 0] = [0.8, 0];
    # round 2: j = 0, u = 0.08, mu = [0.8 - 0.16, 0]
    assert np.allclose(th4, [0.5 + 0.1 + 0.08, -1.0], rtol=1e-15, atol=0)
    assert np.allclose(mu4, [0.64, 0.0], rtol=1e-15, atol=0)
