"""LSTD and LSTDLambda (RSRL_LSTD, RSRL_LSTD_LAMBDA; 25 and 26) without a GPU: the library's solve restated (tests/lstd_batch_numpy.py lu_solve) against
LAPACK on the matrices the restated rules produce from random MountainCar episodes, its abandoned solves and its tie-breaking, hand-worked batches
for both rules, the header / binding / Python constants, the supported and refused configurations, and examples/lstd_lambda.cpp compiles."""
import os
import re

import numpy as np
import pytest

import rsrl_amd
from rsrl_amd import _abi
from tests.agent_contract import compile_example, create_rc
from tests.lstd_batch_numpy import accumulate_lstd, accumulate_lstd_lambda, handle, initial_state, lu_solve, residual, solve, state_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EHIP = -1, -2
EPS = np.finfo(np.float64).eps
SUPPORTED = [(rsrl_amd.MOUNTAIN_CAR, o) for o in (1, 2, 3, 4, 5)] + [(rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]
ALGOS = [(rsrl_amd.LSTD, "RSRL_LSTD"), (rsrl_amd.LSTD_LAMBDA, "RSRL_LSTD_LAMBDA")]
BASE = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=rsrl_amd.LSTD, policy=rsrl_amd.RANDOM, n_envs=4, max_episode_steps=50)


def episode(orc, order, cap, rng):
    """one MountainCar episode under random actions, at most cap transitions -> [(phi_s, phi_ns, r, terminal)]"""
    dom = rsrl_amd.MOUNTAIN_CAR
    s, out = orc.domain_reset(dom), []
    for _ in range(cap):
        ns, r, term = orc.domain_step(dom, s, int(rng.integers(0, 3)))
        out.append((orc.fourier_project(dom, order, s), orc.fourier_project(dom, order, ns), r, term))
        s = ns
        if term:
            break
    return out


@pytest.mark.parametrize("lam", [None, 0.8, 0.9], ids=["lstd", "lambda0.8", "lambda0.9"])
@pytest.mark.parametrize("order,cap", [(1, 7), (3, 23), (5, 40)])
def test_lu_solve_against_lapack_on_the_rules_matrices(orc, order, cap, lam):
    """four episodes into one learner, solved after each: the normalised residual of the restated solve is at most F eps (a backward-stable
    solve's is a small multiple of eps; these inputs give at most 0.40 eps for the restatement and 0.39 eps for LAPACK, at conditions up to
    2.5e9) and no pivot is zero"""
    F, gamma = (order + 1) ** 2, 0.95
    rng = np.random.default_rng(1000 * order + cap)
    st = initial_state(F, lam)
    for _ in range(4):
        batch = episode(orc, order, cap, rng)
        handle(st, batch, gamma, lam)
        A, b = np.array(st["A"]), np.array(st["b"])
        x = lu_solve(A, b)
        assert x is not None and st["singular"] == 0 and x == st["theta"]
        r_lu, r_np = residual(A, b, x), residual(A, b, np.linalg.solve(A, b))
        print("order %d cap %d lambda %s: residual %.3g eps (LAPACK %.3g eps), condition %.3g" % (order, cap, lam, r_lu / EPS, r_np / EPS, np.linalg.cond(A)))
        assert r_lu <= F * EPS and r_np <= F * EPS, (r_lu, r_np)
    assert np.abs(st["theta"]).max() > 0


def test_lu_solve_abandons_a_zero_pivot_and_breaks_ties_by_the_first_index():
    rng = np.random.default_rng(2)
    A = rng.normal(size=(5, 5))
    b = rng.normal(size=5)
    assert np.allclose(lu_solve(A, b), np.linalg.solve(A, b), rtol=1e-12, atol=0)
    two_equal = A.copy()
    two_equal[3] = two_equal[1]
    assert lu_solve(two_equal, b) is None
    zero_column = A.copy()
    zero_column[:, 2] = 0.0
    assert lu_solve(zero_column, b) is None
    assert lu_solve([[0.0]], [1.0]) is None and lu_solve([[2.0]], [1.0]) == [0.5]
    # a column of equal magnitudes: row 0 is the pivot.  With rows 0 and 1 of column 0 equal in magnitude, m = a[1][0] / a[0][0] = -1 exactly
    # and x follows in the order the rows were taken: (x0, x1) solves 2 x0 + x1 = 3, -2 x0 + x1 = 1
    assert lu_solve([[2.0, 1.0], [-2.0, 1.0]], [3.0, 1.0]) == [0.5, 2.0]
    # first index, observably: on |a[0][0]| = |a[1][0]| the two choices round x0 differently -- the same system with its rows exchanged makes the
    # other row the first
    A, rhs = [[0.1, 0.1], [-0.1, 0.3]], [0.1, 1.1]
    x1 = (1.1 - (-0.1 / 0.1) * 0.1) / (0.3 - (-0.1 / 0.1) * 0.1)
    assert lu_solve(A, rhs) == [(0.1 - 0.1 * x1) / 0.1, x1] == [-2.0000000000000004, 3.0000000000000004]
    assert lu_solve([A[1], A[0]], [rhs[1], rhs[0]]) == [-1.9999999999999996, 3.0000000000000004]
    # used rows are not candidates again: a permuted triangular system is solved exactly
    P = [[0.0, 0.0, 4.0], [2.0, 0.0, 1.0], [1.0, 8.0, 1.0]]
    assert lu_solve(P, [8.0, 4.0, 19.0]) == [1.0, 2.0, 2.0]


def test_hand_worked_batches():
    # LSTD, first to last, gamma = 0.5.  Transition 1 (non-terminal, r = 2): phi_s = [1, 0], phi_ns = [0, 1]: b = [2, 0]; pd = [-1, 0.5];
    # A -= phi_s (x) pd = [[1e-6 + 1, -0.5], [0, 1e-6]].  Transition 2 (terminal, r = 1): phi_s = [0, 1]: b = [2, 1]; A[1][1] += 1
    st = initial_state(2)
    td = handle(st, [([1.0, 0.0], [0.0, 1.0], 2.0, False), ([0.0, 1.0], [9.0, 9.0], 1.0, True)], 0.5)
    assert td == [2.0, 1.0]                                         # theta was 0
    assert st["A"] == [[1e-6 + 1.0, 0.5 - 1.0 + 0.0], [0.0, 1e-6 + 1.0]] and st["b"] == [2.0, 1.0] and st["singular"] == 0
    x1 = 1.0 / (1e-6 + 1.0)
    assert st["theta"] == [(2.0 - (-0.5) * x1) / (1e-6 + 1.0), x1]
    # LSTDLambda, LAST TO FIRST, gamma = 0.5, lambda = 0.5 (c = 0.25).  The terminal transition comes first: z = [0, 1], b = [0, 1],
    # A += z (x) phi_s = [[1e-6, 0], [0, 1e-6 + 1]], z = 0.  Then transition 1: z = [1, 0], b = [2, 1], pd = [1, -0.5], A[0] += [1, -0.5]
    sl = initial_state(2, 0.5)
    handle(sl, [([1.0, 0.0], [0.0, 1.0], 2.0, False), ([0.0, 1.0], [9.0, 9.0], 1.0, True)], 0.5, 0.5)
    assert sl["A"] == [[1e-6 + 1.0, -0.5], [0.0, 1e-6 + 1.0]] and sl["b"] == [2.0, 1.0] and sl["z"] == [1.0, 0.0]
    # z survives the batch: the next batch's first visit decays it
    accumulate_lstd_lambda(sl, [([0.0, 1.0], [1.0, 0.0], 1.0, False)], 0.5, 0.5)
    assert sl["z"] == [0.25, 1.0] and sl["b"] == [2.25, 2.0]
    # the walks differ: the same two non-terminal transitions in the two orders give LSTDLambda different traces
    a, b = initial_state(2, 0.5), initial_state(2, 0.5)
    t1, t2 = ([1.0, 0.0], [0.0, 1.0], 1.0, False), ([0.0, 1.0], [1.0, 0.0], 1.0, False)
    accumulate_lstd_lambda(a, [t1, t2], 0.5, 0.5)
    accumulate_lstd_lambda(b, [t2, t1], 0.5, 0.5)
    assert a["z"] == [1.0, 0.25] and b["z"] == [0.25, 1.0]
    # an abandoned solve keeps theta and counts
    s0 = state_of([7.0, 8.0], [[1.0, 2.0], [1.0, 2.0]], [1.0, 1.0])
    solve(s0)
    assert s0["theta"] == [7.0, 8.0] and s0["singular"] == 1
    # an empty batch is still solved (the ABI's length 0 is "no call" instead: the binding's business)
    e = initial_state(2)
    accumulate_lstd(e, [], 0.5)
    assert e["A"] == [[1e-6, 0.0], [0.0, 1e-6]]


def test_header_binding_table_and_python_constants_agree():
    h = open(os.path.join(ROOT, "include", "rsrl_hip.h")).read()
    assert re.search(r"RSRL_LSTD\s*=\s*25\b", h) and re.search(r"RSRL_LSTD_LAMBDA\s*=\s*26\b", h)
    enum = h.split("rsrl_algo;")[0].split("typedef enum { RSRL_QLEARNING")[1]
    assert not re.search(r"=\s*24\b\s*[,}]", enum) and "(24 is no algo.)" in enum
    assert (rsrl_amd.LSTD, rsrl_amd.LSTD_LAMBDA) == (25, 26) and (rsrl_amd.context.LSTD, rsrl_amd.context.LSTD_LAMBDA) == (25, 26)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pub const RSRL_LSTD: i32 = 25;" in doc and "pub const RSRL_LSTD_LAMBDA: i32 = 26;" in doc
    for sym, n_args in (("rsrl_hip_handle_transitions", 9), ("rsrl_hip_lstd_solve", 1), ("rsrl_hip_get_lstd_batch_state", 7),
                        ("rsrl_hip_set_lstd_batch_state", 7)):
        assert "int %s(" % sym in h and len(_abi.SYMBOLS[sym][1]) == n_args, sym
        assert hasattr(_abi.lib(), sym)
    assert "NO SVD fallback" in h and "singular_solves" in h


def test_supported_configurations_reach_the_device_query():
    for algo, _ in ALGOS:
        for domain, order in SUPPORTED:
            for extra in (dict(), dict(steps_per_launch=1), dict(max_episode_steps=1), dict(max_episode_steps=1000, gamma=0.99, lam=0.9)):
                rc, msg = create_rc(BASE, algo=algo, domain=domain, order=order, **extra)
                # no GPU: every admission rule has passed and the device query answers "no device"; with one, the ctx is created
                assert rc == 0 or (rc == EHIP and "device" in msg), (algo, domain, order, extra, rc, msg)


def test_other_configurations_are_refused_with_a_message():
    bad = [dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(order=7), dict(domain=rsrl_amd.CART_POLE, order=2),
           dict(domain=rsrl_amd.CART_POLE, order=7), dict(domain=rsrl_amd.ACROBOT, order=3), dict(weight_mode=rsrl_amd.W_SHARED),
           dict(domain=rsrl_amd.CART_POLE, order=7, weight_dtype=rsrl_amd.W_BF16), dict(weight_dtype=rsrl_amd.W_BF16),
           dict(domain=rsrl_amd.HIV_TREATMENT, order=1), dict(policy=rsrl_amd.EPSILON_GREEDY), dict(policy=rsrl_amd.GREEDY),
           dict(policy=rsrl_amd.SOFTMAX), dict(agent_policy=rsrl_amd.RANDOM), dict(agent_policy=rsrl_amd.SOFTMAX), dict(epsilon_decay=0.99)]
    for algo, name in ALGOS:
        for b in bad:
            rc, msg = create_rc(BASE, algo=algo, **b)
            assert rc == EINVAL and name in msg and "register-family Fourier" in msg, (algo, b, rc, msg)
        rc, msg = create_rc(BASE, algo=algo, max_episode_steps=0)
        assert rc == EINVAL and name in msg and "max_episode_steps" in msg and "no record size" in msg, (rc, msg)
    for algo in (24, 27, 1000):
        for kw in (dict(), dict(max_episode_steps=0)):
            rc, msg = create_rc(BASE, algo=algo, **kw)
            assert rc == EINVAL and "unknown algo %d" % algo in msg, (algo, kw, rc, msg)


def test_example_compiles(tmp_path):
    compile_example(tmp_path, "lstd_lambda")
