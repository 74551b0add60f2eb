"""LambdaLSPE (RSRL_LAMBDA_LSPE, 39) without a GPU: hand-computed batches pin the restated rule (tests/lspe_numpy.py: the backwards walk, the
terminal row without theta . phi(s), delta's reset and carry), the row rule (deferred below F rows), an abandoned elimination, the zeroing after a
success; the admission grid of 38 / 39 / 40 equals its fixture and 39 is admitted exactly where LSTDLambda (26) is; the header, the Python constant
and the Rust block agree on 39 with ABI 9 and 96 exports; examples/lambda_lspe.cpp compiles."""
import importlib.util
import json
import os
import re

import pytest

import rsrl_amd
from rsrl_amd import _abi
from tests.agent_contract import compile_example, create_rc
from tests.lspe_numpy import accumulate, handle, initial_state, solve, state_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EHIP = -1, -2
BASE = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=39, policy=rsrl_amd.RANDOM, n_envs=4, max_episode_steps=50)
E = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]      # the unit vectors of F = 4
ZERO = [[0.0] * 4 for _ in range(4)]


@pytest.fixture(scope="module")
def matrix():
    spec = importlib.util.spec_from_file_location("admission_matrix", os.path.join(ROOT, "scripts", "admission_matrix.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_hand_computed_batch_with_a_terminal_last_row():
    # F = 4, gamma = lambda = 0.5 (c = 0.25), theta = [1, 2, 3, 4], A = b = 0, delta = 4, no rows.  LAST TO FIRST.
    # Row 2 (terminal, r = 1, phi_s = e1): delta = 4 * 0.25 = 1; b += (delta + r) e1 = 2 e1 -- NOT (2 + theta . e1) e1 = 4 e1; A[1][1] = 1; delta = 0.
    # Row 1 (r = 2, phi_s = e0, phi_ns = e1): delta = 0 * 0.25 = 0; v_s = 1, v_n = 2; residual = 2 + 0.5 * 2 - 1 = 2; delta = 2;
    #   b += (v_s + delta) e0 = 3 e0; A[0][0] = 1.  Two rows of four: the solve is deferred and delta = 2 stays for the next batch.
    st = state_of([1.0, 2.0, 3.0, 4.0], ZERO, [0.0] * 4, delta=4.0, rows=0)
    td, did = handle(st, [(E[0], E[1], 2.0, False), (E[1], [9.0] * 4, 1.0, True)], 0.5, 0.5, 0.5)
    assert td == [2.0, 1.0 - 2.0] and did == "deferred"
    assert st["b"] == [3.0, 2.0, 0.0, 0.0] and st["A"] == [[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0.0] * 4, [0.0] * 4]
    assert st["delta"] == 2.0 and st["rows"] == 2 and st["theta"] == [1.0, 2.0, 3.0, 4.0] and st["singular"] == 0
    # (walked first to last the same batch gives b = [4, 1.75, 0, 0]: the order is observable)


def test_hand_computed_batch_with_a_non_terminal_last_row():
    # the same start.  Row 2 (r = 1, phi_s = e2, phi_ns = e3): delta = 1; v_s = 3, v_n = 4; residual = 1 + 0.5 * 4 - 3 = 0; delta = 1;
    #   b += (3 + 1) e2.  Row 1 (terminal, r = 2, phi_s = e0): delta = 0.25; b += (0.25 + 2) e0; delta = 0 -- the reset: nothing is carried out
    st = state_of([1.0, 2.0, 3.0, 4.0], ZERO, [0.0] * 4, delta=4.0, rows=0)
    td = accumulate(st, [(E[0], [9.0] * 4, 2.0, True), (E[2], E[3], 1.0, False)], 0.5, 0.5)
    assert td == [2.0 - 1.0, 0.0]
    assert st["b"] == [2.25, 0.0, 4.0, 0.0] and st["A"] == [[1.0, 0, 0, 0], [0.0] * 4, [0, 0, 1.0, 0], [0.0] * 4]
    assert st["delta"] == 0.0 and st["rows"] == 2
    # an outer product's element is phi_r * phi_j, and the scalar in front of phi(s) is one sum: b_r = b_r + (v_s + delta) * phi_r
    st = state_of([0.5, 0.0, 0.0, 0.0], ZERO, [0.0] * 4, delta=0.0, rows=0)
    phi = [0.1, 0.2, 0.3, 0.7]
    accumulate(st, [(phi, [0.0] * 4, 1.0, False)], 0.9, 0.5)
    v_s = 0.0 + 0.1 * 0.5 + 0.2 * 0.0 + 0.3 * 0.0 + 0.7 * 0.0
    delta = 0.0 * (0.9 * 0.5) + (1.0 + 0.9 * 0.0 - v_s)
    assert st["delta"] == delta and st["b"] == [0.0 + (v_s + delta) * p for p in phi]
    assert st["A"] == [[0.0 + p * q for q in phi] for p in phi]


def test_row_rule_defers_twice_and_solves_on_the_third_batch():
    F, alpha, gamma, lam = 4, 0.25, 0.5, 0.5
    st = state_of([1.0, 2.0, 3.0, 4.0], ZERO, [0.0] * 4, delta=0.0, rows=0)
    nxt = [0.0] * 4
    done = []
    deltas = []
    for batch in ([(E[0], nxt, 1.0, False)], [(E[1], nxt, 1.0, False), (E[2], nxt, 1.0, False)], [(E[3], nxt, 1.0, False)]):      # 1, F - 2, 1 rows
        before = st["theta"][:]
        done.append(handle(st, batch, alpha, gamma, lam)[1])
        deltas.append(st["delta"])
        if done[-1] == "deferred":
            assert st["theta"] == before and st["singular"] == 0
    assert done == ["deferred", "deferred", "solved"]
    # delta carries across the deferred solves: batch 1 leaves 1 - 1 = 0; batch 2 walks e2 (residual 1 - 3 = -2: delta = -2) then e1 (delta =
    # -2 * 0.25 + (1 - 2) = -1.5), and batch 3 starts from that: delta = -1.5 * 0.25 + (1 - 4) = -3.375, b[3] = v_s + delta = 0.625
    assert deltas[:2] == [0.0, -1.5]
    # A = I, b = [v_s + delta per row] = [1, 0.5, 1, 0.625]: x = b, theta = 0.75 theta + 0.25 x
    assert st["theta"] == [0.75 * 1.0 + 0.25 * 1.0, 0.75 * 2.0 + 0.25 * 0.5, 0.75 * 3.0 + 0.25 * 1.0, 0.75 * 4.0 + 0.25 * 0.625]
    assert st["A"] == ZERO and st["b"] == [0.0] * 4 and st["delta"] == 0.0 and st["rows"] == 0 and st["singular"] == 0
    # the count saturates at F, and the initial state (the identity's F rows) solves at its first batch, whatever its length
    st = state_of([0.0] * 4, E, [0.0] * 4, rows=3)
    accumulate(st, [(E[0], nxt, 0.0, False)] * 3, gamma, lam)
    assert st["rows"] == F
    first = initial_state(F)
    assert first["rows"] == F and first["delta"] == 0.0 and first["A"][2][2] == 1e-6 and handle(first, [(E[0], nxt, 1.0, False)], alpha, gamma, lam)[1] == "solved"
    assert first["theta"] == [0.25 * ((0.0 + 1.0) / (1e-6 + 1.0)), 0.0, 0.0, 0.0]


def test_abandoned_elimination_keeps_all_four_quantities_and_counts():
    A = [[1.0, 2.0, 0.0, 0.0], [1.0, 2.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]      # two equal rows
    st = state_of([7.0, 8.0, 9.0, 10.0], A, [1.0, 1.0, 1.0, 1.0], delta=0.25, rows=4)
    assert solve(st, 0.5) == "abandoned"
    assert st == state_of([7.0, 8.0, 9.0, 10.0], A, [1.0, 1.0, 1.0, 1.0], delta=0.25, rows=4, singular=1)
    # a None from the solver, whatever the matrix: the same; and below F rows the solver is not even asked
    st = state_of([7.0, 8.0, 9.0, 10.0], E, [1.0] * 4, delta=0.25, rows=4)
    assert solve(st, 0.5, solver=lambda A, b: None) == "abandoned" and st == state_of([7.0, 8.0, 9.0, 10.0], E, [1.0] * 4, delta=0.25, rows=4, singular=1)
    st["rows"] = 3
    assert solve(st, 0.5, solver=lambda A, b: 1 / 0) == "deferred" and st["singular"] == 1


def test_success_relaxes_theta_and_zeroes_the_rest():
    st = state_of([1.0, 2.0, 3.0, 4.0], [[2.0, 0, 0, 0], [0, 4.0, 0, 0], [0, 0, 5.0, 0], [0, 0, 0, 10.0]], [2.0, 4.0, 10.0, 10.0], delta=0.25, rows=4, singular=3)
    assert solve(st, 0.25) == "solved"
    assert st == state_of([0.75 * 1.0 + 0.25 * 1.0, 0.75 * 2.0 + 0.25 * 1.0, 0.75 * 3.0 + 0.25 * 2.0, 0.75 * 4.0 + 0.25 * 1.0], ZERO, [0.0] * 4, 0.0, 0, 3)
    # 1 - alpha is computed once and each element is three rounded operations
    st = state_of([0.1, 0.2, 0.3, 0.4], E, [0.7, 0.7, 0.7, 0.7], rows=4)
    solve(st, 0.3)
    assert st["theta"] == [(1.0 - 0.3) * t + 0.3 * 0.7 for t in (0.1, 0.2, 0.3, 0.4)]


def test_admission_grid_equals_its_fixture_and_39_is_admitted_where_26_is(matrix):
    assert dict(matrix.GRID_LSPE)["algo"] == [38, 39, 40] and [n for n, _ in matrix.GRID] == [n for n, _ in matrix.GRID_LSPE]
    assert all(v == w for (n, v), (_, w) in zip(matrix.GRID, matrix.GRID_LSPE) if n != "algo"), "the grid's other axes are the first's"
    entry = [g for g in matrix.GRIDS + matrix.GRIDS_SINCE if g[1] == matrix.LSPE_FIXTURE]
    assert len(entry) == 1 and entry[0][0] is matrix.GRID_LSPE and entry[0][2] == {"max_episode_steps": 200}
    doc = json.load(open(matrix.LSPE_FIXTURE))
    assert doc["grid"] == [[n, v] for n, v in matrix.GRID_LSPE] and doc["fixed"] == entry[0][2], "GRID_LSPE and its fixture drifted apart"
    res = matrix.sweep(matrix.GRID_LSPE, entry[0][2])
    assert {rc for rc, _ in res.values()} <= {EINVAL, EHIP, 0}
    assert sorted(k for k, (rc, _) in res.items() if rc != EINVAL) == doc["admitted"] and doc["admitted"], "the library against the fixture"
    ia = [n for n, _ in matrix.GRID].index("algo")
    assert {k[ia] for k in doc["admitted"]} == {"1"}                      # 39 only
    for k, (rc, msg) in res.items():
        if k[ia] != "1":
            assert rc == EINVAL and "unknown algo %d" % (38, 39, 40)[int(k[ia])] in msg, (k, rc, msg)
    # exactly LSTDLambda's admission: the same grid with 26 on the algo axis
    grid26 = [(n, [26] if n == "algo" else v) for n, v in matrix.GRID]
    of26 = sorted(k[:ia] + "_" + k[ia + 1:] for k, (rc, _) in matrix.sweep(grid26, entry[0][2]).items() if rc != EINVAL)
    assert of26 and of26 == sorted(k[:ia] + "_" + k[ia + 1:] for k in doc["admitted"])


def test_refusals_name_the_agent_and_alpha_must_be_finite():
    for bad in (dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(domain=rsrl_amd.CART_POLE, order=2), dict(weight_mode=rsrl_amd.W_SHARED),
                dict(policy=rsrl_amd.GREEDY), dict(agent_policy=rsrl_amd.RANDOM), dict(epsilon_decay=0.99)):
        rc, msg = create_rc(BASE, **bad)
        assert rc == EINVAL and "RSRL_LAMBDA_LSPE" in msg and "register-family Fourier" in msg, (bad, rc, msg)
    rc, msg = create_rc(BASE, max_episode_steps=0)
    assert rc == EINVAL and "RSRL_LAMBDA_LSPE" in msg and "no record size" in msg, (rc, msg)
    for alpha in (float("nan"), float("inf"), -float("inf")):
        rc, msg = create_rc(BASE, alpha=alpha)
        assert rc == EINVAL and "RSRL_LAMBDA_LSPE" in msg and "alpha" in msg and "finite" in msg, (alpha, rc, msg)
        rc, msg = create_rc(BASE, algo=rsrl_amd.LSTD_LAMBDA, alpha=alpha)      # (LSTDLambda does not read it)
        assert rc in (0, EHIP), (alpha, rc, msg)
    for alpha in (0.0, 1.0, -0.5, 2.0):
        rc, msg = create_rc(BASE, alpha=alpha, gamma=0.99, lam=0.8)
        assert rc == 0 or (rc == EHIP and "device" in msg), (alpha, rc, msg)
    for algo in (38, 40):
        rc, msg = create_rc(BASE, algo=algo)
        assert rc == EINVAL and "unknown algo %d" % algo in msg, (algo, rc, msg)


def test_header_python_constant_and_rust_block_agree_on_39():
    h = open(os.path.join(ROOT, "include", "rsrl_hip.h")).read()
    assert re.search(r"RSRL_LAMBDA_LSPE\s*=\s*39\b", h)
    enum = h.split("rsrl_algo;")[0].split("typedef enum { RSRL_QLEARNING")[1]
    assert not re.search(r"=\s*(38|40)\b\s*[,}]", enum) and "(40 is no algo.)" in enum and "neither is 38" in enum
    assert "Not built: LambdaLSPE" not in h and "lambda_lspe.rs:27-107" in h and "z[0] = delta" in h and "z[1] = rows" in h
    assert rsrl_amd.LAMBDA_LSPE == 39 and rsrl_amd.context.LAMBDA_LSPE == 39
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pub const RSRL_LAMBDA_LSPE: i32 = 39;" in doc
    # no new entry point: ABI 9, 96 exports
    assert re.search(r"#define\s+RSRL_HIP_ABI_VERSION\s+9\b", h) and _abi.lib().rsrl_hip_abi_version() == 9
    assert len(_abi.SYMBOLS) == 96 and len(re.findall(r"^\s*pub fn rsrl_hip_\w+\(", doc, flags=re.M)) == 96


def test_example_compiles(tmp_path):
    compile_example(tmp_path, "lambda_lspe")
