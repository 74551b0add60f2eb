"""REINFORCE and BaselineREINFORCE (RSRL_REINFORCE, RSRL_BASELINE_REINFORCE) without a GPU: the f64 rule on a hand-worked batch (the return
runs forward), the header and the Python constants agree, the configurations admitted are exactly ActorCritic's, examples/reinforce.cpp
compiles."""
import ctypes as C
import itertools
import json
import os
import re

import numpy as np

import rsrl_amd
from rsrl_amd import _abi
from tests.agent_contract import compile_example, create_rc
from tests.reinforce_numpy import reinforce_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EHIP = -1, -2
FIXTURE = os.path.join(ROOT, "tests", "golden", "create_admission.json")


BASE = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=rsrl_amd.REINFORCE, policy=rsrl_amd.SOFTMAX, n_envs=4)


def test_rule_on_a_hand_worked_batch():
    # F = 2, A = 2, theta = 0, gamma = 0.5, alpha = 0.1, tau = 1; (phi, a, r) = ([1,0], 0, 1), ([0,1], 1, 2), ([1,0], 0, 3)
    phis = [np.array([1.0, 0.0]), np.array([0.0, 1.0]), np.array([1.0, 0.0])]
    acts, rews = [0, 1, 0], [1.0, 2.0, 3.0]
    Th, rets = reinforce_batch(np.zeros((2, 2)), phis, acts, rews, gamma=0.5, alpha=0.1, tau=1.0)
    # forward: g = 1, 1*0.5 + 2 = 2.5, 2.5*0.5 + 3 = 4.25 (the return-to-go would be 2.75, 3.5, 3)
    assert np.allclose(rets, [1.0, 2.5, 4.25])
    # e = 0.1, 0.25, 0.425.  Step 1: p = (0.5, 0.5), row 0 += 0.1 * (0.5, -0.5).  Step 2: row 1 is still zero, p = (0.5, 0.5),
    # row 1 += 0.25 * (-0.5, 0.5).  Step 3 reads the row 0 step 1 wrote: p_0 = 1 / (1 + exp(-0.1)), row 0 += 0.425 * (1 - p_0, p_0 - 1)
    q = 1.0 - 1.0 / (1.0 + np.exp(-0.1))
    assert np.allclose(Th, [[0.05 + 0.425 * q, -0.05 - 0.425 * q], [-0.125, 0.125]], rtol=0, atol=1e-15)
    # a baseline subtracts B[:, a] . phi from each g: with B[0, 0] = 1, steps 1 and 3 use g - 1
    B = np.array([[1.0, 0.0], [0.0, 0.0]])
    ThB, retsB = reinforce_batch(np.zeros((2, 2)), phis, acts, rews, gamma=0.5, alpha=0.1, tau=1.0, B=B)
    assert retsB == rets and np.allclose(ThB[1], Th[1]) and np.allclose(ThB[0], [0.0 + 0.325 * 0.5, 0.0 - 0.325 * 0.5])
    # B = 0 is REINFORCE exactly
    Th0, _ = reinforce_batch(np.zeros((2, 2)), phis, acts, rews, gamma=0.5, alpha=0.1, tau=1.0, B=np.zeros((2, 2)))
    assert np.array_equal(Th0, Th)


def test_header_and_constants_agree():
    h = open(os.path.join(ROOT, "include", "rsrl_hip.h")).read()
    assert re.search(r"RSRL_REINFORCE\s*=\s*15\b", h) and re.search(r"RSRL_BASELINE_REINFORCE\s*=\s*16\b", h)
    assert rsrl_amd.REINFORCE == 15 and rsrl_amd.BASELINE_REINFORCE == 16
    enum = h.split("rsrl_algo;")[0].split("typedef enum { RSRL_QLEARNING")[1]
    assert not re.search(r"=\s*1[24]\b\s*[,}]", enum)
    assert re.search(r"#define RSRL_HIP_ABI_VERSION 9\b", h)
    for name in ("rsrl_hip_handle_batch", "rsrl_hip_get_behaviour_weights", "rsrl_hip_set_behaviour_weights", "rsrl_hip_get_return_carry",
                 "rsrl_hip_set_return_carry"):
        assert re.search(r"\bint " + name + r"\(", h), name
        assert hasattr(_abi.lib(), name), name


def _grid():
    return [(n, v) for n, v in json.load(open(FIXTURE))["grid"]]


def _sweep(algo):
    """the admission axes of the stored fixture with algo fixed -> the admitted index strings (the algo axis' index written as ActorCritic's)"""
    grid = _grid()
    ia = [n for n, _ in grid].index("algo")
    ac_index = grid[ia][1].index(rsrl_amd.ACTOR_CRITIC)
    L = _abi.lib()
    base = _abi.Config()
    assert L.rsrl_hip_config_init(C.byref(base)) == 0
    h = C.c_void_p()
    admitted, codes = set(), set()
    axes = [(n, v) for n, v in grid if n != "algo"]
    for idx in itertools.product(*(range(len(v)) for _, v in axes)):
        cfg = _abi.Config.from_buffer_copy(base)
        cfg.algo = algo
        for (name, vals), i in zip(axes, idx):
            setattr(cfg, name, vals[i])
        rc = L.rsrl_hip_create(C.byref(cfg), C.byref(h))
        if rc == 0:
            L.rsrl_hip_destroy(h)
        codes.add(rc)
        if rc in (0, EHIP):
            full = list(idx)
            full.insert(ia, ac_index)
            admitted.add("".join("%x" % i for i in full))
    return admitted, codes


def test_admitted_set_is_actor_critics():
    grid = _grid()
    ia = [n for n, _ in grid].index("algo")
    ac_index = grid[ia][1].index(rsrl_amd.ACTOR_CRITIC)
    want = {k for k in json.load(open(FIXTURE))["admitted"] if int(k[ia], 16) == ac_index}
    assert want
    for algo in (rsrl_amd.REINFORCE, rsrl_amd.BASELINE_REINFORCE):
        got, codes = _sweep(algo)
        assert codes <= {0, EINVAL, EHIP}, codes
        assert got == want, (algo, sorted(got ^ want)[:10])


def test_refusals_name_the_algo():
    bad = [dict(basis=rsrl_amd.TILE_CODING), dict(order=6), dict(order=7), dict(domain=rsrl_amd.CART_POLE, order=2),
           dict(weight_mode=rsrl_amd.W_SHARED), dict(weight_dtype=rsrl_amd.W_BF16), dict(domain=rsrl_amd.HIV_TREATMENT, order=1),
           dict(policy=rsrl_amd.EPSILON_GREEDY), dict(policy=rsrl_amd.RANDOM), dict(agent_policy=rsrl_amd.SOFTMAX), dict(epsilon_decay=0.99)]
    for algo, name in ((rsrl_amd.REINFORCE, "RSRL_REINFORCE"), (rsrl_amd.BASELINE_REINFORCE, "RSRL_BASELINE_REINFORCE")):
        for b in bad:
            rc, msg = create_rc(BASE, algo=algo, **b)
            assert rc == EINVAL and name in msg and "register-family Fourier" in msg, (algo, b, rc, msg)
    for algo in (12, 14, 17, -1):
        rc, msg = create_rc(BASE, algo=algo)
        assert rc == EINVAL and "unknown algo %d" % algo in msg


def test_reinforce_example_compiles(tmp_path):
    compile_example(tmp_path, "reinforce")
