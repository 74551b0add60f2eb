"""ActorCritic without a GPU: the public header and the Python package expose it, examples/a2c.cpp compiles, and the numpy actor step the GPU tests
compare against is the gradient of log softmax(theta^T phi)[a] (a finite-difference check that pins the restatement independently of the device)."""
import os
import re

import numpy as np

import rsrl_amd
from rsrl_amd import _abi
from tests.ac_numpy import actor_step, softmax
from tests.agent_contract import compile_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_algos_and_the_policy_weight_exports():
    h = open(os.path.join(ROOT, "include", "rsrl_hip.h")).read()
    assert re.search(r"RSRL_ACTOR_CRITIC\s*=\s*10\b", h) and re.search(r"RSRL_Q_ACTOR_CRITIC\s*=\s*11\b", h)
    for name in ("rsrl_hip_get_policy_weights", "rsrl_hip_set_policy_weights"):
        assert re.search(r"\bint\s+" + name + r"\(rsrl_hip_ctx\* ctx, int64_t env_index, (const )?float\* theta", h), name
        assert name in _abi.SYMBOLS
    assert (rsrl_amd.ACTOR_CRITIC, rsrl_amd.Q_ACTOR_CRITIC) == (10, 11)
    assert hasattr(rsrl_amd.Context, "get_policy_weights") and hasattr(rsrl_amd.Context, "set_policy_weights")


def test_a2c_example_compiles(tmp_path):
    compile_example(tmp_path, "a2c")


def test_actor_step_is_the_gradient_of_log_pi():
    rng = np.random.default_rng(1)
    F, A, eps = 9, 3, 1e-6
    for _ in range(5):
        Th = rng.normal(0.0, 0.5, size=(F, A))
        phi = rng.uniform(-1.0, 1.0, size=F)
        a = int(rng.integers(0, A))
        grad = np.zeros_like(Th)
        for f in range(F):
            for b in range(A):
                d = np.zeros_like(Th)
                d[f, b] = eps
                lp = np.log(softmax((Th + d).T @ phi, 1.0)[a])
                lm = np.log(softmax((Th - d).T @ phi, 1.0)[a])
                grad[f, b] = (lp - lm) / (2 * eps)
        step = actor_step(Th, phi, a, 1.0, 1.0) - Th
        assert np.allclose(step, grad, atol=1e-7, rtol=1e-6)
