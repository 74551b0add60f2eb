"""ActorCritic with the TD(0) state-value critic (RSRL_TD_ACTOR_CRITIC) without a GPU: the header declares it, every supported configuration
passes admission and reaches the device query while every other one is refused with a message, examples/tdac.cpp compiles, and the f64 rule the
GPU tests compare against reproduces a hand-checked case -- a terminal transition included, whose critic reads V of the terminal state."""
import os
import re

import numpy as np

import rsrl_amd
from tests.agent_contract import compile_example, create_rc
from tests.tdac_numpy import tdac_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EHIP = -1, -2
SUPPORTED = [(rsrl_amd.MOUNTAIN_CAR, o) for o in (1, 2, 3, 4, 5)] + [(rsrl_amd.CART_POLE, 1), (rsrl_amd.ACROBOT, 1)]


BASE = dict(domain=rsrl_amd.MOUNTAIN_CAR, order=3, algo=rsrl_amd.TD_ACTOR_CRITIC, policy=rsrl_amd.SOFTMAX, n_envs=4)


def test_header_declares_the_algo():
    h = open(os.path.join(ROOT, "include", "rsrl_hip.h")).read()
    assert re.search(r"RSRL_TD_ACTOR_CRITIC\s*=\s*13\b", h)
    assert not re.search(r"=\s*12\b\s*[,}]", h.split("rsrl_algo;")[0].split("typedef enum { RSRL_QLEARNING")[1])
    assert rsrl_amd.TD_ACTOR_CRITIC == 13


def test_supported_configurations_reach_the_device_query():
    for domain, order in SUPPORTED:
        for extra in (dict(), dict(steps_per_launch=1), dict(tau=0.5, max_episode_steps=100)):
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
        assert rc == EINVAL and "RSRL_TD_ACTOR_CRITIC" in msg and "register-family Fourier" in msg, (b, rc, msg)
    rc, msg = create_rc(BASE, algo=12)
    assert rc == EINVAL and "unknown algo 12" in msg
    rc, msg = create_rc(BASE, algo=14)
    assert rc == EINVAL and "unknown algo 14" in msg


def test_tdac_example_compiles(tmp_path):
    compile_example(tmp_path, "tdac")


def test_rule_on_a_hand_checked_case():
    # F = 3, A = 2, theta = 0 (p = [0.5, 0.5]), a = 1, r = -1, gamma = 0.5, lr = 0.1, alpha = 0.2, tau = 1
    w = np.array([0.2, 0.4, -0.1])
    Th = np.zeros((3, 2))
    phi_s, phi_n = np.array([1.0, 0.5, 0.0]), np.array([1.0, 0.0, 1.0])
    kw = dict(gamma=0.5, lr=0.1, alpha=0.2, tau=1.0)
    # non-terminal: V(s) = 0.4, V(s') = 0.1, delta = -1 + 0.05 - 0.4; w' = w - 0.135 phi(s); c = -1 + 0.5 V'(s') - V'(s) = -1 - 0.0175 - 0.23125
    d, w2, T2 = tdac_rule(w, Th, phi_s, phi_n, 1, -1.0, False, **kw)
    assert np.isclose(d, -1.35)
    assert np.allclose(w2, [0.065, 0.3325, -0.1])
    c = -1.24875
    assert np.allclose(T2, 0.2 * c * np.outer(phi_s, [-0.5, 0.5]))
    assert np.allclose(T2[:, 0], [0.124875, 0.0624375, 0.0])
    # terminal: delta = r - V(s) = -1.4; w' = w - 0.14 phi(s) = [0.06, 0.33, -0.1]; c = r - V'(s') = -1 - (0.06 - 0.1) = -0.96 (V of s', not of s)
    d, w2, T2 = tdac_rule(w, Th, phi_s, phi_n, 1, -1.0, True, **kw)
    assert np.isclose(d, -1.4)
    assert np.allclose(w2, [0.06, 0.33, -0.1])
    assert np.allclose(T2[:, 0], [0.096, 0.048, 0.0]) and np.allclose(T2[:, 1], [-0.096, -0.048, 0.0])
    # the actor's step for a given critic target is ActorCritic's (tests/ac_numpy.py), w is untouched by theta
    d2, w3, _ = tdac_rule(w, np.ones((3, 2)), phi_s, phi_n, 1, -1.0, True, **kw)
    assert d2 == d and np.array_equal(w3, w2)
