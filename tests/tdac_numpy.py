"""The TD ActorCritic's rule restated in f64 numpy (control/ac.rs:32-52, :108-114 with prediction/td/td.rs:31-59 as its evaluator, in the order of
examples/tdac.rs): TD(0) on V first, then TDCritic's target from the UPDATED V, then the Gibbs actor's step.  Shared by the CPU and GPU tests."""
import numpy as np

from tests.ac_numpy import actor_step


def tdac_rule(w, Th, phi_s, phi_n, a, r, term, gamma, lr, alpha, tau):
    """one transition -> (delta, w', theta').  w: V's weights (F,) or (F, 1); Th: the actor's (F, A).  On a terminal transition the critic reads
    V of the terminal state s' itself: c = r - V'(s')"""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    v_s, v_n = w @ phi_s, w @ phi_n
    d = r - v_s if term else r + gamma * v_n - v_s
    w2 = w + lr * d * phi_s
    c = r - w2 @ phi_n if term else r + gamma * (w2 @ phi_n) - w2 @ phi_s
    return d, w2, actor_step(Th, phi_s, a, alpha * c, tau)
