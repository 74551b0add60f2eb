"""REINFORCE's and BaselineREINFORCE's Handler<&Batch>::handle restated in f64 numpy (control/mc/reinforce.rs, control/mc/baseline_reinforce.rs):
the batch is walked FORWARD and each transition's update is applied before the next one's probabilities are taken.  Shared by the CPU and GPU
tests."""
import numpy as np

from tests.ac_numpy import actor_step


def reinforce_batch(Th, phis, actions, rewards, gamma, alpha, tau, B=None):
    """one batch -> (theta', [g_t]).  g_t = r_t + gamma * g_{t-1} from g = 0 (the discounted sum of the rewards seen so far, as the reference's
    loop computes it); e_t = alpha * g_t, or alpha * (g_t - B[:, a_t] . phi_t) with a baseline B (F, A); theta's step is ActorCritic's actor_step
    with the current theta"""
    Th = np.asarray(Th, dtype=np.float64)
    g, rets = 0.0, []
    for phi, a, r in zip(phis, actions, rewards):
        g = r + gamma * g
        e = alpha * g if B is None else alpha * (g - np.asarray(B, dtype=np.float64)[:, a] @ phi)
        Th = actor_step(Th, phi, int(a), e, tau)
        rets.append(g)
    return Th, rets
