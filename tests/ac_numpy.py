"""ActorCritic's rule restated in f64 numpy (control/ac.rs:108-114, sarsa.rs:43-73, softmax.rs:113-130, examples/a2c.rs:38-49): the critic's SARSA
step, then the Gibbs actor's step with the critic's target from the updated weights.  Shared by the CPU and GPU tests."""
import numpy as np


def softmax(h, tau):
    z = np.exp((h - np.max(h)) / tau)
    return z / z.sum()


def actor_step(Th, phi_s, a, scale, tau):
    """theta += scale * grad_log pi(a|s): column b moves by (1[b==a] - p_b) * phi(s), p from the pre-update theta (no 1/tau: softmax.rs:113-130)"""
    p = softmax(Th.T @ phi_s, tau)
    g = -p
    g[a] += 1.0
    return Th + scale * np.outer(phi_s, g)


def ac_rule(orc, q_critic, W, Th, phi_s, phi_n, a, r, term, gamma, lr, alpha, tau, x_inner):
    """one transition -> (delta, W', theta').  The critic's inner draw na ~ pi_theta(s') uses the oracle's Softmax sample on x_inner"""
    qsa = W[:, a] @ phi_s
    if term:
        d = r - qsa
    else:
        na = orc.policy_sample(orc.SOFTMAX, Th.T @ phi_n, x_inner, tau=tau)
        d = r + gamma * (W[:, na] @ phi_n) - qsa
    W2 = W.copy()
    W2[:, a] += lr * d * phi_s
    q2 = W2.T @ phi_s
    c = q2[a] if q_critic else q2[a] - q2 @ softmax(Th.T @ phi_s, tau)
    return d, W2, actor_step(Th, phi_s, a, alpha * c, tau)
