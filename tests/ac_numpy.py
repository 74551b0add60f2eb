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


def near_boundary(p, x, margin=1e-5):
    """the draw's uniform lies within margin of a cumulative-probability boundary: an fp32 rounding may pick the neighbour"""
    u = (int(x[2]) >> 8) / 16777216.0
    return bool(np.min(np.abs(np.cumsum(p)[:-1] - u), initial=1.0) < margin)


def ac_restated_loop(orc, critic_q, domain, order, N, K, cap, seed, gamma, lr, alpha, tau, S0, A0, t0=0, env_offset=0, W0=None, Th0=None):
    """the driver loop per learner in f64 on the same draws (W0 / Th0: lists of the learners' initial matrices, default zeros) -- batch-steps t0 .. t0 + K - 1 of the learners env_offset .. env_offset + N - 1 -> (actions
    [K][N] after every batch-step, W, theta, learners with a draw within 1e-5 of a cumulative-probability boundary: the critic's inner draw moves W
    without changing any action the loop shows)"""
    F, A = (order + 1) ** S0.shape[0], 2 if domain == orc.CART_POLE else 3
    acts, out_W, out_T, near = np.zeros((K, N), dtype=np.int64), [], [], np.zeros(N, dtype=bool)
    for i in range(N):
        W = np.zeros((F, A)) if W0 is None else np.array(W0[i], dtype=np.float64)
        Th = np.zeros((F, A)) if Th0 is None else np.array(Th0[i], dtype=np.float64)
        s, a, ep = S0[:, i].copy(), int(A0[i]), 0
        for k in range(K):
            t, gid = t0 + k, env_offset + i
            ns, r, term = orc.domain_step(domain, s, a, prec="f32d")
            ns = np.asarray(ns, dtype=np.float32)
            ep += 1
            trunc = (not term) and cap > 0 and ep >= cap
            if term:
                ns = orc.domain_reset(domain, prec="f32")
            phi_s, phi_n = orc.fourier_project(domain, order, s), orc.fourier_project(domain, order, ns)
            xin = orc.draw(seed, gid, t, orc.BLK_INNER)
            near[i] |= (not term) and near_boundary(orc.policy_probs(orc.SOFTMAX, Th.T @ phi_n, tau=tau), xin)
            _, W, Th = ac_rule(orc, critic_q, W, Th, phi_s, phi_n, a, float(np.float32(r)), term, gamma, lr, alpha, tau, xin)
            if term or trunc:
                ep = 0
                ns = orc.domain_reset(domain, prec="f32")
            xs = orc.draw(seed, gid, t, orc.BLK_RESET if trunc else orc.BLK_STEP)
            hn = Th.T @ orc.fourier_project(domain, order, ns)
            near[i] |= near_boundary(orc.policy_probs(orc.SOFTMAX, hn, tau=tau), xs)
            a = orc.policy_sample(orc.SOFTMAX, hn, xs, tau=tau)
            acts[k, i] = a
            s = np.asarray(ns, dtype=np.float32)
        out_W.append(W); out_T.append(Th)
    return acts, out_W, out_T, near
