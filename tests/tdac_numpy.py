"""The TD ActorCritic's rule restated in f64 numpy (control/ac.rs:32-52, :108-114 with prediction/td/td.rs:31-59 as its evaluator, in the order of
examples/tdac.rs): TD(0) on V first, then TDCritic's target from the UPDATED V, then the Gibbs actor's step.  Shared by the CPU and GPU tests."""
import numpy as np

from tests.ac_numpy import actor_step, near_boundary


def tdac_rule(w, Th, phi_s, phi_n, a, r, term, gamma, lr, alpha, tau):
    """one transition -> (delta, w', theta').  w: V's weights (F,) or (F, 1); Th: the actor's (F, A).  On a terminal transition the critic reads
    V of the terminal state s' itself: c = r - V'(s')"""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    v_s, v_n = w @ phi_s, w @ phi_n
    d = r - v_s if term else r + gamma * v_n - v_s
    w2 = w + lr * d * phi_s
    c = r - w2 @ phi_n if term else r + gamma * (w2 @ phi_n) - w2 @ phi_s
    return d, w2, actor_step(Th, phi_s, a, alpha * c, tau)


def tdac_restated_loop(orc, domain, order, N, K, cap, seed, gamma, lr, alpha, tau, S0, A0, t0=0, env_offset=0, w0=None, Th0=None):
    """the driver loop per learner in f64 on the same draws (w0 / Th0: lists of the learners' initial weights, default zeros) -- batch-steps t0 .. t0 + K - 1 of the learners env_offset .. env_offset + N - 1 -> (actions
    [K][N] after every batch-step, w, theta, learners with a draw within 1e-5 of a cumulative-probability boundary)"""
    F, A = (order + 1) ** S0.shape[0], 2 if domain == orc.CART_POLE else 3
    acts, out_w, out_T, near = np.zeros((K, N), dtype=np.int64), [], [], np.zeros(N, dtype=bool)
    for i in range(N):
        w = np.zeros(F) if w0 is None else np.array(w0[i], dtype=np.float64).reshape(-1)
        Th = np.zeros((F, A)) if Th0 is None else np.array(Th0[i], dtype=np.float64)
        s, a, ep = S0[:, i].copy(), int(A0[i]), 0
        for k in range(K):
            ns, r, term = orc.domain_step(domain, s, a, prec="f32d")
            ns = np.asarray(ns, dtype=np.float32)                     # a terminal transition's s' is the terminal state: the critic reads it
            ep += 1
            trunc = (not term) and cap > 0 and ep >= cap
            phi_s, phi_n = orc.fourier_project(domain, order, s), orc.fourier_project(domain, order, ns)
            _, w, Th = tdac_rule(w, Th, phi_s, phi_n, a, float(np.float32(r)), term, gamma, lr, alpha, tau)
            if term or trunc:
                ep = 0
                ns = orc.domain_reset(domain, prec="f32")
            xs = orc.draw(seed, env_offset + i, t0 + k, orc.BLK_RESET if trunc else orc.BLK_STEP)
            hn = Th.T @ orc.fourier_project(domain, order, ns)
            near[i] |= near_boundary(orc.policy_probs(orc.SOFTMAX, hn, tau=tau), xs)
            a = orc.policy_sample(orc.SOFTMAX, hn, xs, tau=tau)
            acts[k, i] = a
            s = np.asarray(ns, dtype=np.float32)
        out_w.append(w); out_T.append(Th)
    return acts, out_w, out_T, near
