"""REINFORCE's and BaselineREINFORCE's Handler<&Batch>::handle restated in f64 numpy (control/mc/reinforce.rs, control/mc/baseline_reinforce.rs):
the batch is walked FORWARD and each transition's update is applied before the next one's probabilities are taken.  Shared by the CPU and GPU
tests."""
import numpy as np

from tests.ac_numpy import actor_step, near_boundary


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


def reinforce_restated_loop(orc, domain, order, N, K, cap, seed, gamma, alpha, tau, S0, A0, B=None, t0=0, env_offset=0, Th0=None):
    """the driver loop per learner in f64 on the same draws (Th0: list of the learners' initial theta = theta_b, default zeros) -- batch-steps t0 .. t0 + K - 1 of the learners env_offset .. env_offset + N - 1 --, each
    episode sampled from theta as it stood when the episode began -> (actions [K][N], theta, theta_b, learners with a draw within 1e-5 of a
    cumulative-probability boundary)"""
    F, A = (order + 1) ** S0.shape[0], 2 if domain == orc.CART_POLE else 3
    acts, out_T, out_b, near = np.zeros((K, N), dtype=np.int64), [], [], np.zeros(N, dtype=bool)
    for i in range(N):
        Th = np.zeros((F, A)) if Th0 is None else np.array(Th0[i], dtype=np.float64)
        Tb, g = Th.copy(), 0.0
        s, a, ep = S0[:, i].copy(), int(A0[i]), 0
        for k in range(K):
            ns, r, term = orc.domain_step(domain, s, a, prec="f32d")
            ep += 1
            trunc = (not term) and cap > 0 and ep >= cap
            phi_s = orc.fourier_project(domain, order, s)
            g = float(np.float32(r)) + gamma * g
            e = alpha * g if B is None else alpha * (g - B[i][:, a] @ phi_s)
            Th = actor_step(Th, phi_s, a, e, tau)
            if term or trunc:
                ep, g, Tb = 0, 0.0, Th.copy()
                ns = orc.domain_reset(domain, prec="f32")
            xs = orc.draw(seed, env_offset + i, t0 + k, orc.BLK_RESET if trunc else orc.BLK_STEP)
            hb = Tb.T @ orc.fourier_project(domain, order, np.asarray(ns, dtype=np.float32))
            near[i] |= near_boundary(orc.policy_probs(orc.SOFTMAX, hb, tau=tau), xs)
            a = orc.policy_sample(orc.SOFTMAX, hb, xs, tau=tau)
            acts[k, i] = a
            s = np.asarray(ns, dtype=np.float32)
        out_T.append(Th); out_b.append(Tb)
    return acts, out_T, out_b, near
