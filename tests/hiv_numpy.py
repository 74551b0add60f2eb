"""numpy f64 restatement of HIVTreatment (rsrl_domains/src/hiv.rs, ode.rs) for the HIV tests: the expressions are the reference's, written in
the same order (numpy's float64 operations are IEEE and never fused), vectorised over learners -- arrays (6, N) of hidden states."""
import numpy as np

# model parameters (hiv.rs:5-25)
LAMBDA1, LAMBDA2, D1, D2, F, K1, K2, DELTA, M1, M2 = 1e4, 31.98, 0.01, 0.01, 0.34, 8e-7, 1e-4, 0.7, 1e-5, 1e-5
NT, C, RHO1, RHO2, LAMBDA_E, BE, KB, DE, KD, DELTA_E = 100.0, 13.0, 1.0, 1.0, 1.0, 0.3, 100.0, 0.25, 500.0, 0.1
DT, SIM_STEPS = 5.0, 1000
DT_STEP = DT / float(SIM_STEPS)
LIMITS = (-5.0, 8.0)
ALL_ACTIONS = np.array([[0.0, 0.0], [0.7, 0.0], [0.0, 0.3], [0.7, 0.3]])
DEFAULT = np.array([163573.0, 11945.0, 5.0, 46.0, 63919.0, 24.0])
D, A = 6, 4


def grad(eps0, eps1, y):
    """HIVTreatment::grad (hiv.rs:73-100); eps0, eps1, y[i]: arrays over learners"""
    t1, t1s, t2, t2s, v, e = y
    tmp1 = (1.0 - eps0) * K1 * v * t1
    tmp2 = (1.0 - F * eps0) * K2 * v * t2
    sum_ts = t1s + t2s
    return np.stack([
        LAMBDA1 - D1 * t1 - tmp1,
        tmp1 - DELTA * t1s - M1 * e * t1s,
        LAMBDA2 - D2 * t2 - tmp2,
        tmp2 - DELTA * t2s - M2 * e * t2s,
        (1.0 - eps1) * NT * DELTA * sum_ts - C * v - ((1.0 - eps0) * RHO1 * K1 * t1 + (1.0 - F * eps0) * RHO2 * K2 * t2) * v,
        LAMBDA_E + BE * sum_ts / (sum_ts + KB) * e - DE * sum_ts / (sum_ts + KD) * e - DELTA_E * e,
    ])


def rk4(eps0, eps1, y, dx):
    """runge_kutta4 (ode.rs:1-43)"""
    k1 = grad(eps0, eps1, y) * dx
    k2 = grad(eps0, eps1, y + k1 / 2.0) * dx
    k3 = grad(eps0, eps1, y + k2 / 2.0) * dx
    k4 = grad(eps0, eps1, y + k3) * dx
    return y + (k1 + 2.0 * k2 + 2.0 * k3 + k4) / 6.0


def observe(y):
    """emit (hiv.rs:112-119): clip!(-5, log10 y, 8); f64::min / max ignore a NaN operand, as np.fmin / np.fmax do"""
    with np.errstate(all="ignore"):
        return np.fmax(LIMITS[0], np.fmin(LIMITS[1], np.log10(y)))


def reward(obs, a):
    eps = ALL_ACTIONS[np.asarray(a)]
    r = 1e3 * obs[5] - 0.1 * obs[4] - 2e4 * eps[:, 0] ** 2 - 2e3 * eps[:, 1] ** 2
    return r / 1e5


def step(y, a):
    """Domain::step (hiv.rs:54-71, :121-135) for every learner: y (6, N) f64, a (N,) -> (y', observation f64, reward f64)"""
    eps = ALL_ACTIONS[np.asarray(a)]
    eps0, eps1 = eps[:, 0], eps[:, 1]
    y = np.array(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        for _ in range(SIM_STEPS):
            y = rk4(eps0, eps1, y, DT_STEP)
    obs = observe(y)
    return y, obs, reward(obs, a)


def coefficients(order, dim):
    """the Fourier basis' coefficient vectors: lexicographic, last dimension fastest, all-zero skipped, the constant (with_bias) last"""
    c = np.array(np.meshgrid(*[np.arange(order + 1)] * dim, indexing="ij")).reshape(dim, -1).T
    return np.concatenate([c[1:], c[:1]])


def fourier(s, order, lo, hi):
    """phi (F, M) in f64 of states s (D, M): cos(pi c . (s - lo) / (hi - lo))"""
    s = np.asarray(s, dtype=np.float64)
    lo = np.asarray(lo, dtype=np.float64).reshape(-1, 1)
    hi = np.asarray(hi, dtype=np.float64).reshape(-1, 1)
    sc = (s - lo) / (hi - lo)
    c = coefficients(order, s.shape[0]).astype(np.float64)
    return np.cos(np.pi * (c @ sc))


def bits_equal(a, b):
    """bitwise equality of f64 arrays, NaNs of any payload counting as equal (the sign / payload of a NaN is not IEEE-specified)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def q_learning_random_loop(orc, lo, hi, order, F, N, K, cap, seed, lr, gamma, t0=0, env_offset=0, W0=None):
    """the driver loop of QLearning under the Random policy from a fresh default env, f64, on the draws of batch-steps t0 .. t0 + K - 1 of the learners
    env_offset .. env_offset + N - 1 -> (first actions, actions, hidden states y, fp32 observations, episode steps, W (N, F, 4), truncations)"""
    first = a = np.array([orc.policy_sample(orc.RANDOM, np.zeros(4), orc.draw(seed, env_offset + i, t0, orc.BLK_INIT)) for i in range(N)])
    y = np.tile(DEFAULT.reshape(6, 1), (1, N))
    obs32 = observe(y).astype(np.float32)
    W = np.zeros((N, F, 4)) if W0 is None else np.array(W0, dtype=np.float64)          # (W0: the learners' initial weights (N, F, 4))
    ep = np.zeros(N, dtype=int)
    n_trunc = 0
    for k in range(K):
        t = t0 + k
        y, obs, r = step(y, a)
        nobs32 = obs.astype(np.float32)
        r32 = r.astype(np.float32).astype(np.float64)
        phi_s, phi_n = fourier(obs32, order, lo, hi), fourier(nobs32, order, lo, hi)
        ep += 1
        for i in range(N):
            qs, qn = W[i].T @ phi_s[:, i], W[i].T @ phi_n[:, i]
            W[i][:, a[i]] += lr * (r32[i] + gamma * qn.max() - qs[a[i]]) * phi_s[:, i]
        a = np.array([orc.policy_sample(orc.RANDOM, np.zeros(4), orc.draw(seed, env_offset + i, t, orc.BLK_STEP)) for i in range(N)])
        done = ep >= cap
        if done.any():
            n_trunc += int(done.sum())
            y[:, done] = DEFAULT.reshape(6, 1)
            nobs32[:, done] = observe(DEFAULT.reshape(6, 1)).astype(np.float32)
            ep[done] = 0
            a = np.where(done, [orc.policy_sample(orc.RANDOM, np.zeros(4), orc.draw(seed, env_offset + i, t, orc.BLK_RESET)) for i in range(N)], a)
        obs32 = nobs32
    return first, a, y, obs32, ep, W, n_trunc
