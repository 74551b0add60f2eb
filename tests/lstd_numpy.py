"""RecursiveLSTD and iLSTD restated literally in f64 numpy (prediction/lstd/recursive_lstd.rs, prediction/lstd/ilstd.rs, utils.rs:6-21 argmaxima),
every product rounded and every dot product summed in index order.  Shared by the CPU and GPU tests."""
import numpy as np

F64_MIN = -np.finfo(np.float64).max


def dot(x, y):
    """sum_j x_j * y_j in index order from 0.0"""
    acc = 0.0
    for a, b in zip(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)):
        acc = acc + float(a) * float(b)
    return acc


def matvec(M, x):
    return np.array([dot(row, x) for row in np.asarray(M, dtype=np.float64)])


def argmaxima(vals):
    """utils.rs argmaxima: the tolerance test comes first (|v - max| < 1e-7 appends v's index without raising max), then v > max restarts the list;
    max starts at f64::MIN"""
    mx, ixs = F64_MIN, []
    for i, v in enumerate(vals):
        v = float(v)
        if abs(v - mx) < 1e-7:
            ixs.append(i)
        elif v > mx:
            mx = v
            ixs = [i]
    return ixs, mx


def recursive_lstd_init(F):
    return np.zeros(F), np.eye(F) * 1e-5


def recursive_lstd(theta, C, phi_s, phi_n, r, term, gamma):
    """RecursiveLSTD::handle -> (residual, theta', C').  The terminal branch zeroes C (after computing v with it)"""
    theta, C = np.array(theta, dtype=np.float64), np.array(C, dtype=np.float64)
    theta_s = dot(phi_s, theta)
    if term:
        v = matvec(C, phi_s)
        a = 1.0 + dot(v, phi_s)
        residual = r - theta_s
        C[:] = 0.0
        theta = theta + (residual / a) * v
        return residual, theta, C
    theta_ns = dot(phi_n, theta)
    pd = (-gamma * np.asarray(phi_n, dtype=np.float64)) + phi_s
    g = matvec(C, pd)
    a = 1.0 + dot(g, phi_s)
    v = matvec(C, phi_s)
    residual = r + gamma * theta_ns - theta_s
    vg = np.outer(v, g)                                      # v_r * g_j, rounded
    C = C + (-1.0 / a) * vg
    theta = theta + (residual / a) * v
    return residual, theta, C


def ilstd_init(F):
    return np.zeros(F), np.eye(F), np.zeros(F)


def ilstd_solve(theta, A, mu, alpha, n_updates, rounds=None):
    """n_updates rounds of iLSTD::solve; rounds (a list): receives mu at the start of every round"""
    theta, mu = np.array(theta, dtype=np.float64), np.array(mu, dtype=np.float64)
    for _ in range(n_updates):
        if rounds is not None:
            rounds.append(mu.copy())
        idx, _ = argmaxima(np.abs(mu))
        for j in idx:                                        # in order: a later j reads the mu an earlier one changed
            u = alpha * mu[j]
            theta[j] += u
            mu = mu + (-u) * A[:, j]
    return theta, mu


def ilstd(theta, A, mu, phi_s, phi_n, r, term, gamma, alpha, n_updates, literal=True, rounds=None):
    """iLSTD::handle -> (diagnostic r + gamma V(s') - V(s) (terminal: r - V(s)) with the pre-update theta, theta', A', mu').  literal=False computes
    (phi_s pd^T) theta as phi_s * (pd . theta), the device's form"""
    theta, A, mu = np.array(theta, dtype=np.float64), np.array(A, dtype=np.float64), np.array(mu, dtype=np.float64)
    phi_s, phi_n = np.asarray(phi_s, dtype=np.float64), np.asarray(phi_n, dtype=np.float64)
    theta_s, theta_ns = dot(phi_s, theta), dot(phi_n, theta)
    diag = r - theta_s if term else r + gamma * theta_ns - theta_s
    mu = mu + r * phi_s
    pd = phi_s if term else (-gamma * phi_n) + phi_s
    delta_a = np.outer(phi_s, pd)
    A = A + delta_a
    mu = mu - (matvec(delta_a, theta) if literal else phi_s * dot(pd, theta))
    theta, mu = ilstd_solve(theta, A, mu, alpha, n_updates, rounds)
    return diag, theta, A, mu


def near_tie_band(mu, margin=1e-9):
    """some pair |mu_i|, |mu_j| (or |mu_j| against the running max) lies within margin of the 1e-7 tie band: a rounding may move a j in or out of
    argmaxima's set"""
    x = np.abs(np.asarray(mu, dtype=np.float64))
    d = np.abs(x[:, None] - x[None, :])
    return bool(np.any(np.abs(d - 1e-7) < margin))


def replay_trait_loop(orc, rlstd, domain, order, F, transitions, gamma, alpha, n_updates, init=None):
    """one learner's recorded transitions [(s, s', r, terminal)] through the rule from the agents' initial state (or init = (theta, matrix, mu))
    -> (theta, matrix, mu)"""
    theta, mat = np.zeros(F), (1e-5 if rlstd else 1.0) * np.eye(F)
    mu = np.zeros(F)
    if init is not None:
        theta, mat = np.array(init[0], dtype=np.float64), np.array(init[1], dtype=np.float64)
        mu = mu if init[2] is None else np.array(init[2], dtype=np.float64)
    for s, ns, r, term in transitions:
        phi_s, phi_n = orc.fourier_project(domain, order, s), orc.fourier_project(domain, order, ns)
        if rlstd:
            _, theta, mat = recursive_lstd(theta, mat, phi_s, phi_n, float(r), bool(term), gamma)
        else:
            _, theta, mat, mu = ilstd(theta, mat, mu, phi_s, phi_n, float(r), bool(term), gamma, alpha, n_updates, literal=False)
    return theta, mat, mu


def random_policy_actions(orc, seed, n_actions, N, t, block, env_offset=0):
    """what the Random policy samples for the learners env_offset .. env_offset + N - 1 from batch-step t's draw of `block`"""
    q = np.zeros(n_actions)
    return np.array([orc.policy_sample(orc.RANDOM, q, orc.draw(seed, env_offset + i, t, block)) for i in range(N)])
