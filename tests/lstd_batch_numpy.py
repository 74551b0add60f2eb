"""The batch least-squares agents restated literally (a plain helper module: no fixtures, no pytest settings): LSTD::handle (lstd.rs:59-81),
LSTDLambda::handle (lstd_lambda.rs:66-103) and the library's solve (kernels_lstd_batch.hpp).  Python floats and index-order loops: every product
and every sum is one rounded f64 operation in the order the device performs it.

A transition is (phi_s, phi_ns, reward, terminal); a state is a dict theta / A / b / z (lists of floats, z only for LSTDLambda) / singular."""
import numpy as np


def lu_solve(A, b):
    """A x = b by Gaussian elimination with partial pivoting on a copy -> x as a list of floats, or None when a column's pivot candidates hold no
    value above 0 (an exactly zero pivot; a column of NaN too).  The pivot of column k is the FIRST row in index order, among the rows not yet
    used, with the largest |a[i][k]|; rows are never moved.  Back substitution subtracts with ascending j."""
    F = len(b)
    a = [[float(A[i][j]) for j in range(F)] for i in range(F)]
    rhs = [float(b[i]) for i in range(F)]
    used = [False] * F
    piv = []
    for k in range(F):
        best, p = -1.0, 0
        for i in range(F):
            x = -1.0 if used[i] else abs(a[i][k])
            if x > best:
                best, p = x, i
        if not best > 0.0:
            return None
        used[p] = True
        piv.append(p)
        for i in range(F):
            if used[i]:
                continue
            m = a[i][k] / a[p][k]
            for j in range(k + 1, F):
                a[i][j] = a[i][j] - m * a[p][j]
            rhs[i] = rhs[i] - m * rhs[p]
    x = [0.0] * F
    for k in range(F - 1, -1, -1):
        p = piv[k]
        s = rhs[p]
        for j in range(k + 1, F):
            s = s - a[p][j] * x[j]
        x[k] = s / a[p][k]
    return x


def initial_state(F, lam=None):
    st = dict(theta=[0.0] * F, A=[[1e-6 if i == j else 0.0 for j in range(F)] for i in range(F)], b=[0.0] * F, singular=0)
    if lam is not None:
        st["z"] = [0.0] * F
    return st


def state_of(theta, A, b, z=None, singular=0):
    st = dict(theta=[float(v) for v in theta], A=[[float(v) for v in row] for row in A], b=[float(v) for v in b], singular=int(singular))
    if z is not None:
        st["z"] = [float(v) for v in z]
    return st


def accumulate_lstd(st, batch, gamma):
    """LSTD's walk, first to last, without the solve"""
    A, b = st["A"], st["b"]
    F = len(b)
    for phi_s, phi_ns, r, term in batch:
        ps, pn, r = [float(v) for v in phi_s], [float(v) for v in phi_ns], float(r)
        for i in range(F):
            b[i] = b[i] + r * ps[i]
        if term:
            for i in range(F):
                for j in range(F):
                    A[i][j] = A[i][j] + ps[i] * ps[j]
        else:
            pd = [gamma * pn[j] - ps[j] for j in range(F)]
            for i in range(F):
                for j in range(F):
                    A[i][j] = A[i][j] - ps[i] * pd[j]


def accumulate_lstd_lambda(st, batch, gamma, lam):
    """LSTDLambda's walk, LAST TO FIRST, without the solve; z survives the batch and only a terminal transition zeroes it"""
    A, b, z = st["A"], st["b"], st["z"]
    F = len(b)
    for phi_s, phi_ns, r, term in reversed(list(batch)):
        ps, pn, r = [float(v) for v in phi_s], [float(v) for v in phi_ns], float(r)
        c = lam * gamma
        for i in range(F):
            z[i] = c * z[i] + ps[i]
        for i in range(F):
            b[i] = b[i] + r * z[i]
        pd = ps if term else [ps[j] - gamma * pn[j] for j in range(F)]
        for i in range(F):
            for j in range(F):
                A[i][j] = A[i][j] + z[i] * pd[j]
        if term:
            for i in range(F):
                z[i] = 0.0


def solve(st):
    """solve(): theta <- lu_solve(A, b); an abandoned solve keeps theta and counts"""
    x = lu_solve(st["A"], st["b"])
    if x is None:
        st["singular"] += 1
    else:
        st["theta"] = x


def handle(st, batch, gamma, lam=None):
    """Handler<&Batch>::handle -> the diagnostic r + gamma V(s') - V(s) (terminal: r - V(s)) per transition, with theta as it stands before the solve"""
    theta = st["theta"]
    td = []
    for phi_s, phi_ns, r, term in batch:
        v_s = v_n = 0.0
        for j in range(len(theta)):
            v_s = v_s + float(phi_s[j]) * theta[j]
            v_n = v_n + float(phi_ns[j]) * theta[j]
        td.append(float(r) - v_s if term else float(r) + gamma * v_n - v_s)
    if lam is None:
        accumulate_lstd(st, batch, gamma)
    else:
        accumulate_lstd_lambda(st, batch, gamma, lam)
    solve(st)
    return td


def residual(A, b, x):
    """the normalised residual |A x - b|_inf / (|A|_inf |x|_inf + |b|_inf)"""
    A, b, x = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(x, dtype=np.float64)
    den = np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()
    return float(np.abs(A @ x - b).max() / den) if den > 0 else 0.0
