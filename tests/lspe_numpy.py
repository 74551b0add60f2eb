"""LambdaLSPE restated literally (a plain helper module: no fixtures, no pytest settings): LambdaLSPE::handle and ::solve (lambda_lspe.rs:47-107)
with the library's elimination (tests/lstd_batch_numpy.py lu_solve) and its row rule (include/rsrl_hip.h RSRL_LAMBDA_LSPE).  Python floats and
index-order loops: every product and every sum is one rounded f64 operation in the order the device performs it.

A transition is (phi_s, phi_ns, reward, terminal); a state is a dict theta / A / b (lists of floats) / delta (float) / rows (int in 0 .. F) /
singular."""
from tests.lstd_batch_numpy import lu_solve


def initial_state(F):
    return dict(theta=[0.0] * F, A=[[1e-6 if i == j else 0.0 for j in range(F)] for i in range(F)], b=[0.0] * F, delta=0.0, rows=F, singular=0)


def state_of(theta, A, b, delta=0.0, rows=0, singular=0):
    return dict(theta=[float(v) for v in theta], A=[[float(v) for v in row] for row in A], b=[float(v) for v in b], delta=float(delta),
                rows=int(rows), singular=int(singular))


def accumulate(st, batch, gamma, lam):
    """the walk, LAST TO FIRST, without the solve -> the diagnostic r + gamma V(s') - V(s) (terminal: r - V(s)) per transition in the batch's order;
    theta does not move, delta survives the batch and only a terminal transition zeroes it"""
    theta, A, b = st["theta"], st["A"], st["b"]
    F = len(b)
    td = [0.0] * len(batch)
    for k in range(len(batch) - 1, -1, -1):
        phi_s, phi_ns, r, term = batch[k]
        ps, pn, r = [float(v) for v in phi_s], [float(v) for v in phi_ns], float(r)
        v_s = v_n = 0.0
        for j in range(F):
            v_s = v_s + ps[j] * theta[j]
            v_n = v_n + pn[j] * theta[j]
        st["delta"] = st["delta"] * (gamma * lam)
        if term:
            td[k] = r - v_s
            coef = st["delta"] + r
        else:
            td[k] = r + gamma * v_n - v_s
            st["delta"] = st["delta"] + td[k]
            coef = v_s + st["delta"]
        for i in range(F):
            b[i] = b[i] + coef * ps[i]
        for i in range(F):
            for j in range(F):
                A[i][j] = A[i][j] + ps[i] * ps[j]
        if term:
            st["delta"] = 0.0
    st["rows"] = min(st["rows"] + len(batch), F)
    return td


def solve(st, alpha, solver=lu_solve):
    """solve() as handle ends with it -> "deferred" (fewer than F rows: nothing moves, nothing counts), "abandoned" (the elimination gave up:
    theta, A, b and delta stay, singular counts) or "solved" (the relaxed step; A, b, delta and rows zeroed)"""
    F = len(st["b"])
    if st["rows"] != F:
        return "deferred"
    x = solver(st["A"], st["b"])
    if x is None:
        st["singular"] += 1
        return "abandoned"
    keep = 1.0 - alpha
    st["theta"] = [keep * st["theta"][i] + alpha * x[i] for i in range(F)]
    st["A"] = [[0.0] * F for _ in range(F)]
    st["b"] = [0.0] * F
    st["delta"] = 0.0
    st["rows"] = 0
    return "solved"


def handle(st, batch, alpha, gamma, lam, solver=lu_solve):
    """Handler<&Batch>::handle -> (the diagnostics, what the solve did); an empty batch is no call"""
    if not len(batch):
        return [], "no call"
    td = accumulate(st, batch, gamma, lam)
    return td, solve(st, alpha, solver)
