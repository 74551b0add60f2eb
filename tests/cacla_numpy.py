"""CACLA over the Gaussian policy with a TD(0) critic (RSRL_CACLA = 33; control/cacla.rs:42-64, policies/gaussian/general.rs:196-212,
prediction/td/td.rs:38-58) restated in numpy.  Shared by the CPU and GPU tests, tests/fuzz_cacla.py and scripts/cacla_rate.py; Softplus, the domain
and Philox are tests/beta_numpy.py's, the policy's parameters, score and sample tests/gaussian_numpy.py's.

  handle        float64, one transition of one learner, in the loop's order: eval.handle (TD), then CACLA::handle whose critic reads the UPDATED w
                    td = r - <w, phi_s> (terminal) | r + gamma <w, phi_n> - <w, phi_s>;   w += lr td phi_s
                    v = <w, phi_s>;  target = r (terminal: r alone) | r + gamma <w, phi_n>;  gate = target > v (strict)
                    gate open:  e = (a - mu) alpha;  w_m += e g_mu phi_s;  w_s += e g_Sigma sigma(x_s) phi_s    (mu, sd, x_s at phi_s, read first)
  td_gate_f32   float32, the TD half and the gate in the DEVICE's operation order (kernels_cont.hpp, CaclaRule::step): tests/gtd_numpy.dot_f32's
                    dot products, k_train_td's expression for the error, one fused multiply-add per element; vectorised over learners
  handle_case   the GPU rule test's inputs: every transition's f64 |target - v| is at least MARGIN, so the device's f32 decision cannot differ
  after         `handle` over every round of a case from given features -> w, the columns, the gates, the TD errors

THE LITERAL RULE: the mean's step is e g_mu = alpha (a - mu)^2 / Sigma >= 0 on either side of the mean (mean_step): what the reference says, not
van Hasselt's mu += alpha (a - mu)."""
import numpy as np

from tests import beta_numpy as bn
from tests import gaussian_numpy as gn
from tests.gtd_numpy import dot_f32
from tests.nac_numpy import fma32

CACLA = 33
F32 = np.float32
MARGIN = 1e-3           # handle_case keeps |target - v| >= MARGIN in f64: seven orders above an f32 dot product's error at these magnitudes
OVERFLOW_LEARNER = 2    # handle_case: its gate is closed in every round and its c_s is not finite in f32 (a = 3e18, x_s = -50: sd = 0.01)
OVERFLOW_ACTION = 3e18


def mean_step(W, phi, a, alpha):
    """the coefficient of phi in the mean's move, e * c_m = alpha (a - mu)^2 / Sigma"""
    xm, xs = gn.prefs(W, phi)
    mu, sd = gn.gauss_params(xm, xs)
    cm, _ = gn.coefs(W, phi, a)
    return float((a - mu) * alpha * cm)


def handle(w, W, phi_s, phi_n, a, r, term, gamma, lr, alpha):
    """one transition -> (td, w', W', gate, target - v); w (F,), W (F, 2): column 0 the mean's, column 1 the stddev's"""
    w, W = np.asarray(w, dtype=np.float64).ravel(), np.asarray(W, dtype=np.float64)
    phi_s, phi_n = np.asarray(phi_s, dtype=np.float64), np.asarray(phi_n, dtype=np.float64)
    td = r - w @ phi_s if term else r + gamma * (w @ phi_n) - w @ phi_s
    w2 = w + lr * td * phi_s
    v = w2 @ phi_s
    target = r if term else r + gamma * (w2 @ phi_n)
    gate = bool(target > v)
    W2 = W.copy()
    if gate:
        xm, xs = gn.prefs(W, phi_s)
        mu, _ = gn.gauss_params(xm, xs)
        e = (a - mu) * alpha
        cm, cs = gn.coefs(W, phi_s, a)
        W2[:, 0] += e * cm * phi_s
        W2[:, 1] += e * cs * phi_s
    return float(td), w2, W2, gate, float(target - v)


def td_gate_f32(w, phi_s, phi_n, r, term, gamma, lr):
    """w, phi_s, phi_n (N, F) float32; r (N,); term (N,) bool -> (td, w', v, target, gate), float32 in the device's order"""
    w, phi_s, phi_n = (np.asarray(x, dtype=F32) for x in (w, phi_s, phi_n))
    r, term = np.asarray(r, dtype=F32), np.asarray(term, dtype=bool)
    gamma, lr = F32(gamma), F32(lr)
    v_s, v_n = dot_f32(w, phi_s), dot_f32(w, phi_n)
    td = np.where(term, (r - v_s).astype(F32), ((r + (gamma * v_n).astype(F32)).astype(F32) - v_s).astype(F32)).astype(F32)
    w2 = fma32((lr * td).astype(F32)[:, None], phi_s, w)
    v, v_n2 = dot_f32(w2, phi_s), dot_f32(w2, phi_n)
    target = np.where(term, r, (r + (gamma * v_n2).astype(F32)).astype(F32)).astype(F32)
    return td, w2, v, target, target > v


def handle_case(order, project, N=67, rounds=3, gamma=0.95, lr=0.01, alpha=0.01):
    """the GPU rule test's inputs.  project(S (2, M)) -> features (F, M) (the oracle's on the CPU, the device's own f32 projection on the GPU).
    Per learner: the policy's columns as tests/gaussian_numpy.handle_case builds them (|x_m| <= 1, x_s in [-1, 3], sd > 0.32) and a random V
    learner w with sum |w| <= 3.  `rounds` rounds of transitions from random states and random actions in [-1.5, 1.5], s' stepped by cmc_step,
    a quarter more of them flagged terminal.  handle takes any reward, so r is CHOSEN: r = f32(V(s) - [gamma V(s')] + u) with u uniform in
    +-[0.05, 0.5] and w as the rounds before left it (f64, TD alone moves it) -- TD's error is then about u, and the margin target - v after the
    update about u (1 - lr (|phi_s|^2 - gamma <phi_s, phi_n>)), of u's sign: both gate outcomes occur, about half each.  A transition whose f64
    margin is below MARGIN is drawn again.  Learner OVERFLOW_LEARNER: u < 0 in every round (closed), its stddev column -50 on the constant
    feature alone and its action 3e18, so c_s overflows f32.
    -> dict(init=[(w (F,), W (F, 2)) f32 per learner], rounds=[(from, a, r, to, term)], margins=[(N,) f64 per round], F, params)"""
    rng = np.random.default_rng(700 + order * 10 + CACLA)
    lo, hi = np.array([bn.X_BOUNDS[0], bn.V_BOUNDS[0]]), np.array([bn.X_BOUNDS[1], bn.V_BOUNDS[1]])
    F = (order + 1) ** 2
    init = []
    for i in range(N):
        W = rng.normal(0.0, 1.0, size=(F, 2))
        W *= rng.uniform(0.2, 1.0, size=2) * np.array([1.0, 2.0]) / np.abs(W).sum(axis=0)
        W[F - 1, 1] += 1.0
        if i == OVERFLOW_LEARNER:
            W[:, 1] = 0.0
            W[F - 1, 1] = -50.0
        w = rng.normal(0.0, 1.0, size=F)
        w *= rng.uniform(0.5, 3.0) / np.abs(w).sum()
        init.append((w.astype(F32), W.astype(F32)))
    w64 = [w.astype(np.float64) for w, _ in init]
    out, margins = [], []
    for _ in range(rounds):
        frm, nxt = np.zeros((2, N), dtype=F32), np.zeros((2, N), dtype=F32)
        a, rew, term, marg = np.zeros(N, dtype=F32), np.zeros(N, dtype=F32), np.zeros(N, dtype=np.uint8), np.zeros(N)
        todo = list(range(N))
        while todo:
            S = rng.uniform(lo, hi, size=(len(todo), 2)).T.astype(F32)
            act = rng.uniform(-1.5, 1.5, size=len(todo)).astype(F32)
            flag = rng.random(len(todo)) < 0.25
            u = rng.uniform(0.05, 0.5, size=len(todo)) * np.where(rng.random(len(todo)) < 0.5, -1.0, 1.0)
            S2, T = np.zeros_like(S), np.zeros(len(todo), dtype=bool)
            for j in range(len(todo)):
                ns, _, t = bn.cmc_step(S[:, j], float(act[j]))
                S2[:, j], T[j] = np.asarray(ns, dtype=F32), bool(t) or bool(flag[j])
            ps, pn = np.asarray(project(S), dtype=np.float64), np.asarray(project(S2), dtype=np.float64)
            again = []
            for j, i in enumerate(todo):
                if i == OVERFLOW_LEARNER:
                    u[j], act[j] = -abs(u[j]), F32(OVERFLOW_ACTION)
                base = w64[i] @ ps[:, j] - (0.0 if T[j] else gamma * (w64[i] @ pn[:, j]))
                r = F32(base + u[j])
                _, w2, _, _, m = handle(w64[i], np.zeros((F, 2)), ps[:, j], pn[:, j], 0.0, float(r), bool(T[j]), gamma, lr, alpha)
                if abs(m) < MARGIN:
                    again.append(i)
                    continue
                frm[:, i], nxt[:, i], a[i], rew[i], term[i], marg[i] = S[:, j], S2[:, j], act[j], r, T[j], m
                w64[i] = w2
            todo = again
        out.append((frm, a, rew, nxt, term))
        margins.append(marg)
    return dict(init=init, rounds=out, margins=margins, F=F, params=dict(gamma=gamma, lr=lr, alpha=alpha))


def after(case, phi_s_rounds, phi_n_rounds):
    """`handle` over every round of `case` in f64 from the features given (phi_*_rounds[k]: (F, N)) -> (w (N, F), columns (N, F, 2) after the last
    round, [gate (N,) bool per round], [td (N,) per round], [target - v (N,) per round])"""
    p = case["params"]
    N = len(case["init"])
    w = [x.astype(np.float64) for x, _ in case["init"]]
    Ws = [W.astype(np.float64) for _, W in case["init"]]
    gates, tds, margins = [], [], []
    for k, (frm, a, rew, nxt, term) in enumerate(case["rounds"]):
        ps, pn = np.asarray(phi_s_rounds[k], dtype=np.float64), np.asarray(phi_n_rounds[k], dtype=np.float64)
        g, d, m = np.zeros(N, dtype=bool), np.zeros(N), np.zeros(N)
        for i in range(N):
            d[i], w[i], Ws[i], g[i], m[i] = handle(w[i], Ws[i], ps[:, i], pn[:, i], float(a[i]), float(rew[i]), bool(term[i]), p["gamma"], p["lr"], p["alpha"])
        gates.append(g)
        tds.append(d)
        margins.append(m)
    return np.stack(w), np.stack(Ws), gates, tds, margins


def figures(c, td_ctx, case):
    """the device on `case`: c a fresh RSRL_CACLA Context of the case's order and parameters, td_ctx an RSRL_TD Context on RSRL_MOUNTAIN_CAR of the
    same order, lr and gamma (or None).  Both are fed every round.  -> dict(cols: max |d column| / max(1, |column|) over the learners whose gate
    opened in some round, against `after` on the device's own projection), and the arrays behind it"""
    N = len(case["init"])
    for i, (w, W) in enumerate(case["init"]):
        c.set_weights(w.reshape(-1, 1), i)
        c.set_policy_weights(W, i)
        if td_ctx is not None:
            td_ctx.set_weights(w.reshape(-1, 1), i)
    phi_s, phi_n, td, td_ref, cols, ws, ws_ref = [], [], [], [], [], [], []
    for frm, a, rew, nxt, term in case["rounds"]:
        phi_s.append(c.project(frm))
        phi_n.append(c.project(nxt))
        td.append(c.handle(frm, a, rew, nxt, term))
        cols.append(np.stack([c.get_policy_weights(i) for i in range(N)]))
        ws.append(np.stack([c.get_weights(i) for i in range(N)]))
        if td_ctx is not None:
            td_ref.append(td_ctx.handle(frm, np.zeros(N, dtype=np.int32), rew, nxt, term))
            ws_ref.append(np.stack([td_ctx.get_weights(i) for i in range(N)]))
    want_w, want_cols, gates, tds, margins = after(case, phi_s, phi_n)
    opened = np.any(np.stack(gates), axis=0)
    got = cols[-1].astype(np.float64)
    rel = np.abs(got - want_cols) / np.maximum(1.0, np.abs(want_cols))
    fig = dict(cols=float(rel[opened].max()))
    return fig, dict(td=td, td_ref=td_ref, cols=cols, ws=ws, ws_ref=ws_ref, gates=gates, tds=tds, margins=margins, want_w=want_w, want_cols=want_cols,
                     opened=opened, phi_s=phi_s, phi_n=phi_n)
