"""ActorCritic::tdac with a TD(0) critic over the Gaussian or the Beta policy (RSRL_CONTINUOUS_TD_ACTOR_CRITIC = 35; control/ac.rs:32-52, :87-115,
prediction/td/td.rs:38-58, policies/gaussian/general.rs:196-212, policies/beta.rs) restated in f64 numpy.  Shared by the CPU and GPU tests,
tests/fuzz_tdac_cont.py and scripts/tdac_cont_rate.py; Softplus, the domain, the Beta score and Philox are tests/beta_numpy.py's, the Gaussian's
parameters, score and sample tests/gaussian_numpy.py's, the device-order TD half tests/cacla_numpy.td_gate_f32's.

  handle        float64, one transition of one learner, in the loop's order: eval.handle (TD), then ActorCritic::handle whose critic reads the UPDATED w
                    td = r - <w, phi_s> (terminal) | r + gamma <w, phi_n> - <w, phi_s>;   w += lr td phi_s
                    nv = <w, phi_n>;  c = r - nv (terminal: V of the terminal state itself) | r + gamma nv - <w, phi_s>;  e = f32(alpha) c
                    policy.handle(s, a, e), always:  GAUSSIAN  w_m += e g_mu phi_s;  w_s += e g_Sigma sigma(x_s) phi_s
                                                     BETA      tests/beta_numpy.beta_step (the action clamped, one shared psi(alpha + beta))
                    (the preferences at phi_s are read before either column moves)
  handle_case   the GPU rule test's inputs, chosen so that every learner stays in the comparison
  after         `handle` over every round of a case from given features -> w, the columns, the critic's c and the TD errors per round
  figures       the device on a case -> max |d column| / max(1, |column|) over ALL learners, and the arrays behind it"""
import numpy as np

from tests import beta_numpy as bn
from tests import gaussian_numpy as gn

TDAC_CONT = 35
GAUSSIAN, BETA = 6, 4
F32 = np.float32
XS_MIN = -3.0           # handle_case, GAUSSIAN: the stddev's preference at every transition's state: sd >= softplus(-3) + 0.01 > 0.058
A_LO, A_HI = 0.02, 0.98      # handle_case, BETA: the actions' interval
C_MIN = 0.02            # handle_case: |c| of every transition in f64, so both signs of c are signs and not roundings


def critic(w, phi_s, phi_n, r, term, gamma, lr):
    """TD::handle then TDCritic::target with the updated w -> (td, w', c)"""
    w = np.asarray(w, dtype=np.float64).ravel()
    phi_s, phi_n = np.asarray(phi_s, dtype=np.float64), np.asarray(phi_n, dtype=np.float64)
    td = r - w @ phi_s if term else r + gamma * (w @ phi_n) - w @ phi_s
    w2 = w + lr * td * phi_s
    nv = w2 @ phi_n
    c = r - nv if term else r + gamma * nv - w2 @ phi_s
    return float(td), w2, float(c)


def policy_step(policy, W, phi, a, e):
    """policy.handle(StateActionUpdate{s, a, error: e}): W (F, 2) f64 -> W'"""
    W, phi = np.asarray(W, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    if policy == BETA:
        return bn.beta_step(W, phi, a, e)
    cm, cs = gn.coefs(W, phi, a)
    out = W.copy()
    out[:, 0] += e * cm * phi
    out[:, 1] += e * cs * phi
    return out


def handle(policy, w, W, phi_s, phi_n, a, r, term, gamma, lr, alpha):
    """one transition -> (td, w', W', c); w (F,), W (F, 2)"""
    td, w2, c = critic(w, phi_s, phi_n, r, term, gamma, lr)
    e = float(F32(alpha)) * c
    return td, w2, policy_step(policy, W, phi_s, a, e), c


def handle_case(order, project, policy, N=67, rounds=3, gamma=0.95, lr=0.01, alpha=0.01):
    """the GPU rule test's inputs.  project(S (2, M)) -> features (F, M) (the oracle's on the CPU, the device's own f32 projection on the GPU).
    Per learner a random V learner w with sum |w| <= 3 and policy columns that are a target preference on the constant feature (the last one)
    plus a random part with sum |w| <= 0.4, so the preference at any state is within 0.4 of its target:
      GAUSSIAN  x_m's target uniform in [-1, 1]; x_s's uniform in [-2.5, 8], every eighth learner's in [10.5, 12] (Softplus's linear branch)
      BETA      x_a's and x_b's targets uniform in [-8, 8], every eighth learner's x_a and every eighth's x_b in [10.5, 12]
    `rounds` rounds of transitions from random states, s' stepped by cmc_step, a quarter more of them flagged terminal.  The f64 state (w and
    the columns) is carried through the rounds, so every round's choices are made at the learner's current parameters:
      the action   GAUSSIAN  mu + sd z with |z| uniform in [0.3, 2] and a random sign: on both sides of the mean, |g_mu| <= 2 / sd
                   BETA      uniform in [A_LO, A_HI]; the domain would see 2a - 1, which is what s' is stepped with
      the reward   handle takes any reward, so r is CHOSEN: r = f32(V(s) - [gamma V(s')] + u), u uniform in +-[0.05, 0.5] -- TD's error is about
                   u and the critic's c about u (1 - lr (|phi_s|^2 - gamma <phi_s, phi_n>)), of u's sign: both signs occur, about half each
    A transition is drawn again if |c| < C_MIN, if (GAUSSIAN) x_s at its state is below XS_MIN, or if anything the rule computes from it is not
    finite: no learner is left out of any comparison.
    -> dict(init=[(w (F,), W (F, 2)) f32 per learner], rounds=[(from, a, r, to, term)], F, policy, params)"""
    rng = np.random.default_rng(900 + order * 10 + policy)
    lo, hi = np.array([bn.X_BOUNDS[0], bn.V_BOUNDS[0]]), np.array([bn.X_BOUNDS[1], bn.V_BOUNDS[1]])
    F = (order + 1) ** 2
    init = []
    for i in range(N):
        W = rng.normal(0.0, 1.0, size=(F, 2))
        W[F - 1] = 0.0
        W *= rng.uniform(0.1, 0.4, size=2) / np.abs(W).sum(axis=0)
        if policy == GAUSSIAN:
            W[F - 1] = [rng.uniform(-1.0, 1.0), rng.uniform(10.5, 12.0) if i % 8 == 5 else rng.uniform(-2.5, 8.0)]
        else:
            W[F - 1] = [rng.uniform(10.5, 12.0) if i % 8 == 5 else rng.uniform(-8.0, 8.0), rng.uniform(10.5, 12.0) if i % 8 == 2 else rng.uniform(-8.0, 8.0)]
        w = rng.normal(0.0, 1.0, size=F)
        w *= rng.uniform(0.5, 3.0) / np.abs(w).sum()
        init.append((w.astype(F32), W.astype(F32)))
    w64 = [w.astype(np.float64) for w, _ in init]
    W64 = [W.astype(np.float64) for _, W in init]
    out = []
    for _ in range(rounds):
        frm, nxt = np.zeros((2, N), dtype=F32), np.zeros((2, N), dtype=F32)
        a, rew, term = np.zeros(N, dtype=F32), np.zeros(N, dtype=F32), np.zeros(N, dtype=np.uint8)
        todo = list(range(N))
        while todo:
            S = rng.uniform(lo, hi, size=(len(todo), 2)).T.astype(F32)
            ps = np.asarray(project(S), dtype=np.float64)
            z = rng.uniform(0.3, 2.0, size=len(todo)) * np.where(rng.random(len(todo)) < 0.5, -1.0, 1.0)
            ua = rng.uniform(A_LO, A_HI, size=len(todo))
            flag = rng.random(len(todo)) < 0.25
            u = rng.uniform(0.05, 0.5, size=len(todo)) * np.where(rng.random(len(todo)) < 0.5, -1.0, 1.0)
            act, S2, T = np.zeros(len(todo), dtype=F32), np.zeros_like(S), np.zeros(len(todo), dtype=bool)
            for j, i in enumerate(todo):
                if policy == GAUSSIAN:
                    mu, sd = gn.gauss_params(*gn.prefs(W64[i], ps[:, j]))
                    act[j] = F32(mu + sd * z[j])
                    ns, _, t = bn.cmc_step(S[:, j], float(act[j]))
                else:
                    act[j] = F32(np.clip(ua[j], A_LO, A_HI))
                    ns, _, t = bn.cmc_step(S[:, j], 2.0 * float(act[j]) - 1.0)
                S2[:, j], T[j] = np.asarray(ns, dtype=F32), bool(t) or bool(flag[j])
            pn = np.asarray(project(S2), dtype=np.float64)
            again = []
            for j, i in enumerate(todo):
                base = w64[i] @ ps[:, j] - (0.0 if T[j] else gamma * (w64[i] @ pn[:, j]))
                r = F32(base + u[j])
                _, w2, W2, c = handle(policy, w64[i], W64[i], ps[:, j], pn[:, j], float(act[j]), float(r), bool(T[j]), gamma, lr, alpha)
                ok = abs(c) >= C_MIN and np.isfinite(W2).all() and np.isfinite(w2).all() and np.isfinite(act[j])
                if policy == GAUSSIAN:
                    ok = ok and gn.prefs(W64[i], ps[:, j])[1] >= XS_MIN + 0.01
                else:
                    ok = ok and A_LO <= act[j] <= A_HI
                if not ok:
                    again.append(i)
                    continue
                frm[:, i], nxt[:, i], a[i], rew[i], term[i] = S[:, j], S2[:, j], act[j], r, T[j]
                w64[i], W64[i] = w2, W2
            todo = again
        out.append((frm, a, rew, nxt, term))
    return dict(init=init, rounds=out, F=F, policy=policy, params=dict(gamma=gamma, lr=lr, alpha=alpha))


def after(case, phi_s_rounds, phi_n_rounds):
    """`handle` over every round of `case` in f64 from the features given (phi_*_rounds[k]: (F, N)) -> (w (N, F), columns (N, F, 2) after the last
    round, [c (N,) per round], [td (N,) per round], [(x0, x1) (N, 2) per round: the preferences at s before the round's move])"""
    p = case["params"]
    N = len(case["init"])
    w = [x.astype(np.float64) for x, _ in case["init"]]
    Ws = [W.astype(np.float64) for _, W in case["init"]]
    cs, tds, xs = [], [], []
    for k, (frm, a, rew, nxt, term) in enumerate(case["rounds"]):
        ps, pn = np.asarray(phi_s_rounds[k], dtype=np.float64), np.asarray(phi_n_rounds[k], dtype=np.float64)
        c, d, x = np.zeros(N), np.zeros(N), np.zeros((N, 2))
        for i in range(N):
            x[i] = gn.prefs(Ws[i], ps[:, i])
            d[i], w[i], Ws[i], c[i] = handle(case["policy"], w[i], Ws[i], ps[:, i], pn[:, i], float(a[i]), float(rew[i]), bool(term[i]), p["gamma"], p["lr"],
                                             p["alpha"])
        cs.append(c)
        tds.append(d)
        xs.append(x)
    return np.stack(w), np.stack(Ws), cs, tds, xs


def keeps_every_learner_in(case, cs, xs, want_w, want_cols):
    """the conditions handle_case promises, on what `after` made of the case: a list of the ones that do not hold (empty: all hold)"""
    bad = []
    N = len(case["init"])
    allx = np.concatenate(xs)
    if not (np.isfinite(want_w).all() and np.isfinite(want_cols).all()):
        bad.append("a result is not finite")
    for k, (frm, a, rew, nxt, term) in enumerate(case["rounds"]):
        if not np.all(np.abs(cs[k]) >= C_MIN / 2):
            bad.append(f"round {k}: |c| below C_MIN / 2")
        if not ((cs[k] > 0).sum() >= N / 4 and (cs[k] < 0).sum() >= N / 4):
            bad.append(f"round {k}: one sign of c is rare")
        if not (term.sum() >= 4 and (term == 0).sum() >= N / 2):
            bad.append(f"round {k}: terminal / non-terminal rows")
        if case["policy"] == GAUSSIAN:
            if not np.all(xs[k][:, 1] >= XS_MIN):
                bad.append(f"round {k}: x_s below XS_MIN")
            side = a.astype(np.float64) > xs[k][:, 0]
            if not (side.sum() >= N / 4 and (~side).sum() >= N / 4):
                bad.append(f"round {k}: the actions lie on one side of the mean")
        elif not np.all((a >= F32(A_LO)) & (a <= F32(A_HI))):
            bad.append(f"round {k}: an action outside [A_LO, A_HI]")
    cols = allx[:, 1:] if case["policy"] == GAUSSIAN else allx
    if not ((cols >= 10.0).sum() >= 3 and (np.abs(cols) < 10.0).sum() >= N and cols.min() < -1.0 and ((cols > 5.0) & (cols < 10.0)).any()):
        bad.append("the preferences do not reach both Softplus branches")
    return bad


def figures(c, td_ctx, case):
    """the device on `case`: c a fresh RSRL_CONTINUOUS_TD_ACTOR_CRITIC Context of the case's order, policy and parameters, td_ctx an RSRL_TD Context
    on RSRL_MOUNTAIN_CAR of the same order, lr and gamma (or None).  Both are fed every round.  -> dict(cols: max |d column| / max(1, |column|) over
    all learners after the last round, against `after` on the device's own projection), and the arrays behind it"""
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
    want_w, want_cols, cs, tds, xs = after(case, phi_s, phi_n)
    rel = np.abs(cols[-1].astype(np.float64) - want_cols) / np.maximum(1.0, np.abs(want_cols))
    fig = dict(cols=float(rel.max()))
    return fig, dict(td=td, td_ref=td_ref, cols=cols, ws=ws, ws_ref=ws_ref, cs=cs, tds=tds, xs=xs, want_w=want_w, want_cols=want_cols, phi_s=phi_s, phi_n=phi_n)
