"""The Gaussian policy (RSRL_GAUSSIAN, policies/gaussian/{mod,general}.rs) and NAC over it (RSRL_NAC on RSRL_CONTINUOUS_MOUNTAIN_CAR, examples/nac.rs)
restated in f64 numpy.  Shared by the CPU and GPU tests and by scripts/nac_gaussian_rate.py; Softplus, the domain and Philox are tests/beta_numpy.py's,
NAC::handle(()) -- which does not read the policy -- tests/nac_numpy.py's (nac_handle, nac_handle_f32).

  params         mu = x_m, sd = softplus(x_s) + 0.01 (MIN_TOL, mod.rs:37, :67); Sigma = sd * sd (into_cov: the builder takes the variance, mod.rs:82)
  pdf            exp(-(a - mu)^2 / (2 Sigma)) / sqrt(2 pi Sigma)
  score          g_mu = (a - mu) / Sigma, g_Sigma = ((a - mu)^2 - Sigma) / (2 Sigma^2): the library's definition (rstat is not in the reference tree)
  coefs          grad_log's two coefficients of phi (general.rs:142-157): (g_mu, g_Sigma sigma(x_s)), literally -- no factor d Sigma / d sd
  psi, Q, sarsa_handle   tests/nac_numpy.py's forms over these coefficients
  normal, sample a = mu + sd z, z = sqrt(-2 ln u1) cos(2 pi u2) from the Philox block at block word purpose + 256, words x and y converted as
                 beta_numpy.beta_sample converts them"""
import numpy as np

from tests import beta_numpy as bn

MIN_TOL = 0.01
BLK_INNER = 2
RULE_SEED = 23          # the ctx seed of the GPU rule test (any: the sampler has no acceptance test, so no learner is ever left out)
Z_MAX = float(np.sqrt(48.0 * np.log(2.0)))      # |z| <= sqrt(-2 ln 2^-24) = 5.768...


def gauss_params(xm, xs):
    """(mu, sd)"""
    return np.asarray(xm, dtype=np.float64), bn.softplus(xs) + MIN_TOL


def gauss_pdf(mu, sd, a):
    var = np.asarray(sd, dtype=np.float64) ** 2
    d = np.asarray(a, dtype=np.float64) - mu
    return np.exp(-d * d / (2.0 * var)) / np.sqrt(2.0 * np.pi * var)


def gauss_logpdf(mu, var, a):
    """the log density in the builder's arguments, the mean and the VARIANCE (what the score differentiates)"""
    return -0.5 * np.log(2.0 * np.pi * var) - (a - mu) ** 2 / (2.0 * var)


def gauss_score(mu, sd, a):
    """(g_mu, g_Sigma)"""
    var = np.asarray(sd, dtype=np.float64) ** 2
    d = np.asarray(a, dtype=np.float64) - mu
    return d / var, (d * d - var) / (2.0 * var * var)


def prefs(W, phi):
    W, phi = np.asarray(W, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    return float(phi @ W[:, 0]), float(phi @ W[:, 1])


def coefs(W, phi, a):
    """(c_m, c_s) at the features phi and the action a, W (F, 2) the policy's columns (the mean's, the stddev's)"""
    xm, xs = prefs(W, phi)
    mu, sd = gauss_params(xm, xs)
    gm, gv = gauss_score(mu, sd, a)
    return float(gm), float(gv * bn.softplus_grad(xs))


def psi(W, phi, a):
    cm, cs = coefs(W, phi, a)
    phi = np.asarray(phi, dtype=np.float64)
    return np.concatenate([cm * phi, cs * phi, phi])


def q_value(w, W, phi, a):
    return float(np.asarray(w, dtype=np.float64).ravel() @ psi(W, phi, a))


def sarsa_handle(w, W, phi_s, a, r, phi_n, na, term, gamma, lr):
    """one transition -> (delta, w'); na: the critic's own draw at s' (not read on a terminal transition)"""
    w = np.asarray(w, dtype=np.float64).ravel()
    q = q_value(w, W, phi_s, a)
    delta = r - q if term else r + gamma * q_value(w, W, phi_n, na) - q
    return delta, w + lr * delta * psi(W, phi_s, a)


def gauss_normal_parts(seed, gid, t, purpose):
    """(z, rad) of (seed, global learner id, t, purpose), gid an array: Box-Muller's cosine normal on the whole block at block word purpose + 256,
    and its radius sqrt(-2 ln u1) beside it (the sample's condition number needs it: tests/continuous_edges.py)"""
    w = bn.philox_block(seed, np.asarray(gid), t, purpose + 256).astype(np.float64)
    u1, u2 = (np.floor(w[..., 0] / 256.0) + 1.0) / 16777216.0, np.floor(w[..., 1] / 256.0) / 16777216.0
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(float(np.float32(6.2831854820251465)) * u2), rad


def gauss_normal(seed, gid, t, purpose):
    """z of (seed, global learner id, t, purpose)"""
    return gauss_normal_parts(seed, gid, t, purpose)[0]


def gauss_sample(seed, gid, t, purpose, mu, sd):
    return mu + sd * gauss_normal(seed, gid, t, purpose)


def handle_case(order, N=67, rounds=3, gamma=0.95, lr=0.01):
    """the GPU rule test's inputs, built as tests/nac_numpy.handle_case builds its own.  Per learner: the mean's column with sum |w| <= 1, so
    |x_m| <= 1 (|phi| <= 1); the stddev's column 1 on the constant feature (the last one) plus a random part with sum |w| <= 2, so x_s lies in
    [-1, 3] and sd >= softplus(-1) + 0.01 > 0.32 -- (a - mu)^2 - Sigma stays well conditioned; a random critic w with sum |w| <= 3.  `rounds`
    rounds of transitions stepped by cmc_step (which clips) from random states and random actions in [-1.5, 1.5] -- learners 0 and 1 act -1 and 1
    exactly -- a quarter more of them flagged terminal"""
    rng = np.random.default_rng(600 + order * 10 + 28)
    lo, hi = np.array([bn.X_BOUNDS[0], bn.V_BOUNDS[0]]), np.array([bn.X_BOUNDS[1], bn.V_BOUNDS[1]])
    F = (order + 1) ** 2
    init = []
    for _ in range(N):
        W = rng.normal(0.0, 1.0, size=(F, 2))
        W *= rng.uniform(0.2, 1.0, size=2) * np.array([1.0, 2.0]) / np.abs(W).sum(axis=0)
        W[F - 1, 1] += 1.0
        w = rng.normal(0.0, 1.0, size=3 * F)
        w *= rng.uniform(0.5, 3.0) / np.abs(w).sum()
        init.append((w.astype(np.float32), W.astype(np.float32)))
    out = []
    for _ in range(rounds):
        frm = rng.uniform(lo, hi, size=(N, 2)).T.astype(np.float32)
        a = rng.uniform(-1.5, 1.5, size=N).astype(np.float32)
        a[0], a[1] = -1.0, 1.0
        nxt, rew, term = np.zeros_like(frm), np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.uint8)
        for i in range(N):
            ns, r, t = bn.cmc_step(frm[:, i], float(a[i]))
            nxt[:, i], rew[i], term[i] = np.asarray(ns, dtype=np.float32), np.float32(r), bool(t)
        term = (term.astype(bool) | (rng.random(N) < 0.25)).astype(np.uint8)
        out.append((frm, a, rew, nxt, term))
    return dict(init=init, rounds=out, F=F, params=dict(gamma=gamma, lr=lr))


def critic_after(case, seed, phi_s_rounds, phi_n_rounds, env_offset=0):
    """SARSA::handle over every round of `case` in f64, from the features given (phi_*_rounds[k]: (F, N), the `from` and `to` states' of round k -- the
    device's own f32 projection in the GPU test).  The inner draw of learner i at round k is gauss_sample(seed, env_offset + i, k, BLK_INNER, ...) at
    the f64 parameters.  -> (w (N, 3F) after the last round, [delta (N,) per round]): every learner, none left out"""
    p = case["params"]
    N = len(case["init"])
    w = [x.astype(np.float64) for x, _ in case["init"]]
    Ws = [W.astype(np.float64) for _, W in case["init"]]
    deltas = []
    for k, (frm, a, rew, nxt, term) in enumerate(case["rounds"]):
        ps, pn = phi_s_rounds[k].astype(np.float64), phi_n_rounds[k].astype(np.float64)
        xm = np.array([pn[:, i] @ Ws[i][:, 0] for i in range(N)])
        xs = np.array([pn[:, i] @ Ws[i][:, 1] for i in range(N)])
        mu, sd = gauss_params(xm, xs)
        na = gauss_sample(seed, env_offset + np.arange(N), k, BLK_INNER, mu, sd)
        d = np.zeros(N)
        for i in range(N):
            d[i], w[i] = sarsa_handle(w[i], Ws[i], ps[:, i], float(a[i]), float(rew[i]), pn[:, i], float(na[i]), bool(term[i]), p["gamma"], p["lr"])
        deltas.append(d)
    return np.stack(w), deltas


SAMPLE_CALLS = 64       # policy_sample(states) calls of figures(): BLK_API's t = 0 .. 63, 67 x 64 = 4 288 draws


def figures(c, case, seed):
    """the device against this restatement on `case`, from the same f32 inputs: the figures scripts/nac_gaussian_rate.py records and
    tests/test_gpu_nac_gaussian.py bounds.  c: a fresh Context of the case's order and parameters created with `seed` (step_count 0, no
    policy_sample(states) call yet: the SAMPLE_CALLS ones below are BLK_API's t = 0, 1, ...).  -> (name -> max |d x| / max(1, |x|), the arrays
    behind them): mu, sd, pdf and sample on the first round's states; q there too, actions outside [-1, 1] included; delta and w over the rounds of
    handle"""
    N = len(case["init"])
    rel = lambda got, want: float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(1.0, np.abs(want))))      # noqa: E731
    for i, (w, W) in enumerate(case["init"]):
        c.set_weights(w.reshape(-1, 1), i)
        c.set_policy_weights(W, i)
    frm, a, _, _, _ = case["rounds"][0]
    phi = c.project(frm).astype(np.float64)
    out = {}
    # ---- the policy side
    Ws = [W.astype(np.float64) for _, W in case["init"]]
    xm, xs = np.array([phi[:, i] @ Ws[i][:, 0] for i in range(N)]), np.array([phi[:, i] @ Ws[i][:, 1] for i in range(N)])
    mu, sd = gauss_params(xm, xs)
    dmu, dsd = c.policy_params(frm)
    out["mu"], out["sd"] = rel(dmu, mu), rel(dsd, sd)
    out["pdf"] = rel(c.policy_pdf(frm, a), gauss_pdf(mu, sd, a.astype(np.float64)))
    smp = np.stack([c.policy_sample(frm) for _ in range(SAMPLE_CALLS)])
    out["sample"] = rel(smp, np.stack([gauss_sample(seed, np.arange(N), t, bn.BLK_API, mu, sd) for t in range(SAMPLE_CALLS)]))
    # ---- Q
    aq = a.copy()
    aq[2], aq[3], aq[4] = -2.5, 1.5, 0.5
    q = c.q_evaluate_f32(frm, aq)
    out["q"] = rel(q, np.array([q_value(w, W, phi[:, i], float(aq[i])) for i, (w, W) in enumerate(case["init"])]))
    # ---- the critic's rule (handle advances step_count: last)
    phi_s, phi_n, td = [], [], []
    for f, act, rew, nxt, term in case["rounds"]:
        phi_s.append(c.project(f))
        phi_n.append(c.project(nxt))
        td.append(c.handle(f, act, rew, nxt, term))
    want, deltas = critic_after(case, seed, phi_s, phi_n)
    got = np.stack([c.get_weights(i)[:, 0] for i in range(N)])
    out["delta"] = max(rel(t, d) for t, d in zip(td, deltas))
    out["w"] = rel(got, want)
    return out, dict(td=td, deltas=deltas, got=got, want=want, mu=mu, sd=sd, dmu=dmu, dsd=dsd, sample=smp, q=q, aq=aq)
