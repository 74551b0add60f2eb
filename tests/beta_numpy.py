"""ContinuousMountainCar, the Beta policy and ActorCritic::tdac over iLSTD with it (RSRL_ILSTD_ACTOR_CRITIC with RSRL_BETA on
RSRL_CONTINUOUS_MOUNTAIN_CAR) restated in f64 numpy, in the order of examples/tdac_beta.rs.  Shared by the CPU and GPU tests.

  the domain    rsrl_domains/src/mountain_car/continuous.rs, literally (action_space.map_onto recalled as a clip)
  Softplus      fa/transforms.rs:196-218 (x for x >= 10, else ln(1 + exp(x)); gradient 1 / the logistic)
  the score     g_a = ln a - psi(alpha) + psi(alpha + beta), g_b = ln(1 - a) - psi(beta) + psi(alpha + beta) with scipy.special.digamma, of the
                action clamped to [2^-24, 1 - 2^-24] (recalled from rstat::univariate::beta; the library's definition)
  the rule      tests/lstd_numpy.ilstd, tests/tdac_lstd_numpy.critic_target on the updated theta, e = f32(alpha * c), then the two columns
  the sampler   Marsaglia-Tsang on the words of orc.draw(seed, id, t, P + 256 (j + 1)), at most 8 rounds per gamma"""
import numpy as np
from scipy.special import digamma, gammaln

from tests.lstd_numpy import ilstd
from tests.tdac_lstd_numpy import critic_target

LO, HI = 2.0 ** -24, 1.0 - 2.0 ** -24
ROUNDS = 8
X_BOUNDS, V_BOUNDS = (-1.2, 0.6), (-0.07, 0.07)
BLK_STEP, BLK_INIT, BLK_API = 0, 3, 4


def clip(lo, x, hi):
    return max(lo, min(hi, x))


def cmc_step(s, a):
    """ContinuousMountainCar::transition on (x, v) with the action a -> ((x', v'), reward, terminal)"""
    x, v = float(s[0]), float(s[1])
    a = clip(-1.0, float(a), 1.0)
    v = clip(V_BOUNDS[0], v + 0.0015 * a - 0.0025 * np.cos(3.0 * x), V_BOUNDS[1])
    x = clip(X_BOUNDS[0], x + v, X_BOUNDS[1])
    term = cmc_is_terminal(x)
    return (x, v), (0.0 if term else -1.0), term


def cmc_start():
    return (-0.5, 0.0)


def cmc_is_terminal(x):
    return x >= X_BOUNDS[1]


def softplus(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x >= 10.0, x, np.log1p(np.exp(np.minimum(x, 10.0))))


def softplus_grad(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x >= 10.0, 1.0, 1.0 / (1.0 + np.exp(-np.minimum(x, 10.0))))


def beta_params(xa, xb):
    """(alpha, beta) = softplus + MIN_TOL (1.0)"""
    return softplus(xa) + 1.0, softplus(xb) + 1.0


def beta_mode(alpha, beta):
    alpha, beta = np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    both = (alpha > 1.0) & (beta > 1.0)
    return np.where(both, (alpha - 1.0) / np.where(both, alpha + beta - 2.0, 1.0), alpha / (alpha + beta))


def beta_clamp(a):
    return np.clip(np.asarray(a, dtype=np.float64), LO, HI)


def beta_pdf(alpha, beta, a):
    a = beta_clamp(a)
    return np.exp((alpha - 1.0) * np.log(a) + (beta - 1.0) * np.log1p(-a) - (gammaln(alpha) + gammaln(beta) - gammaln(alpha + beta)))


def beta_score(alpha, beta, a):
    a = beta_clamp(a)
    p = digamma(alpha + beta)
    return np.log(a) - digamma(alpha) + p, np.log1p(-a) - digamma(beta) + p


def beta_step(W, phi, a, e):
    """the policy's handle: W (F, 2) f64 (column 0 alpha's) -> W'; both parameters are read before either column moves"""
    W, phi = np.asarray(W, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    xa, xb = float(phi @ W[:, 0]), float(phi @ W[:, 1])
    alpha, beta = beta_params(xa, xb)
    ga, gb = beta_score(alpha, beta, a)
    out = W.copy()
    out[:, 0] += e * ga * softplus_grad(xa) * phi
    out[:, 1] += e * gb * softplus_grad(xb) * phi
    return out


def tdac_beta_rule(theta, A, mu, W, phi_s, phi_n, a, r, term, gamma, lr, n_updates, alpha, rounds=None, phi32=None):
    """one transition -> (iLSTD's diagnostic, theta', A', mu', W').  lr is iLSTD's alpha, alpha ActorCritic's.  phi32: the features the actor reads
    (the device's f32 projection), default the f64 ones"""
    diag, theta2, A2, mu2 = ilstd(theta, A, mu, phi_s, phi_n, r, term, gamma, lr, n_updates, literal=False, rounds=rounds)
    c = critic_target(theta2, phi_s, phi_n, r, term, gamma)
    e = float(np.float32(alpha * c))                          # the one rounding out of f64
    return diag, theta2, A2, mu2, beta_step(W, phi_s if phi32 is None else phi32, a, e)


# ---- Philox4x32-10 on numpy arrays: the words of orc.draw(seed, id, t, block) for block words > 2 (whole blocks; tests hold it to orc.draw)
def philox_block(seed, gid, t, block):
    """gid, block: arrays (broadcast) -> uint32 (..., 4)"""
    gid, block = np.broadcast_arrays(np.asarray(gid, dtype=np.uint64), np.asarray(block, dtype=np.uint64))
    c = [np.full(gid.shape, int(t) & 0xFFFFFFFF, dtype=np.uint64), np.full(gid.shape, (int(t) >> 32) & 0xFFFFFFFF, dtype=np.uint64), gid.copy(), block.copy()]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    M = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & M, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & M]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def beta_sample(seed, gid, t, purpose, alpha, beta, words=None):
    """the sample of (seed, global learner id, t, purpose) for arrays gid / alpha / beta -> (x in [LO, HI], margin): margin is the smallest
    |ln u - rhs| over the acceptance tests the sample evaluated -- where it is tiny a rounded test may decide the other way.  words(j): the
    round's Philox blocks (default: philox_block at block word purpose + 256 (j + 1))"""
    gid = np.asarray(gid)
    alpha, beta = np.broadcast_to(np.asarray(alpha, dtype=np.float64), gid.shape), np.broadcast_to(np.asarray(beta, dtype=np.float64), gid.shape)
    d = [alpha - 1.0 / 3.0, beta - 1.0 / 3.0]
    c = [1.0 / np.sqrt(9.0 * d[0]), 1.0 / np.sqrt(9.0 * d[1])]
    g = [d[0].copy(), d[1].copy()]
    got = [np.zeros(gid.shape, dtype=bool), np.zeros(gid.shape, dtype=bool)]
    margin = np.full(gid.shape, np.inf)
    for j in range(ROUNDS):
        live = ~(got[0] & got[1])                             # (a learner that has both leaves the loop: it evaluates no further test)
        if not live.any():
            break
        w = (philox_block(seed, gid, t, purpose + 256 * (j + 1)) if words is None else words(j)).astype(np.float64)
        u1, u2 = ((np.floor(w[..., 0] / 256.0)) + 1.0) / 16777216.0, np.floor(w[..., 1] / 256.0) / 16777216.0
        rad = np.sqrt(-2.0 * np.log(u1))
        ang = float(np.float32(6.2831854820251465)) * u2
        n = [rad * np.cos(ang), rad * np.sin(ang)]
        for q in (0, 1):
            u = (np.floor(w[..., 2 + q] / 256.0) + 1.0) / 16777216.0
            tt = 1.0 + c[q] * n[q]
            v = tt * tt * tt
            with np.errstate(invalid="ignore", divide="ignore"):
                rhs = 0.5 * n[q] * n[q] + d[q] - d[q] * v + d[q] * np.log(np.where(v > 0.0, v, 1.0))
                ok = (v > 0.0) & (np.log(u) < rhs)
                m = np.where(v > 0.0, np.abs(np.log(u) - rhs), np.abs(tt))      # (v <= 0 is t <= 0: the rounded quantity is t = 1 + c n)
            need = live & ~got[q]                             # (a gamma already drawn reads no further test's outcome)
            margin = np.where(need, np.minimum(margin, m), margin)
            take = need & ok
            g[q] = np.where(take, d[q] * v, g[q])
            got[q] = got[q] | take
    return np.clip(g[0] / (g[0] + g[1]), LO, HI), margin


def columns_for(alpha, beta, F):
    """policy columns (F, 2) f32 whose preferences are Softplus^-1(alpha - 1), Softplus^-1(beta - 1) at EVERY state: all weight on the constant
    feature (the last one)"""
    W = np.zeros((F, 2), dtype=np.float32)
    W[F - 1] = [k - 1.0 if k - 1.0 >= 10.0 else np.log(np.expm1(k - 1.0)) for k in (alpha, beta)]      # (Softplus is the identity from 10 on)
    return W


def handle_case(orc, order, N=67, rounds=3, gamma=0.95, lr=0.05, n_updates=3, alpha=0.3):
    """the GPU rule test's inputs and what the rule makes of them, built as tests/tdac_lstd_numpy.handle_case builds them: a well-conditioned random
    iLSTD state per learner, random policy columns with |x| <= 3 (sum |w| <= 3 and |phi| <= 1), `rounds` rounds of transitions stepped by
    cmc_step from random states and random actions in [0, 1] -- learners 0 and 1 act 0 and 1 exactly, which the update clamps -- a quarter more
    of them flagged terminal.  -> dict(init, rounds = [(from, a, r, to, term)], diag, skipped); the f64 rule's final state is computed by the
    caller from the device's f32 features (tdac_beta_rule's phi32)"""
    from tests.lstd_numpy import near_tie_band
    rng = np.random.default_rng(400 + order * 10 + 21)
    lo, hi = np.array([X_BOUNDS[0], V_BOUNDS[0]]), np.array([X_BOUNDS[1], V_BOUNDS[1]])
    F = (order + 1) ** 2
    init = []
    for _ in range(N):
        M = rng.normal(0.0, 1.0, size=(F, F))
        W = rng.normal(0.0, 1.0, size=(F, 2))
        W *= rng.uniform(0.5, 3.0, size=2) / np.abs(W).sum(axis=0)
        init.append((rng.normal(0.0, 0.5, size=F), np.eye(F) + 0.1 * M / np.sqrt(F), rng.normal(0.0, 1.0, size=F), W.astype(np.float32)))
    cur = [[t, m, u] for t, m, u, _ in init]
    out_rounds, diag, skipped = [], np.zeros((rounds, N)), np.zeros(N, dtype=bool)
    for k in range(rounds):
        frm = rng.uniform(lo, hi, size=(N, 2)).T.astype(np.float32)
        a = rng.uniform(0.0, 1.0, size=N).astype(np.float32)
        a[0], a[1] = 0.0, 1.0
        nxt, rew, term = np.zeros_like(frm), np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.uint8)
        for i in range(N):
            ns, r, t = cmc_step(frm[:, i], a[i])
            nxt[:, i], rew[i], term[i] = np.asarray(ns, dtype=np.float32), np.float32(r), bool(t)
        term = (term.astype(bool) | (rng.random(N) < 0.25)).astype(np.uint8)
        out_rounds.append((frm, a, rew, nxt, term))
        for i in range(N):
            phi_s, phi_n = orc.fourier_project(orc.MOUNTAIN_CAR, order, frm[:, i]), orc.fourier_project(orc.MOUNTAIN_CAR, order, nxt[:, i])
            mus = []
            diag[k, i], *cur[i] = ilstd(*cur[i], phi_s, phi_n, float(rew[i]), bool(term[i]), gamma, lr, n_updates, literal=False, rounds=mus)
            skipped[i] |= any(near_tie_band(m) for m in mus)
    return dict(init=init, rounds=out_rounds, diag=diag, skipped=skipped, F=F, params=dict(gamma=gamma, lr=lr, n_steps=n_updates, alpha=alpha))


def actor_after(orc, case, order, phi32_rounds):
    """the f64 rule's policy columns after every round of `case`, from the SAME f32 inputs the device read: phi32_rounds[k] = the device's f32
    features (F, N) of round k's `from` states -> [W (N, F, 2) after round k]"""
    p = case["params"]
    N = len(case["init"])
    cur = [[t, m, u, W.astype(np.float64)] for t, m, u, W in case["init"]]
    out = []
    for k, (frm, a, rew, nxt, term) in enumerate(case["rounds"]):
        for i in range(N):
            phi_s, phi_n = orc.fourier_project(orc.MOUNTAIN_CAR, order, frm[:, i]), orc.fourier_project(orc.MOUNTAIN_CAR, order, nxt[:, i])
            _, *cur[i] = tdac_beta_rule(*cur[i], phi_s, phi_n, float(a[i]), float(rew[i]), bool(term[i]), p["gamma"], p["lr"], p["n_steps"], p["alpha"],
                                        phi32=phi32_rounds[k][:, i].astype(np.float64))
        out.append(np.stack([c[3] for c in cur]))
    return out
