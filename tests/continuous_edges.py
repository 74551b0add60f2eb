"""Crafted preferences and actions for the continuous policies' device code (cont_policy.hpp: softplus_dev .. beta_sample,
gauss_params .. gauss_coef) and the f64 answers on them.  The f64 formulas are tests/gaussian_numpy.py's and tests/beta_numpy.py's; nothing is restated.

table(policy) -> (p0, p1, a float32 (n,), groups (n,) of str): a FIXED list (no random numbers), deduplicated by bit pattern.  The two preferences go in
through the weights (columns(): every row zero but the constant feature, the last one, phi = 1), so they are the device's preferences at every state.

  GAUSSIAN  (x_m, x_s, a).  x_s over XS (the 0.01 floor of sd, Softplus's switch at 10 from both sides, sd^2 beyond fp32), x_m cycled over XM, the
            action fl32(mu + k sd) from the f64 parameters for k of KS -- k = +-1 is where d^2 - Sigma cancels, +-13 / +-14 the two sides of the
            density's underflow -- and the absolute actions of ABS
  BETA      (x_a, x_b, a).  every ordered pair of PREFS_PAIR and the diagonal of PREFS, the actions of beta_actions (the clamp's edges, the f64 mode)
  nonfinite(policy)  NaN, +inf, -inf in either preference, one at a time: the read-only legs only

Groups.  range: an fp32 intermediate of the reference's expression (d^2, Sigma, Sigma^2, sigma(x)) or the f64 result itself leaves fp32's normal range
(Beta: the density does); cancel: k = +-1, +-(1 + 2^-10) (Beta: the action is the mode, or both parameters are within a few ulps of 1 -- beta_mode's
two differences); tail: |k| >= 6 or an absolute action (Beta: an action the clamp moves or that sits on its edge); switch: a preference of SWITCH;
floor: a preference <= -5 (sd within 0.007 of its floor; alpha - 1 <= 0.007); general: the rest.  The first that applies, in this order.

THE COMPARISON is staged, so that each stage has a bound one can state.

  stage A   parameters from preferences: mu is the crafted value bit for bit; sd, alpha, beta against f64 RELATIVE TO THEMSELVES (not to
            max(1, |x|): sd = 0.01 off by 1e-5 of itself is a finding).  The bar of sd is 4 * SD_NUMPY, the figure of
            float32(log1p(exp(x32))) + float32(0.01) on the table's own x_s; alpha's and beta's is 4 * 2^-24 (two roundings: Softplus's, the sum's;
            the factor 4 is the project's usual one, for exp_dev's 1.5 ulp and the library logarithm; the device's beta_params keeps the literal
            ln(1 + e^x), whose 6e-8 is within this bar beside the + 1 -- only sd needs softplus_rel_dev)
  stage B   everything downstream, evaluated in f64 AT THE DEVICE'S OWN fp32 PARAMETERS (policy_params), in units of 2^-24 * cond(row), cond the
            first-order condition number of the quantity in its fp32 inputs and operations -- see gauss_b / beta_b.  One constant per quantity: the
            device's worst figure must not exceed 4 * K_NUMPY[quantity], the worst of a plain float32 numpy evaluation of the reference's formulas
            (gauss_f32 / beta_f32, Softplus in the log1p form) over the same rows.  Measured against the reference's arithmetic, never the device

units(got, want, cond, floor) states the rules that hold on every row: NaN exactly where f64 is NaN; an f64 result beyond FLT_MAX must come back as the
infinity of that sign; one below 2^-150 (half the smallest subnormal, and not an exact
cancellation: 2^-24 cond is below it too) as zero; everything else within units of 2^-24 cond + floor.  floor is what no
fp32 value can do better than: 2^-126 for the densities (the issue's), 2^-149 elsewhere (results below the normal range are multiples of it), and for
the coefficients that carry sigma(x) |g| 2^-149 (sigma itself is an fp32 value: below 2^-126 it is a multiple of 2^-149).

gauss_f32(..., literal=True) is the reference's expression rounded after every operation.  It is what K_NUMPY is measured with, on the rows that are
not `range`: on those its intermediates overflow (Sigma = sd^2 = inf from sd = 1.85e19 on: (d^2 - inf) / (2 inf) = NaN).  literal=False is the
rearrangement the device uses (d / sd, 1 / sd: no square before the division), same conditioning, and tests/test_continuous_edges_cpu.py shows that it
meets every bar on every row that is not declared: the bars are attainable in fp32.

declared(policy) lists the rows that are left out of one quantity's bar, each with the device's rule in words; at most 2 % of a table."""
import functools

import numpy as np
from scipy.special import digamma, gammaln

from tests import beta_numpy as bn
from tests import gaussian_numpy as gn

GAUSSIAN, BETA = 6, 4
F32, F64 = np.float32, np.float64
EPS = 2.0 ** -24
FLT_MAX = float(np.finfo(F32).max)
TINY, SUB = 2.0 ** -126, 2.0 ** -149
B10, A10 = F32(np.nextafter(F32(10.0), F32(0.0))), F32(np.nextafter(F32(10.0), F32(20.0)))
GROUPS = ("floor", "switch", "cancel", "tail", "range", "general")
SEED, OFFSET = 91, 3000

XM = (0.0, -0.0, 1e-3, -1e-3, 0.5, -0.5, 1.0, -1.0, 3.0, -3.0, 1e4, -1e4)
XS = (-100.0, -87.5, -30.0, -20.0, -17.0, -16.6, -12.0, -10.3, -5.0, -3.0, -1.0, 0.0, 1.0, 5.0, 9.5, B10, 10.0, A10, 12.0, 30.0, 1e3, 1e6, 1e10, 2e19, 1e30)
SWITCH = (9.5, float(B10), 10.0, float(A10), 12.0)
KS = (0.0, 2.0 ** -12, 0.5, 1.0, 1.0 + 2.0 ** -10, 2.0, 6.0, 13.0, 14.0, 40.0)
KS = tuple(s * k for k in KS for s in ((1.0, -1.0) if k else (1.0,)))
CANCEL_K = (1.0, 1.0 + 2.0 ** -10)
ABS = (1e10, -1e10, 3e18, -3e18, FLT_MAX, -FLT_MAX)
PREFS = XS[:22]                                                                       # ... up to 1e6
PREFS_PAIR = (-100.0, -17.0, -10.3, -3.0, 0.0, 1.0, 9.5, B10, 10.0, A10, 30.0, 1e6)
LO32, HI32 = F32(bn.LO), F32(bn.HI)

# ---- recorded: the float32 numpy evaluation of the reference on these tables (tests/test_continuous_edges_cpu.py re-measures them; the bars are 4 x)
SD_NUMPY = 2.132e-07             # max |sd32 - sd64| / sd64 of float32(log1p(exp(x32))) + float32(0.01) over the table's x_s
K_NUMPY = {                      # max units of 2^-24 cond, gauss_f32(literal=True) / beta_f32 at their own fp32 parameters
    (GAUSSIAN, "pdf"): 1.971, (GAUSSIAN, "cm"): 2.015, (GAUSSIAN, "cs"): 3.958, (GAUSSIAN, "sample"): 0.8734,
    (BETA, "pdf"): 2.138, (BETA, "mode"): 1.600, (BETA, "ca"): 4.865, (BETA, "cb"): 4.791,
}
PARAM_BAR = 4 * EPS              # alpha, beta relative to themselves
BETA_SAMPLE_BAR = 4 * 4.649e-7   # |x - x64| of a Beta sample clear of an acceptance boundary: tests/test_gpu_tdac_beta.py's bar for this quantity
BETA_MARGIN = 2e-5               # tests/fuzz_beta.py's (nac_numpy.MARGIN): an acceptance test this close to its boundary may go the other way in fp32
BETA_LEFT_OUT = 0.05


def sd_bar():
    return 4 * SD_NUMPY


def bar(policy, quantity):
    return 4 * K_NUMPY[(policy, quantity)]


# ------------------------------------------------------------------------------------------------------------------------------- the tables
def _key(*v):
    return np.array(v, dtype=F32).tobytes()


def _gauss_group(xs, k, mu, sd, a):
    d, var = float(a) - mu, sd * sd
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        gm, gv = gn.gauss_score(mu, sd, float(a))
        res = [float(gm), float(gv * bn.softplus_grad(xs))]
        mids = [d * d, var, var * var, float(gv)]
        sig = float(bn.softplus_grad(xs))
    if any(abs(x) > FLT_MAX for x in mids + res) or any(0.0 < abs(x) < TINY for x in res + [sig]):
        return "range"
    if k is not None and abs(k) in CANCEL_K:
        return "cancel"
    if k is None or abs(k) >= 6.0:
        return "tail"
    if float(xs) in SWITCH:
        return "switch"
    return "floor" if xs <= -5.0 else "general"


def _build_gaussian():
    rows, seen = [], set()
    acts = [("k", k) for k in KS] + [("abs", v) for v in ABS]
    for i, xs in enumerate(XS):
        xs = F32(xs)
        for j, (kind, v) in enumerate(acts):
            for rep in range(3):
                xm = F32(XM[(5 * i + 7 * j + 4 * rep) % len(XM)])
                mu, sd = (float(x) for x in gn.gauss_params(xm, xs))
                a = F32(mu + v * sd) if kind == "k" else F32(v)
                key = _key(xm, xs, a)
                if key in seen:
                    continue
                seen.add(key)
                rows.append((xm, xs, a, _gauss_group(xs, v if kind == "k" else None, mu, sd, a)))
    return rows


def beta_actions(alpha, beta):
    """the action list of one (alpha, beta): the clamp's edges from both sides, the f64 mode rounded, two actions the clamp moves"""
    return [0.0, -0.0, SUB, 2.0 ** -25, 2.0 ** -24, float(np.nextafter(LO32, F32(1.0))), 1e-3, 0.25, 0.5, ("mode", float(F32(bn.beta_mode(alpha, beta)))), 0.75,
            1.0 - 2.0 ** -12, 1.0 - 2.0 ** -23, 1.0 - 2.0 ** -24, 1.0, -0.5, 1.5]


def _beta_group(xa, xb, a, is_mode, alpha, beta):
    with np.errstate(over="ignore", under="ignore"):
        pdf = float(bn.beta_pdf(alpha, beta, float(a)))
    if pdf > FLT_MAX or pdf < TINY:
        return "range"
    if not (float(np.nextafter(LO32, F32(1.0))) < a < 1.0 - 2.0 ** -23):
        return "tail"
    if is_mode or (xa <= -10.0 and xb <= -10.0):
        return "cancel"
    if float(xa) in SWITCH or float(xb) in SWITCH:
        return "switch"
    return "floor" if min(xa, xb) <= -5.0 else "general"


def _build_beta():
    pairs = [(x, y) for x in PREFS_PAIR for y in PREFS_PAIR if x != y] + [(x, x) for x in PREFS]
    rows, seen = [], set()
    for xa, xb in pairs:
        xa, xb = F32(xa), F32(xb)
        alpha, beta = (float(x) for x in bn.beta_params(xa, xb))
        for act in beta_actions(alpha, beta):
            is_mode = isinstance(act, tuple)
            a = F32(act[1] if is_mode else act)
            key = _key(xa, xb, a)
            if key in seen:
                continue
            seen.add(key)
            rows.append((xa, xb, a, _beta_group(xa, xb, a, is_mode, alpha, beta)))
    return rows


@functools.lru_cache(maxsize=None)
def table(policy):
    rows = _build_gaussian() if policy == GAUSSIAN else _build_beta()
    out = [np.array([r[k] for r in rows], dtype=F32) for k in range(3)] + [np.array([r[3] for r in rows])]
    for x in out:
        x.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def nonfinite(policy):
    """(p0, p1, a): NaN, +inf, -inf in either preference, one at a time, the other preference and the action moderate"""
    others = {GAUSSIAN: ((0.5, 1.0, -12.0), (0.25, -3.0)), BETA: ((0.0, 12.0, -12.0), (0.25, 0.0, 1.0))}[policy]
    rows = []
    for bad in (np.nan, np.inf, -np.inf):
        for col in (0, 1):
            for o in others[0]:
                for a in others[1]:
                    rows.append((bad, o, a) if col == 0 else (o, bad, a))
    out = tuple(np.array([r[k] for r in rows], dtype=F32) for k in range(3))
    for x in out:
        x.setflags(write=False)
    return out


def columns(F, p0, p1):
    """(F, 2) policy columns whose preferences are (p0, p1) at EVERY state: all weight on the constant feature (the last one, phi = 1)"""
    W = np.zeros((F, 2), dtype=F32)
    W[F - 1] = (p0, p1)
    return W


def finite_coefficients(policy):
    """the rows the driver-loop legs use: both coefficients finite in fp32 at the first sample whatever it is -- preferences of moderate size (0 * c must
    stay 0 through an update with alpha = 0, and the loop's own actions are not the table's)"""
    p0, p1, _, _ = table(policy)
    keep = (np.abs(p0) <= 1e4) & (np.abs(p1) <= 1e6) & ~((p0 == 0) & np.signbit(p0))
    _, first = np.unique(np.stack([p0, p1]).view(np.uint32), axis=1, return_index=True)      # one learner per pair of preferences
    pick = np.zeros(len(p0), dtype=bool)
    pick[first] = True
    return keep & pick


# ------------------------------------------------------------------------------------------------------------------------------- stage A
def rel_self(got, want):
    """|got - want| / |want|, 0 where both are the same infinity or both NaN"""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r = np.abs(got - want) / np.abs(want)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    return np.where(same, 0.0, np.where(np.isnan(r), np.inf, r))


def sd64(xs):
    return gn.gauss_params(0.0, np.asarray(xs, dtype=F64))[1]


def softplus32(x, literal=False):
    """Softplus in float32 numpy: log1p(exp(x)), or the reference's ln(1 + exp(x)) taken literally"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        e = np.exp(np.minimum(x, F32(10.0)))
        sp = np.log(F32(1.0) + e) if literal else np.log1p(e)
    assert sp.dtype == F32
    return np.where(x >= F32(10.0), x, sp).astype(F32)


def sigma32(x):
    """Softplus's gradient in float32 numpy, the logistic as e^x / (1 + e^x) below 0 (1 / (1 + e^-x) overflows for x < -88.7) and 1 / (1 + e^-x) above"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        e = np.exp(-np.abs(np.minimum(x, F32(10.0))))
        s = np.where(x >= 0, F32(1.0) / (F32(1.0) + e), e / (F32(1.0) + e))
    return np.where(x >= F32(10.0), F32(1.0), s).astype(F32)


def sd32(xs, literal=False):
    return (softplus32(xs, literal) + F32(gn.MIN_TOL)).astype(F32)


# ------------------------------------------------------------------------------------------------------------------------------- stage B
def units(got, want, cond, floor=SUB):
    """per row: 0 where the rule for the row's f64 result holds exactly (NaN for NaN, the infinity of the sign beyond FLT_MAX, zero below 2^-150),
    inf where it does not, else |got - want| / (2^-24 cond + floor)"""
    got, want, cond = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64), np.asarray(cond, dtype=F64)
    floor = np.broadcast_to(np.asarray(floor, dtype=F64), want.shape)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        u = np.abs(got - want) / (EPS * cond + floor)
        u = np.where(got == want, 0.0, u)
        u = np.where(np.isnan(u), np.inf, u)                                            # (0 / 0 with got != want, inf - inf, a NaN on one side)
        over, under = np.abs(want) > FLT_MAX, (np.abs(want) < SUB / 2) & (EPS * cond < SUB / 2)      # (underflow, not an exact cancellation)
        u = np.where(over, np.where(got == np.sign(want) * np.inf, 0.0, np.inf), u)
        u = np.where(under & ~over, np.where(got == 0.0, 0.0, np.inf), u)
        u = np.where(np.isnan(want), np.where(np.isnan(got), 0.0, np.inf), u)
    return u


def gauss_b(mu, sd, xs, a):
    """the f64 answers at the fp32 parameters (mu, sd) and their condition numbers -> {quantity: (want, cond, floor)}.  d = a - mu, Sigma = sd^2; a
    relative perturbation eps of an input or an operation moves
      pdf = exp(-d^2 / (2 Sigma)) / sqrt(2 pi Sigma)   by pdf (d^2 / Sigma) eps through d, by pdf (d^2 / (2 Sigma) + 1 / 2) eps through Sigma, by
                                                       pdf eps through each of the last operations: cond = pdf (1 + d^2 / Sigma)
      c_m = d / Sigma                                  by |c_m| eps each: cond = |d| / Sigma
      c_s = sigma(x_s) (d^2 - Sigma) / (2 Sigma^2)     the numerator's two terms move separately (that is the cancellation at |d| = sd), by
                                                       d^2 eps and Sigma eps: cond = sigma (d^2 + Sigma) / (2 Sigma^2) >= |c_s|"""
    mu, sd, a, xs = (np.asarray(x, dtype=F64) for x in (mu, sd, a, xs))
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        d, var = a - mu, sd * sd
        pdf = gn.gauss_pdf(mu, sd, a)
        gm, gv = gn.gauss_score(mu, sd, a)
        sig = bn.softplus_grad(xs)
        k2 = (d / sd) ** 2
        out = {"pdf": (pdf, pdf * (1.0 + k2), TINY),
               "cm": (gm, np.abs(d) / var, SUB),
               "cs": (gv * sig, sig * (k2 + 1.0) / (2.0 * var), SUB + np.abs(gv) * SUB)}
    return out


normal_parts = gn.gauss_normal_parts          # (z, rad) in f64 of the Philox block at block word purpose + 256


def gauss_sample_b(mu, sd, z, rad):
    """a = mu + sd z, z = rad cos(2 pi u2): the angle's rounding (2 pi u2 eps) moves z by at most 2 pi rad eps, the radius' and the cosine's by |z| eps
    each, the fused multiply-add by |a| eps <= (|mu| + sd |z|) eps: cond = |mu| + sd (|z| + 2 pi rad)"""
    mu, sd = np.asarray(mu, dtype=F64), np.asarray(sd, dtype=F64)
    with np.errstate(over="ignore", invalid="ignore"):
        return mu + sd * z, np.abs(mu) + sd * (np.abs(z) + 2.0 * np.pi * rad), SUB


def normal32(seed, gid, t, purpose):
    """Box-Muller's cosine normal in float32 numpy on the same words"""
    w = bn.philox_block(seed, np.asarray(gid), t, purpose + 256)
    u1 = ((w[..., 0] >> 8).astype(F32) + F32(1.0)) * F32(1.0 / 16777216.0)
    u2 = (w[..., 1] >> 8).astype(F32) * F32(1.0 / 16777216.0)
    with np.errstate(divide="ignore"):
        z = np.sqrt(F32(-2.0) * np.log(u1)) * np.cos(F32(6.2831854820251465) * u2)
    assert z.dtype == F32
    return z


def gauss_f32(xm, xs, a, literal=True):
    """the reference's formulas in float32 numpy, rounded after every operation -> dict(mu, sd, pdf, cm, cs).  literal: Sigma = sd * sd formed first,
    as the reference's builder does; else d / sd and 1 / sd (no square before the division) -- the form that cannot overflow where the result does not"""
    xm, xs, a = (np.asarray(x, dtype=F32) for x in (xm, xs, a))
    sd, sig = sd32(xs), sigma32(xs)
    d = a - xm
    two_pi = F32(6.2831854820251465)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        if literal:
            var = sd * sd
            pdf = np.exp(-(d * d) / (F32(2.0) * var)) / np.sqrt(two_pi * var)
            cm = d / var
            cs = (d * d - var) / (F32(2.0) * (var * var)) * sig
        else:
            t, inv = d / sd, F32(1.0) / sd
            pdf = np.exp(F32(-0.5) * t * t) * (inv * F32(0.3989422804014327))
            cm = t * inv
            cs = F32(0.5) * (cm * (cm * sig) - (inv * inv) * sig)          # (sigma inside the square: a tiny sigma meets g_mu before g_mu^2 overflows)
    out = dict(mu=xm, sd=sd, pdf=pdf, cm=cm, cs=cs)
    assert all(v.dtype == F32 for v in out.values())
    return out


def digamma32(x):
    """digamma for x >= 1 in float32 numpy: the recurrence up to an argument >= 6, then the asymptotic series (the textbook evaluation)"""
    x = np.array(x, dtype=F32)
    acc = np.zeros_like(x)
    for _ in range(6):
        low = x < F32(6.0)
        acc = np.where(low, acc - F32(1.0) / x, acc).astype(F32)
        x = np.where(low, x + F32(1.0), x).astype(F32)
    inv = F32(1.0) / x
    inv2 = inv * inv
    p = F32(1.0 / 240.0)
    p = p * inv2 - F32(1.0 / 252.0)
    p = p * inv2 + F32(1.0 / 120.0)
    p = p * inv2 - F32(1.0 / 12.0)
    out = acc + (np.log(x) - F32(0.5) * inv + p * inv2)
    assert out.dtype == F32
    return out


def beta_b(alpha, beta, xa, xb, a):
    """the f64 answers at the fp32 parameters (alpha, beta) and their condition numbers -> {quantity: (want, cond, floor)}.  a_c the clamped action.
      pdf = exp(E), E = (alpha - 1) ln a_c + (beta - 1) ln(1 - a_c) - ln G(alpha) - ln G(beta) + ln G(alpha + beta): each term of E is rounded, a
            relative eps in one moves pdf by pdf |term| eps, exp itself by pdf eps: cond = pdf (1 + sum |terms|)
      c_a = sigma(x_a) (ln a_c - psi(alpha) + psi(alpha + beta)): three rounded terms: cond = sigma (|ln a_c| + |psi(alpha)| + |psi(alpha + beta)|);
            c_b likewise with ln(1 - a_c) and psi(beta)
      mode  both parameters above 1: p / (p + q) with p = alpha - 1, q = beta - 1.  Both differences are exact below 2 (Sterbenz) and rounded
            relative to THEMSELVES above; the sum of two positive numbers and the quotient are each one relative rounding: d mode / mode =
            (1 - mode)(e_p - e_q) - e_sum + e_div, so cond = mode (at most four roundings of it).  Else the mean alpha / (alpha + beta): two relative
            roundings, cond = mode again"""
    alpha, beta, xa, xb = (np.asarray(x, dtype=F64) for x in (alpha, beta, xa, xb))
    ac = bn.beta_clamp(a)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        terms = [(alpha - 1.0) * np.log(ac), (beta - 1.0) * np.log1p(-ac), gammaln(alpha), gammaln(beta), gammaln(alpha + beta)]
        pdf = bn.beta_pdf(alpha, beta, a)
        ga, gb = bn.beta_score(alpha, beta, a)
        sa, sb = bn.softplus_grad(xa), bn.softplus_grad(xb)
        pab = np.abs(digamma(alpha + beta))
        mode = bn.beta_mode(alpha, beta)
        out = {"pdf": (pdf, pdf * (1.0 + sum(np.abs(t) for t in terms)), TINY),
               "mode": (mode, np.abs(mode), SUB),
               "ca": (ga * sa, sa * (np.abs(np.log(ac)) + np.abs(digamma(alpha)) + pab), SUB + np.abs(ga) * SUB),
               "cb": (gb * sb, sb * (np.abs(np.log1p(-ac)) + np.abs(digamma(beta)) + pab), SUB + np.abs(gb) * SUB)}
    return out


def beta_f32(xa, xb, a):
    """the reference's formulas in float32 numpy, rounded after every operation -> dict(alpha, beta, pdf, mode, ca, cb); ln Gamma is the library's
    float32 one, digamma digamma32, the mode beta_mode's two differences"""
    xa, xb, a = (np.asarray(x, dtype=F32) for x in (xa, xb, a))
    one = F32(1.0)
    alpha, beta = (softplus32(xa) + one).astype(F32), (softplus32(xb) + one).astype(F32)
    ac = np.clip(a, LO32, HI32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        lnb = gammaln(alpha) + gammaln(beta) - gammaln(alpha + beta)
        pdf = np.exp((alpha - one) * np.log(ac) + (beta - one) * np.log(one - ac) - lnb)
        pab = digamma32(alpha + beta)
        ca = (np.log(ac) - digamma32(alpha) + pab) * sigma32(xa)
        cb = (np.log(one - ac) - digamma32(beta) + pab) * sigma32(xb)
        am, bm = alpha - one, beta - one
        mode = np.where((alpha > one) & (beta > one), am / np.where(am + bm > 0, am + bm, one), alpha / (alpha + beta))
    out = dict(alpha=alpha, beta=beta, pdf=pdf, mode=mode.astype(F32), ca=ca, cb=cb)
    assert all(v.dtype == F32 for v in out.values()), {k: v.dtype for k, v in out.items()}
    return out


def stage_b(policy, p0, p1, a, got):
    """got: dict with the fp32 parameters (mu, sd | alpha, beta) and any of the quantities -> {quantity: units (n,)} against f64 AT those parameters"""
    if policy == GAUSSIAN:
        ref = gauss_b(got["mu"], got["sd"], p1, a)
    else:
        ref = beta_b(got["alpha"], got["beta"], p0, p1, a)
    return {q: units(got[q], *ref[q]) for q in ref if q in got}


# ------------------------------------------------------------------------------------------------------------------------------- declared rows
def declared(policy):
    """{quantity: [(mask over the table, the device's rule in words)]}: rows left out of that quantity's stage-B bar.  The GPU test pins each rule."""
    p0, p1, a, _ = table(policy)
    out = {}
    if policy == GAUSSIAN:
        pass
    return out


def declared_mask(policy, quantity):
    n = len(table(policy)[0])
    m = np.zeros(n, dtype=bool)
    for mask, _ in declared(policy).get(quantity, []):
        m |= mask
    return m
