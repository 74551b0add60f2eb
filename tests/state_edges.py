"""Crafted states for the code that produces and consumes a state -- the four domain transitions (rsrl_amd/csrc/device_core.hpp Domain<0|1|2|4>::step,
the Pre form, Domain<2>::step_uniform), the Fourier projections and the tile coder -- and the f64 answers on them.  Shared by the CPU and GPU tests.

table(domain) -> (S float32 (D, n), names (n,) of str): a FIXED list (no random numbers), deduplicated by bit pattern, n no multiple of 64.  Every row is
stepped under every action of actions(domain).  The classes (the part of a name before the first ':'):

  bound      a dimension at lo, hi and their inner neighbours                 zero    0, -0.0, +-2^-149 (the smallest subnormal)
  scaled     the scaled position s~ = 0, 1/4, 1/2, 3/4, 1 and +-2 ulps of the state: sincospi01's rint(2 s~) ties and quadrant select
  out        lo - w, hi + w for w = 1 ulp, half a width, 3 widths             limit   MountainCar's x and CartPole's theta at the ABI's admission limit
  cross      the product of a few values of both dimensions (2-D domains)
  quadrant   MountainCar: 3x on sincos_cw's quadrant boundaries +-pi/4, +-3pi/4, +-2 ulps
  goal, wall MountainCar: x + v' lands -2..+2 ulps around 0.6 / -1.2 (crafted in f64 for every action); vclip: v + dv lands around +-0.07
  start      MountainCar: x = 0.6f (already terminal) and its neighbours as a start state
  clip       CartPole: one RK4 step carries x' across +-6 / theta' across +-2, by more than 1e-3 (far) and by less than 1e-6 (the two floats at the flip)
  thr        CartPole: the same for the terminal thresholds x = +-2.4, theta = +-12 deg;  onthr: a start state on a threshold
  wrap       Acrobot: the step takes theta1 / theta2 / both past +pi or -pi;  pi: a start state on +-(float)pi
  vclip      Acrobot: theta1' across +-4pi, theta2' across +-9pi, both sides;  line: both sides of cos t1 + cos(t1 + t2) = -1, far and at the flip

The crafted rows are found by bisection over fp32 values on the oracle's f64 transition (never on the code under test).  Acrobot's angles stay within 3
widths: wrapf is a loop.  Every state is finite, and answers() refuses a table whose fp32 successor before the wraps is not (a loop that would not end).

ANSWERS.  answers(domain, prec) -> dict(next (n, A, D), reward (n, A), term (n, A), raw (n, A, D) the successor before clips and wraps) from the oracle's
instantiation prec on the fp32 inputs.  THE COMPARISON: err(domain, got, want64) = |got - want| / (1 + |want|); Acrobot's two angles are compared ON THE
CIRCLE (theta = (float)pi is above the f64 pi: the reference wraps it to -pi and fp32 keeps it -- one point of the circle, 2 pi apart as numbers).
Every bitwise comparison is on bit patterns (bits()), so that -0.0 counts.

THE BARS are measured, not chosen: four times the largest error of the oracle's _f32 instantiation (libm, the reference's formulas in float32) against
f64 on the same rows -- F32_STEP / F32_PHI below, re-measured by tests/test_state_edges_cpu.py.  Rows are split in three sets with a bar each, `in` (every
component within [lo, hi]), `limit` (the rows at the admission limit: s~ up to 1001, its rounding alone is 6e-5) and `out` (the rest: 1 ulp to 3 widths
outside): one bar over all would let the limit rows set the bar of the rest.  Each bar is therefore at most what one bar over all rows would be.  phi_bar() is capped by the assertions that exist (3e-6 MountainCar order 5,
6e-6 elsewhere: tests/test_gpu_parity_mc.py, test_gpu_parity_more.py) on the `in` rows.

DECISIONS.  (1) term is the domain's predicate on the returned next state, exactly; (2) reward is the constant that goes with term, exactly; (3) term is
f64's wherever f64's deciding quantity -- margin(): the x before its clip minus 0.6; CartPole's four margins; cos t1 + cos(t1 + t2) + 1 -- is farther
from 0 than band(domain).  band = the row's bar times the size of the quantity (MountainCar 1 + 0.6; CartPole 1 + 2.4; Acrobot 3 (1 + pi) for the three
angles in the sum, plus 4e-7 for the two fp32 cosines and their sum).  Rows inside the band are left out of (3) only; at most 5 % of a domain's pairs."""
import functools
import json
import os

import numpy as np

from oracle import oracle as orc

MC, CP, AC, CMC = 0, 1, 2, 4
DOMAINS = (MC, CP, AC, CMC)
F32, F64 = np.float32, np.float64
SUB = F32(2.0 ** -149)
PI32 = F32(np.pi)
TW64 = np.pi / 15.0
LEFT_OUT = 0.05
CMC_ACTIONS = (-3.0, -1.0, -0.2, 0.0, 0.7, 1.0, 3.0, float(np.nextafter(F32(1.0), F32(2.0))), float(np.nextafter(F32(-1.0), F32(-2.0))))

# ---- recorded: the oracle's _f32 instantiation against f64 on these tables (tests/test_state_edges_cpu.py re-measures every figure; the bars are 4 x)
F32_STEP = {          # max |next32 - next64| / (1 + |next64|) over rows x actions, per row set
    (MC, "in"): 2.749e-08, (MC, "out"): 2.534e-08, (MC, "limit"): 3.67e-08, (CP, "in"): 4.983e-08,
    (CP, "out"): 4.374e-08, (CP, "limit"): 1.379e-06, (AC, "in"): 3.951e-06, (AC, "out"): 0.00241,
    (CMC, "in"): 3.016e-08, (CMC, "out"): 2.611e-08, (CMC, "limit"): 3.678e-08,
}
F32_PHI = {           # max |phi32 - phi64| over rows x features, (the table's domain, order, set)
    (MC, 1, "in"): 4.545e-07, (MC, 1, "out"): 1.332e-06, (MC, 1, "limit"): 0.0001678, (MC, 2, "in"): 8.905e-07,
    (MC, 2, "out"): 2.776e-06, (MC, 2, "limit"): 0.0004315, (MC, 3, "in"): 1.537e-06, (MC, 3, "out"): 4.074e-06,
    (MC, 3, "limit"): 0.0006474, (MC, 4, "in"): 1.781e-06, (MC, 4, "out"): 5.372e-06, (MC, 4, "limit"): 0.0008633,
    (MC, 5, "in"): 1.965e-06, (MC, 5, "out"): 6.92e-06, (MC, 5, "limit"): 0.001079, (MC, 6, "in"): 2.815e-06,
    (MC, 6, "out"): 8.218e-06, (MC, 6, "limit"): 0.001295, (MC, 7, "in"): 2.873e-06, (MC, 7, "out"): 9.516e-06,
    (MC, 7, "limit"): 0.001511, (CP, 1, "in"): 3.025e-07, (CP, 1, "out"): 4.055e-07, (CP, 1, "limit"): 7.853e-05,
    (CP, 2, "in"): 5.46e-07, (CP, 2, "out"): 9.092e-07, (CP, 2, "limit"): 0.0001571, (CP, 7, "in"): 2.18e-06,
    (CP, 7, "out"): 3.36e-06, (CP, 7, "limit"): 0.0005497, (AC, 1, "in"): 4.473e-07, (AC, 1, "out"): 5.649e-07,
    (AC, 3, "in"): 1.2e-06, (AC, 3, "out"): 1.72e-06, (AC, 7, "in"): 3.218e-06, (AC, 7, "out"): 3.977e-06,
    (CMC, 1, "in"): 4.545e-07, (CMC, 1, "out"): 1.332e-06, (CMC, 1, "limit"): 0.0001678, (CMC, 2, "in"): 8.905e-07,
    (CMC, 2, "out"): 2.776e-06, (CMC, 2, "limit"): 0.0004315, (CMC, 3, "in"): 1.537e-06, (CMC, 3, "out"): 4.074e-06,
    (CMC, 3, "limit"): 0.0006474, (CMC, 4, "in"): 1.781e-06, (CMC, 4, "out"): 5.372e-06, (CMC, 4, "limit"): 0.0008633,
    (CMC, 5, "in"): 1.965e-06, (CMC, 5, "out"): 6.92e-06, (CMC, 5, "limit"): 0.001079,
}
DEV_F32 = {           # max err of the f32d instantiation (the device's polynomials) against _f32 (libm): what the polynomials alone move
    (MC, "in"): 1.813e-09, (MC, "out"): 5.818e-11, (MC, "limit"): 0, (CP, "in"): 0,
    (CP, "out"): 0, (CP, "limit"): 2.406e-08, (AC, "in"): 1.457e-06, (AC, "out"): 2.87e-05,
    (CMC, "in"): 2.325e-10, (CMC, "out"): 2.324e-10, (CMC, "limit"): 0,
}
PHI_ORDERS = {MC: (1, 2, 3, 4, 5, 6, 7), CP: (1, 2, 7), AC: (1, 3, 7), CMC: (1, 2, 3, 4, 5)}      # register family, generic (the largest admitted: 7 in 2-D, else the wave family's); domain 4's own
PHI_CAP = {(MC, 5): 3e-6}
PHI_CAP_OTHER = 6e-6


def basis_domain(domain):
    return MC if domain == CMC else domain


def bounds(domain):
    """(lo64, hi64, lo32, hi32) of the state space"""
    lo, hi = orc.domain_bounds(basis_domain(domain))
    return lo, hi, lo.astype(F32), hi.astype(F32)


def actions(domain):
    return CMC_ACTIONS if domain == CMC else tuple(range(orc.lib().orc_domain_actions(domain)))


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def _ord(x):
    i = int(F32(x).view(np.int32))
    return i if i >= 0 else -(i & 0x7FFFFFFF)


def _unord(i):
    return np.array([i if i >= 0 else ((-i) | 0x80000000)], dtype=np.uint32).view(F32)[0]


def ulps(x, k):
    """the fp32 value k places above x"""
    return _unord(_ord(x) + k)


def around(x, k=1):
    return [ulps(x, j) for j in range(-k, k + 1)]


def flip(pred, a, b):
    """pred(a) != pred(b), a < b -> the adjacent fp32 pair (below, above) of one flip of pred in between"""
    ia, ib = _ord(a), _ord(b)
    pa = bool(pred(_unord(ia)))
    assert ia < ib and bool(pred(_unord(ib))) != pa, (a, b)
    while ib - ia > 1:
        m = (ia + ib) // 2
        if bool(pred(_unord(m))) == pa:
            ia = m
        else:
            ib = m
    return _unord(ia), _unord(ib)


# ------------------------------------------------------------------------------------------------------------------------------- the tables
def _dim_values(lo64, hi64):
    lo, hi = F32(lo64), F32(hi64)
    w = float(hi64 - lo64)
    out = [("bound", v) for v in (lo, hi, ulps(lo, 1), ulps(hi, -1))]
    out += [("zero", F32(v)) for v in (0.0, -0.0)] + [("zero", SUB), ("zero", -SUB)]
    for p in (0.0, 0.25, 0.5, 0.75, 1.0):
        out += [("scaled", v) for v in around(F32(lo64 + p * w), 2)]
    out += [("out", ulps(lo, -1)), ("out", ulps(hi, 1))]
    out += [("out", F32(lo64 - f * w)) for f in (0.5, 3.0)] + [("out", F32(hi64 + f * w)) for f in (0.5, 3.0)]
    return out


def _generic(domain, bases):
    lo64, hi64, _, _ = bounds(domain)
    rows = []
    for nb, b in enumerate(bases):
        for d in range(len(lo64)):
            for cls, v in _dim_values(lo64[d], hi64[d]):
                # Acrobot's velocities 3 widths out, from a moving base: one RK4 step of dt = 0.2 diverges (angles of 1e5 before the wrap, velocities of
                # 1e11 in f64, other figures in fp32): nothing to compare, and wrap! is a loop.  From rest the same velocities stay moderate and are kept
                if domain == AC and d >= 2 and nb > 0 and abs(float(v)) > 2.0 * hi64[d]:
                    continue
                s = list(b)
                s[d] = v
                rows.append(("%s:d%d" % (cls, d), s))
    return rows


def _mc_rows(domain):
    force = 0.0015 if domain == CMC else 0.001
    acts = (-1.0, 0.7, 1.0) if domain == CMC else (-1.0, 0.0, 1.0)
    dv = lambda x, a: force * a - 0.0025 * np.cos(3.0 * float(x))
    rows = _generic(domain, [(-0.5, 0.0), (0.3, 0.03), (-1.0, -0.05)])
    lo64, hi64, _, _ = bounds(domain)
    xs = [F32(lo64[0] + p * 1.8) for p in (0.0, 0.25, 0.5, 0.75, 1.0)] + [F32(0.0), F32(-0.0), SUB]
    vs = [F32(lo64[1] + p * 0.14) for p in (0.0, 0.25, 0.5, 0.75, 1.0)] + [F32(-0.0), SUB, -SUB]
    rows += [("cross", (x, v)) for x in xs for v in vs]
    for t in (np.pi / 12, -np.pi / 12, np.pi / 4, -np.pi / 4):
        rows += [("quadrant", (x, v)) for x in around(F32(t), 2) for v in (F32(0.0), F32(0.03))]
    for a in acts:
        for k in range(-2, 3):
            for x0 in (F32(0.55), F32(0.58)):
                rows.append(("goal:a%g" % a, (x0, F32(float(ulps(F32(0.6), k)) - float(x0) - dv(x0, a)))))
            x0 = F32(-1.15)
            rows.append(("wall:a%g" % a, (x0, F32(float(ulps(F32(-1.2), k)) - float(x0) - dv(x0, a)))))
            for x0 in (F32(-0.5), F32(0.3)):
                for edge in (0.07, -0.07):
                    rows.append(("vclip:a%g" % a, (x0, F32(float(ulps(F32(edge), k)) - dv(x0, a)))))
    rows += [("goal:clipped", (x, F32(0.07))) for x in around(F32(F32(0.6) - F32(0.07)), 3)]       # v' = 0.07f exactly, x + 0.07f around 0.6f
    rows += [("wall:clipped", (x, F32(-0.07))) for x in around(F32(F32(-1.2) + F32(0.07)), 3)]
    rows += [("start", (x, v)) for x in around(F32(0.6), 1) for v in (0.0, -0.07, 0.07, -0.03)]
    rows.append(("limit", (F32(lo64[0] - 1000.0 * 1.8), 0.01)))
    rows.append(("limit", (0.1, F32(hi64[1] + 1000.0 * 0.14))))
    return rows


def _neg(s):
    return tuple(-F32(v) for v in s)


def _cp_rows():
    rows = _generic(CP, [(0.0, 0.0, 0.0, 0.0), (0.5, -1.0, 0.05, 0.7)])
    raw = lambda s, a: orc.domain_step_raw(CP, np.array(s, dtype=F32), a, "f64")

    def crafted(cls, base, vary, out, a, lo, hi, bound, far):
        """the positive side: vary base[vary] in [lo, hi] until raw[out] passes bound; the negative side is the mirror image under the other action"""
        def st(v):
            s = list(base)
            s[vary] = v
            return tuple(F32(x) for x in s)
        below, above = flip(lambda v: raw(st(v), a)[out] >= bound, lo, hi)
        for tag, v in (("near", below), ("near", above), ("far", F32(below - far)), ("far", F32(above + far))):
            rows.append(("%s:%s:+d%d" % (cls, tag, out), st(v)))
            rows.append(("%s:%s:-d%d" % (cls, tag, out), _neg(st(v))))
    crafted("clip", (0.0, 0.0, 0.0, 0.0), 1, 1, 1, 5.0, 6.0, np.nextafter(6.0, 7.0), 0.01)          # x' over 6 (clip acts above the bound)
    crafted("clip", (0.0, 0.0, 0.0, 0.0), 3, 3, 0, 1.0, 2.0, np.nextafter(2.0, 3.0), 0.01)          # theta' over 2
    crafted("thr", (0.0, 1.0, 0.0, 0.0), 0, 0, 1, 2.0, 2.39, 2.4, 0.01)                              # x reaches 2.4 (terminal at >=)
    crafted("thr", (0.0, 0.0, 0.0, 0.5), 2, 2, 0, 0.1, 0.209, TW64, 0.005)                           # theta reaches 12 degrees
    for v in around(F32(2.4), 1):
        rows += [("onthr:d0", (v, 0.3, 0.01, -0.2)), ("onthr:d0", _neg((v, 0.3, 0.01, -0.2)))]
    for v in around(F32(TW64), 1):
        rows += [("onthr:d2", (0.2, 0.3, v, -0.2)), ("onthr:d2", _neg((0.2, 0.3, v, -0.2)))]
    lo64, hi64, _, _ = bounds(CP)
    rows.append(("limit", (0.0, 0.0, F32(hi64[2] + 1000.0 * 2 * TW64), 0.0)))
    rows.append(("limit", (F32(lo64[0] - 1000.0 * 4.8), 0.0, 0.0, 0.0)))
    return rows


def _ac_rows():
    rows = _generic(AC, [(0.0, 0.0, 0.0, 0.0), (1.0, -2.0, 3.0, -5.0)])
    raw = lambda s, a: orc.domain_step_raw(AC, np.array(s, dtype=F32), a, "f64")
    for cls, s in (("wrap:t1", (3.1, 0.0, 2.0, 0.0)), ("wrap:t2", (0.0, 3.1, 0.0, 3.0)), ("wrap:both", (3.1, 3.1, 2.0, 3.0)), ("wrap:both", (3.1, -3.1, 2.0, -3.0))):
        rows += [(cls, tuple(F32(v) for v in s)), (cls, _neg(s))]
    for v in around(PI32, 1):
        for s in ((v, 0.5, 0.0, 0.0), (0.5, v, 0.0, 0.0), (v, v, 0.3, -0.3), (v, -v, -1.0, 2.0)):
            rows += [("pi", tuple(F32(x) for x in s)), ("pi", _neg(s))]

    def crafted(cls, base, vary, pred, a, lo, hi, far):
        def st(v):
            s = list(base)
            s[vary] = v
            return tuple(F32(x) for x in s)
        below, above = flip(lambda v: pred(raw(st(v), a)), lo, hi)
        for tag, v in (("near", below), ("near", above), ("far", F32(below - far)), ("far", F32(above + far))):
            rows.append(("%s:%s:+" % (cls, tag), st(v)))
            rows.append(("%s:%s:-" % (cls, tag), _neg(st(v))))
    crafted("vclip:d2", (0.3, 0.2, 0.0, 0.0), 3, lambda r: r[2] > 4.0 * np.pi, 2, 30.0, 34.0, 0.05)      # (gravity brakes theta1' = 4 pi within one step:
    crafted("vclip:d3", (0.3, 0.2, 0.0, 0.0), 3, lambda r: r[3] > 9.0 * np.pi, 1, 26.0, 28.0, 0.05)      #  the second link's swing is what carries it over)
    line = lambda r: np.cos(r[0]) + np.cos(r[0] + r[1]) < -1.0
    crafted("line", (0.0, 0.0, 0.0, 0.0), 0, line, 1, 1.5, 2.6, 0.01)
    crafted("line", (0.0, 1.0, 0.5, -0.5), 0, line, 2, 0.8, 2.4, 0.01)
    return rows


@functools.lru_cache(maxsize=None)
def table(domain):
    raw = {MC: lambda: _mc_rows(MC), CMC: lambda: _mc_rows(CMC), CP: _cp_rows, AC: _ac_rows}[domain]()
    rows, seen = [], set()
    for name, s in raw:
        s = np.array(s, dtype=F32)
        assert np.all(np.isfinite(s)), (name, s)
        if s.tobytes() not in seen:
            seen.add(s.tobytes())
            rows.append((name, s))
    if len(rows) % 64 == 0:                                       # a partial wave and a partial block: one more row, the default start's neighbour
        rows.append(("bound:pad", np.array(orc.domain_reset(basis_domain(domain), "f32"), dtype=F32) + F32(0.125)))
    S = np.ascontiguousarray(np.stack([s for _, s in rows], axis=1))
    names = np.array([n for n, _ in rows])
    S.setflags(write=False)
    names.setflags(write=False)
    return S, names


def classes(domain):
    return sorted({n.split(":")[0] for n in table(domain)[1]})


SETS = ("in", "out", "limit")


def row_set(domain):
    """(n,) of str: `limit` the rows at the ABI's admission limit (1000 widths out: s~ carries 6e-5 of rounding), `in` every component within
    [lo32, hi32], `out` the rest (1 ulp .. 3 widths outside)"""
    names = table(domain)[1]
    lim = np.array([n.split(":")[0] == "limit" for n in names])
    return np.where(lim, "limit", np.where(in_range(domain), "in", "out"))


def sets(domain):
    """[(name, mask)] of the non-empty row sets"""
    rs = row_set(domain)
    return [(w, rs == w) for w in SETS if np.any(rs == w)]


def in_range(domain, S=None):
    """(n,) bool: every component within [lo32, hi32]"""
    _, _, lo, hi = bounds(domain)
    S = table(domain)[0] if S is None else S
    return np.all((S >= lo[:, None]) & (S <= hi[:, None]), axis=0)


# ------------------------------------------------------------------------------------------------------------------------------- the answers
def _step(domain, s, a, prec):
    if domain == CMC:
        return orc.cmc_step(s, a, prec)
    raw = orc.domain_step_raw(domain, s, a, prec)
    assert np.all(np.isfinite(raw)) and (domain != AC or np.all(np.abs(raw[:2]) < 1e4)), (domain, s, a, raw)      # (before the step: wrap! is a loop)
    ns, r, t = orc.domain_step(domain, s, a, prec)
    return ns, r, t, raw


@functools.lru_cache(maxsize=None)
def answers(domain, prec):
    S, _ = table(domain)
    acts = actions(domain)
    dt = F64 if prec == "f64" else F32
    D, n = S.shape
    out = dict(next=np.zeros((n, len(acts), D), dtype=dt), raw=np.zeros((n, len(acts), D), dtype=dt), reward=np.zeros((n, len(acts)), dtype=dt),
               term=np.zeros((n, len(acts)), dtype=bool))
    for i in range(n):
        for j, a in enumerate(acts):
            out["next"][i, j], out["reward"][i, j], out["term"][i, j], out["raw"][i, j] = _step(domain, S[:, i].astype(dt), a, prec)
    for v in out.values():
        v.setflags(write=False)
    return out


def err(domain, got, want):
    """|got - want| / (1 + |want|) per component (..., D); Acrobot's angles on the circle"""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    d = got - want
    if domain == AC:
        d = d.copy()
        d[..., :2] = (d[..., :2] + np.pi) % (2.0 * np.pi) - np.pi
    return np.abs(d) / (1.0 + np.abs(want))


def predicate(domain, nxt, prec="f32d"):
    """the domain's terminal predicate on next states (m, D), in the instantiation's own arithmetic"""
    nxt = np.asarray(nxt)
    return np.array([orc.domain_is_terminal(basis_domain(domain), s, prec) for s in nxt.reshape(-1, nxt.shape[-1])]).reshape(nxt.shape[:-1])


def reward_of(domain, term):
    term = np.asarray(term, dtype=bool)
    return np.where(term, F32(-1.0), F32(0.0)) if domain == CP else np.where(term, F32(0.0), F32(-1.0))


def margin(domain):
    """f64's deciding quantity per (row, action): the decision is term = (margin >= 0) for MountainCar, (margin <= 0) for CartPole (the smallest of
    its four), (margin < 0) for Acrobot; |margin| is how far the row is from the other decision"""
    a = answers(domain, "f64")
    if domain in (MC, CMC):
        return a["raw"][..., 0] - 0.6
    if domain == CP:
        r = a["raw"]
        m = np.stack([r[..., 0] + 2.4, 2.4 - r[..., 0], r[..., 2] + TW64, TW64 - r[..., 2]], axis=-1)
        return np.min(m, axis=-1)
    n = a["next"]
    return np.cos(n[..., 0]) + np.cos(n[..., 0] + n[..., 1]) + 1.0


def step_bar(domain, which):
    return 4.0 * F32_STEP[(domain, which)]


def row_bars(domain):
    """(n,) the transition bar of every row"""
    return np.array([step_bar(domain, w) for w in row_set(domain)])


def band(domain):
    """(n,) how close to 0 f64's deciding quantity may be for the fp32 decision to go either way: the row's bar times the size of the quantity"""
    b = row_bars(domain)
    return {MC: 1.6 * b, CMC: 1.6 * b, CP: 3.4 * b, AC: 3.0 * (1.0 + np.pi) * b + 4e-7}[domain]


def decided(domain):
    """(n, A) bool: f64's decision stands clear of its threshold"""
    return np.abs(margin(domain)) > band(domain)[:, None]


# ------------------------------------------------------------------------------------------------------------------------------- the bases
@functools.lru_cache(maxsize=None)
def phi(domain, order, prec):
    """(F, n) features of the table's rows; domain 4 has domain 0's basis"""
    S, _ = table(domain)
    return np.stack([orc.fourier_project(basis_domain(domain), order, S[:, i], prec) for i in range(S.shape[1])], axis=1)


def phi_bar(domain, order, which):
    b = 4.0 * F32_PHI[(domain, order, which)]
    return min(b, PHI_CAP.get((basis_domain(domain), order), PHI_CAP_OTHER)) if which == "in" else b


def phi_row_bars(domain, order):
    return np.array([phi_bar(domain, order, w) for w in row_set(domain)])


def tile_configs(domain):
    """(n_tilings, tiles_per_dim): the smallest and largest n_tilings of tests/golden/create_admission.json's grid, and 16, which the library also
    instantiates (model_list.hpp) though the grid has no such point; tiles_per_dim has no axis there -- its admitted range is [1, 64] -- so 1 (u = 0
    everywhere), 2 and 64 on the 2-D domain; 1, 2 and 32 on the 4-D ones (64^4 cells x 8 tilings x 3 actions is a 1.6 GB table even when shared)"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "create_admission.json")) as f:
        T = dict(json.load(f)["grid"])["n_tilings"]
    lo, hi = min(T), max(T)
    return ((lo, 1), (lo, 2), (hi, 64), (16, 8)) if domain == MC else ((lo, 1), (lo, 2), (hi, 32), (16, 8))


@functools.lru_cache(maxsize=None)
def tile_table(domain, T, B):
    """(D, m) states for tile_indices: per dimension and tiling, the states that put s~ (B - 1) + off_t on an integer (+-1 ulp), then the transition
    table's bound, scaled, out and limit rows"""
    lo64, hi64, _, _ = bounds(domain)
    D = len(lo64)
    base = np.array(orc.domain_reset(domain, "f32"), dtype=F32)
    rows = []
    for i in range(D):
        for t in range(T):
            off = ((t * (2 * i + 1)) % T) / T
            for k in sorted({1, max(1, (B - 1) // 2), B - 1}):
                if B == 1:
                    continue
                sc = (k - off) / (B - 1)
                for v in around(F32(lo64[i] + sc * (hi64[i] - lo64[i])), 1):
                    s = base.copy()
                    s[i] = v
                    rows.append(s)
    S, names = table(domain)
    keep = np.array([n.split(":")[0] in ("bound", "scaled", "out", "limit", "zero") for n in names])
    out = np.concatenate([np.array(rows, dtype=F32).reshape(-1, D).T, S[:, keep]], axis=1)
    out = np.ascontiguousarray(out[:, np.unique(out.view(np.uint32), axis=1, return_index=True)[1]])
    if out.shape[1] % 64 == 0:                                    # one more row, never one fewer: the default start's neighbour
        out = np.ascontiguousarray(np.concatenate([out, (base + F32(0.125))[:, None]], axis=1))
    out.setflags(write=False)
    return out


def tile_numpy(domain, T, B, S):
    """rsrl_amd/csrc/models.hpp:124-125 in plain float32 numpy: s~ = (s - lo) / (hi - lo); u = s~ (B - 1); off_i(t) = ((t (2i + 1)) mod T) / T;
    cell = clamp((int)floor(u + off), 0, B - 1); idx(t) = t B^D + sum_i cell_i B^i  -> (T, m) int32"""
    _, _, lo, hi = bounds(domain)
    D, m = S.shape
    idx = np.zeros((T, m), dtype=np.int64)
    for t in range(T):
        lin = np.zeros(m, dtype=np.int64)
        for i in range(D):
            sc = ((S[i] - lo[i]).astype(F32) / F32(hi[i] - lo[i])).astype(F32)
            u = (sc * F32(B - 1)).astype(F32)
            off = F32(F32((t * (2 * i + 1)) % T) / F32(T))
            cell = np.clip(np.floor((u + off).astype(F32)).astype(np.int64), 0, B - 1)
            lin += cell * B ** i
        idx[t] = t * B ** D + lin
    return idx.astype(np.int32)
