"""Crafted action-value vectors for the policy / Enumerable code of device_core.hpp (find_max, argmaxima_mask, argmax_first, kth_set_bit,
greedy_sample, softmax_probs, sample_probs, policy_sample / _mode / _probs), and the reference's f64 answers on them.

table(A) / table(A, bf16=True) -> (Q (n, A) float32, groups (n,) of str): a FIXED list (no random numbers), a few hundred vectors per A, built from
an alphabet of fp32 (bf16-representable) values.  Groups:
  tie       exact ties: pairs, triples, all-equal, +0 / -0, ties below the maximum
  chain     near-tie chains around argmaxima's 1e-7 band (utils.rs:6-21), every order: the reference does not raise its running maximum on a
            near-tie, so the answer depends on the order.  x, x + 1 ulp, x + 2 ulp with x in [0.5, 1) (one ulp = 5.96e-8 inside, two outside), at
            x = 1 (one ulp = 1.19e-7 outside), at |x| ~ 1e-3 (1 ulp = 1.16e-10: also x, x + 500 ulp, x + 1000 ulp -- 5.8e-8 and 1.16e-7).
            bf16: an ulp is below 1e-7 only for |x| < 1.2e-5, so the chains sit at 2^-17 (one ulp = 5.96e-8) and 2^-20 (6 and 14 ulps)
  mag       magnitudes: +-MAX, its predecessor, +-1e30, the smallest normal, the smallest subnormals, 5e-8, 1.5e-7, 0
  nonfinite -inf, +inf, NaN beside finite values in every position (position 0 goes through the v_med3_f32 fold), two at a time, -inf beside
            -MAX, all -inf, all NaN, all +inf
  spread    (max - min) / tau = 0, 1, 87, 88.5, 100, 1e4 for each tau of TAUS (the vector is (0, -s tau, ..): exact at 0, rounded once elsewhere)

Every expectation is the oracle's f64 instantiation (pinned to the reference's own tables by tests/test_oracle_golden.py) -- except where the reference
panics: the vectors without any maximum (every entry NaN or -inf; utils.rs:70-76 "No valid maxima").  There the expectation is the device's stated rule
(device_core.hpp greedy_sample / policy_probs), written out below: a uniform pick mulhi(x, A) among ALL actions, and a greedy probability part of zero
(Greedy: all 0; EpsilonGreedy: eps / A each).  find_min, expected_value and the policy's Function<(S, A)> are a few lines of numpy f64 after core.rs."""
import itertools

import numpy as np

GREEDY, EGREEDY, SOFTMAX, RANDOM = 0, 1, 2, 3
TAUS = (1e-7, 1e-3, 0.05, 0.7, 1.0, 50.0, 1e6)
EPSILON = 0.3
SPREADS = (0.0, 1.0, 87.0, 88.5, 100.0, 1e4)
FLT_MAX = np.float32(3.4028234663852886e38)
BAND = 2e-6          # softmax samples: u within BAND of a cumulative f64 probability is left out (four probabilities at the 3e-7 bar + the fp32 running sum)


def _bf16(x):
    """round-to-nearest-even to bf16, as a float32"""
    u = np.array(x, dtype=np.float32).reshape(1).view(np.uint32)
    if np.isnan(np.float32(x)):
        return np.float32(np.nan)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & np.uint32(0xFFFF0000)
    return u.view(np.float32)[0]


def _ulps(x, k, bf16):
    """x moved by k units in the last place of its format (fp32, or bf16: 2^16 fp32 steps), away from zero for k > 0"""
    u = np.array(x, dtype=np.float32).reshape(1).view(np.uint32).astype(np.int64)
    return (u + k * (0x10000 if bf16 else 1)).astype(np.uint32).view(np.float32)[0]


def _dropped(A, bf16):
    """vectors the generator below would produce but the table leaves out: the f64 and the fp32 formulation do not make the same discrete decision on
    them, so no fp32 kernel can be held to the reference there (tests/test_policy_edges_cpu.py asserts that nothing of this kind is left).  All four
    are Softmax modes: argmax_first's 1e-7 test on probabilities that differ by about 1e-7 (0.25 +- 4e-8 at tau = 0.7; 0.5 +- 5e-8 at tau = 50)"""
    if A == 4 and not bf16:
        one, a, b = np.float32(1.0), _ulps(1.0, 1, False), _ulps(1.0, 2, False)
        return [(one, a, a, b), (one, a, b, a), (one, b, a, a)]
    if A == 2 and bf16:
        return [(_bf16(-100.0 * 1e-7), np.float32(0.0))]
    return []


def _build(A, bf16):
    r = _bf16 if bf16 else np.float32
    mx = r(3.3895313892515355e38) if bf16 else FLT_MAX                 # the format's largest finite value
    rows = []

    def add(group, v):
        assert len(v) == A
        rows.append((group, tuple(np.float32(x) for x in v)))

    lo, hi, fill = r(-2.0), r(1.0), [r(0.25), r(-1.0), r(3.0)]
    idx = range(A)
    # ---- exact ties
    for n in range(2, A + 1):
        for sub in itertools.combinations(idx, n):
            add("tie", [hi if i in sub else lo for i in idx])                           # at the maximum
            if n < A:
                top = min(set(idx) - set(sub))
                add("tie", [lo if i in sub else (r(4.0) if i == top else r(-3.0)) for i in idx])     # below the maximum
    for v in (0.0, -0.0, 1.0, -1.0, 1e30, -1e30, float(mx), -float(mx), 1e-45 if not bf16 else 9.183549615799121e-41):
        add("tie", [r(v)] * A)
    for sub in itertools.combinations(idx, 1):
        add("tie", [r(-0.0) if i in sub else r(0.0) for i in idx])                      # +0 == -0
        add("tie", [r(0.0) if i in sub else r(-0.0) for i in idx])
    # ---- near-tie chains, every order
    if bf16:
        chains = [(r(2.0 ** -17), (0, 1, 2)), (-r(2.0 ** -17), (0, 1, 2)), (r(2.0 ** -20), (0, 6, 14)), (r(2.0 ** -20), (0, 1, 2)), (r(1.5 * 2.0 ** -18), (0, 3, 4))]
    else:
        chains = [(r(0.5), (0, 1, 2)), (r(0.75), (0, 1, 2)), (r(0.99999994), (0, 1, 2)), (r(-0.75), (0, 1, 2)), (r(1.0), (0, 1, 2)),
                  (r(1e-3), (0, 1, 2)), (r(1e-3), (0, 500, 1000)), (r(-1e-3), (0, 500, 1000)), (r(1e-3), (0, 859, 863))]
    for x, ks in chains:
        c = [_ulps(x, k, bf16) for k in ks]
        if A == 2:
            sets = [(c[0], c[1]), (c[0], c[2]), (c[1], c[2])]
        elif A == 3:
            sets = [tuple(c)]
        else:
            sets = [tuple(c) + (lo,), tuple(c) + (c[1],)]
        for s in sets:
            for p in sorted(set(itertools.permutations(s))):
                add("chain", p)
    # ---- magnitudes: every ordered pair of the alphabet, the other positions filled with moderate values, the pair's place rotating
    sub_min = 9.183549615799121e-41 if bf16 else 1e-45
    alpha = [float(mx), -float(mx), float(_ulps(mx, -1, bf16)), 1e30, -1e30, 1.1754943508222875e-38, sub_min, -sub_min, 5e-8, 1.5e-7, 0.0]
    alpha = [r(v) for v in alpha]
    for i, j in itertools.permutations(range(len(alpha)), 2):
        v = fill[:A - 2]
        at = (i + j) % (A - 1)
        v = v[:at] + [alpha[i], alpha[j]] + v[at:]
        add("mag", v)
    # ---- non-finite values
    ninf, pinf, nan = r(-np.inf), r(np.inf), r(np.nan)
    for nf in (ninf, pinf, nan):
        for rest in (fill, [hi, hi, hi], [-mx, -mx, -mx], [mx, r(0.0), -mx]):
            for at in idx:
                v = list(rest[:A - 1])
                add("nonfinite", v[:at] + [nf] + v[at:])
    for a, b in itertools.product((ninf, pinf, nan), repeat=2):                         # two at a time; the rest (if any) finite
        for at in itertools.combinations(idx, 2):
            v = [r(0.25), r(-1.0)]
            add("nonfinite", [a if i == at[0] else b if i == at[1] else v.pop() for i in idx])
    for n in range(1, A):                                                               # -inf beside -MAX
        for sub in itertools.combinations(idx, n):
            add("nonfinite", [-mx if i in sub else ninf for i in idx])
    for v in (ninf, nan, pinf):
        add("nonfinite", [v] * A)
    for at in idx:                                                                      # no maximum: NaN and -inf mixed
        add("nonfinite", [nan if i == at else ninf for i in idx])
    # ---- softmax spreads
    for tau in TAUS:
        for s in SPREADS:
            d = r(-s * tau)
            for v in ([r(0.0), d, r(d / 2), r(0.0)][:A], [d, r(d / 2), d, r(0.0)][:A] if A > 2 else [d, r(0.0)]):
                add("spread", v)
    seen, out = {np.array(v, dtype=np.float32).tobytes() for v in _dropped(A, bf16)}, []
    for g, v in rows:                                                                   # one copy of each vector (bit patterns: -0 and NaN kept apart)
        key = np.array(v, dtype=np.float32).tobytes()
        if key not in seen:
            seen.add(key)
            out.append((g, v))
    return np.array([v for _, v in out], dtype=np.float32), np.array([g for g, _ in out])


_CACHE = {}


def table(A, bf16=False):
    if (A, bf16) not in _CACHE:
        Q, g = _build(A, bf16)
        Q.setflags(write=False)
        _CACHE[(A, bf16)] = (Q, g)
    return _CACHE[(A, bf16)]


def moderate(Q):
    """rows the driver-loop legs use: finite and of moderate size (0 * delta stays 0 through an update with lr = 0), no -0 (w + 0 must keep w's bits)"""
    with np.errstate(invalid="ignore"):
        return np.all(np.isfinite(Q) & (np.abs(Q) <= 1e4) & ~((Q == 0) & np.signbit(Q)), axis=1)


def is_bf16(Q):
    u = np.ascontiguousarray(Q, dtype=np.float32).view(np.uint32)
    return np.all((u & 0xFFFF) == 0)


# ----------------------------------------------------------------------------------------------------------------- the reference's answers (f64)
def no_maximum(q):
    """every entry NaN or -inf: argmaxima's set is empty (the reference panics in Greedy::sample; the device's rule applies)"""
    q = np.asarray(q, dtype=np.float64)
    return bool(np.all(np.isnan(q) | (q == -np.inf)))


def mulhi(x, n):
    return (int(x) * int(n)) >> 32


def ref_probs(orc, policy, q, eps=EPSILON, tau=1.0):
    q = np.asarray(q, dtype=np.float64)
    A = len(q)
    if no_maximum(q) and policy in (GREEDY, EGREEDY):
        return np.zeros(A) if policy == GREEDY else np.full(A, eps / A)
    return orc.policy_probs(policy, q, eps=eps, tau=tau, prec="f64")


def ref_sample(orc, policy, q, x, eps=EPSILON, tau=1.0):
    q = np.asarray(q, dtype=np.float64)
    if no_maximum(q) and policy in (GREEDY, EGREEDY):
        if policy == EGREEDY and (int(x[0]) >> 8) < orc.lib().orc_eps_threshold(eps):
            return mulhi(x[1], len(q))
        return mulhi(x[2], len(q))
    return orc.policy_sample(policy, q, x, eps=eps, tau=tau, prec="f64")


def ref_mode(orc, policy, q, tau=1.0):
    return orc.policy_mode(policy, np.asarray(q, dtype=np.float64), tau=tau, prec="f64")


def find_min(q):
    """core.rs:86-94: fold (i, x): if acc.1 < x {acc} else {(i, x)} -- ties and unordered comparisons go to the LAST index"""
    bi, bv = 0, q[0]
    for i in range(1, len(q)):
        if not (bv < q[i]):
            bi, bv = i, q[i]
    return bi, bv


def find_max(q):
    """core.rs:96-105, for the dtype given (the helper's own restatement; the oracle's is orc.find_max)"""
    bi, bv = 0, q[0]
    for i in range(1, len(q)):
        if not (bv > q[i]):
            bi, bv = i, q[i]
    return bi, bv


def expected_value(q, p):
    """core.rs:107-116: fold 0.0, acc + x * p, in f64 -> (the sum, sum |x p|)"""
    q, p = np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64)
    acc = mag = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for x, w in zip(q, p):
            acc = acc + x * w
            mag = mag + abs(x * w)
    return acc, mag


def prob_sa(orc, policy, q, a, eps=EPSILON, tau=1.0):
    """Function<(S, A)> of the policy: P(a | s); Softmax's is the raw action value (softmax.rs:84-92)"""
    if policy == SOFTMAX:
        return float(np.asarray(q, dtype=np.float64)[a])
    return float(ref_probs(orc, policy, q, eps, tau)[a])


def prob_rows(A):
    """a few probability rows for expected_value, zeros among them; dyadic and summing to 1, so that every product with a normal number is exact and
    no partial sum leaves the range of the vector"""
    rows = {2: [(0.5, 0.5), (1, 0), (0, 1), (0.25, 0.75)],
            3: [(0.5, 0.25, 0.25), (1, 0, 0), (0, 0, 1), (0.25, 0, 0.75), (0.125, 0.375, 0.5)],
            4: [(0.25, 0.25, 0.25, 0.25), (1, 0, 0, 0), (0, 0, 0, 1), (0.5, 0, 0.5, 0), (0.125, 0.375, 0.25, 0.25)]}[A]
    return [np.asarray(r, dtype=np.float32) for r in rows]


def softmax_in_band(orc, q, x, tau):
    """True when u = (x.z >> 8) / 2^24 lies within BAND of a cumulative f64 probability: the sample is then left out of the exact comparison"""
    p = orc.policy_probs(SOFTMAX, np.asarray(q, dtype=np.float64), tau=tau, prec="f64")
    u = (int(x[2]) >> 8) / 16777216.0
    with np.errstate(invalid="ignore", over="ignore"):
        cum = np.cumsum(p)
    return bool(np.any(np.abs(cum - u) <= BAND))
