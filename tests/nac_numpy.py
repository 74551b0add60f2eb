"""NAC with the Beta policy and a SARSA critic over the stable compatible basis (RSRL_NAC on RSRL_CONTINUOUS_MOUNTAIN_CAR, examples/nac_beta.rs)
restated in numpy.  Shared by the CPU and GPU tests; the score, the parameters, the sampler and Philox are tests/beta_numpy.py's.

  psi(s, a)      SCB::project (fa/linear.rs:79-103): grad_log pi(a|s) (policies/beta.rs:119-129) chained with phi(s), 3F features
                     [ g_a sigma(x_a) phi ; g_b sigma(x_b) phi ; phi ]
  Q(s, a)        <w, psi(s, a)> (linear.rs:253-261)
  sarsa_handle   SARSA::handle (control/td/sarsa.rs:53-75) with SGD (linear.rs:277-288); the caller supplies the inner draw na
  nac_handle     NAC::handle(()) (control/nac.rs:47-59): g = w[0 .. 2F-1], norm = max(sqrt(sum g^2), 1e-3), the columns += (alpha / norm) g
  nac_handle_f32 the same in float32 in the DEVICE's operation order: the squares rounded and added in index order, sqrt and the division
                 correctly rounded, one fused multiply-add per element (fma32 below: numpy has none)

Everything but nac_handle_f32 is f64, in the reference's form."""
import numpy as np

from tests import beta_numpy as bn

BLK_INNER = 2
RULE_SEED = 17         # the ctx seed of the GPU rule test: chosen on the CPU (tests/test_nac_beta_cpu.py) so that critic_after names at most 3 of 67 learners
MARGIN = 2e-5         # tests/test_gpu_tdac_beta.py's: an acceptance test this close to its boundary (in f64) may be decided the other way in f32


def coefs(W, phi, a):
    """(c_a, c_b) = (g_a sigma(x_a), g_b sigma(x_b)) at the features phi and the action a, W (F, 2) the policy's columns"""
    W, phi = np.asarray(W, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    xa, xb = float(phi @ W[:, 0]), float(phi @ W[:, 1])
    alpha, beta = bn.beta_params(xa, xb)
    ga, gb = bn.beta_score(alpha, beta, a)
    return float(ga * bn.softplus_grad(xa)), float(gb * bn.softplus_grad(xb))


def psi(W, phi, a):
    ca, cb = coefs(W, phi, a)
    phi = np.asarray(phi, dtype=np.float64)
    return np.concatenate([ca * phi, cb * phi, phi])


def q_value(w, W, phi, a):
    return float(np.asarray(w, dtype=np.float64).ravel() @ psi(W, phi, a))


def sarsa_handle(w, W, phi_s, a, r, phi_n, na, term, gamma, lr):
    """one transition -> (delta, w'); na: the critic's own draw at s' (not read on a terminal transition)"""
    w = np.asarray(w, dtype=np.float64).ravel()
    q = q_value(w, W, phi_s, a)
    delta = r - q if term else r + gamma * q_value(w, W, phi_n, na) - q
    return delta, w + lr * delta * psi(W, phi_s, a)


def nac_handle(w, W, alpha):
    """-> (W', norm), f64"""
    w, W = np.asarray(w, dtype=np.float64).ravel(), np.asarray(W, dtype=np.float64)
    F = W.shape[0]
    g = w[:2 * F]
    norm = max(float(np.sqrt(np.sum(g * g))), 1e-3)
    out = W.copy()
    out[:, 0] += alpha / norm * g[:F]
    out[:, 1] += alpha / norm * g[F:]
    return out, norm


def fma32(a, b, c):
    """the float32 fused multiply-add, correctly rounded, on arrays of float32 values: the product is exact in f64, TwoSum gives the f64 sum's
    error, and where the f64 sum is exactly halfway between two float32 neighbours the error's sign decides (else rounding the f64 sum is exact:
    the sum lies at least one f64 ulp from the midpoint, the error within half of one)"""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    rd = r.astype(np.float64)
    other = np.nextafter(r, np.where(s > rd, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float64)
    tie = (rd != s) & (np.abs(s - rd) == np.abs(other - s))
    hi, lo = np.maximum(rd, other), np.minimum(rd, other)
    return np.where(tie & (err > 0), hi, np.where(tie & (err < 0), lo, rd)).astype(np.float32)


def nac_handle_f32(w, W, alpha):
    """float32, the device's operation order -> (W' (F, 2) float32, norm float32)"""
    w, W = np.asarray(w, dtype=np.float32).ravel(), np.asarray(W, dtype=np.float32)
    F = W.shape[0]
    g = w[:2 * F]
    ss = np.float32(0.0)
    for j in range(2 * F):
        ss = np.float32(ss + np.float32(g[j] * g[j]))
    norm = np.maximum(np.sqrt(ss, dtype=np.float32), np.float32(1e-3))
    scale = np.float32(np.float32(alpha) / norm)
    out = np.empty_like(W)
    out[:, 0] = fma32(scale, g[:F], W[:, 0])
    out[:, 1] = fma32(scale, g[F:], W[:, 1])
    return out, np.float32(norm)


def handle_case(order, N=67, rounds=3, gamma=0.95, lr=0.01):
    """the GPU rule test's inputs, built as tests/beta_numpy.handle_case builds its own: per learner random policy columns with |x| <= 3 (sum |w| <= 3
    per column, |phi| <= 1) and a random critic w with sum |w| <= 3; `rounds` rounds of transitions stepped by cmc_step on 2a - 1 from random states and
    random actions in [0, 1] -- learners 0 and 1 act 0 and 1 exactly, which the score clamps -- a quarter more of them flagged terminal"""
    rng = np.random.default_rng(500 + order * 10 + 28)
    lo, hi = np.array([bn.X_BOUNDS[0], bn.V_BOUNDS[0]]), np.array([bn.X_BOUNDS[1], bn.V_BOUNDS[1]])
    F = (order + 1) ** 2
    init = []
    for _ in range(N):
        W = rng.normal(0.0, 1.0, size=(F, 2))
        W *= rng.uniform(0.5, 3.0, size=2) / np.abs(W).sum(axis=0)
        w = rng.normal(0.0, 1.0, size=3 * F)
        w *= rng.uniform(0.5, 3.0) / np.abs(w).sum()
        init.append((w.astype(np.float32), W.astype(np.float32)))
    out = []
    for _ in range(rounds):
        frm = rng.uniform(lo, hi, size=(N, 2)).T.astype(np.float32)
        a = rng.uniform(0.0, 1.0, size=N).astype(np.float32)
        a[0], a[1] = 0.0, 1.0
        nxt, rew, term = np.zeros_like(frm), np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.uint8)
        for i in range(N):
            ns, r, t = bn.cmc_step(frm[:, i], 2.0 * float(a[i]) - 1.0)
            nxt[:, i], rew[i], term[i] = np.asarray(ns, dtype=np.float32), np.float32(r), bool(t)
        term = (term.astype(bool) | (rng.random(N) < 0.25)).astype(np.uint8)
        out.append((frm, a, rew, nxt, term))
    return dict(init=init, rounds=out, F=F, params=dict(gamma=gamma, lr=lr))


def critic_after(case, seed, phi_s_rounds, phi_n_rounds, env_offset=0):
    """SARSA::handle over every round of `case` in f64, from the features given (phi_*_rounds[k]: (F, N), the `from` and `to` states' of round k -- the
    device's own f32 projection in the GPU test).  The inner draw of learner i at round k is bn.beta_sample(seed, env_offset + i, k, BLK_INNER, ...) at
    the f64 parameters.  -> (w (N, 3F) after the last round, [delta (N,) per round], skipped (N,): a learner whose inner draw of a non-terminal
    transition evaluated an acceptance test within MARGIN of its boundary)"""
    p = case["params"]
    N = len(case["init"])
    w = [x.astype(np.float64) for x, _ in case["init"]]
    Ws = [W.astype(np.float64) for _, W in case["init"]]
    deltas, skipped = [], np.zeros(N, dtype=bool)
    for k, (frm, a, rew, nxt, term) in enumerate(case["rounds"]):
        ps, pn = phi_s_rounds[k].astype(np.float64), phi_n_rounds[k].astype(np.float64)
        xa = np.array([pn[:, i] @ Ws[i][:, 0] for i in range(N)])
        xb = np.array([pn[:, i] @ Ws[i][:, 1] for i in range(N)])
        al, be = bn.beta_params(xa, xb)
        na, margin = bn.beta_sample(seed, env_offset + np.arange(N), k, BLK_INNER, al, be)
        skipped |= (margin < MARGIN) & (term == 0)
        d = np.zeros(N)
        for i in range(N):
            d[i], w[i] = sarsa_handle(w[i], Ws[i], ps[:, i], float(a[i]), float(rew[i]), pn[:, i], float(na[i]), bool(term[i]), p["gamma"], p["lr"])
        deltas.append(d)
    return np.stack(w), deltas, skipped
