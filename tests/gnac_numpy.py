"""NAC over the Gibbs policy with a SARSA critic over the stable compatible basis (RSRL_GIBBS_NAC, examples/nac_softmax.rs) restated in numpy.
Shared by the CPU and GPU tests.

  psi(s, a)      SCB::project with the flattening of CompatibleBasis::project (fa/linear.rs:42-46): grad_log pi(a|s) (policies/softmax.rs:113-128,
                 the (F, A) matrix whose column b is (1[b==a] - p_b) phi) flattened ROW-MAJOR, then phi: (A+1) F features
  q_value        <w, psi(s, a)>
  sarsa_handle   SARSA::handle (control/td/sarsa.rs:53-75) with SGD; the caller supplies the inner draw na
  nac_handle     NAC::handle(()) (control/nac.rs:47-59): grad = w[0 .. F A - 1] reshaped row-major to (F, A), norm = max(||grad||, 1e-3),
                 theta += (alpha / norm) grad
  nac_handle_f32 the same in float32 in the DEVICE's operation order (tests/nac_numpy.fma32 is the fused multiply-add)
  rule_f32       SARSA::handle in float32 in the device's operation order: the four-chain dots, the oracle's f32 softmax and sampler
  bars           the GPU rule test's bounds, DERIVED: gamma_n = n u / (1 - n u), u = 2^-24, n the longest chain of a dot in the device's order
                 (ceil(F / 4) fused multiply-adds and two additions), applied to the sums of absolute terms; plus the project's own 1e-6 bound on
                 a probability (tests/test_gpu_actor_critic.py) propagated through c_b into Q, delta and the weight moves
  gnac_restated_loop   the driver loop (nac_softmax.rs:57-78) per learner in f64 on the device's draws, as tests/ac_numpy.ac_restated_loop

Two deliberately WRONG rules, for the CPU test that shows the bars are not blind: psi_column0 (the reference's SCB::project as it stands: column 0
of grad_log only, zero-padded to (A+1) F) and nac_handle_colmajor (the critic's first F A weights reshaped column-major).

Everything but nac_handle_f32 and rule_f32 is f64, in the reference's form."""
import numpy as np

from tests.ac_numpy import near_boundary, softmax
from tests.nac_numpy import fma32

U = 2.0 ** -24
EP = 1e-6              # the project's bound on a device probability against the f64 one (tests/test_gpu_actor_critic.py)
RULE_SEED = 17         # the ctx seed of the GPU rule test
LOOP_SEED = 31         # the ctx seed of the GPU driver-loop test: chosen on the CPU (tests/test_gibbs_nac_cpu.py) so that the restated loop alone flags at most a quarter of the learners near
# the rule test's parameters are binary fractions: the same numbers in f32 and in f64
RULE = dict(gamma=0.9375, lr=0.0625, tau=1.0)
LOOP = dict(N=67, K=48, cap=20, P=3, gamma=0.95, lr=0.05, alpha=0.002, tau=0.5)
CASES = [(0, 1), (0, 2), (0, 5), (1, 1), (2, 1)]      # (domain, order): MountainCar 1, 2 (the non-packed F), 5; CartPole 1 (A = 2); Acrobot 1


def n_actions(domain):
    return 2 if domain == 1 else 3


def probs(Th, phi, tau):
    return softmax(np.asarray(Th, dtype=np.float64).T @ np.asarray(phi, dtype=np.float64), tau)


def score_coefs(Th, phi, a, tau):
    """c_b = 1[b==a] - p_b"""
    c = -probs(Th, phi, tau)
    c[a] += 1.0
    return c


def psi(Th, phi, a, tau):
    phi = np.asarray(phi, dtype=np.float64)
    return np.concatenate([np.outer(phi, score_coefs(Th, phi, a, tau)).ravel(), phi])      # row-major (F, A): index f * A + b


def psi_column0(Th, phi, a, tau):
    """WRONG on purpose -- SCB::project as the reference has it (fa/linear.rs:91-102): column 0 of grad_log chained with phi, 2F values; zero-padded"""
    phi = np.asarray(phi, dtype=np.float64)
    A = np.asarray(Th).shape[1]
    return np.concatenate([score_coefs(Th, phi, a, tau)[0] * phi, phi, np.zeros((A - 1) * len(phi))])


def q_value(w, Th, phi, a, tau, psi_fn=psi):
    return float(np.asarray(w, dtype=np.float64).ravel() @ psi_fn(Th, phi, a, tau))


def sarsa_handle(w, Th, phi_s, a, r, phi_n, na, term, gamma, lr, tau, psi_fn=psi):
    """one transition -> (delta, w'); na: the critic's own draw at s' (not read on a terminal transition)"""
    w = np.asarray(w, dtype=np.float64).ravel()
    q = q_value(w, Th, phi_s, a, tau, psi_fn)
    delta = r - q if term else r + gamma * q_value(w, Th, phi_n, na, tau, psi_fn) - q
    return delta, w + lr * delta * psi_fn(Th, phi_s, a, tau)


def nac_handle(w, Th, alpha, order="C"):
    """-> (theta', norm), f64"""
    w, Th = np.asarray(w, dtype=np.float64).ravel(), np.asarray(Th, dtype=np.float64)
    F, A = Th.shape
    g = w[:F * A].reshape((F, A), order=order)
    norm = max(float(np.sqrt(np.sum(g * g))), 1e-3)
    return Th + alpha / norm * g, norm


def nac_handle_colmajor(w, Th, alpha):
    """WRONG on purpose: the critic's first F A weights read back column-major"""
    return nac_handle(w, Th, alpha, order="F")


def nac_handle_f32(w, Th, alpha):
    """float32, the device's operation order -> (theta' (F, A) float32, norm float32)"""
    w, Th = np.asarray(w, dtype=np.float32).ravel(), np.asarray(Th, dtype=np.float32)
    F, A = Th.shape
    ss = np.float32(0.0)
    for j in range(F * A):
        ss = np.float32(ss + np.float32(w[j] * w[j]))
    norm = np.maximum(np.sqrt(ss, dtype=np.float32), np.float32(1e-3))
    scale = np.float32(np.float32(alpha) / norm)
    return fma32(scale, w[:F * A].reshape(F, A), Th), np.float32(norm)


# ---- float32, the device's order
def dot32(W, phi):
    """<W[k], phi> for every row k in WBuf::q's order: chain f % 4 takes feature f, ascending, one fused multiply-add each; (c0 + c1) + (c2 + c3)"""
    W, phi = np.asarray(W, dtype=np.float32), np.asarray(phi, dtype=np.float32)
    acc = np.zeros((4, W.shape[0]), dtype=np.float32)
    for f in range(W.shape[1]):
        acc[f % 4] = fma32(phi[f], W[:, f], acc[f % 4])
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])).astype(np.float32)


def blocks(w, F, A):
    """the critic's (A+1) F weights as the A score blocks and the basis block: (A + 1, F), row b = w[f * A + b], row A = w[F A + f]"""
    w = np.asarray(w).ravel()
    return np.concatenate([w[:F * A].reshape(F, A).T, w[F * A:].reshape(1, F)])


def unblocks(B):
    return np.concatenate([B[:-1].T.ravel(), B[-1]])


def _q32(orc, B, Th, phi, a, tau):
    p = orc.policy_probs(orc.SOFTMAX, dot32(np.asarray(Th, dtype=np.float32).T, phi), tau=tau, prec="f32")
    d = dot32(B, phi)
    A = len(p)
    c = np.array([np.float32(np.float32(1.0 if b == a else 0.0) - p[b]) for b in range(A)], dtype=np.float32)
    q = d[A]
    for b in range(A - 1, -1, -1):
        q = fma32(c[b], d[b], q)
    return np.float32(q), c, p


def rule_f32(orc, w, Th, phi_s, a, r, phi_n, term, x_inner, gamma, lr, tau):
    """SARSA::handle in float32, the device's order -> (delta f32, w' f32[(A+1) F], the inner action, p(s') f32)"""
    Th = np.asarray(Th, dtype=np.float32)
    F, A = Th.shape
    B = blocks(np.asarray(w, dtype=np.float32), F, A)
    p_n = orc.policy_probs(orc.SOFTMAX, dot32(Th.T, phi_n), tau=tau, prec="f32")
    na = sample_probs32(p_n, x_inner)
    boot, _, _ = _q32(orc, B, Th, phi_n, na, tau)
    qsa, c, _ = _q32(orc, B, Th, phi_s, a, tau)
    r = np.float32(r)
    delta = np.float32(r - qsa) if term else np.float32(fma32(np.float32(gamma), boot, r) - qsa)
    sc = np.float32(np.float32(lr) * delta)
    sb = np.array([np.float32(sc * c[b]) for b in range(A)] + [sc], dtype=np.float32)
    phi_s = np.asarray(phi_s, dtype=np.float32)
    B2 = np.stack([fma32(sb[k], phi_s, B[k]) for k in range(A + 1)])
    return delta, unblocks(B2), na, p_n


def sample_probs32(p, x):
    """sample_probs_with_rng in float32: the first index whose cumulative probability exceeds u, else the last (policies/mod.rs:45-61)"""
    u = np.float32(np.float32(int(x[2]) >> 8) * np.float32(1.0 / 16777216.0))
    acc = np.float32(0.0)
    for i, pi in enumerate(np.asarray(p, dtype=np.float32)):
        acc = np.float32(acc + pi)
        if acc > u:
            return i
    return len(p) - 1


# ---- the bars
def gamma_n(n):
    return n * U / (1.0 - n * U)


def n_chain(F):
    """the longest rounding chain of a length-F dot in WBuf::q's order: ceil(F / 4) fused multiply-adds, then two additions"""
    return -(-F // 4) + 2


def _q_bar(B, Th, phi, a, tau):
    """(Q in f64, its bound).  With c_b = 1[b==a] - p_b (|error| <= EC = EP + u: the probability's bound and one subtraction), d_b = <w_b, phi>
    (|error| <= gamma_n S_b, S_b = sum_f |w_bf phi_f|) and the chain fma(c_0, d_0, ... fma(c_{A-1}, d_{A-1}, d_v)) of A roundings over
    terms bounded by (|c_b| + EC) (1 + gamma_n) S_b and (1 + gamma_n) S_v:
        |dQ| <= sum_b [ (|c_b| + EC) (gamma_n + gamma_A (1 + gamma_n)) S_b + EC S_b ] + (gamma_n + gamma_A (1 + gamma_n)) S_v"""
    F = len(phi)
    A = B.shape[0] - 1
    c = score_coefs(Th, phi, a, tau)
    S = np.abs(B * phi).sum(axis=1)
    g = gamma_n(n_chain(F))
    g = g + gamma_n(A) * (1.0 + g)
    ec = EP + U
    q = float(c @ (B[:A] @ phi) + B[A] @ phi)
    return q, float(np.sum((np.abs(c) + ec) * g * S[:A] + ec * S[:A]) + g * S[A]), c, ec


def bars(w, Th, phi_s, a, r, phi_n, na, term, gamma, lr, tau):
    """-> (bound on |delta - delta64|, bound on |w' - w'64| per entry, in w's order), from the f64 rule's own quantities.
        delta: |d delta| <= gamma E_Q(s', na) + E_Q(s, a) + u (|fma(gamma, Q', r)| + |delta|)      (terminal: E_Q(s, a) + u |delta|)
        sc = lr delta: E_sc = lr E_delta + u |sc|
        block b moves by m_b phi, m_b = sc c_b: E_m = (|c_b| + EC) E_sc + |sc| EC + u |m_b|; the basis block by sc phi: E_sc
        an entry: |d w'| <= E_m |phi_f| + u |w'| (one fused multiply-add)"""
    Th = np.asarray(Th, dtype=np.float64)
    F, A = Th.shape
    phi_s, phi_n = np.asarray(phi_s, dtype=np.float64), np.asarray(phi_n, dtype=np.float64)
    B = blocks(np.asarray(w, dtype=np.float64), F, A)
    q, e_q, c, ec = _q_bar(B, Th, phi_s, a, tau)
    if term:
        delta = r - q
        e_delta = e_q + U * abs(delta)
    else:
        qn, e_qn, _, _ = _q_bar(B, Th, phi_n, na, tau)
        delta = r + gamma * qn - q
        e_delta = gamma * e_qn + e_q + U * (abs(gamma * qn + r) + gamma * e_qn + abs(delta) + e_q + gamma * e_qn)
    sc = lr * delta
    e_sc = lr * e_delta + U * (abs(sc) + lr * e_delta)
    m = np.concatenate([sc * c, [sc]])
    e_m = np.concatenate([(np.abs(c) + ec) * e_sc + abs(sc) * ec + U * (np.abs(sc * c) + (np.abs(c) + ec) * e_sc + abs(sc) * ec), [e_sc]])
    B2 = B + m[:, None] * phi_s
    e_B = e_m[:, None] * np.abs(phi_s) + U * (np.abs(B2) + e_m[:, None] * np.abs(phi_s))
    return float(e_delta), unblocks(e_B)


# ---- the GPU rule test's inputs
def project(orc, domain, order, S, prec="f32d"):
    """(F, N) features of the (D, N) states"""
    return np.stack([orc.fourier_project(domain, order, S[:, i], prec) for i in range(S.shape[1])], axis=1)


def handle_case(orc, domain, order, N=67):
    """per learner a random theta with sum_f |theta_bf| in [0.3, 1.2] per column and a random critic w with sum |w| in [0.5, 3]; random states and
    actions stepped by the oracle's device-order transition, a quarter of the transitions forced terminal"""
    rng = np.random.default_rng(700 + domain * 100 + order * 10)
    A, lo_hi = n_actions(domain), orc.domain_bounds(domain)
    D = len(lo_hi[0])
    F = (order + 1) ** D
    w, th = np.zeros((N, (A + 1) * F), dtype=np.float32), np.zeros((N, F, A), dtype=np.float32)
    for i in range(N):
        T = rng.normal(size=(F, A))
        T *= rng.uniform(0.3, 1.2, size=A) / np.abs(T).sum(axis=0)
        x = rng.normal(size=(A + 1) * F)
        x *= rng.uniform(0.5, 3.0) / np.abs(x).sum()
        w[i], th[i] = x, T
    frm = rng.uniform(lo_hi[0], lo_hi[1], size=(N, D)).T.astype(np.float32)
    a = rng.integers(0, A, size=N).astype(np.int32)
    nxt, rew, term = np.zeros_like(frm), np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.uint8)
    for i in range(N):
        ns, r, t = orc.domain_step(domain, frm[:, i], int(a[i]), prec="f32d")
        nxt[:, i], rew[i], term[i] = np.asarray(ns, dtype=np.float32), np.float32(r), bool(t)
    term = (term.astype(bool) | (rng.random(N) < 0.25)).astype(np.uint8)
    return dict(domain=domain, order=order, F=F, A=A, w=w, theta=th, frm=frm, a=a, rew=rew, nxt=nxt, term=term)


def rule_reference(orc, case, seed, phi_s, phi_n, t=0, psi_fn=psi):
    """SARSA::handle in f64 on the case, from the features given ((F, N) each) -> (delta (N,), w' (N, (A+1) F), e_delta (N,), e_w like w', left
    out (N,): a non-terminal learner whose inner draw lies within 1e-5 of a cumulative boundary).  The bars are always the right rule's"""
    N, tau, gamma, lr = len(case["a"]), RULE["tau"], RULE["gamma"], RULE["lr"]
    delta, w2 = np.zeros(N), np.zeros(case["w"].shape)
    e_d, e_w, out = np.zeros(N), np.zeros(case["w"].shape), np.zeros(N, dtype=bool)
    for i in range(N):
        Th, w = case["theta"][i].astype(np.float64), case["w"][i].astype(np.float64)
        ps, pn = phi_s[:, i].astype(np.float64), phi_n[:, i].astype(np.float64)
        x = orc.draw(seed, i, t, orc.BLK_INNER)
        p_n = probs(Th, pn, tau)
        term = bool(case["term"][i])
        out[i] = (not term) and near_boundary(p_n, x)
        na = orc.policy_sample(orc.SOFTMAX, Th.T @ pn, x, tau=tau)
        delta[i], w2[i] = sarsa_handle(w, Th, ps, int(case["a"][i]), float(case["rew"][i]), pn, na, term, gamma, lr, tau, psi_fn)
        e_d[i], e_w[i] = bars(w, Th, ps, int(case["a"][i]), float(case["rew"][i]), pn, na, term, gamma, lr, tau)
    return delta, w2, e_d, e_w, out


# ---- the driver loop
def loop_start(orc, domain, N, rng):
    """random states, half of the learners started beside the goal (MountainCar), random actions"""
    lo, hi = orc.domain_bounds(domain)
    S0 = rng.uniform(lo, hi, size=(N, len(lo))).T.astype(np.float32)
    S0[0, : N // 2] = rng.uniform(0.40, 0.49, size=N // 2).astype(np.float32)
    S0[1, : N // 2] = rng.uniform(0.03, 0.07, size=N // 2).astype(np.float32)
    return S0, rng.integers(0, n_actions(domain), size=N).astype(np.int32)


def gnac_restated_loop(orc, domain, order, N, K, cap, P, seed, gamma, lr, alpha, tau, S0, A0, t0=0, env_offset=0):
    """the driver loop per learner in f64 on the same draws, from zero weights: transition, critic.handle, the behaviour sample (after the restart
    if the episode ended or was cut), then NAC::handle(()) if the step's 0-based index in its episode is a multiple of P -> (actions [K][N] after
    every batch-step, w, theta, learners with a draw within 1e-5 of a cumulative-probability boundary)"""
    F, A = (order + 1) ** S0.shape[0], n_actions(domain)
    acts, out_w, out_T, near = np.zeros((K, N), dtype=np.int64), [], [], np.zeros(N, dtype=bool)
    for i in range(N):
        w, Th = np.zeros((A + 1) * F), np.zeros((F, A))
        s, a, ep = S0[:, i].copy(), int(A0[i]), 0
        for k in range(K):
            t, gid = t0 + k, env_offset + i
            update = ep % P == 0
            ns, r, term = orc.domain_step(domain, s, a, prec="f32d")
            ns = np.asarray(ns, dtype=np.float32)
            ep += 1
            trunc = (not term) and cap > 0 and ep >= cap
            if term:
                ns = orc.domain_reset(domain, prec="f32")
            phi_s, phi_n = orc.fourier_project(domain, order, s), orc.fourier_project(domain, order, ns)
            xin = orc.draw(seed, gid, t, orc.BLK_INNER)
            near[i] |= (not term) and near_boundary(probs(Th, phi_n, tau), xin)
            na = orc.policy_sample(orc.SOFTMAX, Th.T @ phi_n, xin, tau=tau)
            _, w = sarsa_handle(w, Th, phi_s, a, float(np.float32(r)), phi_n, na, term, gamma, lr, tau)
            if term or trunc:
                ep = 0
                ns = orc.domain_reset(domain, prec="f32")
            xs = orc.draw(seed, gid, t, orc.BLK_RESET if trunc else orc.BLK_STEP)
            hn = Th.T @ orc.fourier_project(domain, order, ns)
            near[i] |= near_boundary(orc.policy_probs(orc.SOFTMAX, hn, tau=tau), xs)
            a = orc.policy_sample(orc.SOFTMAX, hn, xs, tau=tau)
            acts[k, i] = a
            if update:
                Th, _ = nac_handle(w, Th, alpha)
            s = np.asarray(ns, dtype=np.float32)
        out_w.append(w); out_T.append(Th)
    return acts, out_w, out_T, near
