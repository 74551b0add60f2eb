"""GTD2 and TDC (RSRL_GTD2, RSRL_TDC; prediction/td/gtd2.rs:27-86, prediction/td/tdc.rs:41-101) restated in numpy, three times.  Shared by the CPU
and GPU tests and by tests/fuzz_gtd.py.

  rule_f32   float32 in the DEVICE's operation order (kernels_gtd.hpp gtd_step), bit for bit: dot products as four interleaved chains of fused
             multiply-adds (feature f goes to chain f mod 4; (a0 + a1) + (a2 + a3)), k_train_td's expression for the TD error, one fused
             multiply-add per element and column move, theta's two moves one after the other.  Vectorised over a leading axis of learners.  The
             features come from the oracle's device-order projection (fourier_project(..., "f32d")), as the oracle's own f32d handles take them
  rule_f64   float64 in the same form (the two scaled moves, no merged gradient)
  literal    float64, the reference's text transcribed: the merged gradient, unit steps (GTD2: both columns; TDC: q_func, with td_est through
             its SGD rate)

lr scales every move of theta, lr_td every move of w: lr = lr_td = 1 is the literal GTD2, lr = 1 the literal TDC over SGD(lr_td)."""
import numpy as np

from tests.nac_numpy import fma32

GTD2, TDC = 30, 31
F32 = np.float32


def dot_f32(w, phi):
    """<w, phi> per learner, (N, F) x (N, F) -> (N,) float32: WBuf::q's summation order"""
    w, phi = np.asarray(w, dtype=F32), np.asarray(phi, dtype=F32)
    acc = [np.zeros(w.shape[0], dtype=F32) for _ in range(4)]
    for f in range(w.shape[1]):
        acc[f % 4] = fma32(phi[:, f], w[:, f], acc[f % 4])
    return ((acc[0] + acc[1]).astype(F32) + (acc[2] + acc[3]).astype(F32)).astype(F32)


def _axpy_f32(x, scale, phi):
    return fma32(np.asarray(scale, dtype=F32)[:, None], phi, x)


def rule_f32(algo, theta, w, phi_s, phi_n, r, term, gamma, lr, lr_td):
    """one transition per learner: theta, w, phi_s, phi_n (N, F) float32; r (N,); term (N,) bool -> (td (N,), theta', w') float32"""
    theta, w, phi_s, phi_n = (np.asarray(x, dtype=F32) for x in (theta, w, phi_s, phi_n))
    r, term = np.asarray(r, dtype=F32), np.asarray(term, dtype=bool)
    gamma, lr, lr_td = F32(gamma), F32(lr), F32(lr_td)
    w_s, th_s, th_n = dot_f32(w, phi_s), dot_f32(theta, phi_s), dot_f32(theta, phi_n)
    live = ((r + (gamma * th_n).astype(F32)).astype(F32) - th_s).astype(F32)
    td = np.where(term, (r - th_s).astype(F32), live).astype(F32)
    w2 = _axpy_f32(w, (lr_td * (td - w_s).astype(F32)).astype(F32), phi_s)
    if algo == GTD2:
        u = (lr * w_s).astype(F32)
        th2 = _axpy_f32(theta, u, phi_s)
        th2 = _axpy_f32(th2, -(gamma * u).astype(F32), phi_n)
    else:
        th2 = _axpy_f32(theta, (lr * td).astype(F32), phi_s)
        th2 = _axpy_f32(th2, -(lr * w_s).astype(F32), phi_n)
    return td, th2, w2


def rule_f64(algo, theta, w, phi_s, phi_n, r, term, gamma, lr, lr_td):
    """one transition of one learner, float64, the device's form -> (td, theta', w')"""
    theta, w, phi_s, phi_n = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (theta, w, phi_s, phi_n))
    w_s, th_s, th_n = w @ phi_s, theta @ phi_s, theta @ phi_n
    td = r - th_s if term else r + gamma * th_n - th_s
    w2 = w + lr_td * (td - w_s) * phi_s
    if algo == GTD2:
        u = lr * w_s
        th2 = theta + u * phi_s
        th2 = th2 - gamma * u * phi_n
    else:
        th2 = theta + lr * td * phi_s
        th2 = th2 - lr * w_s * phi_n
    return float(td), th2, w2


def literal(algo, theta, w, phi_s, phi_n, r, term, gamma, sgd_rate=1.0):
    """gtd2.rs:51-85 / tdc.rs:69-100 as written, float64 -> (td_error, theta', w').  sgd_rate: TDC's td_est optimiser (not read by GTD2, whose
    updates all bypass it)"""
    theta, w, phi_s, phi_n = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (theta, w, phi_s, phi_n))
    w_s = w @ phi_s
    theta_s = theta @ phi_s
    td_error = r - theta_s if term else r + gamma * (theta @ phi_n) - theta_s
    if algo == GTD2:
        grad_s = phi_s.copy()
        w2 = w + (td_error - w_s) * grad_s                          # ScaledGradientUpdate: scaled_addto, no rate
        grad_s = grad_s - gamma * phi_n                             # merge_inplace(|x, y| x - gamma y)
        th2 = theta + w_s * grad_s
    else:
        w2 = w + sgd_rate * (td_error - w_s) * phi_s                # StateUpdate through td_est's SGD
        grad = td_error * phi_s - w_s * phi_n                       # merge(|x, y| td_error x - w_s y): no gamma
        th2 = theta + grad                                          # GradientUpdate: addto, no rate
    return float(td_error), th2, w2


def project(orc, domain, order, S, prec="f32d"):
    """states (D, N) -> features (N, F): the device's float32 values ("f32d") or the reference precision's ("f64")"""
    return np.stack([orc.fourier_project(domain, order, S[:, i], prec) for i in range(S.shape[1])])
