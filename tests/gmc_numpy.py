"""GradientMC (rsrl/src/prediction/mc.rs:26-58) restated literally in f64: every-visit Monte-Carlo prediction through SGD(lr), the trajectory walked
last transition to first.  It takes feature rows, so it needs no basis of its own.  Plain helper module (no fixtures, no pytest settings)."""
import numpy as np


def gradient_mc(w, phis, rewards, gamma, lr):
    """handle(&Trajectory) on w (F,) with phis[k] = phi(from of transition k) and rewards[k] its reward
    -> (w', the errors sum - pred in visit order (last transition first), the returns indexed by transition)"""
    w = np.array(w, dtype=np.float64)
    n = len(rewards)
    errors, returns, total = [], np.zeros(n), 0.0
    for k in range(n - 1, -1, -1):
        total = float(rewards[k]) + gamma * total
        phi = np.asarray(phis[k], dtype=np.float64)
        pred = float(phi @ w)                                  # with w as the previous visit left it
        w = w + lr * (total - pred) * phi                     # StateUpdate -> ScalarLFA::update -> SGD(lr)
        errors.append(total - pred)
        returns[k] = total
    return w, errors, returns


def f32_returns(rewards, gamma):
    """sum = r + gamma * sum from the last reward backwards, an f32 multiply followed by an f32 add, as the device forms it -> f32 (n,), by transition"""
    g, gm, out = np.float32(0.0), np.float32(gamma), np.zeros(len(rewards), dtype=np.float32)
    for k in range(len(rewards) - 1, -1, -1):
        g = np.float32(np.float32(rewards[k]) + np.float32(gm * g))
        out[k] = g
    return out


def td_chain(orc, ag, w, states, rewards, gamma, prec):
    """the device-order reference: a backward chain of TD's terminal-transition update with r := the return, oracle.handle_td(..., term=True).  w is
    updated in place (f64 for prec "f64", f32 for "f32d"); the return is formed in f32 for "f32d", in f64 otherwise -> (errors in visit order, returns)"""
    n = len(rewards)
    rets = f32_returns(rewards, gamma) if prec == "f32d" else np.zeros(n)
    total, errors = 0.0, []
    for k in range(n - 1, -1, -1):
        if prec != "f32d":
            total = float(rewards[k]) + gamma * total
            rets[k] = total
        errors.append(orc.handle_td(ag, w, None, states[k], float(rets[k]), states[k], True, prec))
    return errors, rets
