"""CliffWalk over the tabular Q restated in numpy (cliff_walk.rs over grid_world.rs; fa/tabular/dense.rs; the one-step agents' handle), shared by
the CPU and GPU tests: the domain step, the row map, the four agents' rules and the driver loop in float32 in the device's operation order
(device_core.hpp td_error / td_error_pal / td_dispatch, kernels_table.hpp table_handle / table_step), and the same rules in f64.

The float32 rule rounds after every operation, as the device does: the library is built without contraction and the one-step rules hold no
fused multiply-add (r + gamma * boot - qsa is a product, a sum and a difference), so nac_numpy.fma32 has no place to stand in here; the policies are
the oracle's device-order functions (prec="f32d") on the oracle's draws."""
import numpy as np

WIDTH, HEIGHT, CELLS, A = 12, 5, 60, 4
QLEARNING, SARSA, EXPECTED_SARSA, PAL = 0, 1, 2, 5
f32 = np.float32


def cell(s, size):
    """a caller's state component as the device reads it: floor(clamp(s, 0, size - 1)), NaN as 0"""
    s = float(s)
    if s != s:
        return 0
    return int(np.floor(min(max(s, 0.0), float(size - 1))))


def row(x, y):
    return x * HEIGHT + y


def row_of_state(s):
    return row(cell(s[0], WIDTH), cell(s[1], HEIGHT))


def step(x, y, a):
    """grid_world.rs:87-125 + cliff_walk.rs:41-62 -> (x', y', reward, terminal)"""
    if a == 0:
        y = min(y + 1, HEIGHT - 1)
    elif a == 1:
        x = min(x + 1, WIDTH - 1)
    elif a == 2:
        y = max(y - 1, 0)
    else:
        x = max(x - 1, 0)
    term = x > 0 and y == 0
    return x, y, ((50.0 if x == WIDTH - 1 else -50.0) if term else 0.0), term


def walk(actions):
    """the reference's known-answer walks: from the start cell -> [(x, y, reward, terminal)] per action"""
    x, y, out = 0, 0, []
    for a in actions:
        x, y, r, t = step(x, y, a)
        out.append((x, y, r, t))
    return out


class Pol:
    """a policy object's parameters: kind (the oracle's numbers), epsilon, tau"""

    def __init__(self, kind, eps=0.1, tau=1.0):
        self.kind, self.eps, self.tau = int(kind), float(eps), float(tau)


def _sample(orc, pol, q, x, prec):
    return orc.policy_sample(pol.kind, q, x, eps=pol.eps, tau=pol.tau, prec=prec)


def rule32(orc, algo, apol, qs, qn, a, r, term, gamma, alpha, x_inner):
    """td_dispatch in float32 -> (delta, the error sent on)"""
    qs, qn = np.asarray(qs, dtype=f32), np.asarray(qn, dtype=f32)
    r, gamma, alpha = f32(r), f32(gamma), f32(alpha)
    if algo == PAL:
        qsa, qna = qs[a], qn[a]
        ast, nast = orc.argmax_first(qs, prec="f32d"), orc.argmax_first(qn, prec="f32d")
        td = f32(f32(r + f32(gamma * qn[ast])) - qsa)
        al = f32(td - f32(alpha * f32(qs[ast] - qsa)))
        alt = f32(td - f32(alpha * f32(qn[nast] - qna)))
        delta = f32(r - qsa) if term else max(al, alt)
        return f32(delta), f32(alpha * delta)
    qsa = qs[a]
    if algo == QLEARNING:
        boot = f32(orc.find_max(qn, prec="f32d")[1])
    elif algo == SARSA:
        boot = qn[_sample(orc, apol, qn, x_inner, "f32d")]
    else:
        p = orc.policy_probs(apol.kind, qn, eps=apol.eps, tau=apol.tau, prec="f32d")
        boot = f32(0.0)
        for i in range(A):
            boot = f32(boot + f32(qn[i] * p[i]))
    delta = f32(r - qsa) if term else f32(f32(r + f32(gamma * boot)) - qsa)
    return delta, (f32(alpha * delta) if algo == EXPECTED_SARSA else delta)


def rule64(orc, algo, apol, qs, qn, a, r, term, gamma, alpha, x_inner):
    """the same rules in f64 (q_learning.rs:51-71, sarsa.rs:53-75, expected_sarsa.rs:45-66, pal.rs:34-60) -> (delta, the error sent on)"""
    qs, qn = np.asarray(qs, dtype=np.float64), np.asarray(qn, dtype=np.float64)
    if algo == PAL:
        ast, nast = orc.argmax_first(qs), orc.argmax_first(qn)
        td = r + gamma * qn[ast] - qs[a]
        delta = (r - qs[a]) if term else max(td - alpha * (qs[ast] - qs[a]), td - alpha * (qn[nast] - qn[a]))
        return delta, alpha * delta
    if algo == QLEARNING:
        boot = qn.max()
    elif algo == SARSA:
        boot = qn[_sample(orc, apol, qn, x_inner, "f64")]
    else:
        boot = float(np.dot(qn, orc.policy_probs(apol.kind, qn, eps=apol.eps, tau=apol.tau)))
    delta = (r - qs[a]) if term else r + gamma * boot - qs[a]
    return delta, (alpha * delta if algo == EXPECTED_SARSA else delta)


def handle32(orc, algo, apol, Q, rs, a, rn, r, term, gamma, lr, alpha, x_inner):
    """table_handle: the rule on rows rs / rn of the (60, 4) float32 table Q, then Q[rs, a] += lr * e in place -> delta"""
    delta, e = rule32(orc, algo, apol, Q[rs], Q[rn], a, r, term, gamma, alpha, x_inner)
    Q[rs, a] = f32(Q[rs, a] + f32(f32(lr) * e))
    return delta


def wave_sum(v):
    """the statistics' reduction over a wave of 64 lanes as the device adds it: v += v[lane ^ o] for o = 32, 16, .., 1 (f64)"""
    v = np.array(v, dtype=np.float64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ o]
    return float(v[0])


def loop32(orc, algo, pol, apol, N, K, cap, seed, gamma, lr, alpha, Q0=None, t0=0, env_offset=0, depth=None):
    """rsrl_hip_reset, then K batch-steps of the driver loop (k_train_mem's order) in float32 on the oracle's draws, `depth` batch-steps per launch
    (None: one launch) -> dict(states (2, N) f32, actions, episode_steps, tables [N] of (60, 4), first = the actions after the reset, stats)"""
    depth = depth or max(K, 1)
    Q = [np.zeros((CELLS, A), dtype=f32) if Q0 is None else np.array(Q0[i], dtype=f32) for i in range(N)]
    X, Y, Ac, Ep = np.zeros(N, int), np.zeros(N, int), np.zeros(N, int), np.zeros(N, int)
    n_ep = n_trunc = sum_len = 0
    n_launch = (K + depth - 1) // depth
    acc_abs, acc_r = np.zeros((n_launch, N), dtype=f32), np.zeros((n_launch, N), dtype=f32)
    for i in range(N):      # rsrl_hip_reset: the initial sample at the start cell, stream BLK_INIT of batch-step t0
        Ac[i] = _sample(orc, pol, Q[i][row(0, 0)], orc.draw(seed, env_offset + i, t0, orc.BLK_INIT), "f32d")
    first = Ac.copy()
    for i in range(N):
        gid, q = env_offset + i, Q[i]
        x = y = ep = 0
        a = int(first[i])
        for k in range(K):
            t = t0 + k
            nx, ny, r, term = step(x, y, a)
            ep += 1
            trunc = (not term) and cap > 0 and ep >= cap
            if term:
                nx = ny = 0
            xin = orc.draw(seed, gid, t, orc.BLK_INNER) if algo == SARSA else (0, 0, 0, 0)
            delta = handle32(orc, algo, apol, q, row(x, y), a, row(nx, ny), r, term, gamma, lr, alpha, xin)
            na = _sample(orc, pol, q[row(nx, ny)], orc.draw(seed, gid, t, orc.BLK_STEP), "f32d")
            L = k // depth
            acc_abs[L, i] = f32(acc_abs[L, i] + abs(delta))
            acc_r[L, i] = f32(acc_r[L, i] + f32(r))
            if term:
                n_ep += 1; sum_len += ep; ep = 0
            if trunc:
                n_ep += 1; n_trunc += 1; sum_len += ep; ep = 0
                nx = ny = 0
                na = _sample(orc, pol, q[row(0, 0)], orc.draw(seed, gid, t, orc.BLK_RESET), "f32d")
            x, y, a = nx, ny, na
        X[i], Y[i], Ac[i], Ep[i] = x, y, a, ep
    # the statistics: every launch adds each wave's f64 butterfly sum of the learners' f32 sums to the wave's slot; the host adds the slots in order
    waves = (N + 63) // 64
    slot_abs, slot_r = np.zeros(waves), np.zeros(waves)
    for L in range(n_launch if K > 0 else 0):
        for w in range(waves):
            va, vr = np.zeros(64), np.zeros(64)
            n = min(64, N - 64 * w)
            va[:n], vr[:n] = acc_abs[L, 64 * w:64 * w + n], acc_r[L, 64 * w:64 * w + n]
            slot_abs[w] += wave_sum(va); slot_r[w] += wave_sum(vr)
    sa = sr = 0.0
    for w in range(waves):
        sa += slot_abs[w]; sr += slot_r[w]
    stats = dict(env_steps=N * K, episodes=n_ep, episodes_truncated=n_trunc, sum_episode_steps=sum_len, sum_abs_td_error=sa, sum_reward=sr)
    return dict(states=np.stack([X, Y]).astype(f32), actions=Ac.astype(np.int32), episode_steps=Ep.astype(np.uint32), tables=Q, first=first.astype(np.int32),
                stats=stats)


def rollout32(orc, pol, Q, step_limit):
    """Domain::rollout(|s| policy.mode(s), Some(step_limit)) from the start cell on the float32 table Q -> (n_states, total reward f32, cells visited)"""
    x = y = 0
    cells, tot, steps, term = [(0, 0)], f32(0.0), 0, False
    while steps < step_limit - 1 and not term:
        a = orc.policy_mode(pol.kind, Q[row(x, y)], tau=pol.tau, prec="f32d")
        x, y, r, term = step(x, y, a)
        cells.append((x, y)); tot = f32(tot + f32(r)); steps += 1
    return steps + 1, tot, cells
