// kernels_lstd_batch.hpp -- the batch least-squares prediction agents (Handler<&Batch>) on the register-family Fourier orders:
//   LSTD         rsrl/src/prediction/lstd/lstd.rs:23-87           theta f64[F], A f64[F][F] (starts at 1e-6 I), b f64[F]
//   LSTDLambda   rsrl/src/prediction/lstd/lstd_lambda.rs:25-110   the same, plus the trace z f64[F]
// LSTD::handle walks the batch FIRST TO LAST (lstd.rs:59-81):
//     b += r * phi(s);   non-terminal: pd = gamma * phi(s') - phi(s), A -= phi(s) (x) pd;   terminal: A += phi(s) (x) phi(s)
// LSTDLambda::handle walks it LAST TO FIRST (`batch.iter().rev()`, lstd_lambda.rs:66-103) -- the trace runs backwards in time, z survives from
// one batch to the next and only a terminal transition zeroes it:
//     c = lambda * gamma;  z = c * z + phi(s);  b += r * z;
//     non-terminal: pd = phi(s) - gamma * phi(s'), A += z (x) pd;   terminal: A += z (x) phi(s), z = 0
// and both end in solve() (lstd.rs:40-50, lstd_lambda.rs:44-54): theta <- A.solve(b).  Everything is f64, the features kernels_lstd.hpp's
// lstd_feature; every product is rounded (-ffp-contract=off) and an outer product's element is one rounded product, then added.
//
// solve().  The reference calls LAPACK and, on an exactly zero pivot, an SVD pseudo-inverse.  The library defines the solve itself, in ONE fixed
// operation order (tests/lstd_batch_numpy.py lu_solve restates it; the two agree bit for bit): Gaussian elimination with partial pivoting on a
// copy of A and b.  For k = 0 .. F-1: the pivot row p_k is the first row in index order, among the rows not yet used, with the largest
// |a[i][k]|; no such value above 0 abandons the solve; every remaining row i takes m = a[i][k] / a[p][k], a[i][j] -= m * a[p][j] (j > k),
// rhs[i] -= m * rhs[p].  Back substitution for k = F-1 .. 0: s = rhs[p_k]; s -= a[p_k][j] * x[j] for j = k+1 .. F-1 ascending; x[k] = s / a[p_k][k].
// DEPARTURE: there is no SVD fallback.  An abandoned solve leaves theta as it was (what the reference does when both of its attempts fail) and
// counts in the learner's singular_solves.
//
// Layout: kernels_lstd.hpp's.  Lane r of the learner's group owns row r of A, b_r, z_r and theta_r; rows never move -- a "swap" is the
// bookkeeping of which lane has been a pivot.  The pivot search is a scan of the group's candidates in its LDS slice, the pivot lane broadcasts
// its row tail and right-hand side through it, back substitution x_k.  The loops over k and j are unrolled: row[] and its copy stay in registers.
// The sweep and the solve run in WAVE-UNIFORM control flow: when any group of a wave has a batch, every lane of the wave runs them, and the
// other groups' results are selected away (the exchange through LDS is ordered by wave barriers, which lanes that branched off would not reach).
// LstdBatchLane::accumulate and ::solve are the ONE update: the driver loop, handle_transitions and lstd_solve run those same two.
#pragma once

#include "launch.hpp"
#include "kernels_lstd.hpp"

namespace rsrl {

// LDS vectors of one group: a broadcast vector (pd / the pivot row), two work vectors, and the pivot's right-hand side
enum : int { LB_V = 0, LB_X = 1, LB_Y = 2, LB_S = 3, LB_N = 4 };

template <int F, bool LAMBDA>
struct LstdBatchLane {
    double row[F];
    double theta, b, z;
    uint32_t sing;

    __device__ __forceinline__ void load(const LstdBatchState& ls, int64_t i, int r) {
        const int rr = r < F ? r : 0;                     // (lanes past F read row 0 and never store)
        const double* p = ls.mat + ((int64_t)i * F + rr) * F;
#pragma unroll
        for (int j = 0; j < F; ++j) row[j] = p[j];
        theta = ls.theta[(int64_t)i * F + rr];
        b = ls.b[(int64_t)i * F + rr];
        z = LAMBDA ? ls.z[(int64_t)i * F + rr] : 0.0;
        sing = ls.sing[i];
    }
    __device__ __forceinline__ void store_solution(const LstdBatchState& ls, int64_t i, int r) const {
        if (r >= F) return;
        ls.theta[(int64_t)i * F + r] = theta;
        if (r == 0) ls.sing[i] = sing;
    }
    __device__ __forceinline__ void store(const LstdBatchState& ls, int64_t i, int r) const {
        if (r >= F) return;
        double* p = ls.mat + ((int64_t)i * F + r) * F;
#pragma unroll
        for (int j = 0; j < F; ++j) p[j] = row[j];
        ls.b[(int64_t)i * F + r] = b;
        if (LAMBDA) ls.z[(int64_t)i * F + r] = z;
        store_solution(ls, i, r);
    }

    // one transition of the lane's learner into A, b (and z).  phs / phn: this lane's features of s and s'.  live: the learner has this
    // transition (the other groups of the wave run along and keep their values).  Returns the diagnostic r + gamma V(s') - V(s) (terminal:
    // r - V(s)) with the theta the learner holds: the agents themselves compute no TD error
    __device__ __forceinline__ double accumulate(const LstdBatchState& ls, double (*lv)[F], int r, double phs, double phn, double rew, bool term, bool live) {
        const double gamma = ls.gamma;
        const bool own = r < F;
        const double pd = term ? phs : (LAMBDA ? phs - gamma * phn : gamma * phn - phs);
        if (own) {
            lv[LB_V][r] = pd;
            lv[LB_X][r] = phs * theta;
            lv[LB_Y][r] = phn * theta;
        }
        lstd_wave_sync();
        const double v_s = lstd_sum<F>(lv[LB_X]);
        const double v_ns = lstd_sum<F>(lv[LB_Y]);
        const double delta = term ? rew - v_s : rew + gamma * v_ns - v_s;
        if constexpr (LAMBDA) {
            const double c = ls.lambda * gamma;
            const double nz = c * z + phs;
            b = live ? b + rew * nz : b;
#pragma unroll
            for (int j = 0; j < F; ++j) row[j] = live ? row[j] + nz * lv[LB_V][j] : row[j];
            z = live ? (term ? 0.0 : nz) : z;
        } else {
            b = live ? b + rew * phs : b;
#pragma unroll
            for (int j = 0; j < F; ++j) {
                const double e = phs * lv[LB_V][j];
                row[j] = live ? (term ? row[j] + e : row[j] - e) : row[j];
            }
        }
        lstd_wave_sync();                                 // (this transition's reads before the next one's writes)
        return delta;
    }

    // theta <- the solution of A x = b by the elimination the header describes, on a copy; commit: the learner takes the result (the other
    // groups of the wave run along).  Every lane of the wave calls it
    __device__ __forceinline__ void solve(double (*lv)[F], int r, bool commit) {
        const bool own = r < F;
        double a[F];
#pragma unroll
        for (int j = 0; j < F; ++j) a[j] = row[j];
        double rhs = b;
        bool used = !own, dead = false;
        int my_k = -1;
#pragma unroll
        for (int k = 0; k < F; ++k) {
            if (own) lv[LB_X][r] = used ? -1.0 : fabs(a[k]);
            lstd_wave_sync();
            double best = -1.0;
            int p = 0;
#pragma unroll
            for (int j = 0; j < F; ++j) {                 // the first row, in index order, with the largest candidate
                const double x = lv[LB_X][j];
                const bool up = x > best;
                best = up ? x : best;
                p = up ? j : p;
            }
            dead = dead || !(best > 0.0);
            const bool piv = own && !used && r == p;
            if (piv) {
#pragma unroll
                for (int j = k; j < F; ++j) lv[LB_V][j] = a[j];
                lv[LB_S][0] = rhs;
            }
            lstd_wave_sync();
            const bool elim = own && !used && !piv;
            const double m = a[k] / lv[LB_V][k];
#pragma unroll
            for (int j = k + 1; j < F; ++j) a[j] = elim ? a[j] - m * lv[LB_V][j] : a[j];
            rhs = elim ? rhs - m * lv[LB_S][0] : rhs;
            used = used || piv;
            my_k = piv ? k : my_k;
        }
#pragma unroll
        for (int k = F - 1; k >= 0; --k) {
            double s = rhs;
#pragma unroll
            for (int j = k + 1; j < F; ++j) s = s - a[j] * lv[LB_Y][j];
            const double xk = s / a[k];
            if (my_k == k) lv[LB_Y][k] = xk;
            lstd_wave_sync();
        }
        const double x = lv[LB_Y][own ? r : 0];
        theta = (commit && !dead) ? x : theta;
        sing = (commit && dead) ? sing + 1u : sing;
        lstd_wave_sync();                                 // (the reads of x before the next exchange's writes)
    }
};

// Handler<&Batch>::handle's walk over learner i's `len` transitions, without the solve: row k of from [rows][D][N] and rew [rows][N].
// to == nullptr: the rows are an episode record -- row k's `to` is row k + 1's `from`, no row is terminal, and the last row's `to` and
// terminal flag are last_to / last_term.  Otherwise to [rows][D][N] and term u8 [rows][N] give them.  len may differ between the groups of a
// wave (0: the group only runs along): the loop runs to the wave's longest.  td_out [rows][N] (may be null): the diagnostic at each row.
// Returns the sum of |diagnostic| over the learner's rows
template <int DOMAIN, int ORDER, bool LAMBDA, int F>
__device__ __forceinline__ double lstd_batch_sweep(LstdBatchLane<F, LAMBDA>& L, const LstdBatchState& ls, double (*lv)[F], int r, const float* from,
                                                   const float* to, const float* rew, const uint8_t* term, int64_t N, int64_t i, int64_t len,
                                                   const float (&last_to)[Domain<DOMAIN>::D], bool last_term, float* __restrict__ td_out) {
    constexpr int D = Domain<DOMAIN>::D;
    double acc = 0.0, carry = 0.0;
    float s0[D];                                          // row 0's `from`: a record walked forwards starts there
#pragma unroll
    for (int d = 0; d < D; ++d) s0[d] = from[(int64_t)d * N + i];
    for (int64_t k = 0; __ballot(k < len) != 0ull; ++k) {
        const bool live = k < len;
        const int64_t idx = live ? (LAMBDA ? len - 1 - k : k) : 0;      // (a group that runs along reads row 0: in bounds, not used)
        const bool last = idx + 1 >= len;
        const double rw = (double)rew[idx * N + i];
        float s[D], ns[D];
        double phs, phn;
        bool tm;
        if (to) {
#pragma unroll
            for (int d = 0; d < D; ++d) { s[d] = from[(idx * D + d) * N + i]; ns[d] = to[(idx * D + d) * N + i]; }
            tm = term[idx * N + i] != 0;
            phs = lstd_feature<DOMAIN, ORDER>(s, r);
            phn = lstd_feature<DOMAIN, ORDER>(ns, r);
        } else if constexpr (LAMBDA) {
            // a record walked backwards: row idx's `to` is the `from` of the row visited before it -- the same state, the same feature bits, kept
            // (the f64 cosine is most of a row's arithmetic); the first visit's is last_to
#pragma unroll
            for (int d = 0; d < D; ++d) s[d] = from[(idx * D + d) * N + i];
            phs = lstd_feature<DOMAIN, ORDER>(s, r);
            phn = k == 0 ? lstd_feature<DOMAIN, ORDER>(last_to, r) : carry;
            carry = phs;
            tm = last && last_term;
        } else {
            // ... walked forwards: row idx's `from` is the `to` of the row visited before it
            const int64_t nx = last ? idx : idx + 1;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                float v = from[(nx * D + d) * N + i];
                // (opaque to the optimiser: a select between this load and last_to[d] otherwise becomes a load through a selected POINTER,
                // which puts last_to into scratch)
                asm volatile("" : "+v"(v));
                ns[d] = last ? last_to[d] : v;
            }
            phn = lstd_feature<DOMAIN, ORDER>(ns, r);
            phs = k == 0 ? lstd_feature<DOMAIN, ORDER>(s0, r) : carry;
            carry = phn;
            tm = last && last_term;
        }
        const double delta = L.accumulate(ls, lv, r, phs, phn, rw, tm, live);
        if (live) {
            acc = acc + fabs(delta);
            if (td_out && r == 0) td_out[idx * N + i] = (float)delta;
        }
    }
    return acc;
}

// the driver loop (Trajectory -> into_batch -> handle, one episode at a time): transition, (from, reward) appended to the learner's record, at
// the episode's end (terminal or max_episode_steps) the sweep over its rows and the solve, then the restart and the Random sample (BLK_STEP;
// BLK_RESET after a cap) -- the environment side is k_train_td's draw for draw, k_train_lstd's loop.  The last row's `to` and terminal flag
// are what the step just produced, passed in registers.  The rows stay in registers for the whole launch.  The statistics' sum |delta| is the
// batch's sum of the diagnostic, booked at the step that ended the episode
template <int DOMAIN, int ORDER, bool LAMBDA>
__global__ __launch_bounds__(kBlock) void k_train_lstd_batch(Common c, LstdBatchState ls, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    using Dom = Domain<DOMAIN>;
    constexpr int D = Dom::D, A = Dom::A, F = FourierReg<DOMAIN, ORDER>::F;
    constexpr int G = LstdGroup<F>::G;
    __shared__ double lds[LstdGroup<F>::kPerBlock][LB_N][F];
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = tid / G;
    const int r = (int)(tid % G);
    const int64_t N = c.n_envs;
    unsigned long long n_ep = 0, n_trunc = 0, sum_len = 0;
    double sum_abs = 0.0, sum_r = 0.0;
    if (i < N) {                                          // (whole groups: a group never straddles the bound)
        double (*lv)[F] = lds[threadIdx.x / G];
        PolicyParams pol = c.pol; pol.kind = POL_RANDOM;
        const float q0[A] = {};
        const uint32_t gid = (uint32_t)(c.env_offset + i);
        const uint32_t cap = c.max_episode_steps;         // (>= 1: admission)
        float s[D];
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] = c.state[(int64_t)d * N + i];
        int a = c.action[i];
        uint32_t ep = c.ep_step[i];
        LstdBatchLane<F, LAMBDA> L;
        L.load(ls, i, r);
        double acc_abs = 0.0, acc_r = 0.0;
        for (int k = 0; k < n_steps; ++k) {
            const uint64_t t = t0 + (uint64_t)k;
            float ns[D];
#pragma unroll
            for (int d = 0; d < D; ++d) ns[d] = s[d];
            float rw;
            const bool term = Dom::step(ns, a, rw);
            ep += 1;
            const bool trunc = !term && ep >= cap;
            const bool has_row = ep <= cap;               // (an episode_steps of cap set from outside: its one step has no row, and ends the episode)
            if (has_row && r == 0) {
                const int64_t row = (int64_t)ep - 1;
#pragma unroll
                for (int d = 0; d < D; ++d) ls.rec_s[(row * D + d) * N + i] = s[d];
                ls.rec_r[row * N + i] = rw;
            }
            lstd_wave_sync();                             // (lane 0's row before the group's reads of it)
            acc_r += (double)rw;
            const bool ended = term || trunc;
            if (__ballot(ended) != 0ull) {
                // (the row-less step: the record's last `to` is this step's `from`, and the step itself is dropped)
                float last_to[D];
#pragma unroll
                for (int d = 0; d < D; ++d) last_to[d] = has_row ? ns[d] : s[d];
                const int64_t len = ended ? (int64_t)(ep < cap ? ep : cap) : 0;
                acc_abs += lstd_batch_sweep<DOMAIN, ORDER, LAMBDA, F>(L, ls, lv, r, ls.rec_s, nullptr, ls.rec_r, nullptr, N, i, len, last_to,
                                                                      has_row && term, nullptr);
                L.solve(lv, r, ended);
            }
            if (term) Dom::reset(ns);
            const U4 x = draw(c.seed, gid, t, BLK_STEP);
            int na = policy_sample<A>(pol, q0, x);
            if (term) { n_ep += 1; sum_len += ep; ep = 0; }
            if (trunc) {
                n_ep += 1; n_trunc += 1; sum_len += ep; ep = 0;
                Dom::reset(ns);
                const U4 xr = draw(c.seed, gid, t, BLK_RESET);
                na = policy_sample<A>(pol, q0, xr);
            }
#pragma unroll
            for (int d = 0; d < D; ++d) s[d] = ns[d];
            a = na;
        }
        L.store(ls, i, r);
        if (r == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) c.state[(int64_t)d * N + i] = s[d];
            c.action[i] = a;
            c.ep_step[i] = ep;
            sum_abs = acc_abs; sum_r = acc_r;
        } else {
            n_ep = 0; n_trunc = 0; sum_len = 0;
        }
    }
    if (stats) block_stats_accumulate(stats, n_ep, n_trunc, sum_len, sum_abs, sum_r);
}

// Handler<&Batch>::handle for every learner: learner i's batch is rows 0 .. len[i]-1 of its column of from / to [T][D][N], rew [T][N] and
// term u8 [T][N] (T >= 1).  The ctx's own record is not touched.  td_out [T][N] (optional): the diagnostic at each handled row, NaN past the
// learner's length.  A learner of length 0 keeps its bytes and is not solved
template <int DOMAIN, int ORDER, bool LAMBDA>
__global__ __launch_bounds__(kBlock) void k_handle_lstd_batch(LstdBatchState ls, const float* __restrict__ from, const float* __restrict__ rew,
                                                              const float* __restrict__ to, const uint8_t* __restrict__ term,
                                                              const uint32_t* __restrict__ len, int64_t T, int64_t N, float* __restrict__ td_out) {
    using Dom = Domain<DOMAIN>;
    constexpr int D = Dom::D, F = FourierReg<DOMAIN, ORDER>::F;
    constexpr int G = LstdGroup<F>::G;
    __shared__ double lds[LstdGroup<F>::kPerBlock][LB_N][F];
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = tid / G;
    const int r = (int)(tid % G);
    if (i >= N) return;                                   // (whole groups: a group never straddles the bound)
    double (*lv)[F] = lds[threadIdx.x / G];
    const int64_t Ln = (int64_t)len[i] < T ? (int64_t)len[i] : T;      // (a device array of lengths is not inspected by the host: clamped here)
    if (td_out && r == 0)
        for (int64_t t = Ln; t < T; ++t) td_out[t * N + i] = __builtin_nanf("");
    if (__ballot(Ln > 0) == 0ull) return;
    LstdBatchLane<F, LAMBDA> L;
    L.load(ls, i, r);
    const float none[D] = {};
    lstd_batch_sweep<DOMAIN, ORDER, LAMBDA, F>(L, ls, lv, r, from, to, rew, term, N, i, Ln, none, false, td_out);
    L.solve(lv, r, Ln > 0);
    if (Ln > 0) L.store(ls, i, r);
}

// the agents' public solve() for every learner: theta <- A.solve(b); A, b and z are not written
template <int DOMAIN, int ORDER, bool LAMBDA>
__global__ __launch_bounds__(kBlock) void k_lstd_batch_solve(LstdBatchState ls, int64_t N) {
    constexpr int F = FourierReg<DOMAIN, ORDER>::F;
    constexpr int G = LstdGroup<F>::G;
    __shared__ double lds[LstdGroup<F>::kPerBlock][LB_N][F];
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = tid / G;
    const int r = (int)(tid % G);
    if (i >= N) return;
    LstdBatchLane<F, LAMBDA> L;
    L.load(ls, i, r);
    L.solve(lds[threadIdx.x / G], r, true);
    L.store_solution(ls, i, r);
}

// ---- LambdaLSPE   rsrl/src/prediction/lstd/lambda_lspe.rs:27-107   theta, A (starts at 1e-6 I), b as above, plus the scalar return correction
// delta and the row count `rows` (LstdBatchState::z holds the pair per learner: z[2 i] = delta, z[2 i + 1] = rows, an exact integer in 0 .. F).
// handle walks the batch LAST TO FIRST (lambda_lspe.rs:72-101); theta does not move during the walk:
//     delta = delta * (gamma * lambda)
//     terminal:      b += (delta + r) phi(s);   A += phi(s) (x) phi(s);   delta = 0            (theta . phi(s) is NOT added: lambda_lspe.rs:81)
//     non-terminal:  v_s = phi(s) . theta, v_n = phi(s') . theta (ascending index, from 0);   delta = delta + (r + gamma * v_n - v_s);
//                    b += (v_s + delta) phi(s);   A += phi(s) (x) phi(s)
// and ends in solve() (lambda_lspe.rs:47-62): x = A.solve(b) by LstdBatchLane::solve's elimination; on success theta_r = (1 - alpha) * theta_r +
// alpha * x_r (1 - alpha once, three rounded operations per element) and A, b, delta are zeroed.  An abandoned elimination keeps theta, A, b AND
// delta (the reference when both of its attempts fail) and counts in singular_solves.
// DEPARTURE, the row rule: the reference's solve() zeroes A and b, so every batch shorter than F leaves a Gram matrix of fewer than F vectors --
// singular in exact arithmetic, answered there by the SVD this library does not have, and in rounding NOT reported by the elimination (pivots near
// 1e-17, one arbitrary member of the solution set).  So each learner counts the rows its A holds: F at create (the identity's), min(rows + len, F)
// after every handled batch, 0 after a successful solve -- and solve() runs the elimination only at rows == F.  Otherwise the solve is DEFERRED:
// nothing moves, singular_solves does not count, the next batch adds to the same A, b and delta.
// The lane is LstdBatchLane<F, false> (row r of A, b_r, theta_r, the elimination) with delta and rows beside it, held redundantly by every lane of
// the group and stored by lane 0.  Instantiated from train_lspe.hip alone: the two agents above keep their machine code.
template <int F>
struct LspeLane {
    LstdBatchLane<F, false> m;
    double delta, rows;

    __device__ __forceinline__ void load(const LstdBatchState& ls, int64_t i, int r) {
        m.load(ls, i, r);
        delta = ls.z[2 * i];
        rows = ls.z[2 * i + 1];
    }
    __device__ __forceinline__ void store_scalars(const LstdBatchState& ls, int64_t i, int r) const {
        if (r != 0) return;
        ls.z[2 * i] = delta;
        ls.z[2 * i + 1] = rows;
    }
    __device__ __forceinline__ void store(const LstdBatchState& ls, int64_t i, int r) const {
        m.store(ls, i, r);
        store_scalars(ls, i, r);
    }

    // one transition of the lane's learner into A, b and delta; arguments and the returned diagnostic as LstdBatchLane::accumulate's -- here the
    // two dot products are part of the rule, and the non-terminal diagnostic IS the rule's residual
    __device__ __forceinline__ double accumulate(const LstdBatchState& ls, double (*lv)[F], int r, double phs, double phn, double rew, bool term, bool live) {
        const double gamma = ls.gamma;
        if (r < F) {
            lv[LB_V][r] = phs;
            lv[LB_X][r] = phs * m.theta;
            lv[LB_Y][r] = phn * m.theta;
        }
        lstd_wave_sync();
        const double v_s = lstd_sum<F>(lv[LB_X]);
        const double v_n = lstd_sum<F>(lv[LB_Y]);
        const double res = term ? rew - v_s : rew + gamma * v_n - v_s;
        const double d0 = delta * (gamma * ls.lambda);
        const double d1 = d0 + res;                       // (non-terminal)
        const double coef = term ? d0 + rew : v_s + d1;
        m.b = live ? m.b + coef * phs : m.b;
#pragma unroll
        for (int j = 0; j < F; ++j) m.row[j] = live ? m.row[j] + phs * lv[LB_V][j] : m.row[j];
        delta = live ? (term ? 0.0 : d1) : delta;
        lstd_wave_sync();                                 // (this transition's reads before the next one's writes)
        return res;
    }

    // the rows a handled batch of `len` transitions adds (len = 0: none)
    __device__ __forceinline__ void count_rows(int64_t len) {
        const double n = rows + (double)len;
        rows = n < (double)F ? n : (double)F;
    }

    // solve() as handle ends with it: the row rule, the relaxed step, the zeroing.  commit: the learner takes part (the other groups of the wave,
    // and the learners whose solve is deferred, run along).  Every lane of the wave calls it
    __device__ __forceinline__ void solve(const LspeState& ls, double (*lv)[F], int r, bool commit) {
        const bool full = commit && rows == (double)F;
        const double theta0 = m.theta;
        const uint32_t sing0 = m.sing;
        m.solve(lv, r, full);                             // theta <- x, or sing + 1
        const bool done = full && m.sing == sing0;
        const double alpha = ls.alpha;
        const double keep = 1.0 - alpha;
        const double relaxed = keep * theta0 + alpha * m.theta;
        m.theta = done ? relaxed : theta0;
#pragma unroll
        for (int j = 0; j < F; ++j) m.row[j] = done ? 0.0 : m.row[j];
        m.b = done ? 0.0 : m.b;
        delta = done ? 0.0 : delta;
        rows = done ? 0.0 : rows;
    }
};

// Handler<&Batch>::handle's walk for LambdaLSPE, without the solve: lstd_batch_sweep's arguments, walked last to first as its LSTDLambda branch
// (a record's phi(s) is kept as the next visit's phi(s'))
template <int DOMAIN, int ORDER, int F>
__device__ __forceinline__ double lspe_sweep(LspeLane<F>& L, const LstdBatchState& ls, double (*lv)[F], int r, const float* from, const float* to,
                                             const float* rew, const uint8_t* term, int64_t N, int64_t i, int64_t len,
                                             const float (&last_to)[Domain<DOMAIN>::D], bool last_term, float* __restrict__ td_out) {
    constexpr int D = Domain<DOMAIN>::D;
    double acc = 0.0, carry = 0.0;
    for (int64_t k = 0; __ballot(k < len) != 0ull; ++k) {
        const bool live = k < len;
        const int64_t idx = live ? len - 1 - k : 0;       // (a group that runs along reads row 0: in bounds, not used)
        const bool last = idx + 1 >= len;
        const double rw = (double)rew[idx * N + i];
        float s[D];
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] = from[(idx * D + d) * N + i];
        const double phs = lstd_feature<DOMAIN, ORDER>(s, r);
        double phn;
        bool tm;
        if (to) {
            float ns[D];
#pragma unroll
            for (int d = 0; d < D; ++d) ns[d] = to[(idx * D + d) * N + i];
            tm = term[idx * N + i] != 0;
            phn = lstd_feature<DOMAIN, ORDER>(ns, r);
        } else {
            phn = k == 0 ? lstd_feature<DOMAIN, ORDER>(last_to, r) : carry;
            carry = phs;
            tm = last && last_term;
        }
        const double res = L.accumulate(ls, lv, r, phs, phn, rw, tm, live);
        if (live) {
            acc = acc + fabs(res);
            if (td_out && r == 0) td_out[idx * N + i] = (float)res;
        }
    }
    return acc;
}

// LambdaLSPE's driver loop: k_train_lstd_batch's, draw for draw -- the record, the episode's end, the restart and the Random sample are that kernel's
// text; the sweep and the solve are this agent's
template <int DOMAIN, int ORDER>
__global__ __launch_bounds__(kBlock) void k_train_lspe(Common c, LspeState ls, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    using Dom = Domain<DOMAIN>;
    constexpr int D = Dom::D, A = Dom::A, F = FourierReg<DOMAIN, ORDER>::F;
    constexpr int G = LstdGroup<F>::G;
    __shared__ double lds[LstdGroup<F>::kPerBlock][LB_N][F];
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = tid / G;
    const int r = (int)(tid % G);
    const int64_t N = c.n_envs;
    unsigned long long n_ep = 0, n_trunc = 0, sum_len = 0;
    double sum_abs = 0.0, sum_r = 0.0;
    if (i < N) {                                          // (whole groups: a group never straddles the bound)
        double (*lv)[F] = lds[threadIdx.x / G];
        PolicyParams pol = c.pol; pol.kind = POL_RANDOM;
        const float q0[A] = {};
        const uint32_t gid = (uint32_t)(c.env_offset + i);
        const uint32_t cap = c.max_episode_steps;         // (>= 1: admission)
        float s[D];
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] = c.state[(int64_t)d * N + i];
        int a = c.action[i];
        uint32_t ep = c.ep_step[i];
        LspeLane<F> L;
        L.load(ls, i, r);
        double acc_abs = 0.0, acc_r = 0.0;
        for (int k = 0; k < n_steps; ++k) {
            const uint64_t t = t0 + (uint64_t)k;
            float ns[D];
#pragma unroll
            for (int d = 0; d < D; ++d) ns[d] = s[d];
            float rw;
            const bool term = Dom::step(ns, a, rw);
            ep += 1;
            const bool trunc = !term && ep >= cap;
            const bool has_row = ep <= cap;               // (an episode_steps of cap set from outside: its one step has no row, and ends the episode)
            if (has_row && r == 0) {
                const int64_t row = (int64_t)ep - 1;
#pragma unroll
                for (int d = 0; d < D; ++d) ls.rec_s[(row * D + d) * N + i] = s[d];
                ls.rec_r[row * N + i] = rw;
            }
            lstd_wave_sync();                             // (lane 0's row before the group's reads of it)
            acc_r += (double)rw;
            const bool ended = term || trunc;
            if (__ballot(ended) != 0ull) {
                // (the row-less step: the record's last `to` is this step's `from`, and the step itself is dropped)
                float last_to[D];
#pragma unroll
                for (int d = 0; d < D; ++d) last_to[d] = has_row ? ns[d] : s[d];
                const int64_t len = ended ? (int64_t)(ep < cap ? ep : cap) : 0;
                acc_abs += lspe_sweep<DOMAIN, ORDER, F>(L, ls, lv, r, ls.rec_s, nullptr, ls.rec_r, nullptr, N, i, len, last_to, has_row && term, nullptr);
                L.count_rows(len);
                L.solve(ls, lv, r, ended);
            }
            if (term) Dom::reset(ns);
            const U4 x = draw(c.seed, gid, t, BLK_STEP);
            int na = policy_sample<A>(pol, q0, x);
            if (term) { n_ep += 1; sum_len += ep; ep = 0; }
            if (trunc) {
                n_ep += 1; n_trunc += 1; sum_len += ep; ep = 0;
                Dom::reset(ns);
                const U4 xr = draw(c.seed, gid, t, BLK_RESET);
                na = policy_sample<A>(pol, q0, xr);
            }
#pragma unroll
            for (int d = 0; d < D; ++d) s[d] = ns[d];
            a = na;
        }
        L.store(ls, i, r);
        if (r == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) c.state[(int64_t)d * N + i] = s[d];
            c.action[i] = a;
            c.ep_step[i] = ep;
            sum_abs = acc_abs; sum_r = acc_r;
        } else {
            n_ep = 0; n_trunc = 0; sum_len = 0;
        }
    }
    if (stats) block_stats_accumulate(stats, n_ep, n_trunc, sum_len, sum_abs, sum_r);
}

// Handler<&Batch>::handle of LambdaLSPE for every learner: k_handle_lstd_batch's arguments and conventions (a learner of length 0 keeps its bytes:
// no rows counted, no solve)
template <int DOMAIN, int ORDER>
__global__ __launch_bounds__(kBlock) void k_handle_lspe(LspeState ls, const float* __restrict__ from, const float* __restrict__ rew,
                                                        const float* __restrict__ to, const uint8_t* __restrict__ term,
                                                        const uint32_t* __restrict__ len, int64_t T, int64_t N, float* __restrict__ td_out) {
    using Dom = Domain<DOMAIN>;
    constexpr int D = Dom::D, F = FourierReg<DOMAIN, ORDER>::F;
    constexpr int G = LstdGroup<F>::G;
    __shared__ double lds[LstdGroup<F>::kPerBlock][LB_N][F];
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = tid / G;
    const int r = (int)(tid % G);
    if (i >= N) return;                                   // (whole groups: a group never straddles the bound)
    double (*lv)[F] = lds[threadIdx.x / G];
    const int64_t Ln = (int64_t)len[i] < T ? (int64_t)len[i] : T;      // (a device array of lengths is not inspected by the host: clamped here)
    if (td_out && r == 0)
        for (int64_t t = Ln; t < T; ++t) td_out[t * N + i] = __builtin_nanf("");
    if (__ballot(Ln > 0) == 0ull) return;
    LspeLane<F> L;
    L.load(ls, i, r);
    const float none[D] = {};
    lspe_sweep<DOMAIN, ORDER, F>(L, ls, lv, r, from, to, rew, term, N, i, Ln, none, false, td_out);
    L.count_rows(Ln);
    L.solve(ls, lv, r, Ln > 0);
    if (Ln > 0) L.store(ls, i, r);
}

// LambdaLSPE's solve() for every learner, exactly as handle ends with it (private in the reference: lambda_lspe.rs:47)
template <int DOMAIN, int ORDER>
__global__ __launch_bounds__(kBlock) void k_lspe_solve(LspeState ls, int64_t N) {
    constexpr int F = FourierReg<DOMAIN, ORDER>::F;
    constexpr int G = LstdGroup<F>::G;
    __shared__ double lds[LstdGroup<F>::kPerBlock][LB_N][F];
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = tid / G;
    const int r = (int)(tid % G);
    if (i >= N) return;
    LspeLane<F> L;
    L.load(ls, i, r);
    L.solve(ls, lds[threadIdx.x / G], r, true);
    L.store(ls, i, r);
}

}  // namespace rsrl
