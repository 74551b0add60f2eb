// kernels_lstd.hpp -- the incremental least-squares prediction agents (Handler<&Transition>) on the register-family Fourier orders:
//   RecursiveLSTD   rsrl/src/prediction/lstd/recursive_lstd.rs    theta f64[F], C f64[F][F] (Sherman-Morrison), C starts at 1e-5 I
//   iLSTD           rsrl/src/prediction/lstd/ilstd.rs             theta f64[F], A f64[F][F] (starts at I), mu f64[F]; solve(): n_updates rounds
//   argmaxima       rsrl/src/utils.rs:6-21                        tolerance first (|v - max| < 1e-7 appends), then v > max restarts the list
// Everything the agents compute is f64, the features included: phi_k(s) = cos(pi * sum_d c_kd * (s_d - lo_d) / (hi_d - lo_d)) evaluated in f64
// from the f32 state (the f32 phi of the other register kernels is up to 3e-6 off, an error of its own inside a least-squares state).
//
// Layout.  A learner is a GROUP of G lanes, G = the power of two >= F (4, 16, 32, 64), 64 / G learners per wave.  Lane r < F owns row r of the
// matrix (F doubles in registers), theta_r and mu_r, and evaluates feature r.  Every matrix-vector product is then lane-local (row r times a
// vector), and iLSTD's column A[:,j] is lane r's element j.  The vectors a row is multiplied with (phi(s), pd, g) and the terms of the dot
// products are broadcast through a slice of LDS per group; dot products are summed in index order by every lane of the group (the same bits in
// each).  A group lies inside one wave: a wave-scope fence is all the exchange needs.  Lanes r >= F carry no state and write nothing.
// State in memory is learner-major: theta [N][F], the matrix [N][F][F] (row-major: each learner's block contiguous), mu [N][F].
//
// RecursiveLSTD::handle, literally (every product rounded, -ffp-contract=off; pd = phi_s - gamma * phi_ns):
//   non-terminal  g = C pd; a = 1 + g . phi_s; v = C phi_s; C[r][j] += (-1/a) * (v_r * g_j); theta += (residual / a) v,
//                 residual = r + gamma * theta.phi_ns - theta.phi_s
//   terminal      v = C phi_s; a = 1 + v . phi_s; C = 0; theta += ((r - theta.phi_s) / a) v
// The terminal branch is computed as the non-terminal one with pd := phi_s (then g = v, the same bits) and C selected to zero.  After a learner's
// first terminal transition C stays zero and theta never moves again: that is what the reference does.
// iLSTD::handle, literally: mu += r phi_s; A += phi_s pd^T (terminal: pd = phi_s); mu -= (phi_s pd^T) theta, computed as phi_s[i] * (pd . theta)
// (a rounding difference against the rounded outer product's row dot theta); then n_updates rounds of solve(): idx = argmaxima(|mu|), and for each j
// in idx IN ORDER: u = alpha * mu[j]; theta[j] += u; mu += (-u) A[:,j] -- a later j reads the mu an earlier one changed.
// The step's delta (handle's td_error_out, the statistics' sum |delta|): RecursiveLSTD's residual; iLSTD computes none and reports the diagnostic
// r + gamma * V(s') - V(s) (terminal: r - V(s)) with theta before the update.
// LstdLane::step is the ONE update both kernels run: train, handle and the trait-granular loop give the same bits.
#pragma once

#include "launch.hpp"

namespace rsrl {

enum : int { LSTD_RECURSIVE = 0, LSTD_INCREMENTAL = 1 };

// lanes per learner: the power of two >= F
template <int F>
struct LstdGroup {
    static constexpr int G = F <= 4 ? 4 : (F <= 16 ? 16 : (F <= 32 ? 32 : 64));
    static_assert(F <= 64, "a learner's rows must fit one wave");
    static constexpr int kPerBlock = kBlock / G;      // learners per block
};

// LDS vectors of one group
enum : int { LV_PHS = 0, LV_PD = 1, LV_X = 2, LV_Y = 3, LV_Z = 4, LV_G = 5, LV_N = 6 };

// the group's LDS slice is private to its wave: ordering the writes before the reads needs no block barrier
__device__ __forceinline__ void lstd_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// feature r of the Fourier basis in f64 (oracle fourier_project(..., "f64")): coefficient vector k = r + 1 (digits of k, dimension 0 most
// significant), the constant feature last (r = F - 1)
template <int DOMAIN, int ORDER>
__device__ __forceinline__ double lstd_feature(const float (&s)[Domain<DOMAIN>::D], int r) {
    using Dom = Domain<DOMAIN>;
    constexpr int D = Dom::D, N1 = ORDER + 1, F = FourierReg<DOMAIN, ORDER>::F;
    int cd[D];
    int rem = r + 1;
#pragma unroll
    for (int d = D - 1; d >= 0; --d) { cd[d] = rem % N1; rem /= N1; }
    double cx = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double sc = ((double)s[d] - Dom::lo_d(d)) / (Dom::hi_d(d) - Dom::lo_d(d));
        cx = cx + (double)cd[d] * sc;
    }
    return r >= F - 1 ? 1.0 : cos(M_PI * cx);
}

// sum_j v[j] in index order from 0.0
template <int F>
__device__ __forceinline__ double lstd_sum(const double* __restrict__ v) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < F; ++j) acc = acc + v[j];
    return acc;
}

// one lane's share of a learner: row r of the matrix, theta_r, mu_r
template <int F, int ALGO>
struct LstdLane {
    double row[F];
    double theta, mu;

    __device__ __forceinline__ void load(const LstdState& ls, int64_t i, int r) {
        const int rr = r < F ? r : 0;                     // (lanes past F read row 0 and never store)
        const double* p = ls.mat + ((int64_t)i * F + rr) * F;
#pragma unroll
        for (int j = 0; j < F; ++j) row[j] = p[j];
        theta = ls.theta[(int64_t)i * F + rr];
        mu = ALGO == LSTD_INCREMENTAL ? ls.mu[(int64_t)i * F + rr] : 0.0;
    }
    __device__ __forceinline__ void store(const LstdState& ls, int64_t i, int r) const {
        if (r >= F) return;
        double* p = ls.mat + ((int64_t)i * F + r) * F;
#pragma unroll
        for (int j = 0; j < F; ++j) p[j] = row[j];
        ls.theta[(int64_t)i * F + r] = theta;
        if (ALGO == LSTD_INCREMENTAL) ls.mu[(int64_t)i * F + r] = mu;
    }

    // one transition of the lane's learner.  phs / phn: this lane's features of s and s'; lv: the group's LDS vectors, lv[LV_PHS] already holds
    // phi(s) of every lane (written and fenced by the caller).  G: the group's lane count (the shuffles of iLSTD's solve).  Returns delta.
    template <int G>
    __device__ __forceinline__ double step(const LstdState& ls, double (*lv)[F], int r, double phs, double phn, double rew, bool term) {
        const double gamma = ls.gamma;
        const bool own = r < F;
        const double pd = term ? phs : phs - gamma * phn;
        if (own) {
            lv[LV_PD][r] = pd;
            lv[LV_X][r] = phs * theta;
            lv[LV_Y][r] = phn * theta;
            if (ALGO == LSTD_INCREMENTAL) lv[LV_Z][r] = pd * theta;
        }
        lstd_wave_sync();
        const double theta_s = lstd_sum<F>(lv[LV_X]);
        const double theta_ns = lstd_sum<F>(lv[LV_Y]);
        const double residual = term ? rew - theta_s : rew + gamma * theta_ns - theta_s;
        if constexpr (ALGO == LSTD_RECURSIVE) {
            double g = 0.0, v = 0.0;
#pragma unroll
            for (int j = 0; j < F; ++j) {
                g = g + row[j] * lv[LV_PD][j];
                v = v + row[j] * lv[LV_PHS][j];
            }
            if (own) { lv[LV_G][r] = g; lv[LV_Z][r] = g * phs; }
            lstd_wave_sync();
            const double a = 1.0 + lstd_sum<F>(lv[LV_Z]);
            const double sc = -1.0 / a;
#pragma unroll
            for (int j = 0; j < F; ++j) row[j] = term ? 0.0 : row[j] + sc * (v * lv[LV_G][j]);
            theta = theta + (residual / a) * v;
            return residual;
        } else {
            const double pdt = lstd_sum<F>(lv[LV_Z]);
            mu = mu + rew * phs;
#pragma unroll
            for (int j = 0; j < F; ++j) row[j] = row[j] + phs * lv[LV_PD][j];
            mu = mu - phs * pdt;
            const double alpha = ls.alpha;
            for (int u = 0; u < ls.n_updates; ++u) {
                // argmaxima(|mu|): every lane of the group scans the same values in index order
                if (own) lv[LV_G][r] = mu;
                lstd_wave_sync();
                double mx = -1.7976931348623157e308;      // f64::MIN
                uint64_t idx = 0;
#pragma unroll
                for (int j = 0; j < F; ++j) {
                    const double x = fabs(lv[LV_G][j]);
                    const bool tie = fabs(x - mx) < 1e-7;
                    const bool up = !tie && x > mx;
                    idx = tie ? (idx | (1ull << j)) : (up ? (1ull << j) : idx);
                    mx = up ? x : mx;
                }
                lstd_wave_sync();                         // (LV_G is written again by the next round)
                // for each j in idx in order; a wave skips the j that none of its groups holds
#pragma unroll
                for (int j = 0; j < F; ++j) {
                    const bool in = (idx >> j) & 1ull;
                    if (__ballot(in) != 0ull) {
                        const double muj = __shfl(mu, j, G);
                        const double upd = alpha * muj;
                        theta = (in && r == j) ? theta + upd : theta;
                        mu = in ? mu + (-upd) * row[j] : mu;
                    }
                }
            }
            return residual;
        }
    }
};

// TDCritic::target (ac.rs:87-98) from an iLSTD lane's UPDATED theta, for the actor-critics that own one (kernels_tdac_lstd.hpp, kernels_tdac_beta.hpp):
// c = r - V(s') (terminal: V of the terminal state itself) | r + gamma*V(s') - V(s), every product rounded, summed in index order.  Called after
// LstdLane::step with its phs / phn.  Returns c in f64: the caller rounds e = (float)(alpha * c) itself (with alpha passed in and the product
// here, k_train_tdac_beta<5> gains two scalar spills).  theta and gamma arrive by REFERENCE: by value they are read before the first wave sync,
// and k_handle_tdac_lstd<0, 4> then takes 322 registers for 256 (one wave per SIMD for two; profiles/group_frame.md)
template <int F>
__device__ __forceinline__ double tdcritic_target(const double& theta, const double& gamma, double (*lv)[F], int r, double phs, double phn,
                                                  double rew, bool term) {
    lstd_wave_sync();                                     // (the solve's reads of the slice before it is written again)
    if (r < F) {
        lv[LV_X][r] = phs * theta;
        lv[LV_Y][r] = phn * theta;
    }
    lstd_wave_sync();
    const double v_s = lstd_sum<F>(lv[LV_X]);
    const double v_n = lstd_sum<F>(lv[LV_Y]);
    return term ? rew - v_n : rew + gamma * v_n - v_s;
}

// ---- Handler<&Transition>::handle's prologue in the lane-group layout, shared by k_handle_lstd, k_handle_tdac_lstd and k_handle_tdac_beta: which
// transition and which row this lane is, the group's LDS slice (the __shared__ array stays declared in the kernel), the return value by lane 0.
// An AGGREGATE made by here(): with a constructor k_handle_tdac_lstd<0, 5> and its unit's driver loop gain scalar spills (profiles/group_frame.md).
// The layout's four DRIVER LOOPS (k_train_lstd, k_train_tdac_lstd, k_train_tdac_beta, k_train_lstd_batch) are on no frame: each keeps its own text,
// with the convention it follows named above it -- on shared learner / tally / episode-end pieces 11 instantiations gained scalar spills
template <int F, int NVEC>
struct GroupId {
    static constexpr int G = LstdGroup<F>::G;
    int64_t i;             // transition (= learner) of this group; whole groups leave at `i >= Mn`: a group never straddles the bound
    int r;                 // lane of the group: row r for r < F; lanes r >= F carry no state and write nothing

    __device__ __forceinline__ static GroupId here() {
        const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        return GroupId{tid / G, (int)(tid % G)};
    }
    __device__ __forceinline__ bool own() const { return r < F; }
    using Slice = double (*)[F];
    __device__ __forceinline__ Slice slice(double (&lds)[LstdGroup<F>::kPerBlock][NVEC][F]) const { return lds[threadIdx.x / G]; }
    __device__ __forceinline__ void report(float* __restrict__ td_out, double delta) const { if (td_out && r == 0) td_out[i] = (float)delta; }
};
// ... and transition i of the caller's batch of Mn.  The kernel reads the reward where the step reads it, (double)rew[i], and an agent's action itself
template <int D>
struct GroupGiven {
    float s[D], ns[D];
    bool term;
    __device__ __forceinline__ void load(const float* __restrict__ from, const float* __restrict__ to, const uint8_t* __restrict__ termf, int64_t Mn, int64_t i) {
#pragma unroll
        for (int d = 0; d < D; ++d) { s[d] = from[(int64_t)d * Mn + i]; ns[d] = to[(int64_t)d * Mn + i]; }
        term = termf[i] != 0;
    }
};

// the driver loop (prediction with a Random behaviour policy, as k_train_td): transition, handle, a' ~ Random (BLK_STEP; BLK_RESET after a cap),
// auto-reset; truncation at max_episode_steps is not terminal.  Every lane of a group steps the learner's environment (the same bits in each);
// the rows stay in registers for the whole launch
template <int DOMAIN, int ORDER, int ALGO>
__global__ __launch_bounds__(kBlock) void k_train_lstd(Common c, LstdState ls, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    using Dom = Domain<DOMAIN>;
    constexpr int D = Dom::D, A = Dom::A, F = FourierReg<DOMAIN, ORDER>::F;
    constexpr int G = LstdGroup<F>::G;
    __shared__ double lds[LstdGroup<F>::kPerBlock][LV_N][F];
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = tid / G;
    const int r = (int)(tid % G);
    const int64_t N = c.n_envs;
    unsigned long long n_ep = 0, n_trunc = 0, sum_len = 0;
    double sum_abs = 0.0, sum_r = 0.0;
    if (i < N) {
        double (*lv)[F] = lds[threadIdx.x / G];
        PolicyParams pol = c.pol; pol.kind = POL_RANDOM;
        const float q0[A] = {};
        const uint32_t gid = (uint32_t)(c.env_offset + i);
        const uint32_t cap = c.max_episode_steps;
        float s[D];
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] = c.state[(int64_t)d * N + i];
        int a = c.action[i];
        uint32_t ep = c.ep_step[i];
        LstdLane<F, ALGO> L;
        L.load(ls, i, r);
        double phs = lstd_feature<DOMAIN, ORDER>(s, r);
        double acc_abs = 0.0, acc_r = 0.0;
        for (int k = 0; k < n_steps; ++k) {
            const uint64_t t = t0 + (uint64_t)k;
            if (r < F) lv[LV_PHS][r] = phs;
            float ns[D];
#pragma unroll
            for (int d = 0; d < D; ++d) ns[d] = s[d];
            float rw;
            const bool term = Dom::step(ns, a, rw);
            ep += 1;
            const bool trunc = !term && cap > 0 && ep >= cap;
            if (term) Dom::reset(ns);
            double phn = lstd_feature<DOMAIN, ORDER>(ns, r);
            const double delta = L.template step<G>(ls, lv, r, phs, phn, (double)rw, term);
            acc_abs += fabs(delta); acc_r += (double)rw;
            const U4 x = draw(c.seed, gid, t, BLK_STEP);
            int na = policy_sample<A>(pol, q0, x);
            if (term) { n_ep += 1; sum_len += ep; ep = 0; }
            if (trunc) {
                n_ep += 1; n_trunc += 1; sum_len += ep; ep = 0;
                Dom::reset(ns);
                phn = lstd_feature<DOMAIN, ORDER>(ns, r);
                const U4 xr = draw(c.seed, gid, t, BLK_RESET);
                na = policy_sample<A>(pol, q0, xr);
            }
#pragma unroll
            for (int d = 0; d < D; ++d) s[d] = ns[d];
            phs = phn;
            a = na;
            lstd_wave_sync();                             // (this step's reads of LV_PHS before the next step's write)
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

// Handler<&Transition>::handle on caller-supplied transitions: transition i is learner i's; the state streams through memory
template <int DOMAIN, int ORDER, int ALGO>
__global__ __launch_bounds__(kBlock) void k_handle_lstd(LstdState ls, const float* __restrict__ from, const float* __restrict__ rew,
                                                        const float* __restrict__ to, const uint8_t* __restrict__ termf, int64_t Mn,
                                                        float* __restrict__ td_out) {
    constexpr int D = Domain<DOMAIN>::D, F = FourierReg<DOMAIN, ORDER>::F;
    using Grp = GroupId<F, LV_N>;
    __shared__ double lds[LstdGroup<F>::kPerBlock][LV_N][F];
    const Grp g = Grp::here();
    if (g.i >= Mn) return;
    double (*lv)[F] = g.slice(lds);
    GroupGiven<D> tr;
    tr.load(from, to, termf, Mn, g.i);
    LstdLane<F, ALGO> L;
    L.load(ls, g.i, g.r);
    const double phs = lstd_feature<DOMAIN, ORDER>(tr.s, g.r);
    const double phn = lstd_feature<DOMAIN, ORDER>(tr.ns, g.r);
    if (g.own()) lv[LV_PHS][g.r] = phs;
    const double delta = L.template step<Grp::G>(ls, lv, g.r, phs, phn, (double)rew[g.i], tr.term);
    L.store(ls, g.i, g.r);
    g.report(td_out, delta);
}

// V(s) = phi(s) . theta in f64, rounded to f32: state i against learner i's theta, one thread per state
template <int DOMAIN, int ORDER>
__global__ __launch_bounds__(kBlock) void k_lstd_v(const double* __restrict__ theta, const float* __restrict__ states, int64_t Mn, float* __restrict__ out) {
    using Dom = Domain<DOMAIN>;
    constexpr int D = Dom::D, F = FourierReg<DOMAIN, ORDER>::F;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    float s[D];
#pragma unroll
    for (int d = 0; d < D; ++d) s[d] = states[(int64_t)d * Mn + i];
    double v = 0.0;
    for (int f = 0; f < F; ++f) v = v + lstd_feature<DOMAIN, ORDER>(s, f) * theta[i * F + f];
    out[i] = (float)v;
}

// Random.sample for the ctx's own learners as the driver loop draws it (batch-step t, stream blk); the actions become the ctx's pending ones
template <int DOMAIN>
__global__ __launch_bounds__(kBlock) void k_lstd_sample(Common c, uint64_t t, uint32_t blk, int32_t* __restrict__ out) {
    constexpr int A = Domain<DOMAIN>::A;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n_envs) return;
    PolicyParams pol = c.pol; pol.kind = POL_RANDOM;
    const float q0[A] = {};
    const int a = policy_sample<A>(pol, q0, draw(c.seed, (uint32_t)(c.env_offset + i), t, blk));
    c.action[i] = a;
    out[i] = a;
}

}  // namespace rsrl
