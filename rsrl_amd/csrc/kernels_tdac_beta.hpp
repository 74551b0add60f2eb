// kernels_tdac_beta.hpp -- ActorCritic::tdac with an iLSTD critic and a Beta policy on ContinuousMountainCar, the agent of examples/tdac_beta.rs:
//   the domain                     rsrl_domains/src/mountain_car/continuous.rs: Domain<4> (device_core.hpp), one f32 action in [-1, 1]
//   ActorCritic::tdac / TDCritic   rsrl/src/control/ac.rs; the V learner iLSTD (prediction/lstd/ilstd.rs): kernels_tdac_lstd.hpp's critic half, unchanged
//   the actor                      Beta (rsrl/src/policies/beta.rs) over two Composition<ScalarLFA, Softplus> (fa/composition.rs:98-115, fa/transforms.rs:196-218)
// Per learner: iLSTD's f64 theta / A / mu (kernels_lstd.hpp's layout) and the policy's two weight columns w_a, w_b f32[2][F][N] (the ctx's auxiliary
// matrix, what rsrl_hip_get/set_policy_weights show as (F, 2): column 0 = alpha's, column 1 = beta's).  With x_a = <w_a, phi32(s)>, x_b likewise:
//     alpha = softplus(x_a) + 1, beta = softplus(x_b) + 1         softplus(x) = x for x >= 10, else ln(1 + exp(x)); MIN_TOL = 1.0 (beta.rs:19, :58-67)
// so both are >= 1 always (the sampler relies on it).  Per transition (s, a, r, s', term), in tdac_beta.rs's order:
//     alpha, beta at s from the PRE-update columns
//     iLSTD   LstdLane<F, LSTD_INCREMENTAL>::step, the bits of an RSRL_ILSTD ctx's on the same transitions
//     critic  TdacLstdLane::step's target from the updated f64 theta (V of the terminal state itself on a terminal transition)
//     e       = (float)(ActorCritic.alpha * c), the one rounding out of f64
//     actor   g_a = ln a - psi(alpha) + psi(alpha + beta),  g_b = ln(1 - a) - psi(beta) + psi(alpha + beta)       (psi = digamma)
//             w_a += e * g_a * sigma(x_a) * phi(s),  w_b += e * g_b * sigma(x_b) * phi(s)      sigma = Softplus's gradient: 1 for x >= 10, else the logistic
// The score is RECALLED from rstat::univariate::beta (the crate is not in the reference tree): the library's definition, DESIGN 6.  The action's
// logarithms are taken of the action clamped to the sample's interval [2^-24, 1 - 2^-24] -- a departure from the reference, which would produce
// infinities for a caller's 0 or 1, in the spirit of clamp_action.
// Sampling: X = Ga / (Ga + Gb), Ga ~ Gamma(alpha, 1), Gb ~ Gamma(beta, 1) by Marsaglia-Tsang (d = k - 1/3, c = 1 / sqrt(9 d)).  Round j of the sample
// for purpose P (BLK_STEP -- BLK_RESET is its alias --, BLK_INIT, BLK_API) takes the WHOLE Philox block at block word P + 256 * (j + 1) (every other
// stream uses block words < 256): words x, y give two normals by Box-Muller (the cosine one is Ga's, the sine one Gb's), word z is Ga's acceptance
// uniform, word w Gb's.  At most kBetaRounds rounds per gamma; a gamma not accepted by then is d.  The loop holds no shuffle, no wave barrier and no
// LDS access: the groups of one wave leave it at different rounds, and every lane of a group runs it on identical inputs.  The sample is a function of
// (seed, global learner id, t, purpose) only.  Mode (beta.rs:141-150; rstat's modes() is not in the tree -- the library's definition):
// (alpha - 1) / (alpha + beta - 2) if both exceed 1, else the mean alpha / (alpha + beta).
//
// Layout: kernels_tdac_lstd.hpp's.  Lane 0 of a learner's group owns w_a, lane 1 owns w_b (G >= 4 at every order; lanes >= 2 carry a copy of w_b and
// never store it); the two preferences are exchanged by shuffle before the scalar chain, which every lane runs.  TdacBetaLane::step is the ONE step
// both kernels below run.
#pragma once

#include "kernels_lstd.hpp"
#include "kernels_tdac.hpp"

namespace rsrl {

constexpr int kCmc = 4;                                   // RSRL_CONTINUOUS_MOUNTAIN_CAR
constexpr int kBetaRounds = 8;
constexpr float kBetaLo = 5.9604644775390625e-08f;        // 2^-24
constexpr float kBetaHi = 0.999999940395355224609375f;    // 1 - 2^-24

// Softplus and its gradient (fa/transforms.rs:196-218).  The sum u = 1 + e^x is a multiple of 2^-23, so the literal ln(u) carries an absolute error
// of 6e-8 for every negative x.  That is nothing beside Beta's + 1 (alpha and beta have that spacing anyway), and softplus_dev stays the literal
// form: the Beta agents' runs keep their bits.  It is 6e-6 of the Gaussian's sd at its 0.01 floor: gauss_params takes softplus_rel_dev, which
// keeps Softplus's RELATIVE accuracy.  The rounding error of the sum, r = (u - 1) - e^x, is exact for x <= 0, and
// ln(1 + e^x) = ln(u - r) = ln(u) - r / u to first order: one v_rcp_f32 (the term is below 6e-8, its own relative error does not matter), where
// log1pf costs 0.37 us per batch-step (tests/continuous_edges.py, profiles/continuous_edges.md)
__device__ __forceinline__ float softplus_dev(float x) { return x >= 10.0f ? x : logf(1.0f + exp_dev(x)); }
__device__ __forceinline__ float softplus_rel_dev(float x) {
    if (x >= 10.0f) return x;
    const float e = exp_dev(x), u = 1.0f + e;
    return fmaf(e - (u - 1.0f), __builtin_amdgcn_rcpf(u), logf(u));
}
__device__ __forceinline__ float softplus_grad_dev(float x) {
    if (x >= 10.0f) return 1.0f;
    // the stable logistic: no overflow on either side.  exp_dev is 0 below -87 where e^x is a subnormal: there e^x = e^(x + 40) e^-40, the sum exact
    const bool far = x < -80.0f;
    const float e0 = exp_dev(far ? x + 40.0f : -fabsf(x));
    const float e = far ? e0 * 4.248354255291589e-18f : e0;
    return x >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}
// digamma for x >= 1: the recurrence psi(x) = psi(x + 1) - 1 / x up to an argument >= 6 (at most five steps), then the asymptotic series
__device__ __forceinline__ float digamma_dev(float x) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const bool low = x < 6.0f;
        acc = low ? acc - 1.0f / x : acc;
        x = low ? x + 1.0f : x;
    }
    const float inv = 1.0f / x, inv2 = inv * inv;
    float p = 1.0f / 240.0f;                              // - 1/(12 x^2) + 1/(120 x^4) - 1/(252 x^6) + 1/(240 x^8)
    p = fmaf(p, inv2, -1.0f / 252.0f);
    p = fmaf(p, inv2, 1.0f / 120.0f);
    p = fmaf(p, inv2, -1.0f / 12.0f);
    return acc + (logf(x) - 0.5f * inv + p * inv2);
}
__device__ __forceinline__ void beta_params(float xa, float xb, float& alpha, float& beta) {
    alpha = softplus_dev(xa) + 1.0f;
    beta = softplus_dev(xb) + 1.0f;
}
// (alpha - 1) / (alpha + beta - 2) with the denominator formed as (alpha - 1) + (beta - 1): both differences are exact, where alpha + beta rounds to
// a multiple of 2^-22 first -- for parameters a few ulps above 1 (preferences in (-17, -10)) that rounding moved the mode by up to a third
// (tests/fuzz_beta.py's finding)
__device__ __forceinline__ float beta_mode(float alpha, float beta) {
    const float am = alpha - 1.0f, bm = beta - 1.0f;
    return (alpha > 1.0f && beta > 1.0f) ? am / (am + bm) : alpha / (alpha + beta);
}
__device__ __forceinline__ float beta_clamp(float a) { return fminf(fmaxf(a, kBetaLo), kBetaHi); }      // (NaN -> kBetaLo)
// the density, through ln Gamma: exp((alpha - 1) ln a + (beta - 1) ln(1 - a) - ln B(alpha, beta)) of the clamped action
__device__ __forceinline__ float beta_pdf(float alpha, float beta, float a) {
    const float ac = beta_clamp(a);
    const float lnb = lgammaf(alpha) + lgammaf(beta) - lgammaf(alpha + beta);
    return expf((alpha - 1.0f) * logf(ac) + (beta - 1.0f) * logf(1.0f - ac) - lnb);
}
// one Marsaglia-Tsang round: the candidate d v of Gamma(k, 1) from the normal n, accepted against the uniform u in (0, 1]
__device__ __forceinline__ bool gamma_round(float d, float c, float n, float u, float& out) {
    const float t = 1.0f + c * n;
    const float v = t * t * t;
    const bool ok = v > 0.0f && logf(u) < 0.5f * n * n + d - d * v + d * logf(v);
    out = d * v;
    return ok;
}
// the sample of (seed, gid, t, purpose); alpha, beta >= 1
__device__ __forceinline__ float beta_sample(uint64_t seed, uint32_t gid, uint64_t t, uint32_t purpose, float alpha, float beta) {
    const float da = alpha - 1.0f / 3.0f, db = beta - 1.0f / 3.0f;
    const float ca = 1.0f / sqrtf(9.0f * da), cb = 1.0f / sqrtf(9.0f * db);
    float ga = da, gb = db;
    bool got_a = false, got_b = false;
    for (int j = 0; j < kBetaRounds; ++j) {
        if (got_a && got_b) break;
        const U4 x = draw_block(seed, gid, t, purpose + 256u * (uint32_t)(j + 1));
        const float u1 = (float)((x.x >> 8) + 1u) * (1.0f / 16777216.0f);      // (0, 1]
        const float u2 = (float)(x.y >> 8) * (1.0f / 16777216.0f);            // [0, 1)
        const float rad = sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincos_cw(6.2831854820251465f * u2, sn, cs);
        const float ua = (float)((x.z >> 8) + 1u) * (1.0f / 16777216.0f);
        const float ub = (float)((x.w >> 8) + 1u) * (1.0f / 16777216.0f);
        float va, vb;
        const bool oka = gamma_round(da, ca, rad * cs, ua, va);
        const bool okb = gamma_round(db, cb, rad * sn, ub, vb);
        if (!got_a && oka) { ga = va; got_a = true; }
        if (!got_b && okb) { gb = vb; got_b = true; }
    }
    return beta_clamp(ga / (ga + gb));
}

template <int ORDER>
struct TdacBetaLane {
    using Bas = FourierReg<kCmc, ORDER>;
    static constexpr int F = Bas::F, G = LstdGroup<F>::G;
    static constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    using Phi = PhiBuf<F, PK>;
    static_assert(G >= 2, "a lane per policy column");

    LstdLane<F, LSTD_INCREMENTAL> L;
    WBuf<1, F, PK> col;                                   // the policy's column min(r, 1)

    __device__ __forceinline__ static int column(int r) { return r < 1 ? 0 : 1; }

    __device__ __forceinline__ void load(const TdacBetaState& ts, int64_t N, int64_t i, int r) {
        L.load(ts.ls, i, r);
        mat_load<1, F, PK>(col, ts.w + (int64_t)column(r) * F * N, N, i);
    }
    __device__ __forceinline__ void store(const TdacBetaState& ts, int64_t N, int64_t i, int r) const {
        L.store(ts.ls, i, r);
        if (r < 2) mat_store<1, F, PK>(col, ts.w + (int64_t)r * F * N, N, i);
    }
    // x_a = <w_a, phi>, x_b = <w_b, phi>: lane b's preference, handed round the group
    __device__ __forceinline__ void prefs(const Phi& phi, float& xa, float& xb) const {
        float hb[1];
        col.q(phi, hb);
        xa = __shfl(hb[0], 0, G);
        xb = __shfl(hb[0], 1, G);
    }

    // one transition of the lane's learner (TdacLstdLane::step's arguments; xa, xb the preferences at s with the pre-update columns, a the action).
    // Returns iLSTD's diagnostic delta.
    __device__ __forceinline__ double step(const TdacBetaState& ts, double (*lv)[F], int r, double phs, double phn, const Phi& phi_s, float xa, float xb,
                                           float a, double rew, bool term) {
        // ---- iLSTD::handle
        const double delta = L.template step<G>(ts.ls, lv, r, phs, phn, rew, term);
        // ---- TDCritic::target with the updated theta
        const float e = (float)(ts.alpha * tdcritic_target<F>(L.theta, ts.ls.gamma, lv, r, phs, phn, rew, term));
        // ---- the actor: this lane's column
        float alpha, beta;
        beta_params(xa, xb, alpha, beta);
        const float ac = beta_clamp(a);
        const float psi_ab = digamma_dev(alpha + beta);
        const float g_a = logf(ac) - digamma_dev(alpha) + psi_ab;
        const float g_b = logf(1.0f - ac) - digamma_dev(beta) + psi_ab;
        const float s_a = e * g_a * softplus_grad_dev(xa);
        const float s_b = e * g_b * softplus_grad_dev(xb);
        const float sb[1] = {r < 1 ? s_a : s_b};
        col.axpy(sb, phi_s);
        return delta;
    }
};

// the driver loop (tdac_beta.rs), modelled on k_train_tdac_lstd: transition, iLSTD, critic + actor, then the behaviour sample a' ~ Beta(alpha, beta)(s')
// with the UPDATED columns, taken after the restart (BLK_STEP; BLK_RESET after a cut episode is its alias).  The sample's preferences are the next step's
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_train_tdac_beta(Common c, TdacBetaState ts, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    using Dom = Domain<kCmc>;
    using Lane = TdacBetaLane<ORDER>;
    using Bas = typename Lane::Bas;
    using Phi = typename Lane::Phi;
    constexpr int D = Dom::D, F = Lane::F, G = Lane::G;
    __shared__ double lds[LstdGroup<F>::kPerBlock][LV_N][F];
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = tid / G;
    const int r = (int)(tid % G);
    const int64_t N = c.n_envs;
    unsigned long long n_ep = 0, n_trunc = 0, sum_len = 0;
    double sum_abs = 0.0, sum_r = 0.0;
    if (i < N) {
        double (*lv)[F] = lds[threadIdx.x / G];
        const uint32_t gid = (uint32_t)(c.env_offset + i);
        const uint32_t cap = c.max_episode_steps;
        float s[D];
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] = c.state[(int64_t)d * N + i];
        float a = ts.action[i];
        uint32_t ep = c.ep_step[i];
        Lane ln;
        ln.load(ts, N, i, r);
        double phs = lstd_feature<kCmc, ORDER>(s, r);
        Phi phi_s;
        float xa, xb;
        ac_project<Bas>(s, phi_s);
        ln.prefs(phi_s, xa, xb);
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
            double phn = lstd_feature<kCmc, ORDER>(ns, r);            // s' itself, the terminal state included: TDCritic reads V(s')
            const double delta = ln.step(ts, lv, r, phs, phn, phi_s, xa, xb, a, (double)rw, term);
            acc_abs += fabs(delta); acc_r += (double)rw;
            if (term) { n_ep += 1; sum_len += ep; ep = 0; }
            if (trunc) { n_ep += 1; n_trunc += 1; sum_len += ep; ep = 0; }
            if (term || trunc) {                                      // the restart state is where the sample is taken
                Dom::reset(ns);
                phn = lstd_feature<kCmc, ORDER>(ns, r);
            }
            // ---- policy.sample(rng, s') with the UPDATED columns
            ac_project<Bas>(ns, phi_s);
            ln.prefs(phi_s, xa, xb);
            float alpha, beta;
            beta_params(xa, xb, alpha, beta);
            a = beta_sample(c.seed, gid, t, BLK_STEP, alpha, beta);
#pragma unroll
            for (int d = 0; d < D; ++d) s[d] = ns[d];
            phs = phn;
            lstd_wave_sync();                             // (this step's reads of the slice before the next step's writes)
        }
        ln.store(ts, N, i, r);
        if (r == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) c.state[(int64_t)d * N + i] = s[d];
            ts.action[i] = a;
            c.ep_step[i] = ep;
            sum_abs = acc_abs; sum_r = acc_r;
        } else {
            n_ep = 0; n_trunc = 0; sum_len = 0;
        }
    }
    if (stats) block_stats_accumulate(stats, n_ep, n_trunc, sum_len, sum_abs, sum_r);
}

// iLSTD::handle then ActorCritic::handle (tdac_beta.rs's order) on caller-supplied transitions: transition i is learner i's
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_handle_tdac_beta(Common c, TdacBetaState ts, const float* __restrict__ from, const float* __restrict__ act,
                                                             const float* __restrict__ rew, const float* __restrict__ to, const uint8_t* __restrict__ termf,
                                                             int64_t Mn, float* __restrict__ td_out) {
    using Dom = Domain<kCmc>;
    using Lane = TdacBetaLane<ORDER>;
    using Bas = typename Lane::Bas;
    constexpr int D = Dom::D, F = Lane::F;
    __shared__ double lds[LstdGroup<F>::kPerBlock][LV_N][F];
    const auto g = GroupId<F, LV_N>::here();
    const int r = g.r;
    if (g.i >= Mn) return;
    double (*lv)[F] = g.slice(lds);
    GroupGiven<D> tr;
    tr.load(from, to, termf, Mn, g.i);
    const float a = act[g.i];
    Lane ln;
    ln.load(ts, c.n_envs, g.i, r);
    const double phs = lstd_feature<kCmc, ORDER>(tr.s, r);
    const double phn = lstd_feature<kCmc, ORDER>(tr.ns, r);
    typename Lane::Phi phi_s;
    float xa, xb;
    ac_project<Bas>(tr.s, phi_s);
    ln.prefs(phi_s, xa, xb);
    if (g.own()) lv[LV_PHS][r] = phs;
    const double delta = ln.step(ts, lv, r, phs, phn, phi_s, xa, xb, a, (double)rew[g.i], tr.term);
    ln.store(ts, c.n_envs, g.i, r);
    g.report(td_out, delta);
}

// ---- the policy side on explicit states, one thread per state: state i against learner i's columns (the single-column forms: the bits of the lanes')
// SAMPLE: out0 = the sample of (t, purpose) (and keep, when non-null: the ctx's pending actions); MODE: out0 = mode; PARAMS: out0 = alpha, out1 = beta;
// PDF: out0 = the density of act_in.  states == nullptr: the ctx's own (c.state, M = n_envs)
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_beta_policy(Common c, const float* __restrict__ w, int op, const float* __restrict__ states, int64_t Mn, uint64_t t,
                                                        uint32_t purpose, const float* __restrict__ act_in, float* __restrict__ out0, float* __restrict__ out1,
                                                        float* __restrict__ keep) {
    using Bas = FourierReg<kCmc, ORDER>;
    constexpr int D = Domain<kCmc>::D, F = Bas::F;
    constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    const int64_t N = c.n_envs;
    const float* sp = states ? states : c.state;
    float s[D];
#pragma unroll
    for (int d = 0; d < D; ++d) s[d] = sp[(int64_t)d * Mn + i];
    PhiBuf<F, PK> phi;
    ac_project<Bas>(s, phi);
    float x[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        WBuf<1, F, PK> col;
        mat_load<1, F, PK>(col, w + (int64_t)b * F * N, N, i);
        float hb[1];
        col.q(phi, hb);
        x[b] = hb[0];
    }
    float alpha, beta;
    beta_params(x[0], x[1], alpha, beta);
    if (op == BETA_OP_SAMPLE) {
        const float a = beta_sample(c.seed, (uint32_t)(c.env_offset + i), t, purpose, alpha, beta);
        if (out0) out0[i] = a;
        if (keep) keep[i] = a;
    } else if (op == BETA_OP_MODE) {
        out0[i] = beta_mode(alpha, beta);
    } else if (op == BETA_OP_PARAMS) {
        out0[i] = alpha; out1[i] = beta;
    } else {
        out0[i] = beta_pdf(alpha, beta, act_in[i]);
    }
}

// reset: every learner at the start state, its initial sample on BLK_INIT at batch-step t (k_reset's convention)
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_beta_reset(Common c, const float* __restrict__ w, uint64_t t, float* __restrict__ action) {
    using Bas = FourierReg<kCmc, ORDER>;
    constexpr int D = Domain<kCmc>::D, F = Bas::F;
    constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    if (i >= N) return;
    float s[D];
    Domain<kCmc>::reset(s);
    PhiBuf<F, PK> phi;
    ac_project<Bas>(s, phi);
    float x[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        WBuf<1, F, PK> col;
        mat_load<1, F, PK>(col, w + (int64_t)b * F * N, N, i);
        float hb[1];
        col.q(phi, hb);
        x[b] = hb[0];
    }
    float alpha, beta;
    beta_params(x[0], x[1], alpha, beta);
#pragma unroll
    for (int d = 0; d < D; ++d) c.state[(int64_t)d * N + i] = s[d];
    action[i] = beta_sample(c.seed, (uint32_t)(c.env_offset + i), t, BLK_INIT, alpha, beta);
    c.ep_step[i] = 0;
}

// Domain::rollout(|s| policy.mode(s)) from the start state (tdac_beta.rs:66): at most step_limit states; n_states and the total reward per learner
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_beta_rollout_mode(Common c, const float* __restrict__ w, int64_t step_limit, uint32_t* __restrict__ n_states,
                                                              float* __restrict__ total) {
    using Dom = Domain<kCmc>;
    using Bas = FourierReg<kCmc, ORDER>;
    constexpr int D = Dom::D, F = Bas::F;
    constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    if (i >= N) return;
    WBuf<1, F, PK> wa, wb;
    mat_load<1, F, PK>(wa, w, N, i);
    mat_load<1, F, PK>(wb, w + (int64_t)F * N, N, i);
    float s[D];
    Dom::reset(s);
    uint32_t n = 1;
    float tot = 0.0f;
    for (int64_t k = 1; k < step_limit; ++k) {
        PhiBuf<F, PK> phi;
        ac_project<Bas>(s, phi);
        float ha[1], hb[1], alpha, beta;
        wa.q(phi, ha);
        wb.q(phi, hb);
        beta_params(ha[0], hb[0], alpha, beta);
        float rw;
        const bool term = Dom::step(s, beta_mode(alpha, beta), rw);
        n += 1; tot += rw;
        if (term) break;
    }
    n_states[i] = n;
    if (total) total[i] = tot;
}

// (the two kernels below are no templates: a second unit that includes this file for its device functions -- train_nac_beta.hip -- defines
// RSRL_BETA_DEVICE_FUNCTIONS_ONLY and leaves their one definition to train_tdac_beta.hip)
#ifndef RSRL_BETA_DEVICE_FUNCTIONS_ONLY
// Domain::transition on the ctx's envs with f32 actions (k_domain_step's contract); actions == nullptr: the ctx's pending ones
__global__ __launch_bounds__(kBlock) void k_cmc_domain_step(Common c, const float* __restrict__ actions, const float* __restrict__ pending,
                                                            float* __restrict__ from_out, float* __restrict__ next_out, float* __restrict__ rew_out,
                                                            uint8_t* __restrict__ term_out) {
    using Dom = Domain<kCmc>;
    constexpr int D = Dom::D;
    const int64_t N = c.n_envs;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float s[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        s[d] = c.state[(int64_t)d * N + i];
        if (from_out) from_out[(int64_t)d * N + i] = s[d];
    }
    const float a = actions ? actions[i] : pending[i];
    float r;
    const bool term = Dom::step(s, a, r);
#pragma unroll
    for (int d = 0; d < D; ++d) {
        c.state[(int64_t)d * N + i] = s[d];
        if (next_out) next_out[(int64_t)d * N + i] = s[d];
    }
    if (rew_out) rew_out[i] = r;
    if (term_out) term_out[i] = term ? 1 : 0;
}
// a device array of actions into the action bounds (NaN -> -1), as k_clamp_actions for the index actions
__global__ void k_cmc_clamp_actions(float* __restrict__ a, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = fminf(fmaxf(a[i], -1.0f), 1.0f);
}
#endif

}  // namespace rsrl
