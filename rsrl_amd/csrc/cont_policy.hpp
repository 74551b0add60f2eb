// cont_policy.hpp -- the two continuous policies on ContinuousMountainCar, their device functions, the trait Cont<P> every continuous agent's
// kernel reads them through, and the policy side on explicit states (sample, mode, params, pdf), reset's initial sample and the mode rollout.
// Per learner two weight columns f32[2][F][N] (the ctx's auxiliary matrix, what rsrl_hip_get/set_policy_weights show as (F, 2)); with the two
// preferences x_0 = <col_0, phi(s)>, x_1 likewise, all f32:
//
// BETA (rsrl/src/policies/beta.rs) over two Composition<ScalarLFA, Softplus> (fa/composition.rs:98-115, fa/transforms.rs:196-218); columns alpha's, beta's
//     alpha = softplus(x_0) + 1, beta = softplus(x_1) + 1         softplus(x) = x for x >= 10, else ln(1 + exp(x)); MIN_TOL = 1.0 (beta.rs:19, :58-67)
//     so both are >= 1 always (the sampler relies on it)
//     score       g_a = ln a - psi(alpha) + psi(alpha + beta),  g_b = ln(1 - a) - psi(beta) + psi(alpha + beta)       (psi = digamma)
//                 RECALLED from rstat::univariate::beta (the crate is not in the reference tree): the library's definition, DESIGN 6.  The action's
//                 logarithms are taken of the action clamped to the sample's interval [2^-24, 1 - 2^-24] -- a departure from the reference, which
//                 would produce infinities for a caller's 0 or 1, in the spirit of clamp_action
//     sample      X = Ga / (Ga + Gb), Ga ~ Gamma(alpha, 1), Gb ~ Gamma(beta, 1) by Marsaglia-Tsang (d = k - 1/3, c = 1 / sqrt(9 d)).  Round j of the
//                 sample for purpose P (BLK_STEP -- BLK_RESET is its alias --, BLK_INNER, BLK_INIT, BLK_API) takes the WHOLE Philox block at block
//                 word P + 256 * (j + 1) (every other stream uses block words < 256): words x, y give two normals by Box-Muller (the cosine one is
//                 Ga's, the sine one Gb's), word z is Ga's acceptance uniform, word w Gb's.  At most kBetaRounds rounds per gamma; a gamma not
//                 accepted by then is d.  The loop holds no shuffle, no wave barrier and no LDS access
//     mode        (beta.rs:141-150; rstat's modes() is not in the tree -- the library's definition): (alpha - 1) / (alpha + beta - 2) if both
//                 exceed 1, else the mean alpha / (alpha + beta)
//
// GAUSSIAN, Gaussian<ScalarLFA, Composition<ScalarLFA, Softplus>> (policies/gaussian/{mod,general}.rs); columns the mean's, the stddev's
//     mu = x_0,   sd = softplus(x_1) + 0.01 (MIN_TOL, mod.rs:37, :67),   Sigma = sd * sd (into_cov, mod.rs:15-17, :82: the builder takes the VARIANCE)
//     sample      a = fma(sd, z, mu),  z = sqrt(-2 ln u1) cos(2 pi u2): Box-Muller's cosine normal on the WHOLE Philox block at block word P + 256,
//                 words x and y converted as beta_sample converts them (u1 in (0, 1], u2 in [0, 1)).  ONE block, no loop, no acceptance test;
//                 u1 >= 2^-24 bounds |z| by sqrt(48 ln 2) < 5.77.  Not clamped: the domain clips (map_onto)
//     mode        mu (general.rs:177)
//     density     exp(-(a - mu)^2 / (2 Sigma)) / sqrt(2 pi Sigma)
//     score       g_mu = (a - mu) / Sigma,   g_Sigma = ((a - mu)^2 - Sigma) / (2 Sigma^2): the derivatives of the log density in the builder's two
//                 arguments, the mean and the variance.  DEFINED here (rstat's normal::Grad is not in the reference tree): DESIGN 6
//     grad_log    [ g_mu phi ; g_Sigma sigma(x_1) phi ] (general.rs:142-157), sigma Softplus's gradient -- literal: the reference does not multiply
//                 the second block by d Sigma / d sd = 2 sd, and neither does this
//     A caller's action is any finite f32, taken as it is.
// Either sample is a function of (seed, global learner id, t, purpose) only.
#pragma once

#include "launch.hpp"      // ContPolicy, BETA_OP_*
#include "kernels_tdac.hpp"

namespace rsrl {

constexpr int kCmc = 4;                                   // RSRL_CONTINUOUS_MOUNTAIN_CAR
constexpr int kBetaRounds = 8;
constexpr float kBetaLo = 5.9604644775390625e-08f;        // 2^-24
constexpr float kBetaHi = 0.999999940395355224609375f;    // 1 - 2^-24
constexpr float kGaussMinTol = 0.01f;                     // MIN_TOL
constexpr float kTwoPi = 6.2831854820251465f;

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
// the score of the clamped action
__device__ __forceinline__ void beta_score(float alpha, float beta, float a, float& g_a, float& g_b) {
    const float ac = beta_clamp(a);
    const float psi_ab = digamma_dev(alpha + beta);
    g_a = logf(ac) - digamma_dev(alpha) + psi_ab;
    g_b = logf(1.0f - ac) - digamma_dev(beta) + psi_ab;
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

__device__ __forceinline__ void gauss_params(float xm, float xs, float& mu, float& sd) {
    mu = xm;
    sd = softplus_rel_dev(xs) + kGaussMinTol;             // (the form that keeps Softplus's relative accuracy: sd's spacing at the floor is 9e-10)
}
// Box-Muller's cosine normal of (seed, gid, t, purpose)
__device__ __forceinline__ float gauss_normal(uint64_t seed, uint32_t gid, uint64_t t, uint32_t purpose) {
    const U4 x = draw_block(seed, gid, t, purpose + 256u);
    const float u1 = (float)((x.x >> 8) + 1u) * (1.0f / 16777216.0f);      // (0, 1]
    const float u2 = (float)(x.y >> 8) * (1.0f / 16777216.0f);            // [0, 1)
    const float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincos_cw(kTwoPi * u2, sn, cs);
    return rad * cs;
}
__device__ __forceinline__ float gauss_sample(uint64_t seed, uint32_t gid, uint64_t t, uint32_t purpose, float mu, float sd) {
    return fmaf(sd, gauss_normal(seed, gid, t, purpose), mu);
}
// the density and the score divide by sd, never by Sigma: sd * sd is infinite in f32 from sd = 1.85e19 on, and (d^2 - inf) / (2 inf) a NaN where the
// result is an ordinary number.  With t = d / sd: density = exp(-t^2 / 2) / (sd sqrt(2 pi)), g_mu = t / sd, and
// g_Sigma sigma(x_s) = (g_mu (g_mu sigma) - sigma / sd^2) / 2 -- sigma inside the square, so that a tiny sigma meets g_mu before g_mu^2 overflows.
// The same conditioning as the expressions above (tests/continuous_edges.py gauss_b)
__device__ __forceinline__ float gauss_pdf(float mu, float sd, float a) {
    const float t = (a - mu) / sd;
    return expf(-0.5f * t * t) * ((1.0f / sd) * 0.3989422804014327f);
}
// grad_log's two coefficients of phi: (g_mu, g_Sigma sigma(x_s))
__device__ __forceinline__ void gauss_coef(float xs, float mu, float sd, float a, float& cm, float& cs) {
    const float inv = 1.0f / sd, sig = softplus_grad_dev(xs);
    cm = ((a - mu) / sd) * inv;
    cs = 0.5f * fmaf(cm, cm * sig, -((inv * inv) * sig));
}

// ---- what a kernel asks of its policy, each in the operation order its call sites had before the trait: (p0, p1) are the policy's two
// parameters at the preferences (x0, x1) -- (mu, sd), or (alpha, beta)
//   coef            psi(s, a)'s two coefficients of phi, the SCB critic's (NAC): the score times what the compositions contribute
//   actor_steps     the TD ActorCritic's two column steps for the error e.  Beta: (e * g) * sigma, where NAC's critic forms sc * (g * sigma) from
//                   coef -- different roundings, both kept
//   domain_action   what this family's driver loops hand the domain for the agent's action a: the action itself (nac.rs; the domain clips it), or
//                   2a - 1 (nac_beta.rs:63, :82; 2a is exact).  The iLSTD Beta ActorCritic's loop (tdac_beta.rs, kernels_tdac_beta.hpp) hands
//                   the domain a itself: the mapping is the loop's, and the kernels below take it as MAP
template <ContPolicy P>
struct Cont;
template <>
struct Cont<ContPolicy::Gaussian> {
    __device__ __forceinline__ static void params(float x0, float x1, float& mu, float& sd) { gauss_params(x0, x1, mu, sd); }
    __device__ __forceinline__ static float sample(uint64_t seed, uint32_t gid, uint64_t t, uint32_t purpose, float mu, float sd) {
        return gauss_sample(seed, gid, t, purpose, mu, sd);
    }
    __device__ __forceinline__ static float mode(float mu, float) { return mu; }
    __device__ __forceinline__ static float pdf(float mu, float sd, float a) { return gauss_pdf(mu, sd, a); }
    __device__ __forceinline__ static void coef(float, float x1, float mu, float sd, float a, float& c0, float& c1) { gauss_coef(x1, mu, sd, a, c0, c1); }
    __device__ __forceinline__ static void actor_steps(float e, float x0, float x1, float mu, float sd, float a, float& s0, float& s1) {
        float cm, cs;
        coef(x0, x1, mu, sd, a, cm, cs);
        s0 = e * cm;
        s1 = e * cs;
    }
    __device__ __forceinline__ static float domain_action(float a) { return a; }
};
template <>
struct Cont<ContPolicy::Beta> {
    __device__ __forceinline__ static void params(float x0, float x1, float& alpha, float& beta) { beta_params(x0, x1, alpha, beta); }
    __device__ __forceinline__ static float sample(uint64_t seed, uint32_t gid, uint64_t t, uint32_t purpose, float alpha, float beta) {
        return beta_sample(seed, gid, t, purpose, alpha, beta);
    }
    __device__ __forceinline__ static float mode(float alpha, float beta) { return beta_mode(alpha, beta); }
    __device__ __forceinline__ static float pdf(float alpha, float beta, float a) { return beta_pdf(alpha, beta, a); }
    __device__ __forceinline__ static void coef(float x0, float x1, float alpha, float beta, float a, float& c0, float& c1) {
        float g_a, g_b;
        beta_score(alpha, beta, a, g_a, g_b);
        c0 = g_a * softplus_grad_dev(x0);
        c1 = g_b * softplus_grad_dev(x1);
    }
    __device__ __forceinline__ static void actor_steps(float e, float x0, float x1, float alpha, float beta, float a, float& s0, float& s1) {
        float g_a, g_b;
        beta_score(alpha, beta, a, g_a, g_b);
        s0 = e * g_a * softplus_grad_dev(x0);
        s1 = e * g_b * softplus_grad_dev(x1);
    }
    __device__ __forceinline__ static float domain_action(float a) { return 2.0f * a - 1.0f; }
};

// the two preferences of state s against learner i's columns (the single-column forms: the bits of the lanes' and of WBuf<2>::q)
template <int ORDER>
__device__ __forceinline__ void cont_prefs_at(const float* __restrict__ w, int64_t N, int64_t i, const float (&s)[Domain<kCmc>::D], float& x0, float& x1) {
    using Bas = FourierReg<kCmc, ORDER>;
    constexpr int F = Bas::F;
    constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
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
    x0 = x[0]; x1 = x[1];
}

// ---- the policy side on explicit states, one thread per state: state i against learner i's columns.  SAMPLE: out0 = the sample of (t, purpose)
// (and keep, when non-null: the ctx's pending actions); MODE: out0 = mode; PARAMS: out0, out1 = the two parameters; PDF: out0 = the density of
// act_in.  states == nullptr: the ctx's own (c.state, M = n_envs)
template <int ORDER, ContPolicy P>
__global__ __launch_bounds__(kBlock) void k_cont_policy(Common c, const float* __restrict__ w, int op, const float* __restrict__ states, int64_t Mn, uint64_t t,
                                                        uint32_t purpose, const float* __restrict__ act_in, float* __restrict__ out0, float* __restrict__ out1,
                                                        float* __restrict__ keep) {
    using Pol = Cont<P>;
    constexpr int D = Domain<kCmc>::D;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    const float* sp = states ? states : c.state;
    float s[D];
#pragma unroll
    for (int d = 0; d < D; ++d) s[d] = sp[(int64_t)d * Mn + i];
    float x0, x1, p0, p1;
    cont_prefs_at<ORDER>(w, c.n_envs, i, s, x0, x1);
    Pol::params(x0, x1, p0, p1);
    if (op == BETA_OP_SAMPLE) {
        const float a = Pol::sample(c.seed, (uint32_t)(c.env_offset + i), t, purpose, p0, p1);
        if (out0) out0[i] = a;
        if (keep) keep[i] = a;
    } else if (op == BETA_OP_MODE) {
        out0[i] = Pol::mode(p0, p1);
    } else if (op == BETA_OP_PARAMS) {
        out0[i] = p0; out1[i] = p1;
    } else {
        out0[i] = Pol::pdf(p0, p1, act_in[i]);
    }
}

// reset: every learner at the start state, its initial sample on BLK_INIT at batch-step t (k_reset's convention)
template <int ORDER, ContPolicy P>
__global__ __launch_bounds__(kBlock) void k_cont_reset(Common c, const float* __restrict__ w, uint64_t t, float* __restrict__ action) {
    constexpr int D = Domain<kCmc>::D;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    if (i >= N) return;
    float s[D];
    Domain<kCmc>::reset(s);
    float x0, x1, p0, p1;
    cont_prefs_at<ORDER>(w, N, i, s, x0, x1);
    Cont<P>::params(x0, x1, p0, p1);
#pragma unroll
    for (int d = 0; d < D; ++d) c.state[(int64_t)d * N + i] = s[d];
    action[i] = Cont<P>::sample(c.seed, (uint32_t)(c.env_offset + i), t, BLK_INIT, p0, p1);
    c.ep_step[i] = 0;
}

// Domain::rollout(|s| policy.mode(s)) from the start state (tdac_beta.rs:66, nac.rs:81), or with MAP (|s| 2 * policy.mode(s) - 1)
// (nac_beta.rs:81-82): at most step_limit states; n_states and the total reward per learner.  (The Gaussian's mode is the mean: the stddev's
// column is named here and not read by the machine code)
template <int ORDER, ContPolicy P, bool MAP>
__global__ __launch_bounds__(kBlock) void k_cont_rollout_mode(Common c, const float* __restrict__ w, int64_t step_limit, uint32_t* __restrict__ n_states,
                                                              float* __restrict__ total) {
    using Dom = Domain<kCmc>;
    using Bas = FourierReg<kCmc, ORDER>;
    constexpr int D = Dom::D, F = Bas::F;
    constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    if (i >= N) return;
    WBuf<1, F, PK> w0, w1;
    mat_load<1, F, PK>(w0, w, N, i);
    mat_load<1, F, PK>(w1, w + (int64_t)F * N, N, i);
    float s[D];
    Dom::reset(s);
    uint32_t n = 1;
    float tot = 0.0f;
    for (int64_t k = 1; k < step_limit; ++k) {
        PhiBuf<F, PK> phi;
        ac_project<Bas>(s, phi);
        float h0[1], h1[1], p0, p1;
        w0.q(phi, h0);
        w1.q(phi, h1);
        Cont<P>::params(h0[0], h1[0], p0, p1);
        const float m = Cont<P>::mode(p0, p1);
        float rw;
        const bool term = Dom::step(s, MAP ? Cont<ContPolicy::Beta>::domain_action(m) : m, rw);
        n += 1; tot += rw;
        if (term) break;
    }
    n_states[i] = n;
    if (total) total[i] = tot;
}

}  // namespace rsrl
