// kernels_gaussian.hpp -- the Gaussian policy, Gaussian<ScalarLFA, Composition<ScalarLFA, Softplus>> (rsrl/src/policies/gaussian/{mod,general}.rs), on
// ContinuousMountainCar: its device functions beside Beta's (kernels_tdac_beta.hpp, whose Softplus they share) and the policy side on explicit states,
// for any agent that holds the policy's two columns -- today NAC (kernels_nac_gauss.hpp).
// Per learner two weight columns w_m, w_s f32[2][F][N] (the ctx's auxiliary matrix, what rsrl_hip_get/set_policy_weights show as (F, 2): column 0 =
// the mean's, column 1 = the stddev's).  With x_m = <w_m, phi(s)>, x_s likewise, all f32:
//     mu = x_m,   sd = softplus(x_s) + 0.01 (MIN_TOL, mod.rs:37, :67),   Sigma = sd * sd (into_cov, mod.rs:15-17, :82: the builder takes the VARIANCE)
//     sample      a = fma(sd, z, mu),  z = sqrt(-2 ln u1) cos(2 pi u2): Box-Muller's cosine normal on the WHOLE Philox block at block word P + 256
//                 (P = BLK_STEP -- BLK_RESET is its alias --, BLK_INNER, BLK_INIT, BLK_API), words x and y converted as beta_sample converts them
//                 (u1 in (0, 1], u2 in [0, 1)).  ONE block, no loop, no acceptance test; u1 >= 2^-24 bounds |z| by sqrt(48 ln 2) < 5.77.  Not
//                 clamped: the domain clips (map_onto).  A function of (seed, global learner id, t, purpose) only
//     mode        mu (general.rs:177)
//     density     exp(-(a - mu)^2 / (2 Sigma)) / sqrt(2 pi Sigma)
//     score       g_mu = (a - mu) / Sigma,   g_Sigma = ((a - mu)^2 - Sigma) / (2 Sigma^2): the derivatives of the log density in the builder's two
//                 arguments, the mean and the variance.  DEFINED here (rstat's normal::Grad is not in the reference tree): DESIGN 6
//     grad_log    [ g_mu phi ; g_Sigma sigma(x_s) phi ] (general.rs:142-157), sigma Softplus's gradient -- literal: the reference does not multiply
//                 the second block by d Sigma / d sd = 2 sd, and neither does this
// A caller's action is any finite f32, taken as it is.
#pragma once

#include "kernels_tdac_beta.hpp"

namespace rsrl {

constexpr float kGaussMinTol = 0.01f;                     // MIN_TOL
constexpr float kTwoPi = 6.2831854820251465f;

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

// the two preferences of state s against learner i's columns (the single-column forms, as k_beta_policy's)
template <int ORDER>
__device__ __forceinline__ void gauss_prefs_at(const float* __restrict__ w, int64_t N, int64_t i, const float (&s)[Domain<kCmc>::D], float& xm, float& xs) {
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
    xm = x[0]; xs = x[1];
}

// ---- the policy side on explicit states, one thread per state: k_beta_policy's contract and operations (BETA_OP_*: PARAMS writes mu and sd)
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_gauss_policy(Common c, const float* __restrict__ w, int op, const float* __restrict__ states, int64_t Mn, uint64_t t,
                                                         uint32_t purpose, const float* __restrict__ act_in, float* __restrict__ out0, float* __restrict__ out1,
                                                         float* __restrict__ keep) {
    constexpr int D = Domain<kCmc>::D;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    const float* sp = states ? states : c.state;
    float s[D];
#pragma unroll
    for (int d = 0; d < D; ++d) s[d] = sp[(int64_t)d * Mn + i];
    float xm, xs, mu, sd;
    gauss_prefs_at<ORDER>(w, c.n_envs, i, s, xm, xs);
    gauss_params(xm, xs, mu, sd);
    if (op == BETA_OP_SAMPLE) {
        const float a = gauss_sample(c.seed, (uint32_t)(c.env_offset + i), t, purpose, mu, sd);
        if (out0) out0[i] = a;
        if (keep) keep[i] = a;
    } else if (op == BETA_OP_MODE) {
        out0[i] = mu;
    } else if (op == BETA_OP_PARAMS) {
        out0[i] = mu; out1[i] = sd;
    } else {
        out0[i] = gauss_pdf(mu, sd, act_in[i]);
    }
}

// reset: every learner at the start state, its initial sample on BLK_INIT at batch-step t (k_beta_reset's contract)
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_gauss_reset(Common c, const float* __restrict__ w, uint64_t t, float* __restrict__ action) {
    constexpr int D = Domain<kCmc>::D;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    if (i >= N) return;
    float s[D];
    Domain<kCmc>::reset(s);
    float xm, xs, mu, sd;
    gauss_prefs_at<ORDER>(w, N, i, s, xm, xs);
    gauss_params(xm, xs, mu, sd);
#pragma unroll
    for (int d = 0; d < D; ++d) c.state[(int64_t)d * N + i] = s[d];
    action[i] = gauss_sample(c.seed, (uint32_t)(c.env_offset + i), t, BLK_INIT, mu, sd);
    c.ep_step[i] = 0;
}

// Domain::rollout(|s| policy.mode(s)) from the start state (nac.rs:81): at most step_limit states; the mode is the mean, so the stddev's column is
// not read.  n_states and the total reward per learner
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_gauss_rollout_mode(Common c, const float* __restrict__ w, int64_t step_limit, uint32_t* __restrict__ n_states,
                                                               float* __restrict__ total) {
    using Dom = Domain<kCmc>;
    using Bas = FourierReg<kCmc, ORDER>;
    constexpr int D = Dom::D, F = Bas::F;
    constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    if (i >= N) return;
    WBuf<1, F, PK> wm;
    mat_load<1, F, PK>(wm, w, N, i);
    float s[D];
    Dom::reset(s);
    uint32_t n = 1;
    float tot = 0.0f;
    for (int64_t k = 1; k < step_limit; ++k) {
        PhiBuf<F, PK> phi;
        ac_project<Bas>(s, phi);
        float hm[1];
        wm.q(phi, hm);
        float rw;
        const bool term = Dom::step(s, hm[0], rw);
        n += 1; tot += rw;
        if (term) break;
    }
    n_states[i] = n;
    if (total) total[i] = tot;
}

}  // namespace rsrl
