// kernels_nac_beta.hpp -- NAC (natural actor-critic) with the Beta policy and a SARSA critic over the stable compatible basis on
// ContinuousMountainCar, the agent and the loop of examples/nac_beta.rs:
//   NAC::handle(())          rsrl/src/control/nac.rs:47-59
//   the critic               SARSA{q_func: LFA::scalar(SCB{policy, basis}, SGD(lr)), policy, gamma}  (control/td/sarsa.rs:53-75)
//   SCB::project((s, a))     rsrl/src/fa/linear.rs:79-103: grad_log pi(a|s) (policies/beta.rs:119-129) chained with basis.project(s), 3F features
//   the policy               Beta over two Composition<ScalarLFA, Softplus>: kernels_tdac_beta.hpp's device functions, included and not copied
// Per learner, all f32: the critic's weights w[3F] (the ctx's weights: rows 0..F-1 belong to alpha's column, F..2F-1 to beta's, 2F..3F-1 to the
// plain basis; [3F][N] in memory, which is WBuf<3, F>'s [3][F][N]) and the policy's two columns (the ctx's auxiliary matrix, [2][F][N]).  With
// x_a = <w_a, phi(s)>, x_b likewise, (alpha, beta) = beta_params(x_a, x_b), g_a / g_b the score of the action clamped to [2^-24, 1 - 2^-24] and
// sigma Softplus's gradient (all as in kernels_tdac_beta.hpp):
//     psi(s, a) = [ c_a phi(s) ; c_b phi(s) ; phi(s) ],   c_a = g_a sigma(x_a), c_b = g_b sigma(x_b)
//     Q(s, a)   = <w, psi(s, a)>  evaluated as  fma(c_a, d_0, fma(c_b, d_1, d_2)),  d_k = <w[kF .. kF+F-1], phi(s)> (WBuf::q's four-chain dot):
//                 THREE LENGTH-F DOTS COMBINED, not the 3F products in index order -- phi(s) is multiplied into each block once
// Per transition (s, a, r, s', term), SARSA::handle:
//     na    ~ Beta(alpha', beta')(s') on the agent's own stream: beta_sample(seed, gid, t, BLK_INNER) (the reference draws from thread_rng())
//     delta = r - Q(s, a)  (terminal)  |  fma(gamma, Q(s', na), r) - Q(s, a)
//     w    += (lr delta) psi(s, a):  block k gets WBuf::axpy with the scalar (lr delta) c_k (1 for the last block)
// The bootstrap is computed whether or not the transition is terminal and selected afterwards (the draws are counter-based).  The policy's columns
// do not move here.  NAC::handle(()), every `period` steps of an episode (nac_beta.rs:69 hard-codes 100):
//     g = w[0 .. 2F-1];  norm = max(sqrt(sum g_j^2), 1e-3), the squares rounded and added in index order;  scale = alpha32 / norm
//     w_a += scale g[0 .. F-1],  w_b += scale g[F .. 2F-1]   (fma per element: WBuf::axpy_buf's form);  the critic's weights are not reset
// One thread per learner with w, both columns and phi(s) in registers (kernels_ac.hpp's layout): the step is a scalar f32 chain -- three digammas,
// two logarithms, two Softplus and gradients per score, a sampler per draw -- that a lane group would only repeat.
// NacBetaLane::step and NacBetaLane::actor are the ONE step and the ONE actor update every kernel below runs.
#pragma once

#include "kernels_tdac_beta.hpp"

namespace rsrl {

template <int ORDER>
struct NacBetaLane {
    using Dom = Domain<kCmc>;
    using Bas = FourierReg<kCmc, ORDER>;
    static constexpr int D = Dom::D, F = Bas::F;
    static constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    using Phi = PhiBuf<F, PK>;

    WBuf<3, F, PK> w;          // the critic's weights, SCB's three blocks
    WBuf<2, F, PK> pol;        // the policy's columns (alpha's, beta's)

    __device__ __forceinline__ void load(const float* __restrict__ W, const float* __restrict__ P, int64_t N, int64_t i) {
        mat_load<3, F, PK>(w, W, N, i);
        mat_load<2, F, PK>(pol, P, N, i);
    }
    // x_a, x_b at phi
    __device__ __forceinline__ void prefs(const Phi& phi, float& xa, float& xb) const {
        float x[2];
        pol.q(phi, x);
        xa = x[0]; xb = x[1];
    }
    // c_a, c_b of psi(s, a): the score of the clamped action times Softplus's gradient (TdacBetaLane::step's expressions)
    __device__ __forceinline__ static void coef(float xa, float xb, float alpha, float beta, float a, float& ca, float& cb) {
        const float ac = beta_clamp(a);
        const float psi_ab = digamma_dev(alpha + beta);
        const float g_a = logf(ac) - digamma_dev(alpha) + psi_ab;
        const float g_b = logf(1.0f - ac) - digamma_dev(beta) + psi_ab;
        ca = g_a * softplus_grad_dev(xa);
        cb = g_b * softplus_grad_dev(xb);
    }
    // Q = <w, psi>: three dots combined
    __device__ __forceinline__ float q(const Phi& phi, float ca, float cb) const {
        float d[3];
        w.q(phi, d);
        return fmaf(ca, d[0], fmaf(cb, d[1], d[2]));
    }
    // Function<(S, A)>::evaluate at (s, a)
    __device__ __forceinline__ float q_at(const float (&s)[D], float a) const {
        Phi phi;
        ac_project<Bas>(s, phi);
        float xa, xb, alpha, beta, ca, cb;
        prefs(phi, xa, xb);
        beta_params(xa, xb, alpha, beta);
        coef(xa, xb, alpha, beta, a, ca, cb);
        return q(phi, ca, cb);
    }

    // SARSA::handle on one transition of learner gid at batch-step t.  Returns delta; xna, xnb: the preferences at s' (the behaviour sample's, while
    // the episode goes on: the columns do not move here).  Only one feature vector is live at a time
    __device__ __forceinline__ float step(const Common& c, const float (&s)[D], float a, float r, bool term, const float (&ns)[D], uint32_t gid, uint64_t t,
                                          float& xna, float& xnb) {
        Phi phi;
        float boot;
        {
            ac_project<Bas>(ns, phi);
            prefs(phi, xna, xnb);
            float alpha, beta, ca, cb;
            beta_params(xna, xnb, alpha, beta);
            const float na = beta_sample(c.seed, gid, t, BLK_INNER, alpha, beta);      // policy.sample(rng, s'), the agent's own draw
            coef(xna, xnb, alpha, beta, na, ca, cb);
            boot = q(phi, ca, cb);
        }
        ac_project<Bas>(s, phi);
        float xa, xb, alpha, beta, ca, cb;
        prefs(phi, xa, xb);
        beta_params(xa, xb, alpha, beta);
        coef(xa, xb, alpha, beta, a, ca, cb);
        const float qsa = q(phi, ca, cb);
        const float delta = term ? (r - qsa) : (fmaf(c.alg.gamma, boot, r) - qsa);
        const float sc = c.alg.lr * delta;
        const float sb[3] = {sc * ca, sc * cb, sc};
        w.axpy(sb, phi);
        return delta;
    }

    // NAC::handle(()): the policy's columns step along the critic's first 2F weights.  Returns Response.norm
    __device__ __forceinline__ float actor(float alpha32) {
        float ss = 0.0f;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int f = 0; f < F; ++f) {
                const float g = w.get(b, f);
                const float sq = g * g;               // (rounded before it is added: the tree is built with -ffp-contract=off)
                ss = ss + sq;
            }
        const float norm = fmaxf(sqrtf(ss), 1e-3f);
        const float scale = alpha32 / norm;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int f = 0; f < F; ++f) pol.put(b, f, fmaf(scale, w.get(b, f), pol.get(b, f)));
        return norm;
    }
};

// the loop's action mapping (nac_beta.rs:63, :82): the domain sees 2a - 1, the agent a (2a is exact)
__device__ __forceinline__ float nac_domain_action(float a) { return 2.0f * a - 1.0f; }

// the driver loop (nac_beta.rs:55-76), i the 0-based index of the step in its episode: transition on 2a - 1, critic.handle, the behaviour sample
// a' ~ Beta(s') with the columns as they stand (after the restart when the episode ended: BLK_STEP, BLK_RESET is its alias), THEN agent.handle(())
// if i % period == 0 -- the next step's psi(s, a) is evaluated with the columns after it (NacBetaLane::step computes the preferences at s itself)
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_train_nac_beta(Common c, NacBetaState st, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    using Lane = NacBetaLane<ORDER>;
    using Dom = typename Lane::Dom;
    using Bas = typename Lane::Bas;
    constexpr int D = Lane::D;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    Tally tally;
    if (i < N) {
        const uint32_t gid = (uint32_t)(c.env_offset + i);
        const uint32_t cap = c.max_episode_steps, period = st.period;
        float s[D];
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] = c.state[(int64_t)d * N + i];
        float a = st.action[i];
        uint32_t ep = c.ep_step[i];
        Lane ln;
        ln.load(c.W, st.pol, N, i);
        for (int k = 0; k < n_steps; ++k) {
            const uint64_t t = t0 + (uint64_t)k;
            const bool update = ep % period == 0;
            float ns[D];
#pragma unroll
            for (int d = 0; d < D; ++d) ns[d] = s[d];
            float rw;
            const bool term = Dom::step(ns, nac_domain_action(a), rw);
            ep += 1;
            const bool trunc = !term && cap > 0 && ep >= cap;
            float xa, xb;
            const float delta = ln.step(c, s, a, rw, term, ns, gid, t, xa, xb);
            if (term || trunc) {                                      // the restart state is where the sample is taken
                tally.episode_end(ep, trunc);
                Dom::reset(ns);
                typename Lane::Phi phi;
                ac_project<Bas>(ns, phi);
                ln.prefs(phi, xa, xb);
            }
            float alpha, beta;
            beta_params(xa, xb, alpha, beta);
            a = beta_sample(c.seed, gid, t, BLK_STEP, alpha, beta);
            tally.step(delta, rw);
            if (update) (void)ln.actor(c.alg.alpha);
#pragma unroll
            for (int d = 0; d < D; ++d) s[d] = ns[d];
        }
#pragma unroll
        for (int d = 0; d < D; ++d) c.state[(int64_t)d * N + i] = s[d];
        st.action[i] = a;
        c.ep_step[i] = ep;
        mat_store<3, Lane::F, Lane::PK>(ln.w, c.W, N, i);
        mat_store<2, Lane::F, Lane::PK>(ln.pol, st.pol, N, i);
    }
    tally.hand_over(stats);
}

// critic.handle (SARSA::handle) on caller-supplied transitions: transition i is learner i's; the inner draw of batch-step t.  The columns stay
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_handle_nac_beta(Common c, NacBetaState st, const float* __restrict__ from, const float* __restrict__ act,
                                                            const float* __restrict__ rew, const float* __restrict__ to, const uint8_t* __restrict__ termf,
                                                            int64_t Mn, uint64_t t, float* __restrict__ td_out) {
    using Lane = NacBetaLane<ORDER>;
    constexpr int D = Lane::D;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    const int64_t N = c.n_envs;
    float s[D], ns[D];
#pragma unroll
    for (int d = 0; d < D; ++d) { s[d] = from[(int64_t)d * Mn + i]; ns[d] = to[(int64_t)d * Mn + i]; }
    Lane ln;
    ln.load(c.W, st.pol, N, i);
    float xa, xb;
    const float delta = ln.step(c, s, act[i], rew[i], termf[i] != 0, ns, (uint32_t)(c.env_offset + i), t, xa, xb);
    mat_store<3, Lane::F, Lane::PK>(ln.w, c.W, N, i);
    if (td_out) td_out[i] = delta;
}

// NAC::handle(()) for the learners of mask (nullptr: every learner); norm_out (may be null): Response.norm, 0 for a learner left out
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_nac_update(Common c, NacBetaState st, const uint8_t* __restrict__ mask, float* __restrict__ norm_out) {
    using Lane = NacBetaLane<ORDER>;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    if (i >= N) return;
    if (mask && mask[i] == 0) {
        if (norm_out) norm_out[i] = 0.0f;
        return;
    }
    Lane ln;
    ln.load(c.W, st.pol, N, i);
    const float norm = ln.actor(c.alg.alpha);
    mat_store<2, Lane::F, Lane::PK>(ln.pol, st.pol, N, i);
    if (norm_out) norm_out[i] = norm;
}

// Function<(S, A)>::evaluate of the critic: state i and action i against learner i's w and columns
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_nac_q(Common c, NacBetaState st, const float* __restrict__ states, const float* __restrict__ act, int64_t Mn,
                                                  float* __restrict__ q_out) {
    using Lane = NacBetaLane<ORDER>;
    constexpr int D = Lane::D;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    float s[D];
#pragma unroll
    for (int d = 0; d < D; ++d) s[d] = states[(int64_t)d * Mn + i];
    Lane ln;
    ln.load(c.W, st.pol, c.n_envs, i);
    q_out[i] = ln.q_at(s, act[i]);
}

// Domain::rollout(|s| 2 * policy.mode(s) - 1) from the start state (nac_beta.rs:81-82): k_beta_rollout_mode with the loop's mapping
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_nac_rollout_mode(Common c, const float* __restrict__ w, int64_t step_limit, uint32_t* __restrict__ n_states,
                                                             float* __restrict__ total) {
    using Dom = Domain<kCmc>;
    using Bas = FourierReg<kCmc, ORDER>;
    constexpr int D = Dom::D, F = Bas::F;
    constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    if (i >= N) return;
    WBuf<2, F, PK> pol;
    mat_load<2, F, PK>(pol, w, N, i);
    float s[D];
    Dom::reset(s);
    uint32_t n = 1;
    float tot = 0.0f;
    for (int64_t k = 1; k < step_limit; ++k) {
        PhiBuf<F, PK> phi;
        ac_project<Bas>(s, phi);
        float x[2], alpha, beta;
        pol.q(phi, x);
        beta_params(x[0], x[1], alpha, beta);
        float rw;
        const bool term = Dom::step(s, nac_domain_action(beta_mode(alpha, beta)), rw);
        n += 1; tot += rw;
        if (term) break;
    }
    n_states[i] = n;
    if (total) total[i] = tot;
}

// (the kernel below is no template: a second unit that includes this file for its device functions -- train_tdac_cont.hip -- defines
// RSRL_NAC_BETA_DEVICE_FUNCTIONS_ONLY and leaves its one definition to train_nac_beta.hip, as RSRL_BETA_DEVICE_FUNCTIONS_ONLY does in kernels_tdac_beta.hpp)
#ifndef RSRL_NAC_BETA_DEVICE_FUNCTIONS_ONLY
// Domain::transition on the ctx's envs (k_cmc_domain_step's contract): explicit actions are the domain's own, taken literally; actions == nullptr
// steps on the ctx's pending actions through the loop's mapping 2a - 1
__global__ __launch_bounds__(kBlock) void k_nac_domain_step(Common c, const float* __restrict__ actions, const float* __restrict__ pending,
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
    const float a = actions ? actions[i] : nac_domain_action(pending[i]);
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
#endif

}  // namespace rsrl
