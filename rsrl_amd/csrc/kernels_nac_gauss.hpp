// kernels_nac_gauss.hpp -- NAC (natural actor-critic) with the Gaussian policy and a SARSA critic over the stable compatible basis on
// ContinuousMountainCar, the agent and the loop of examples/nac.rs:
//   NAC::handle(())          rsrl/src/control/nac.rs:47-59
//   the critic               SARSA{q_func: LFA::scalar(SCB{policy, basis}, SGD(lr)), policy, gamma}  (control/td/sarsa.rs:53-75)
//   SCB::project((s, a))     rsrl/src/fa/linear.rs:79-103: grad_log pi(a|s) (policies/gaussian/general.rs:142-157) chained with basis.project(s), 3F features
//   the policy               Gaussian over a ScalarLFA and a Composition<ScalarLFA, Softplus>: kernels_gaussian.hpp's device functions
// The layout, the critic's rule and the actor's update are kernels_nac_beta.hpp's: per learner the critic's w[3F] (rows 0..F-1 belong to the mean's
// column, F..2F-1 to the stddev's, 2F..3F-1 to the plain basis) and the policy's two columns, one thread per learner with w, both columns and phi(s) in
// registers.  With (mu, sd) = gauss_params(x_m, x_s):
//     psi(s, a) = [ c_m phi(s) ; c_s phi(s) ; phi(s) ],   c_m = g_mu, c_s = g_Sigma sigma(x_s)     (gauss_coef)
//     Q(s, a)   = fma(c_m, d_0, fma(c_s, d_1, d_2)),  d_k = <w[kF .. kF+F-1], phi(s)>: three length-F dots combined
// Per transition (s, a, r, s', term), SARSA::handle:
//     na    ~ N(mu', sd'^2)(s') on the agent's own stream: gauss_sample(seed, gid, t, BLK_INNER)
//     delta = r - Q(s, a)  (terminal)  |  fma(gamma, Q(s', na), r) - Q(s, a)
//     w    += (lr delta) psi(s, a)
// NAC::handle(()) is NacBetaLane::actor's arithmetic in its operation order; the kernel that runs it on its own is k_nac_update itself
// (kernels_nac_beta.hpp: it reads w's first 2F rows and the two columns, whatever the policy).  NacBetaLane's step is NOT shared: the Beta agent's
// machine code stays as it is.  The loop differs from nac_beta.rs's in one thing: the domain sees the action itself, no 2a - 1.
// The step holds no data-dependent loop, no shuffle and no LDS access.
#pragma once

#include "kernels_gaussian.hpp"

namespace rsrl {

template <int ORDER>
struct NacGaussLane {
    using Dom = Domain<kCmc>;
    using Bas = FourierReg<kCmc, ORDER>;
    static constexpr int D = Dom::D, F = Bas::F;
    static constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    using Phi = PhiBuf<F, PK>;

    WBuf<3, F, PK> w;          // the critic's weights, SCB's three blocks
    WBuf<2, F, PK> pol;        // the policy's columns (the mean's, the stddev's)

    __device__ __forceinline__ void load(const float* __restrict__ W, const float* __restrict__ P, int64_t N, int64_t i) {
        mat_load<3, F, PK>(w, W, N, i);
        mat_load<2, F, PK>(pol, P, N, i);
    }
    // x_m, x_s at phi
    __device__ __forceinline__ void prefs(const Phi& phi, float& xm, float& xs) const {
        float x[2];
        pol.q(phi, x);
        xm = x[0]; xs = x[1];
    }
    // Q = <w, psi>: three dots combined
    __device__ __forceinline__ float q(const Phi& phi, float cm, float cs) const {
        float d[3];
        w.q(phi, d);
        return fmaf(cm, d[0], fmaf(cs, d[1], d[2]));
    }
    // Q(s, a) at phi = phi(s); xm, xs: the preferences there; cm, cs: psi's coefficients
    __device__ __forceinline__ float q_phi(const Phi& phi, float a, float& xm, float& xs, float& cm, float& cs) const {
        float mu, sd;
        prefs(phi, xm, xs);
        gauss_params(xm, xs, mu, sd);
        gauss_coef(xs, mu, sd, a, cm, cs);
        return q(phi, cm, cs);
    }
    // Function<(S, A)>::evaluate at (s, a)
    __device__ __forceinline__ float q_at(const float (&s)[D], float a) const {
        Phi phi;
        ac_project<Bas>(s, phi);
        float xm, xs, cm, cs;
        return q_phi(phi, a, xm, xs, cm, cs);
    }

    // SARSA::handle on one transition of learner gid at batch-step t.  Returns delta; xnm, xns: the preferences at s' (the behaviour sample's, while
    // the episode goes on: the columns do not move here).  Only one feature vector is live at a time
    __device__ __forceinline__ float step(const Common& c, const float (&s)[D], float a, float r, bool term, const float (&ns)[D], uint32_t gid, uint64_t t,
                                          float& xnm, float& xns) {
        Phi phi;
        float boot;
        {
            ac_project<Bas>(ns, phi);
            prefs(phi, xnm, xns);
            float mu, sd, cm, cs;
            gauss_params(xnm, xns, mu, sd);
            const float na = gauss_sample(c.seed, gid, t, BLK_INNER, mu, sd);      // policy.sample(rng, s'), the agent's own draw
            gauss_coef(xns, mu, sd, na, cm, cs);
            boot = q(phi, cm, cs);
        }
        ac_project<Bas>(s, phi);
        float xm, xs, cm, cs;
        const float qsa = q_phi(phi, a, xm, xs, cm, cs);
        const float delta = term ? (r - qsa) : (fmaf(c.alg.gamma, boot, r) - qsa);
        const float sc = c.alg.lr * delta;
        const float sb[3] = {sc * cm, sc * cs, sc};
        w.axpy(sb, phi);
        return delta;
    }

    // NAC::handle(()): NacBetaLane::actor's operations in its order (k_nac_update runs that one: the two must leave the same bits)
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

// the driver loop (nac.rs:55-76), i the 0-based index of the step in its episode: transition on the action itself, critic.handle, the behaviour sample
// a' ~ N(mu, sd^2)(s') with the columns as they stand (after the restart when the episode ended: BLK_STEP, BLK_RESET is its alias), THEN
// agent.handle(()) if i % period == 0 -- the next step's psi(s, a) is evaluated with the columns after it
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_train_nac_gauss(Common c, NacBetaState st, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    using Lane = NacGaussLane<ORDER>;
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
            const bool term = Dom::step(ns, a, rw);                   // (the domain clips the action: map_onto)
            ep += 1;
            const bool trunc = !term && cap > 0 && ep >= cap;
            float xm, xs;
            const float delta = ln.step(c, s, a, rw, term, ns, gid, t, xm, xs);
            if (term || trunc) {                                      // the restart state is where the sample is taken
                tally.episode_end(ep, trunc);
                Dom::reset(ns);
                typename Lane::Phi phi;
                ac_project<Bas>(ns, phi);
                ln.prefs(phi, xm, xs);
            }
            float mu, sd;
            gauss_params(xm, xs, mu, sd);
            a = gauss_sample(c.seed, gid, t, BLK_STEP, mu, sd);
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
__global__ __launch_bounds__(kBlock) void k_handle_nac_gauss(Common c, NacBetaState st, const float* __restrict__ from, const float* __restrict__ act,
                                                             const float* __restrict__ rew, const float* __restrict__ to, const uint8_t* __restrict__ termf,
                                                             int64_t Mn, uint64_t t, float* __restrict__ td_out) {
    using Lane = NacGaussLane<ORDER>;
    constexpr int D = Lane::D;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    const int64_t N = c.n_envs;
    float s[D], ns[D];
#pragma unroll
    for (int d = 0; d < D; ++d) { s[d] = from[(int64_t)d * Mn + i]; ns[d] = to[(int64_t)d * Mn + i]; }
    Lane ln;
    ln.load(c.W, st.pol, N, i);
    float xm, xs;
    const float delta = ln.step(c, s, act[i], rew[i], termf[i] != 0, ns, (uint32_t)(c.env_offset + i), t, xm, xs);
    mat_store<3, Lane::F, Lane::PK>(ln.w, c.W, N, i);
    if (td_out) td_out[i] = delta;
}

// Function<(S, A)>::evaluate of the critic: state i and action i against learner i's w and columns
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_nac_gauss_q(Common c, NacBetaState st, const float* __restrict__ states, const float* __restrict__ act, int64_t Mn,
                                                        float* __restrict__ q_out) {
    using Lane = NacGaussLane<ORDER>;
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

}  // namespace rsrl
