// kernels_tdac_cont.hpp -- ActorCritic::tdac with a TD(0) state-value critic over the continuous policies (Gaussian, Beta) on ContinuousMountainCar:
//   ActorCritic::tdac / TDCritic   rsrl/src/control/ac.rs:32-52, :87-98, :100-115     generic over the policy
//   the V learner                  TD{v_func = ScalarLFA(basis, SGD(lr)), gamma} (prediction/td/td.rs:38-58): the caller's `eval`, trained before the agent
//                                  sees the transition (the order of tdac.rs and tdac_beta.rs)
//   the policies                   Gaussian over a ScalarLFA and a Composition<ScalarLFA, Softplus> (kernels_gaussian.hpp's device functions;
//                                  Gaussian::handle(StateActionUpdate) is policies/gaussian/general.rs:196-212) and Beta over two
//                                  Composition<ScalarLFA, Softplus> (kernels_tdac_beta.hpp's device functions), both unchanged
// This is RSRL_TD_ACTOR_CRITIC's arithmetic (kernels_tdac.hpp) for the critic half and CACLA's layout (kernels_cacla.hpp) for everything else.
// Three one-column approximators per learner: the V learner's w f32[F][N] (the ctx's weights, TD's layout) and the policy's two columns col0, col1
// f32[2][F][N] (the ctx's auxiliary matrix: the mean's and the stddev's, or alpha's and beta's).  One thread per learner with w, both columns,
// phi(s) and phi(s') in registers (5F floats, 180 at order 5): k_train_cacla's layout and launch bounds.  Per transition (s, a, r, s', term), all
// f32, in this order:
//     1.  x0 = <col0, phi(s)>, x1 = <col1, phi(s)>       (the columns before any move)
//     2.  TD::handle, tdac_step's expressions:   v_s = <w, phi(s)>, v_n = <w, phi(s')>;  td = r - v_s (terminal) | r + gamma * v_n - v_s;
//                                                w += (lr * td) phi(s), one fma per element
//     3.  TDCritic::target with the UPDATED w (ac.rs:40-50):   nv = <w, phi(s')>;  c = r - nv (terminal: V of the terminal state itself, as
//         RSRL_TD_ACTOR_CRITIC) | r + gamma * nv - <w, phi(s)>;   e = alpha * c
//     4.  policy.handle(StateActionUpdate{s, a, error: e}), always -- there is no gate:
//         Gaussian   (mu, sd) = gauss_params(x0, x1);  (c_m, c_s) = gauss_coef(x1, mu, sd, a);  w_m += (e * c_m) phi(s);  w_s += (e * c_s) phi(s)
//         Beta       (alpha, beta) = beta_params(x0, x1);  ac = beta_clamp(a);  psi_ab = digamma(alpha + beta);
//                    g_a = ln ac - digamma(alpha) + psi_ab;  g_b = ln(1 - ac) - digamma(beta) + psi_ab;
//                    s_a = e * g_a * sigma(x0);  s_b = e * g_b * sigma(x1);  w_a += s_a phi(s);  w_b += s_b phi(s)      (TdacBetaLane::step's expressions)
// There is no safeguard: a coefficient that is not finite propagates, as in the reference.  There is no inner draw.  tdac_cont_step is the ONE step
// both kernels below run: train, handle and the trait-granular loop give the same bits, and w / td are the bits of a TD ctx's on the same transitions
// whatever the columns are.
// The loop's action mapping is each policy's: the domain sees the action itself under Gaussian (nac.rs's convention, as CACLA) and 2a - 1 under Beta
// (nac_domain_action, nac_beta.rs's mapping of the sample's [0, 1] onto the domain's [-1, 1]); the agent sees a.
// The step holds no data-dependent loop, no shuffle and no LDS access; the Beta sample's bounded gamma loop stands outside it, in the driver loop.
#pragma once

#include "kernels_gaussian.hpp"
#include "kernels_nac_beta.hpp"

namespace rsrl {

// the policy's parameters at the preferences x, then the behaviour sample of (seed, gid, t, purpose)
template <ContPolicy POLICY>
__device__ __forceinline__ float tdac_cont_sample(const Common& c, uint32_t gid, uint64_t t, uint32_t purpose, float x0, float x1) {
    if constexpr (POLICY == ContPolicy::Gaussian) {
        float mu, sd;
        gauss_params(x0, x1, mu, sd);
        return gauss_sample(c.seed, gid, t, purpose, mu, sd);
    } else {
        float alpha, beta;
        beta_params(x0, x1, alpha, beta);
        return beta_sample(c.seed, gid, t, purpose, alpha, beta);
    }
}
// what the domain is handed for the agent's action a
template <ContPolicy POLICY>
__device__ __forceinline__ float tdac_cont_domain_action(float a) {
    if constexpr (POLICY == ContPolicy::Gaussian) return a;
    else return nac_domain_action(a);
}

// one transition on projected phi(s), phi(s').  Returns TD's error
template <int F, bool PK, ContPolicy POLICY>
__device__ __forceinline__ float tdac_cont_step(const Common& c, WBuf<1, F, PK>& w, WBuf<2, F, PK>& pol, const PhiBuf<F, PK>& phi_s, const PhiBuf<F, PK>& phi_n,
                                                float a, float r, bool term) {
    const float gamma = c.alg.gamma, lr = c.alg.lr;
    float x[2];
    pol.q(phi_s, x);
    // ---- TD::handle (the expressions of k_train_td / k_handle_td, as tdac_step states them)
    float v_s[1], v_n[1];
    w.q(phi_s, v_s);
    w.q(phi_n, v_n);
    const float td = term ? (r - v_s[0]) : (r + gamma * v_n[0] - v_s[0]);
    const float sb[1] = {lr * td};
    w.axpy(sb, phi_s);
    // ---- TDCritic::target with the updated V
    w.q(phi_s, v_s);
    w.q(phi_n, v_n);
    const float target = term ? (r - v_n[0]) : (r + gamma * v_n[0] - v_s[0]);
    const float e = c.alg.alpha * target;
    // ---- policy.handle(StateActionUpdate{s, a, error: e})
    float sp[2];
    if constexpr (POLICY == ContPolicy::Gaussian) {
        float mu, sd, cm, cs;
        gauss_params(x[0], x[1], mu, sd);
        gauss_coef(x[1], mu, sd, a, cm, cs);
        sp[0] = e * cm;
        sp[1] = e * cs;
    } else {
        float alpha, beta;
        beta_params(x[0], x[1], alpha, beta);
        const float ac = beta_clamp(a);
        const float psi_ab = digamma_dev(alpha + beta);
        const float g_a = logf(ac) - digamma_dev(alpha) + psi_ab;
        const float g_b = logf(1.0f - ac) - digamma_dev(beta) + psi_ab;
        sp[0] = e * g_a * softplus_grad_dev(x[0]);
        sp[1] = e * g_b * softplus_grad_dev(x[1]);
    }
    pol.axpy(sp, phi_s);
    return td;
}

// the driver loop: transition on the policy's domain action, eval.handle, agent.handle, then the behaviour sample with the UPDATED columns, after
// the restart when the episode ended, terminal or cut (restart_then_sample's convention; BLK_STEP, BLK_RESET is its alias).  s' is projected as it
// is, the terminal state included (TDCritic reads V(s')); phi(s') becomes the next step's phi(s) (two buffers that swap roles) unless the episode
// ended: then the restart state is projected in its place.  The statistics' sum |delta| is TD's
template <int ORDER, ContPolicy POLICY>
__global__ __launch_bounds__(kBlock) void k_train_tdac_cont(Common c, TdacContState st, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    using Dom = Domain<kCmc>;
    using Bas = FourierReg<kCmc, ORDER>;
    constexpr int D = Dom::D, F = Bas::F;
    constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    using Phi = PhiBuf<F, PK>;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    Tally tally;
    if (i < N) {
        const uint32_t gid = (uint32_t)(c.env_offset + i);
        const uint32_t cap = c.max_episode_steps;
        float s[D];
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] = c.state[(int64_t)d * N + i];
        float a = st.action[i];
        uint32_t ep = c.ep_step[i];
        WBuf<1, F, PK> w;
        WBuf<2, F, PK> pol;
        mat_load<1, F, PK>(w, c.W, N, i);
        mat_load<2, F, PK>(pol, st.pol, N, i);
        Phi phi_a, phi_b;
        ac_project<Bas>(s, phi_a);

        ping_pong(phi_a, phi_b, t0, n_steps, [&](const Phi& phi_s, Phi& phi_n, uint64_t t) {
            float rw;
            const bool term = Dom::step(s, tdac_cont_domain_action<POLICY>(a), rw);      // s <- s' (the domain clips the action: map_onto)
            ep += 1;
            const bool trunc = !term && cap > 0 && ep >= cap;
            ac_project<Bas>(s, phi_n);
            const float td = tdac_cont_step<F, PK, POLICY>(c, w, pol, phi_s, phi_n, a, rw, term);
            if (term || trunc) {                                      // the restart state is where the sample is taken
                tally.episode_end(ep, trunc);
                Dom::reset(s);
                ac_project<Bas>(s, phi_n);
            }
            float x[2];
            pol.q(phi_n, x);
            a = tdac_cont_sample<POLICY>(c, gid, t, BLK_STEP, x[0], x[1]);
            tally.step(td, rw);
        });
#pragma unroll
        for (int d = 0; d < D; ++d) c.state[(int64_t)d * N + i] = s[d];
        st.action[i] = a;
        c.ep_step[i] = ep;
        mat_store<1, F, PK>(w, c.W, N, i);
        mat_store<2, F, PK>(pol, st.pol, N, i);
    }
    tally.hand_over(stats);
}

// eval.handle then ActorCritic::handle on caller-supplied transitions: transition i is learner i's
template <int ORDER, ContPolicy POLICY>
__global__ __launch_bounds__(kBlock) void k_handle_tdac_cont(Common c, TdacContState st, const float* __restrict__ from, const float* __restrict__ act,
                                                             const float* __restrict__ rew, const float* __restrict__ to, const uint8_t* __restrict__ termf,
                                                             int64_t Mn, float* __restrict__ td_out) {
    using Bas = FourierReg<kCmc, ORDER>;
    constexpr int D = Domain<kCmc>::D, F = Bas::F;
    constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    const int64_t N = c.n_envs;
    Given<D> tr;
    tr.load(from, rew, to, termf, Mn, i);
    PhiBuf<F, PK> phi_s, phi_n;
    ac_project<Bas>(tr.s, phi_s);
    ac_project<Bas>(tr.ns, phi_n);
    WBuf<1, F, PK> w;
    WBuf<2, F, PK> pol;
    mat_load<1, F, PK>(w, c.W, N, i);
    mat_load<2, F, PK>(pol, st.pol, N, i);
    const float td = tdac_cont_step<F, PK, POLICY>(c, w, pol, phi_s, phi_n, act[i], tr.r, tr.term);
    mat_store<1, F, PK>(w, c.W, N, i);
    mat_store<2, F, PK>(pol, st.pol, N, i);
    if (td_out) td_out[i] = td;
}

}  // namespace rsrl
