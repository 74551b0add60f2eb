// kernels_gtd.hpp -- gradient-TD prediction on the register family, the prediction siblings of GreedyGQ (kernels_gq.hpp):
//   GTD2::handle   rsrl/src/prediction/td/gtd2.rs:27-86     fa_theta, fa_w: two ScalarLFAs on one basis; gamma
//   TDC::handle    rsrl/src/prediction/td/tdc.rs:41-101     q_func, td_est likewise
// Two one-column approximators per learner: theta f32[F][N] (the ctx's weights, TD's layout: the value function) and w f32[F][N] (the ctx's
// auxiliary matrix: fa_w / td_est).  Per transition (s, r, s', term) with phi = phi(s), phi' = phi(s'), everything read before anything moves:
//     w_s = <w, phi>;  th_s = <theta, phi>;  th_n = <theta, phi'>;   td = r - th_s (terminal) | r + gamma*th_n - th_s      (k_train_td's expression)
//     w += lr_td * (td - w_s) * phi
//     GTD2:  u = lr * w_s;  theta += u * phi;          theta += -(gamma * u) * phi'       (ScaledGradientUpdate{alpha: w_s, jacobian: phi - gamma phi'})
//     TDC :                 theta += (lr * td) * phi;  theta += -(lr * w_s) * phi'        (GradientUpdate(td phi - w_s phi'): no gamma, tdc.rs:91)
// Two axpys per move of theta and no merged gradient vector: no F registers beyond theta, w and the two feature buffers (4F floats).
// Neither rule has a terminal case for the gradient: phi' of a terminal transition is the terminal state's own features and is subtracted as on
// any other step, so the driver loop projects s' as it is (k_train_tdac's convention) -- NOT k_train_td's, which projects the restart state there.
// DEPARTURE: the reference sends these updates past the optimiser (fa/linear.rs:170-196), step size 1 -- all but TDC's td_est, which goes through
// its SGD (linear.rs:237-248).  On a Fourier basis both rules diverge with unit steps (include/rsrl_hip.h, RSRL_GTD2), so config.lr scales every
// move of theta and config.lr_td every move of w; 1.0f is exact, so lr = lr_td = 1 is the literal GTD2 and lr = 1 the literal TDC over SGD(lr_td).
// TDC with w = 0 and lr_td = 0 is k_train_td's arithmetic: its first axpy is TD's, its second adds a zero.
// gtd_step is the ONE step both kernels below run: train, handle and the trait-granular loop give the same bits.
#pragma once

#include "launch.hpp"
#include "kernels_ac.hpp"

namespace rsrl {

// one transition on projected phi(s), phi(s').  Returns the TD error
template <int F, bool PK, bool TDC>
__device__ __forceinline__ float gtd_step(const Common& c, float lr_td, WBuf<1, F, PK>& th, WBuf<1, F, PK>& w, const PhiBuf<F, PK>& phi_s,
                                          const PhiBuf<F, PK>& phi_n, float r, bool term) {
    const float gamma = c.alg.gamma, lr = c.alg.lr;
    float w_s[1], th_s[1], th_n[1];
    w.q(phi_s, w_s);
    th.q(phi_s, th_s);
    th.q(phi_n, th_n);
    const float td = term ? (r - th_s[0]) : (r + gamma * th_n[0] - th_s[0]);
    const float sw[1] = {lr_td * (td - w_s[0])};
    w.axpy(sw, phi_s);
    if constexpr (TDC) {
        const float s1[1] = {lr * td}, s2[1] = {-(lr * w_s[0])};
        th.axpy(s1, phi_s);
        th.axpy(s2, phi_n);
    } else {
        const float u = lr * w_s[0];
        const float s1[1] = {u}, s2[1] = {-(gamma * u)};
        th.axpy(s1, phi_s);
        th.axpy(s2, phi_n);
    }
    return td;
}

// the driver loop (TD's, with a Random behaviour policy): transition, handle on s' ITSELF (the terminal state included), then the restart and the
// Random sample (BLK_STEP; BLK_RESET after a cap, its alias) -- the environment side is k_train_td's draw for draw.  theta and w stay in
// registers for the whole launch; phi(s') becomes the next step's phi(s) (two buffers that swap roles, as k_train_td's) unless the episode
// ended: then the restart state is projected in its place
template <int DOMAIN, int ORDER, bool TDC>
__global__ __launch_bounds__(kBlock) void k_train_gtd(Common c, GtdState gs, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    using Dom = Domain<DOMAIN>;
    using Bas = FourierReg<DOMAIN, ORDER>;
    constexpr int D = Dom::D, A = Dom::A, F = Bas::F;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    Tally tally;
    if (i < N) {
        Learner<D> env;
        env.load(c, i);
        PolicyParams pol = c.pol; pol.kind = POL_RANDOM;
        const float q0[A] = {};                        // Random ignores the action values
        constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
        using Phi = PhiBuf<F, PK>;
        WBuf<1, F, PK> th, w;
        mat_load<1, F, PK>(th, c.W, N, i);
        mat_load<1, F, PK>(w, gs.w, N, i);
        Phi phi_a, phi_b;
        ac_project<Bas>(env.s, phi_a);

        ping_pong(phi_a, phi_b, t0, n_steps, [&](const Phi& phi_s, Phi& phi_n, uint64_t t) {
            Transition<D> tr = env.template step<Dom>();
            ac_project<Bas>(tr.ns, phi_n);                  // s' itself: the gradient subtracts phi' on a terminal transition too
            const float td = gtd_step<F, PK, TDC>(c, gs.lr_td, th, w, phi_s, phi_n, tr.r, tr.term);
            restart_then_sample<Dom>(c, env, tally, tr, td, t,
                [&](const float (&ns)[D], bool ended) { if (ended) ac_project<Bas>(ns, phi_n); },
                [&](const U4& x) { return policy_sample<A>(pol, q0, x); });
        });
        env.store(c, i);
        mat_store<1, F, PK>(th, c.W, N, i);
        mat_store<1, F, PK>(w, gs.w, N, i);
    }
    tally.hand_over(stats);
}

// Handler<&Transition>::handle of GTD2 / TDC on caller-supplied transitions: transition i is learner i's; tdc: runtime flag
template <int DOMAIN, int ORDER>
__global__ __launch_bounds__(kBlock) void k_handle_gtd(Common c, GtdState gs, int tdc, const float* __restrict__ from, const float* __restrict__ rew,
                                                       const float* __restrict__ to, const uint8_t* __restrict__ termf, int64_t Mn,
                                                       float* __restrict__ td_out) {
    using Dom = Domain<DOMAIN>;
    using Bas = FourierReg<DOMAIN, ORDER>;
    constexpr int D = Dom::D, F = Bas::F;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    const int64_t N = c.n_envs;
    constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    Given<D> tr;
    tr.load(from, rew, to, termf, Mn, i);
    PhiBuf<F, PK> phi_s, phi_n;
    ac_project<Bas>(tr.s, phi_s);
    ac_project<Bas>(tr.ns, phi_n);
    WBuf<1, F, PK> th, w;
    mat_load<1, F, PK>(th, c.W, N, i);
    mat_load<1, F, PK>(w, gs.w, N, i);
    const float td = tdc ? gtd_step<F, PK, true>(c, gs.lr_td, th, w, phi_s, phi_n, tr.r, tr.term)
                         : gtd_step<F, PK, false>(c, gs.lr_td, th, w, phi_s, phi_n, tr.r, tr.term);
    mat_store<1, F, PK>(th, c.W, N, i);
    mat_store<1, F, PK>(w, gs.w, N, i);
    if (td_out) td_out[i] = td;
}

}  // namespace rsrl
