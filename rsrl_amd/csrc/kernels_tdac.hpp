// kernels_tdac.hpp -- ActorCritic with a TD(0) state-value critic (TDCritic) on the register family:
//   ActorCritic::tdac / TDCritic   rsrl/src/control/ac.rs:32-52, :87-98, :108-114     driver rsrl/examples/tdac.rs (eval.handle, agent.handle, sample)
//   the V learner                  TD{v_func = ScalarLFA(basis, SGD(lr)), gamma} (prediction/td/td.rs:31-59), in place of tdac.rs's iLSTD (with iLSTD: kernels_tdac_lstd.hpp)
//   the actor                      Gibbs::standard(LFA::vector(basis, SGD(1.0), A)) = Softmax(tau), as in kernels_ac.hpp
// Two approximators per learner: the V learner's weights w f32[F][N] (the ctx's weights, ONE column, TD's layout) and the actor's preferences
// theta f32[A][F][N] (the ctx's auxiliary matrix).  Per transition (s, a, r, s', term), in tdac.rs's order:
//     p       = softmax_stable(theta^T phi(s) / tau)                    (theta BEFORE this step's update)
//     TD(0)   delta = r - <w,phi(s)> (terminal) | r + gamma*<w,phi(s')> - <w,phi(s)>;   w += lr*delta*phi(s)      (k_train_td's arithmetic)
//     critic  c = r - <w',phi(s')> (terminal: V of the terminal state itself) | r + gamma*<w',phi(s')> - <w',phi(s)>, w' the UPDATED w
//     actor   theta[:,b] += alpha*c*(1[b==a] - p_b)*phi(s) for every b            (grad_log without 1/tau, as kernels_ac.hpp)
// There is no inner draw.  s' of a terminal transition is the terminal state (what rsrl_hip_domain_step reports): the driver loop projects it
// for the critic and projects the restart state afterwards, on terminal and truncated steps only.
// tdac_step is the ONE step both kernels below run: train, handle and the trait-granular loop give the same bits, and w / delta are the bits
// of a TD ctx's on the same transitions whatever theta is.
#pragma once

#include "kernels_ac.hpp"

namespace rsrl {

// one transition of learner i on projected phi(s), phi(s'); p_s = pi_theta(s) with the pre-update theta.  Returns the TD(0) error.
// actor(sa) applies theta[:,b] += sa[b] * phi(s): the driver loop's theta is in registers throughout, handle's is loaded only for the update (w,
// theta and both feature vectors at once do not fit MountainCar order 5's registers without scratch)
template <int A, int F, bool PK, class Actor>
__device__ __forceinline__ float tdac_step(const Common& c, WBuf<1, F, PK>& w, const PhiBuf<F, PK>& phi_s, const PhiBuf<F, PK>& phi_n, const float (&p_s)[A],
                                           int a, float r, bool term, Actor&& actor) {
    const float gamma = c.alg.gamma, lr = c.alg.lr;
    // ---- TD::handle (the expressions of k_train_td / k_handle_td)
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
    const float sc = c.alg.alpha * target;
    float sa[A];
#pragma unroll
    for (int b = 0; b < A; ++b) sa[b] = sc * (((a == b) ? 1.0f : 0.0f) - p_s[b]);      // grad_log: (1[b==a] - p_b) phi(s)
    actor(sa);
    return td;
}

// handle's theta, one column of F weights in registers at a time (all of theta next to w and both feature vectors does not fit MountainCar order
// 5's registers without scratch).  Column b of WBuf<A, F, PK>'s q / axpy is computed on its own: these give the same bits as ac_probs / th.axpy
template <int A, int F, bool PK>
__device__ __forceinline__ void tdac_probs_mem(const Common& c, const float* __restrict__ theta, int64_t N, int64_t i, const PhiBuf<F, PK>& phi, float (&p)[A]) {
    float h[A];
#pragma unroll
    for (int b = 0; b < A; ++b) {
        WBuf<1, F, PK> col;
        mat_load<1, F, PK>(col, theta + (int64_t)b * F * N, N, i);
        float hb[1];
        col.q(phi, hb);
        h[b] = hb[0];
    }
    softmax_probs<A>(h, c.pol.tau, p);
}
template <int A, int F, bool PK>
__device__ __forceinline__ void tdac_actor_mem(float* __restrict__ theta, int64_t N, int64_t i, const float (&sa)[A], const PhiBuf<F, PK>& phi) {
#pragma unroll
    for (int b = 0; b < A; ++b) {
        __builtin_amdgcn_sched_barrier(0);                // (one column in flight: the scheduler would otherwise hoist every column's loads)
        WBuf<1, F, PK> col;
        mat_load<1, F, PK>(col, theta + (int64_t)b * F * N, N, i);
        const float sb[1] = {sa[b]};
        col.axpy(sb, phi);
        mat_store<1, F, PK>(col, theta + (int64_t)b * F * N, N, i);
    }
}

// the driver loop (tdac.rs): transition, TD(0), critic + actor, then the behaviour sample a' ~ pi_theta'(s') with the UPDATED theta (BLK_STEP; an
// episode cut by max_episode_steps restarts and samples there on BLK_RESET, a terminal one restarts before the sample).  w and theta stay in
// registers for the whole launch; phi(s') becomes the next step's phi(s) (two buffers that swap roles every step, as k_train_td's), and the
// sample's probabilities are the next step's p (theta does not move in between)
template <int DOMAIN, int ORDER>
__global__ __launch_bounds__(kBlock) void k_train_tdac(Common c, float* __restrict__ theta, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    using Dom = Domain<DOMAIN>;
    using Bas = FourierReg<DOMAIN, ORDER>;
    constexpr int D = Dom::D, A = Dom::A, F = Bas::F;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    Tally tally;
    if (i < N) {
        Learner<D> env;
        env.load(c, i);
        constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
        using Phi = PhiBuf<F, PK>;
        WBuf<1, F, PK> w;
        WBuf<A, F, PK> th;
        mat_load<1, F, PK>(w, c.W, N, i);
        mat_load<A, F, PK>(th, theta, N, i);
        Phi phi_a, phi_b;
        float p_s[A];
        ac_project<Bas>(env.s, phi_a);
        ac_probs<A, F, PK>(c, th, phi_a, p_s);

        ping_pong(phi_a, phi_b, t0, n_steps, [&](const Phi& phi_s, Phi& phi_n, uint64_t t) {
            Transition<D> tr = env.template step<Dom>();
            ac_project<Bas>(tr.ns, phi_n);                  // s' itself, the terminal state included: TDCritic reads V(s')
            const float delta = tdac_step<A, F, PK>(c, w, phi_s, phi_n, p_s, env.a, tr.r, tr.term, [&](const float (&sa)[A]) { th.axpy(sa, phi_s); });
            // ---- policy.sample(rng, s') with the UPDATED theta; the restart state is projected on terminal and truncated steps only
            restart_then_sample<Dom>(c, env, tally, tr, delta, t,
                [&](const float (&ns)[D], bool ended) { if (ended) ac_project<Bas>(ns, phi_n); ac_probs<A, F, PK>(c, th, phi_n, p_s); },
                [&](const U4& x) { return sample_probs<A>(p_s, x.z); });
        });
        env.store(c, i);
        mat_store<1, F, PK>(w, c.W, N, i);
        mat_store<A, F, PK>(th, theta, N, i);
    }
    tally.hand_over(stats);
}

// TD::handle then ActorCritic::handle (tdac.rs's order) on caller-supplied transitions: transition i is learner i's
template <int DOMAIN, int ORDER>
__global__ __launch_bounds__(kBlock) void k_handle_tdac(Common c, float* __restrict__ theta, const float* __restrict__ from, const int32_t* __restrict__ act,
                                                        const float* __restrict__ rew, const float* __restrict__ to, const uint8_t* __restrict__ termf,
                                                        int64_t Mn, float* __restrict__ td_out) {
    using Dom = Domain<DOMAIN>;
    using Bas = FourierReg<DOMAIN, ORDER>;
    constexpr int D = Dom::D, A = Dom::A, F = Bas::F;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    const int64_t N = c.n_envs;
    constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    Given<D> tr;
    tr.template load<A>(from, act, rew, to, termf, Mn, i);
    PhiBuf<F, PK> phi_s, phi_n;
    ac_project<Bas>(tr.s, phi_s);
    ac_project<Bas>(tr.ns, phi_n);
    float p_s[A];
    tdac_probs_mem<A, F, PK>(c, theta, N, i, phi_s, p_s);
    WBuf<1, F, PK> w;
    mat_load<1, F, PK>(w, c.W, N, i);
    const float delta = tdac_step<A, F, PK>(c, w, phi_s, phi_n, p_s, tr.a, tr.r, tr.term, [&](const float (&sa)[A]) { tdac_actor_mem<A, F, PK>(theta, N, i, sa, phi_s); });
    mat_store<1, F, PK>(w, c.W, N, i);
    if (td_out) td_out[i] = delta;
}

}  // namespace rsrl
