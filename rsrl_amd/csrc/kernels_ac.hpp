// kernels_ac.hpp -- ActorCritic with a Gibbs actor and a SARSA critic on the register family:
//   ActorCritic::handle   rsrl/src/control/ac.rs:108-114      driver rsrl/examples/a2c.rs:22-67
//   critic target         the a2c example's closure (a2c.rs:38-49): Q'(s,a) - sum_b Q'(s,b) p_b   | QCritic (ac.rs:23-31, :77-84): Q'(s,a)
//   the critic's learner  SARSA{q_func, policy = the actor, gamma} (sarsa.rs:43-73), q_func = LFA::vector(basis, SGD(lr), A)
//   the actor             Gibbs::standard(LFA::vector(basis, SGD(1.0), A)) = Softmax(tau): softmax.rs:113-130 (grad_log), :154-163, :216-222
// Two approximators per learner, both f32[A][F][N]: the critic's weights W (the ctx's weights) and the actor's preferences theta (the ctx's
// auxiliary matrix, GreedyGQ's layout).  Per transition (s, a, r, s', term), in the reference's order:
//     p       = softmax_stable(theta^T phi(s) / tau)                    (theta BEFORE this step's update)
//     critic  qsa = <W[:,a], phi(s)>;  na ~ pi_theta(s') on the agent's own draw (BLK_INNER, sarsa.rs:61; not drawn for a terminal transition)
//             delta = r - qsa (terminal) | r + gamma*<W[:,na], phi(s')> - qsa;   W[:,a] += lr*delta*phi(s)
//     actor   c = the critic target from the UPDATED W;  theta[:,b] += alpha*c*(1[b==a] - p_b)*phi(s) for every b
// grad_log does not divide by tau (softmax.rs:113-130 differentiates the preferences, not the scaled ones): kept literally.  The actor's
// SGD(1.0) never acts -- ScaledGradientUpdate adds alpha*c*jacobian to the weights directly (softmax.rs:216-222).
// ac_step is the ONE step both kernels below run (the driver loop with W and theta in registers, handle with them loaded from memory): train,
// handle and the trait-granular loop give the same bits.
#pragma once

#include "models.hpp"
#include "driver_loop.hpp"

namespace rsrl {

enum : int { AC_CRITIC_ADVANTAGE = 0,     // RSRL_ACTOR_CRITIC (a2c.rs's closure)
             AC_CRITIC_Q = 1 };           // RSRL_Q_ACTOR_CRITIC (ActorCritic::qac)

// q[a] by a select chain on OPAQUE values: select_a's chain on the arrays of this step was still folded into a select of addresses (the arrays
// then live in scratch); values that come out of an empty asm are not loads, so nothing can be turned into an indexed load
template <int A>
__device__ __forceinline__ float ac_pick(const float (&q)[A], int a) {
    float v = q[0];
    asm("" : "+v"(v));
#pragma unroll
    for (int i = 1; i < A; ++i) {
        float x = q[i];
        asm("" : "+v"(x));
        v = (a == i) ? x : v;
    }
    return v;
}

// phi(s) of a state the caller still holds: the copy goes through an empty asm so that two projections of one state are not merged into one
// (the merged phi would stay live across the whole update: 36 more registers than MountainCar order 5 has to spare)
template <class Bas, int D, int F, bool PK>
__device__ __forceinline__ void ac_project(const float (&s)[D], PhiBuf<F, PK>& phi) {
    float so[D];
#pragma unroll
    for (int d = 0; d < D; ++d) { so[d] = s[d]; asm("" : "+v"(so[d])); }
    float ph[F];
    Bas::project(so, ph);
    phi.set(ph);
}

// the actor's probabilities pi_theta(s) = softmax(theta^T phi(s) / tau)
template <int A, int F, bool PK>
__device__ __forceinline__ void ac_probs(const Common& c, const WBuf<A, F, PK>& th, const PhiBuf<F, PK>& phi, float (&p)[A]) {
    float h[A];
    th.q(phi, h);
    softmax_probs<A>(h, c.pol.tau, p);
}

// one transition of learner i: the critic, then the actor.  p_s = pi_theta(s) with the pre-update theta; returns the critic's delta.
// Only one feature vector is live at a time: phi(s') for the critic's bootstrap first, then phi(s) for both updates (W and theta hold 2 x 108
// registers at MountainCar order 5)
template <class Bas, int A, int F, bool PK, int CRITIC, int D>
__device__ __forceinline__ float ac_step(const Common& c, WBuf<A, F, PK>& w, WBuf<A, F, PK>& th, const float (&s)[D], const float (&p_s)[A],
                                         int a, float r, bool term, const float (&ns)[D], const U4& xin) {
    PhiBuf<F, PK> phi;
    // ---- critic: SARSA::handle.  The bootstrap is computed whether or not the transition is terminal and selected afterwards (the draws are
    // counter-based: nothing is consumed), so that the step is one basic block
    float boot;
    {
        float q_n[A], h_n[A], p_n[A];
        ac_project<Bas>(ns, phi);
        w.q(phi, q_n);
        th.q(phi, h_n);
        softmax_probs<A>(h_n, c.pol.tau, p_n);
        const int na = sample_probs<A>(p_n, xin.z);                  // policy.sample(rng, s'), the agent's own draw
        boot = ac_pick<A>(q_n, na);
    }
    ac_project<Bas>(s, phi);
    float q_s[A];
    w.q(phi, q_s);
    const float qsa = ac_pick<A>(q_s, a);
    const float delta = term ? (r - qsa) : (fmaf(c.alg.gamma, boot, r) - qsa);
    const float sc1 = c.alg.lr * delta;
    float sb[A];
#pragma unroll
    for (int b = 0; b < A; ++b) sb[b] = (a == b) ? sc1 : 0.0f;
    w.axpy(sb, phi);
    // ---- actor: the critic's target from the updated W (only column a moved: the other columns' values are the bits of q_s)
    float q2[A];
    w.q(phi, q2);
    const float qa2 = ac_pick<A>(q2, a);
    float target = qa2;
    if constexpr (CRITIC == AC_CRITIC_ADVANTAGE) {
        float v = 0.0f;
#pragma unroll
        for (int b = 0; b < A; ++b) v = fmaf(q2[b], p_s[b], v);      // fold(0.0, |acc, (x, p)| acc + x * p)
        target = qa2 - v;
    }
    const float sc2 = c.alg.alpha * target;
#pragma unroll
    for (int b = 0; b < A; ++b) sb[b] = sc2 * (((a == b) ? 1.0f : 0.0f) - p_s[b]);      // grad_log: (1[b==a] - p_b) phi(s)
    th.axpy(sb, phi);
    return delta;
}

// the driver loop (a2c.rs:55-67): transition, critic, actor, then the behaviour sample a' ~ pi_theta'(s') with the UPDATED theta (BLK_STEP; an
// episode cut by max_episode_steps restarts and samples there on BLK_RESET, a terminal one restarts before the sample) -- the one-step agents'
// convention.  W and theta stay in registers for the whole launch (k_train_gq's layout); the sample's probabilities are the next step's p
// (theta does not move in between)
template <int DOMAIN, int ORDER, int CRITIC>
__global__ __launch_bounds__(kBlock) void k_train_ac(Common c, float* __restrict__ theta, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
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
        WBuf<A, F, PK> w, th;
        mat_load<A, F, PK>(w, c.W, N, i);
        mat_load<A, F, PK>(th, theta, N, i);
        float p_s[A];
        { PhiBuf<F, PK> phi; ac_project<Bas>(env.s, phi); ac_probs<A, F, PK>(c, th, phi, p_s); }
        for (int k = 0; k < n_steps; ++k) {
            const uint64_t t = t0 + (uint64_t)k;
            Transition<D> tr = env.template step<Dom>();
            terminal_to_restart<Dom>(tr);                   // a terminal transition never reads s': go straight to the restart state
            const U4 xin = draw(c.seed, env.gid, t, BLK_INNER);
            const float delta = ac_step<Bas, A, F, PK, CRITIC>(c, w, th, env.s, p_s, env.a, tr.r, tr.term, tr.ns, xin);
            // ---- policy.sample(rng, s') with the UPDATED theta (a cut episode restarts first: its restart state is where the one sample is taken)
            restart_then_sample<Dom>(c, env, tally, tr, delta, t,
                [&](const float (&ns)[D], bool) { PhiBuf<F, PK> phi; ac_project<Bas>(ns, phi); ac_probs<A, F, PK>(c, th, phi, p_s); },
                [&](const U4& x) { return sample_probs<A>(p_s, x.z); });
        }
        env.store(c, i);
        mat_store<A, F, PK>(w, c.W, N, i);
        mat_store<A, F, PK>(th, theta, N, i);
    }
    tally.hand_over(stats);
}

// Handler<&Transition>::handle of ActorCritic (with the critic's SARSA::handle before it, as a2c.rs:62-63) on caller-supplied transitions:
// transition i is learner i's; the inner draw of batch-step t
template <int DOMAIN, int ORDER, int CRITIC>
__global__ __launch_bounds__(kBlock) void k_handle_ac(Common c, float* __restrict__ theta, const float* __restrict__ from, const int32_t* __restrict__ act,
                                                      const float* __restrict__ rew, const float* __restrict__ to, const uint8_t* __restrict__ termf,
                                                      int64_t Mn, uint64_t t, float* __restrict__ td_out) {
    using Dom = Domain<DOMAIN>;
    using Bas = FourierReg<DOMAIN, ORDER>;
    constexpr int D = Dom::D, A = Dom::A, F = Bas::F;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    const int64_t N = c.n_envs;
    constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    Given<D> tr;
    tr.template load<A>(from, act, rew, to, termf, Mn, i);
    WBuf<A, F, PK> w, th;
    mat_load<A, F, PK>(w, c.W, N, i);
    mat_load<A, F, PK>(th, theta, N, i);
    float p_s[A];
    { PhiBuf<F, PK> phi; ac_project<Bas>(tr.s, phi); ac_probs<A, F, PK>(c, th, phi, p_s); }
    const U4 xin = draw(c.seed, (uint32_t)(c.env_offset + i), t, BLK_INNER);
    const float delta = ac_step<Bas, A, F, PK, CRITIC>(c, w, th, tr.s, p_s, tr.a, tr.r, tr.term, tr.ns, xin);
    mat_store<A, F, PK>(w, c.W, N, i);
    mat_store<A, F, PK>(th, theta, N, i);
    if (td_out) td_out[i] = delta;
}

}  // namespace rsrl
