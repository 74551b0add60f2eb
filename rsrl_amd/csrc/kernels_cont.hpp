// kernels_cont.hpp -- the thread-per-learner continuous-action agents on ContinuousMountainCar, over the policies of cont_policy.hpp (Cont<P>): one
// thread per learner with its weights, the policy's two columns pol f32[2][F][N] (the ctx's auxiliary matrix) and the features in registers.
// Every step below holds no data-dependent loop, no shuffle and no LDS access; the Beta sample's bounded gamma loop stands outside the rules, in
// the driver loops.  The loops take driver_loop.hpp's Tally, ping_pong, Given and mat_load / mat_store and keep the learner's state in locals,
// with the episode's end in restart_then_sample's convention (ONE behaviour sample per step, at the restart state when the episode ended,
// terminal or cut, on BLK_STEP; BLK_RESET is its alias), and each shared loop IS the __global__ function: the form whose machine code is the
// parents'.  The one other form measured -- Learner<D, float> / Transition behind a thin per-agent entry point over a __forceinline__ loop -- ran
// 2-3 % slower in six of ten (loop, order) rows; the two were not timed apart (profiles/cont_frame.md).
// The family table (ctx.hpp) reports the agents' kernel names, as labels: k_train_cacla and k_train_tdac_cont are
// k_train_td0_cont<ORDER, CaclaRule | TdacContRule<P>>, k_train_nac_gauss and k_train_nac_beta are k_train_nac<ORDER, P>.
//
// THE TD(0)-CRITIC PAIR: three one-column approximators per learner, the V learner's w f32[F][N] (the ctx's weights, TD's layout) and the two
// columns; 5F floats in registers with phi(s) and phi(s'), 180 at order 5.  The V learner is TD{v_func = ScalarLFA(basis, SGD(lr)), gamma}
// (prediction/td/td.rs:38-58): the caller's `eval`, trained before the agent sees the transition (the order of tdac.rs, tdac_beta.rs and nac.rs).
// Per transition (s, a, r, s', term), all f32, in this order:
//     1.  x0 = <col0, phi(s)>, x1 = <col1, phi(s)>       (the columns before any move)
//     2.  TD::handle, tdac_step's expressions:   v_s = <w, phi(s)>, v_n = <w, phi(s')>;  td = r - v_s (terminal) | r + gamma * v_n - v_s;
//                                                w += (lr * td) phi(s), one fma per element;   then v_s, v_n again with the UPDATED w
//   CACLA::handle (rsrl/src/control/cacla.rs:42-64) over the Gaussian policy, Gaussian::handle(StateActionUpdate) of general.rs:196-212:
//     3.  target = r (terminal: r alone, not r - V(s')) | r + gamma * v_n;   gate = target > v_s   (strict; a NaN on either side closes it)
//     4.  gate open only:   (mu, sd) = params;  e = (a - mode) * alpha;  (c_m, c_s) = gauss_coef;  w_m += (e * c_m) phi(s);  w_s += (e * c_s) phi(s)
//     A closed gate leaves both columns' BITS as they were, whatever the coefficients would have been (they are not even computed): the update
//     sits behind the gate itself, never behind a product with 0 -- fma(0, phi, -0.0) is +0.0, and 0 * inf a NaN.
//     THE LITERAL RULE: the mean's step is e * c_m = alpha (a - mu)^2 / Sigma >= 0 whatever side of the mean the action lay on -- the reference
//     hands the policy `error: (a - mode) * alpha` and the policy multiplies it by its score once more.  This is not van Hasselt's
//     mu += alpha (a - mu); it is what cacla.rs and general.rs say.  There is no safeguard: sd is floored at 0.01 only, the coefficients reach 1e4.
//   ActorCritic::tdac / TDCritic (control/ac.rs:32-52, :87-98, :100-115) over either policy; RSRL_TD_ACTOR_CRITIC's arithmetic (kernels_tdac.hpp):
//     3.  TDCritic::target (ac.rs:40-50):   c = r - v_n (terminal: V of the terminal state itself) | r + gamma * v_n - v_s;   e = alpha * c
//     4.  policy.handle(StateActionUpdate{s, a, error: e}), always -- there is no gate: Cont<P>::actor_steps.  A coefficient that is not finite
//         propagates, as in the reference.
//   There is no inner draw.  w / td are the bits of a TD ctx's on the same transitions whatever the columns are.
//
// NAC (rsrl/src/control/nac.rs:47-59; the loops of examples/nac.rs and nac_beta.rs) with a SARSA critic over the stable compatible basis:
//   the critic               SARSA{q_func: LFA::scalar(SCB{policy, basis}, SGD(lr)), policy, gamma}  (control/td/sarsa.rs:53-75)
//   SCB::project((s, a))     rsrl/src/fa/linear.rs:79-103: grad_log pi(a|s) chained with basis.project(s), 3F features
//   Per learner the critic's w[3F] (the ctx's weights: rows 0..F-1 belong to column 0, F..2F-1 to column 1, 2F..3F-1 to the plain basis; [3F][N]
//   in memory, which is WBuf<3, F>'s [3][F][N]) and the two columns.  With (c_0, c_1) = Cont<P>::coef:
//     psi(s, a) = [ c_0 phi(s) ; c_1 phi(s) ; phi(s) ]
//     Q(s, a)   = <w, psi(s, a)>  evaluated as  fma(c_0, d_0, fma(c_1, d_1, d_2)),  d_k = <w[kF .. kF+F-1], phi(s)> (WBuf::q's four-chain dot):
//                 THREE LENGTH-F DOTS COMBINED, not the 3F products in index order -- phi(s) is multiplied into each block once
//   Per transition, SARSA::handle:
//     na    ~ policy(s') on the agent's own stream: Cont<P>::sample(seed, gid, t, BLK_INNER) (the reference draws from thread_rng())
//     delta = r - Q(s, a)  (terminal)  |  fma(gamma, Q(s', na), r) - Q(s, a)
//     w    += (lr delta) psi(s, a):  block k gets WBuf::axpy with the scalar (lr delta) c_k (1 for the last block)
//   The bootstrap is computed whether or not the transition is terminal and selected afterwards (the draws are counter-based).  The columns do
//   not move here.  NAC::handle(()), every `period` steps of an episode (nac_beta.rs:69 hard-codes 100):
//     g = w[0 .. 2F-1];  norm = max(sqrt(sum g_j^2), 1e-3), the squares rounded and added in index order;  scale = alpha32 / norm
//     col_0 += scale g[0 .. F-1],  col_1 += scale g[F .. 2F-1]   (fma per element);  the critic's weights are not reset
#pragma once

#include "cont_policy.hpp"

namespace rsrl {

template <int ORDER>
struct ContShape {
    using Dom = Domain<kCmc>;
    using Bas = FourierReg<kCmc, ORDER>;
    static constexpr int D = Dom::D, F = Bas::F;
    static constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    using Phi = PhiBuf<F, PK>;
};

// ---- the TD(0)-critic pair's rules: one transition on projected phi(s), phi(s').  Return TD's error; `moved`: whether the policy's columns did.
// TD::handle (the expressions of k_train_td / k_handle_td, as tdac_step states them), then V at s and s' again with the updated w
template <int F, bool PK>
__device__ __forceinline__ float td0_critic(WBuf<1, F, PK>& w, const PhiBuf<F, PK>& phi_s, const PhiBuf<F, PK>& phi_n, float gamma, float lr, float r, bool term,
                                            float& v_s_new, float& v_n_new) {
    float v_s[1], v_n[1];
    w.q(phi_s, v_s);
    w.q(phi_n, v_n);
    const float td = term ? (r - v_s[0]) : (r + gamma * v_n[0] - v_s[0]);
    const float sb[1] = {lr * td};
    w.axpy(sb, phi_s);
    w.q(phi_s, v_s);
    w.q(phi_n, v_n);
    v_s_new = v_s[0]; v_n_new = v_n[0];
    return td;
}
struct CaclaRule {
    static constexpr ContPolicy kPolicy = ContPolicy::Gaussian;
    template <int F, bool PK>
    __device__ __forceinline__ static float step(const Common& c, WBuf<1, F, PK>& w, WBuf<2, F, PK>& pol, const PhiBuf<F, PK>& phi_s,
                                                 const PhiBuf<F, PK>& phi_n, float a, float r, bool term, bool& moved) {
        using Pol = Cont<kPolicy>;
        const float gamma = c.alg.gamma, lr = c.alg.lr;
        float x[2], v_s, v_n;
        pol.q(phi_s, x);
        const float td = td0_critic<F, PK>(w, phi_s, phi_n, gamma, lr, r, term, v_s, v_n);
        const float target = term ? r : (r + gamma * v_n);
        moved = target > v_s;
        if (moved) {
            float mu, sd, sp[2];
            Pol::params(x[0], x[1], mu, sd);
            const float e = (a - Pol::mode(mu, sd)) * c.alg.alpha;
            Pol::actor_steps(e, x[0], x[1], mu, sd, a, sp[0], sp[1]);
            pol.axpy(sp, phi_s);
        }
        return td;
    }
};
template <ContPolicy P>
struct TdacContRule {
    static constexpr ContPolicy kPolicy = P;
    template <int F, bool PK>
    __device__ __forceinline__ static float step(const Common& c, WBuf<1, F, PK>& w, WBuf<2, F, PK>& pol, const PhiBuf<F, PK>& phi_s,
                                                 const PhiBuf<F, PK>& phi_n, float a, float r, bool term, bool& moved) {
        const float gamma = c.alg.gamma, lr = c.alg.lr;
        float x[2], v_s, v_n;
        pol.q(phi_s, x);
        const float td = td0_critic<F, PK>(w, phi_s, phi_n, gamma, lr, r, term, v_s, v_n);
        const float target = term ? (r - v_n) : (r + gamma * v_n - v_s);
        const float e = c.alg.alpha * target;
        float p0, p1, sp[2];
        Cont<P>::params(x[0], x[1], p0, p1);
        Cont<P>::actor_steps(e, x[0], x[1], p0, p1, a, sp[0], sp[1]);
        pol.axpy(sp, phi_s);
        moved = true;
        return td;
    }
};

// the pair's driver loop (k_train_cacla, k_train_tdac_cont): transition on the policy's domain action, eval.handle, agent.handle, then the behaviour sample with the UPDATED
// columns.  s' is projected as it is, the terminal state included (TDCritic reads V(s'); TD and CACLA's gate do not read it there); phi(s')
// becomes the next step's phi(s) (two buffers that swap roles) unless the episode ended: then the restart state is projected in its place.
// The statistics' sum |delta| is TD's
template <int ORDER, class Rule>
__global__ __launch_bounds__(kBlock) void k_train_td0_cont(Common c, ContState st, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    using Sh = ContShape<ORDER>;
    using Dom = typename Sh::Dom;
    using Bas = typename Sh::Bas;
    using Phi = typename Sh::Phi;
    using Pol = Cont<Rule::kPolicy>;
    constexpr int D = Sh::D, F = Sh::F;
    constexpr bool PK = Sh::PK;
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
            const bool term = Dom::step(s, Pol::domain_action(a), rw);      // s <- s' (the domain clips the action: map_onto)
            ep += 1;
            const bool trunc = !term && cap > 0 && ep >= cap;
            ac_project<Bas>(s, phi_n);
            bool moved;
            const float td = Rule::template step<F, PK>(c, w, pol, phi_s, phi_n, a, rw, term, moved);
            if (term || trunc) {                                      // the restart state is where the sample is taken
                tally.episode_end(ep, trunc);
                Dom::reset(s);
                ac_project<Bas>(s, phi_n);
            }
            float x[2], p0, p1;
            pol.q(phi_n, x);
            Pol::params(x[0], x[1], p0, p1);
            a = Pol::sample(c.seed, gid, t, BLK_STEP, p0, p1);
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
// eval.handle then the rule's handle on caller-supplied transitions: transition i is learner i's.  The columns are stored only where the policy moved
template <int ORDER, class Rule>
__global__ __launch_bounds__(kBlock) void k_handle_td0_cont(Common c, ContState st, const float* __restrict__ from, const float* __restrict__ act,
                                                            const float* __restrict__ rew, const float* __restrict__ to, const uint8_t* __restrict__ termf,
                                                            int64_t Mn, float* __restrict__ td_out) {
    using Sh = ContShape<ORDER>;
    using Bas = typename Sh::Bas;
    constexpr int D = Sh::D, F = Sh::F;
    constexpr bool PK = Sh::PK;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    const int64_t N = c.n_envs;
    Given<D> tr;
    tr.load(from, rew, to, termf, Mn, i);
    typename Sh::Phi phi_s, phi_n;
    ac_project<Bas>(tr.s, phi_s);
    ac_project<Bas>(tr.ns, phi_n);
    WBuf<1, F, PK> w;
    WBuf<2, F, PK> pol;
    mat_load<1, F, PK>(w, c.W, N, i);
    mat_load<2, F, PK>(pol, st.pol, N, i);
    bool moved;
    const float td = Rule::template step<F, PK>(c, w, pol, phi_s, phi_n, act[i], tr.r, tr.term, moved);
    mat_store<1, F, PK>(w, c.W, N, i);
    if (moved) mat_store<2, F, PK>(pol, st.pol, N, i);
    if (td_out) td_out[i] = td;
}

// ---- NAC.  NacWeights: what a learner holds, and the actor's update, whatever the policy; NacLane: the critic over the policy's SCB
template <int ORDER>
struct NacWeights : ContShape<ORDER> {
    using Sh = ContShape<ORDER>;
    using Phi = typename Sh::Phi;
    static constexpr int F = Sh::F;
    static constexpr bool PK = Sh::PK;

    WBuf<3, F, PK> w;          // the critic's weights, SCB's three blocks
    WBuf<2, F, PK> pol;        // the policy's columns

    __device__ __forceinline__ void load(const float* __restrict__ W, const float* __restrict__ P, int64_t N, int64_t i) {
        mat_load<3, F, PK>(w, W, N, i);
        mat_load<2, F, PK>(pol, P, N, i);
    }
    // x_0, x_1 at phi
    __device__ __forceinline__ void prefs(const Phi& phi, float& x0, float& x1) const {
        float x[2];
        pol.q(phi, x);
        x0 = x[0]; x1 = x[1];
    }
    // Q = <w, psi>: three dots combined
    __device__ __forceinline__ float q(const Phi& phi, float c0, float c1) const {
        float d[3];
        w.q(phi, d);
        return fmaf(c0, d[0], fmaf(c1, d[1], d[2]));
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
template <int ORDER, ContPolicy P>
struct NacLane : NacWeights<ORDER> {
    using Base = NacWeights<ORDER>;
    using Bas = typename Base::Bas;
    using Phi = typename Base::Phi;
    using Pol = Cont<P>;
    static constexpr int D = Base::D;

    // Q(s, a) at phi = phi(s); x0, x1: the preferences there; c0, c1: psi's coefficients
    __device__ __forceinline__ float q_phi(const Phi& phi, float a, float& x0, float& x1, float& c0, float& c1) const {
        float p0, p1;
        this->prefs(phi, x0, x1);
        Pol::params(x0, x1, p0, p1);
        Pol::coef(x0, x1, p0, p1, a, c0, c1);
        return this->q(phi, c0, c1);
    }
    // Function<(S, A)>::evaluate at (s, a)
    __device__ __forceinline__ float q_at(const float (&s)[D], float a) const {
        Phi phi;
        ac_project<Bas>(s, phi);
        float x0, x1, c0, c1;
        return q_phi(phi, a, x0, x1, c0, c1);
    }
    // SARSA::handle on one transition of learner gid at batch-step t.  Returns delta; xn0, xn1: the preferences at s' (the behaviour sample's, while
    // the episode goes on: the columns do not move here).  Only one feature vector is live at a time
    __device__ __forceinline__ float step(const Common& c, const float (&s)[D], float a, float r, bool term, const float (&ns)[D], uint32_t gid, uint64_t t,
                                          float& xn0, float& xn1) {
        Phi phi;
        float boot;
        {
            ac_project<Bas>(ns, phi);
            this->prefs(phi, xn0, xn1);
            float p0, p1, c0, c1;
            Pol::params(xn0, xn1, p0, p1);
            const float na = Pol::sample(c.seed, gid, t, BLK_INNER, p0, p1);      // policy.sample(rng, s'), the agent's own draw
            Pol::coef(xn0, xn1, p0, p1, na, c0, c1);
            boot = this->q(phi, c0, c1);
        }
        ac_project<Bas>(s, phi);
        float x0, x1, c0, c1;
        const float qsa = q_phi(phi, a, x0, x1, c0, c1);
        const float delta = term ? (r - qsa) : (fmaf(c.alg.gamma, boot, r) - qsa);
        const float sc = c.alg.lr * delta;
        const float sb[3] = {sc * c0, sc * c1, sc};
        this->w.axpy(sb, phi);
        return delta;
    }
};

// NAC's driver loop (k_train_nac_gauss, k_train_nac_beta; nac.rs:55-76, nac_beta.rs:55-76), i the 0-based index of the step in its episode: transition on the policy's domain action,
// critic.handle, the behaviour sample a' ~ policy(s') with the columns as they stand, THEN agent.handle(()) if i % period == 0 -- the next step's
// psi(s, a) is evaluated with the columns after it (NacLane::step computes the preferences at s itself)
template <int ORDER, ContPolicy P>
__global__ __launch_bounds__(kBlock) void k_train_nac(Common c, ContState st, uint32_t period, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    using Lane = NacLane<ORDER, P>;
    using Dom = typename Lane::Dom;
    using Pol = Cont<P>;
    constexpr int D = Lane::D;
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
        Lane ln;
        ln.load(c.W, st.pol, N, i);
        for (int k = 0; k < n_steps; ++k) {
            const uint64_t t = t0 + (uint64_t)k;
            const bool update = ep % period == 0;
            float ns[D];
#pragma unroll
            for (int d = 0; d < D; ++d) ns[d] = s[d];
            float rw;
            const bool term = Dom::step(ns, Pol::domain_action(a), rw);      // (the domain clips the action: map_onto)
            ep += 1;
            const bool trunc = !term && cap > 0 && ep >= cap;
            float x0, x1;
            const float delta = ln.step(c, s, a, rw, term, ns, gid, t, x0, x1);
            if (term || trunc) {                                      // the restart state is where the sample is taken
                tally.episode_end(ep, trunc);
                Dom::reset(ns);
                typename Lane::Phi phi;
                ac_project<typename Lane::Bas>(ns, phi);
                ln.prefs(phi, x0, x1);
            }
            float p0, p1;
            Pol::params(x0, x1, p0, p1);
            a = Pol::sample(c.seed, gid, t, BLK_STEP, p0, p1);
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
template <int ORDER, ContPolicy P>
__global__ __launch_bounds__(kBlock) void k_handle_nac(Common c, ContState st, const float* __restrict__ from, const float* __restrict__ act,
                                                       const float* __restrict__ rew, const float* __restrict__ to, const uint8_t* __restrict__ termf,
                                                       int64_t Mn, uint64_t t, float* __restrict__ td_out) {
    using Lane = NacLane<ORDER, P>;
    constexpr int D = Lane::D;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    const int64_t N = c.n_envs;
    float s[D], ns[D];      // (not Given: with the reward and the flag read before the weights, <2, Gaussian> takes 82 registers for 74 and loses a wave)
#pragma unroll
    for (int d = 0; d < D; ++d) { s[d] = from[(int64_t)d * Mn + i]; ns[d] = to[(int64_t)d * Mn + i]; }
    Lane ln;
    ln.load(c.W, st.pol, N, i);
    float xn0, xn1;
    const float delta = ln.step(c, s, act[i], rew[i], termf[i] != 0, ns, (uint32_t)(c.env_offset + i), t, xn0, xn1);
    mat_store<3, Lane::F, Lane::PK>(ln.w, c.W, N, i);
    if (td_out) td_out[i] = delta;
}

// NAC::handle(()) for the learners of mask (nullptr: every learner); norm_out (may be null): Response.norm, 0 for a learner left out
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_nac_update(Common c, ContState st, const uint8_t* __restrict__ mask, float* __restrict__ norm_out) {
    using Lane = NacWeights<ORDER>;
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
template <int ORDER, ContPolicy P>
__global__ __launch_bounds__(kBlock) void k_nac_q(Common c, ContState st, const float* __restrict__ states, const float* __restrict__ act, int64_t Mn,
                                                  float* __restrict__ q_out) {
    using Lane = NacLane<ORDER, P>;
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
