// kernels_gibbs_nac.hpp -- NAC over the Gibbs policy with a SARSA critic over the stable compatible basis on the register family, the agent and
// loop of rsrl/examples/nac_softmax.rs:
//   NAC::handle(())          rsrl/src/control/nac.rs:47-59          driver rsrl/examples/nac_softmax.rs:57-78
//   the critic               SARSA{q_func: LFA::scalar(SCB{policy, basis}, SGD(lr)), policy, gamma}  (control/td/sarsa.rs:53-75)
//   the actor                Gibbs::standard(LFA::vector(basis, SGD(1.0), A)) = Softmax(tau): grad_log softmax.rs:113-128, the step :208-221
// THE ONE DEFECT TAKEN OUT: SCB::project (fa/linear.rs:91-102) chains column 0 of grad_log with phi -- 2F features against the (A+1) F weights
// SCB::n_features (:85-89) announces: for A > 1 the example stops at its first critic.handle.  Built with the flattening of the sibling
// CompatibleBasis::project (:42-46), grad_log(..).into_shape(n_features), row-major -- the order NAC::handle reads back:
//     psi(s, a)[f*A + b] = (1[b==a] - p_b) phi(s)[f]   (f < F, b < A)        psi(s, a)[F*A + f] = phi(s)[f]
//     Q(s, a) = <w, psi(s, a)>,   w f32[(A+1) F] per learner, zero at create;   p = softmax_stable(theta^T phi(s) / tau), no 1/tau in grad_log
// Per learner the critic's w (the ctx's weights, ONE column of (A+1) F rows in the order above: row f*A + b is wbuf[b][f], row F*A + f is
// wbuf[A][f]) and the actor's theta f32[A][F][N] (the ctx's auxiliary matrix, ActorCritic's layout).  All f32:
//     c_b = 1[b==a] - p_b;   d_b = <w_b, phi> for the A score blocks, d_v = <w_v, phi> for the basis block (WBuf::q's four-chain dot)
//     Q(s, a) = fma(c_0, d_0, fma(c_1, d_1, ... fma(c_{A-1}, d_{A-1}, d_v)))
//   SARSA::handle:  na = sample_probs(p(s'), the agent's own draw BLK_INNER .z)  (computed whether or not the transition is terminal: counter-based)
//     delta = r - Q(s, a) (terminal) | fma(gamma, Q(s', na), r) - Q(s, a);   sc = lr delta
//     block b += (sc c_b) phi,  the basis block += sc phi, one fma per entry;  theta does not move.  Only one feature vector is live at a time
//   NAC::handle(()), every `period` steps of an episode:
//     ss = sum_{j = 0 .. F*A-1} w[j]^2 in that order, each square rounded before it is added;  norm = max(sqrt(ss), 1e-3);  scale = alpha32 / norm
//     theta[f][b] = fma(scale, w[f*A + b], theta[f][b]);   the critic is not reset;  the response is norm
#pragma once

#include "kernels_ac.hpp"

namespace rsrl {

template <int DOMAIN, int ORDER>
struct GibbsNacLane {
    using Dom = Domain<DOMAIN>;
    using Bas = FourierReg<DOMAIN, ORDER>;
    static constexpr int D = Dom::D, A = Dom::A, F = Bas::F;
    static constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    using Phi = PhiBuf<F, PK>;

    WBuf<A + 1, F, PK> w;      // the critic's weights: the A score blocks, then the basis block
    WBuf<A, F, PK> th;         // the actor's preferences

    // (the learner's base address goes through an empty asm: mat_load's reason)
    __device__ __forceinline__ void load_w(const float* __restrict__ W, int64_t N, int64_t i) {
        const float* p = W + i;
        asm("" : "+v"(p));
#pragma unroll
        for (int f = 0; f < F; ++f)
#pragma unroll
            for (int b = 0; b < A; ++b) w.put(b, f, p[(int64_t)(f * A + b) * N]);
#pragma unroll
        for (int f = 0; f < F; ++f) w.put(A, f, p[(int64_t)(F * A + f) * N]);
    }
    __device__ __forceinline__ void store_w(float* __restrict__ W, int64_t N, int64_t i) const {
        float* p = W + i;
        asm("" : "+v"(p));
#pragma unroll
        for (int f = 0; f < F; ++f)
#pragma unroll
            for (int b = 0; b < A; ++b) p[(int64_t)(f * A + b) * N] = w.get(b, f);
#pragma unroll
        for (int f = 0; f < F; ++f) p[(int64_t)(F * A + f) * N] = w.get(A, f);
    }
    __device__ __forceinline__ void load(const float* __restrict__ W, const float* __restrict__ theta, int64_t N, int64_t i) {
        load_w(W, N, i);
        mat_load<A, F, PK>(th, theta, N, i);
    }
    // Q(s, a) at phi = phi(s) with p = pi_theta(s)
    __device__ __forceinline__ float q(const Phi& phi, const float (&p)[A], int a) const {
        float d[A + 1];
        w.q(phi, d);
        float acc = d[A];
#pragma unroll
        for (int b = A - 1; b >= 0; --b) acc = fmaf(((a == b) ? 1.0f : 0.0f) - p[b], d[b], acc);
        return acc;
    }
    // SARSA::handle on one transition.  Returns delta; p_n = pi_theta(ns) (the behaviour sample's while the episode goes on, or -- after
    // terminal_to_restart -- at the restart state: theta does not move here)
    __device__ __forceinline__ float step(const Common& c, const float (&s)[D], int a, float r, bool term, const float (&ns)[D], const U4& xin,
                                          float (&p_n)[A]) {
        Phi phi;
        float boot;
        {
            ac_project<Bas>(ns, phi);
            ac_probs<A, F, PK>(c, th, phi, p_n);
            const int na = sample_probs<A>(p_n, xin.z);                  // policy.sample(rng, s'), the agent's own draw
            boot = q(phi, p_n, na);
        }
        ac_project<Bas>(s, phi);
        float p_s[A];
        ac_probs<A, F, PK>(c, th, phi, p_s);
        float d[A + 1], cb[A];
        w.q(phi, d);
        float qsa = d[A];
#pragma unroll
        for (int b = A - 1; b >= 0; --b) {
            cb[b] = ((a == b) ? 1.0f : 0.0f) - p_s[b];
            qsa = fmaf(cb[b], d[b], qsa);
        }
        const float delta = term ? (r - qsa) : (fmaf(c.alg.gamma, boot, r) - qsa);
        const float sc = c.alg.lr * delta;
        float sb[A + 1];
#pragma unroll
        for (int b = 0; b < A; ++b) sb[b] = sc * cb[b];
        sb[A] = sc;
        w.axpy(sb, phi);
        return delta;
    }
    // NAC::handle(()): theta steps along the critic's first F*A weights, read back row-major as (F, A).  Returns Response.norm
    __device__ __forceinline__ float actor(float alpha32) {
        float ss = 0.0f;
#pragma unroll
        for (int f = 0; f < F; ++f)
#pragma unroll
            for (int b = 0; b < A; ++b) {
                const float g = w.get(b, f);
                const float sq = g * g;               // (rounded before it is added: the tree is built with -ffp-contract=off)
                ss = ss + sq;
            }
        const float norm = fmaxf(sqrtf(ss), 1e-3f);
        const float scale = alpha32 / norm;
#pragma unroll
        for (int b = 0; b < A; ++b)
#pragma unroll
            for (int f = 0; f < F; ++f) th.put(b, f, fmaf(scale, w.get(b, f), th.get(b, f)));
        return norm;
    }
};

// the driver loop (nac_softmax.rs:57-78), i the 0-based index of the step in its episode: transition, critic.handle, the behaviour sample
// a' ~ pi_theta(s') with theta as it stands (after the restart if the episode ended or was cut; BLK_STEP / BLK_RESET as k_train_ac), THEN
// NAC::handle(()) if i % period == 0, i = 0 included.  w and theta stay in registers for the whole launch.  The statistics' sum |delta| is SARSA's
template <int DOMAIN, int ORDER>
__global__ __launch_bounds__(kBlock) void k_train_gibbs_nac(Common c, float* __restrict__ theta, uint32_t period, uint64_t t0, int n_steps,
                                                            DevStats* __restrict__ stats) {
    using Lane = GibbsNacLane<DOMAIN, ORDER>;
    using Dom = typename Lane::Dom;
    constexpr int D = Lane::D, A = Lane::A;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    Tally tally;
    if (i < N) {
        Learner<D> env;
        env.load(c, i);
        Lane ln;
        ln.load(c.W, theta, N, i);
        for (int k = 0; k < n_steps; ++k) {
            const uint64_t t = t0 + (uint64_t)k;
            const bool update = env.ep % period == 0;
            Transition<D> tr = env.template step<Dom>();
            terminal_to_restart<Dom>(tr);                   // a terminal transition never reads s': go straight to the restart state
            const U4 xin = draw(c.seed, env.gid, t, BLK_INNER);
            float p_n[A];
            const float delta = ln.step(c, env.s, env.a, tr.r, tr.term, tr.ns, xin, p_n);
            // (p_n already is pi_theta at the state the sample is taken at, unless the episode was cut: its restart state is projected then)
            const bool cut = tr.trunc;
            restart_then_sample<Dom>(c, env, tally, tr, delta, t,
                [&](const float (&ns)[D], bool) {
                    if (cut) { typename Lane::Phi phi; ac_project<typename Lane::Bas>(ns, phi); ac_probs<A, Lane::F, Lane::PK>(c, ln.th, phi, p_n); }
                },
                [&](const U4& x) { return sample_probs<A>(p_n, x.z); });
            if (update) (void)ln.actor(c.alg.alpha);
        }
        env.store(c, i);
        ln.store_w(c.W, N, i);
        mat_store<A, Lane::F, Lane::PK>(ln.th, theta, N, i);
    }
    tally.hand_over(stats);
}

// critic.handle (SARSA::handle) on caller-supplied transitions: transition i is learner i's; the inner draw of batch-step t.  theta stays
template <int DOMAIN, int ORDER>
__global__ __launch_bounds__(kBlock) void k_handle_gibbs_nac(Common c, const float* __restrict__ theta, const float* __restrict__ from,
                                                             const int32_t* __restrict__ act, const float* __restrict__ rew, const float* __restrict__ to,
                                                             const uint8_t* __restrict__ termf, int64_t Mn, uint64_t t, float* __restrict__ td_out) {
    using Lane = GibbsNacLane<DOMAIN, ORDER>;
    constexpr int D = Lane::D, A = Lane::A;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    const int64_t N = c.n_envs;
    Given<D> tr;
    tr.template load<A>(from, act, rew, to, termf, Mn, i);
    Lane ln;
    ln.load(c.W, theta, N, i);
    const U4 xin = draw(c.seed, (uint32_t)(c.env_offset + i), t, BLK_INNER);
    float p_n[A];
    const float delta = ln.step(c, tr.s, tr.a, tr.r, tr.term, tr.ns, xin, p_n);
    ln.store_w(c.W, N, i);
    if (td_out) td_out[i] = delta;
}

// NAC::handle(()) for the learners of mask (nullptr: every learner); norm_out (may be null): Response.norm, 0 for a learner left out
template <int DOMAIN, int ORDER>
__global__ __launch_bounds__(kBlock) void k_gibbs_nac_update(Common c, float* __restrict__ theta, const uint8_t* __restrict__ mask,
                                                             float* __restrict__ norm_out) {
    using Lane = GibbsNacLane<DOMAIN, ORDER>;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    if (i >= N) return;
    if (mask && mask[i] == 0) {
        if (norm_out) norm_out[i] = 0.0f;
        return;
    }
    Lane ln;
    ln.load(c.W, theta, N, i);
    const float norm = ln.actor(c.alg.alpha);
    mat_store<Lane::A, Lane::F, Lane::PK>(ln.th, theta, N, i);
    if (norm_out) norm_out[i] = norm;
}

// Function<(S, A)>::evaluate of the critic for every action: q_out f32[A][Mn], row b = Q(s_i, b) against learner i's w and theta; reads only
template <int DOMAIN, int ORDER>
__global__ __launch_bounds__(kBlock) void k_gibbs_nac_q(Common c, const float* __restrict__ theta, const float* __restrict__ states, int64_t Mn,
                                                        float* __restrict__ q_out) {
    using Lane = GibbsNacLane<DOMAIN, ORDER>;
    constexpr int D = Lane::D, A = Lane::A;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    float s[D];
#pragma unroll
    for (int d = 0; d < D; ++d) s[d] = states[(int64_t)d * Mn + i];
    Lane ln;
    ln.load(c.W, theta, c.n_envs, i);
    typename Lane::Phi phi;
    ac_project<typename Lane::Bas>(s, phi);
    float p[A];
    ac_probs<A, Lane::F, Lane::PK>(c, ln.th, phi, p);
#pragma unroll
    for (int b = 0; b < A; ++b) q_out[(int64_t)b * Mn + i] = ln.q(phi, p, b);
}

}  // namespace rsrl
