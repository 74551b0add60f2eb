// kernels_reinforce.hpp -- the Monte-Carlo policy-gradient agents with a Gibbs policy on the register family:
//   REINFORCE<P>             rsrl/src/control/mc/reinforce.rs            (Handler<&Batch>::handle)
//   BaselineREINFORCE<B, P>  rsrl/src/control/mc/baseline_reinforce.rs   (the same, minus a read-only baseline B(s, a))
//   the policy               Gibbs::standard(LFA::vector(basis, SGD(1.0), A)) = Softmax(tau), as in kernels_ac.hpp
// handle(&batch) walks the batch FORWARD, first transition to last, and applies each update as it goes:
//     g       = r + gamma * g                                           (g = 0 before the batch's first transition)
//     e       = alpha * g          | BaselineREINFORCE: alpha * (g - <B[:,a], phi(s)>)
//     p       = softmax(theta^T phi(s) / tau)                           (theta as it stands: after the previous transition's update)
//     theta[:,b] += e * (1[b==a] - p_b) * phi(s) for every b            (grad_log without 1/tau, as kernels_ac.hpp)
// So g is the discounted sum of the rewards seen SO FAR, sum_{k<=t} gamma^(t-k) r_k, not the return-to-go: the reference's loop, restated literally.
// Because the return runs forward and the updates apply in order, handling an episode's batch at its end gives the bits of applying each update as
// soon as its transition exists, provided the episode's actions come from the policy as it stood when the episode began (Trajectory::into_batch:
// the batch is collected first).  The driver loop therefore needs no episode buffer: per learner it carries theta (the agent's weights, updated
// online), theta_b (the behaviour snapshot, theta at the start of the open episode) and g (the open episode's running return); an episode's end
// sets theta_b <- theta and g <- 0.
// B is the ctx's weight matrix W, f32[A][F][N], read-only (only `policy` is #[weights]); REINFORCE has none.  theta is the ctx's auxiliary matrix
// and theta_b a second one of its shape; g is f32[N].
// reinforce_step is the ONE update both kernels below run: the driver loop, handle_batch and the trait-granular loop give the same bits.
#pragma once

#include "kernels_ac.hpp"

namespace rsrl {

// one transition (s, a, r) of learner i: g <- r + gamma*g, then theta's step with p = pi_theta(s) (theta before this step).  Returns g.
// B's column a is loaded from memory for the baseline: a third register-resident matrix next to theta and theta_b would not leave MountainCar
// order 5 a spare register
template <int A, int F, bool PK, bool BASELINE>
__device__ __forceinline__ float reinforce_step(const Common& c, WBuf<A, F, PK>& th, const PhiBuf<F, PK>& phi, const float (&p)[A], int a, float r,
                                                float& g, int64_t N, int64_t i) {
    g = r + c.alg.gamma * g;                                     // (-ffp-contract=off: a multiply and an add, as the reference's f64 is restated in f32)
    float e;
    if constexpr (BASELINE) {
        WBuf<1, F, PK> col;
        mat_load<1, F, PK>(col, c.W + (int64_t)clamp_action<A>(a) * F * N, N, i);
        float v[1];
        col.q(phi, v);
        e = c.alg.alpha * (g - v[0]);
    } else {
        e = c.alg.alpha * g;
    }
    float sa[A];
#pragma unroll
    for (int b = 0; b < A; ++b) sa[b] = e * (((a == b) ? 1.0f : 0.0f) - p[b]);      // grad_log: (1[b==a] - p_b) phi(s)
    th.axpy(sa, phi);
    return g;
}

// the driver loop (Trajectory -> into_batch -> handle, one episode at a time, restated online): transition, reinforce_step on (s, a, r), on an
// episode's end (terminal or max_episode_steps) theta_b <- theta, g <- 0 and the restart, then the behaviour sample a' ~ pi_theta_b(s') (BLK_STEP;
// BLK_RESET after a cap, its alias).  theta and theta_b stay in registers for the whole launch.  One projection per step: phi(s') is the next
// step's phi(s), and one pass over it gives both preferences, theta's (the next step's p) and theta_b's (the sample)
template <int DOMAIN, int ORDER, bool BASELINE>
__global__ __launch_bounds__(kBlock) void k_train_reinforce(Common c, ReinforceState rs, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    using Dom = Domain<DOMAIN>;
    using Bas = FourierReg<DOMAIN, ORDER>;
    constexpr int D = Dom::D, A = Dom::A, F = Bas::F;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    Tally tally;
    if (i < N) {
        Learner<D> env;
        env.load(c, i);
        float g = rs.g[i];
        constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
        WBuf<A, F, PK> th, thb;
        mat_load<A, F, PK>(th, rs.theta, N, i);
        mat_load<A, F, PK>(thb, rs.theta_b, N, i);
        PhiBuf<F, PK> phi;
        float p[A];
        ac_project<Bas>(env.s, phi);
        ac_probs<A, F, PK>(c, th, phi, p);
        for (int k = 0; k < n_steps; ++k) {
            const uint64_t t = t0 + (uint64_t)k;
            Transition<D> tr = env.template step<Dom>();
            const float ret = reinforce_step<A, F, PK, BASELINE>(c, th, phi, p, env.a, tr.r, g, N, i);
            // a new episode samples from theta as it stands now: skipped by a wave none of whose learners ended, a select per register otherwise
            const bool ended = tr.ended();
            if (__ballot(ended) != 0ull) {
#pragma unroll
                for (int b = 0; b < A; ++b)
#pragma unroll
                    for (int f = 0; f < F; ++f) thb.put(b, f, ended ? th.get(b, f) : thb.get(b, f));
            }
            g = ended ? 0.0f : g;
            // ---- phi(s') once: the next step's p from theta, the behaviour sample from theta_b
            float pb[A];
            restart_then_sample<Dom>(c, env, tally, tr, ret, t,
                [&](const float (&ns)[D], bool) {
                    ac_project<Bas>(ns, phi);
                    float h[A], hb[A];
                    th.q(phi, h);
                    thb.q(phi, hb);
                    softmax_probs<A>(h, c.pol.tau, p);
                    softmax_probs<A>(hb, c.pol.tau, pb);
                },
                [&](const U4& x) { return sample_probs<A>(pb, x.z); });
        }
        env.store(c, i);
        rs.g[i] = g;
        mat_store<A, F, PK>(th, rs.theta, N, i);
        mat_store<A, F, PK>(thb, rs.theta_b, N, i);
    }
    tally.hand_over(stats);
}

// Handler<&Batch>::handle for every learner: learner i walks rows 0 .. len[i]-1 of its column of the batch (states [T][D][N], actions and rewards
// [T][N]) with its own g from 0.  theta_b and the carried g are not touched.  ret_out [T][N] (optional): g at each handled transition, NaN in
// the rows past the learner's length
template <int DOMAIN, int ORDER, bool BASELINE>
__global__ __launch_bounds__(kBlock) void k_handle_reinforce(Common c, float* __restrict__ theta, const float* __restrict__ states,
                                                             const int32_t* __restrict__ act, const float* __restrict__ rew,
                                                             const uint32_t* __restrict__ len, int64_t T, float* __restrict__ ret_out) {
    using Dom = Domain<DOMAIN>;
    using Bas = FourierReg<DOMAIN, ORDER>;
    constexpr int D = Dom::D, A = Dom::A, F = Bas::F;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    if (i >= N) return;
    const int64_t L = (int64_t)len[i] < T ? (int64_t)len[i] : T;      // (a device array of lengths is not inspected by the host: clamped here)
    if (ret_out)
        for (int64_t t = L; t < T; ++t) ret_out[t * N + i] = __builtin_nanf("");
    if (L == 0) return;
    constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    WBuf<A, F, PK> th;
    mat_load<A, F, PK>(th, theta, N, i);
    float g = 0.0f;
    for (int64_t t = 0; t < L; ++t) {
        float s[D];
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] = states[(t * D + d) * N + i];
        const int a = clamp_action<A>(act[t * N + i]);
        const float r = rew[t * N + i];
        PhiBuf<F, PK> phi;
        ac_project<Bas>(s, phi);
        float p[A];
        ac_probs<A, F, PK>(c, th, phi, p);
        reinforce_step<A, F, PK, BASELINE>(c, th, phi, p, a, r, g, N, i);
        if (ret_out) ret_out[t * N + i] = g;
    }
    mat_store<A, F, PK>(th, theta, N, i);
}

// a new episode for the learners in mask (all when mask is null): theta_b <- theta, g <- 0.  One thread per (element, learner), learners fastest
__global__ __launch_bounds__(256) void k_reinforce_restart(ReinforceState rs, int64_t N, int64_t FA, const uint8_t* __restrict__ mask) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= FA * N) return;
    const int64_t i = idx % N;
    if (mask && !mask[i]) return;
    rs.theta_b[idx] = rs.theta[idx];
    if (idx < N) rs.g[idx] = 0.0f;
}

}  // namespace rsrl
