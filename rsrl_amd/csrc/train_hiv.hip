// train_hiv.hip -- every kernel of the HIVTreatment domain (kernels_hiv.hpp) and their launchers (launch.hpp): the driver loop, Handler::handle,
// Domain::transition / default, the Q / policy operations and the rollouts.  One-step agents (QLearning, SARSA, ExpectedSARSA, PAL) on
// per-learner f32 weights over the Fourier basis of orders 1-3 (FourierGenericModel<3>: F = 64 / 729 / 4 096, W f32[A][F][N]).
// Kept in a translation unit of its own so that no other kernel's machine code moves.
#include "launch.hpp"
#include "kernels_hiv.hpp"

namespace rsrl {

using HivModel = FourierGenericModel<3>;

// Domain::default() + initial policy.sample (rsrl_hip_reset), as k_reset with the hidden state
__global__ __launch_bounds__(kBlock) void k_hiv_reset(Common c, BasisGeom g, double* __restrict__ Y, uint64_t t) {
    constexpr int A = hiv::A;
    const int64_t N = c.n_envs;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double y[hiv::D]; float s[hiv::D];
    hiv::reset(y, s);
    HivModel::Feat ft; float q[A];
    HivModel::features(s, g, ft);
    HivModel::q_all(c, i, g, ft, q);
    const U4 x = draw(c.seed, (uint32_t)(c.env_offset + i), t, BLK_INIT);
    hiv::store(Y, N, i, y);
#pragma unroll
    for (int d = 0; d < hiv::D; ++d) c.state[(int64_t)d * N + i] = s[d];
    c.action[i] = policy_sample<A>(c.pol, q, x);
    c.ep_step[i] = 0;
}

// Domain::transition on the ctx's envs (as k_domain_step): the observation before and after, the reward; never terminal
__global__ __launch_bounds__(kBlock) void k_hiv_domain_step(Common c, double* __restrict__ Y, const int32_t* __restrict__ actions, float* __restrict__ from_out,
                                                            float* __restrict__ next_out, float* __restrict__ rew_out, uint8_t* __restrict__ term_out) {
    const int64_t N = c.n_envs;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (from_out) {
#pragma unroll
        for (int d = 0; d < hiv::D; ++d) from_out[(int64_t)d * N + i] = c.state[(int64_t)d * N + i];
    }
    const int a = clamp_action<hiv::A>(actions ? actions[i] : c.action[i]);
    double y[hiv::D]; float s[hiv::D];
    hiv::load(Y, N, i, y);
    const float r = hiv::step(y, s, a);
    hiv::store(Y, N, i, y);
#pragma unroll
    for (int d = 0; d < hiv::D; ++d) {
        c.state[(int64_t)d * N + i] = s[d];
        if (next_out) next_out[(int64_t)d * N + i] = s[d];
    }
    if (rew_out) rew_out[i] = r;
    if (term_out) term_out[i] = 0;
}

// Domain::default() for the masked envs (all of them for mask == nullptr); the episode's step count restarts
__global__ __launch_bounds__(kBlock) void k_hiv_domain_reset(Common c, double* __restrict__ Y, const uint8_t* __restrict__ mask) {
    const int64_t N = c.n_envs;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (mask && !mask[i]) return;
    double y[hiv::D]; float s[hiv::D];
    hiv::reset(y, s);
    hiv::store(Y, N, i, y);
#pragma unroll
    for (int d = 0; d < hiv::D; ++d) c.state[(int64_t)d * N + i] = s[d];
    c.ep_step[i] = 0;
}

// the observation of the hidden state (rsrl_hip_set_hidden_states); from_obs: the hidden state first becomes 10^obs of the given observation
// (rsrl_hip_set_states: the exact inverse inside (-5, 8); a clipped component cannot be inverted and becomes 10^-5 / 10^8)
__global__ __launch_bounds__(kBlock) void k_hiv_emit(double* __restrict__ Y, float* __restrict__ state, int64_t N, int from_obs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double y[hiv::D], obs[hiv::D]; float s[hiv::D];
    if (from_obs) {
#pragma unroll
        for (int d = 0; d < hiv::D; ++d) y[d] = pow(10.0, (double)state[(int64_t)d * N + i]);
        hiv::store(Y, N, i, y);
    } else {
        hiv::load(Y, N, i, y);
    }
    hiv::observe(y, obs, s);
#pragma unroll
    for (int d = 0; d < hiv::D; ++d) state[(int64_t)d * N + i] = s[d];
}

// Function / Enumerable / Policy / basis.project on caller states (observations), as k_qop
__global__ __launch_bounds__(kBlock) void k_hiv_qop(Common c, BasisGeom g, int op, const float* __restrict__ states, int64_t Mn, uint64_t call,
                                                    float* __restrict__ fout, int32_t* __restrict__ iout, const float* __restrict__ fin,
                                                    const int32_t* __restrict__ iin) {
    constexpr int A = hiv::A;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    float s[hiv::D];
#pragma unroll
    for (int d = 0; d < hiv::D; ++d) s[d] = states[(int64_t)d * Mn + i];
    HivModel::Feat ft;
    HivModel::features(s, g, ft);
    if (op == QOP_FEATURES) { HivModel::write_features(g, ft, Mn, i, fout, iout); return; }
    float q[A];
    HivModel::q_all(c, i, g, ft, q);
    qop_finish<A>(c, op, q, Mn, i, call, fout, iout, fin, iin);
}

// Handler<&Transition>::handle on caller-supplied transitions, per-learner weights (as k_handle)
__global__ __launch_bounds__(kBlock) void k_hiv_handle(Common c, BasisGeom g, const float* __restrict__ from, const int32_t* __restrict__ act,
                                                       const float* __restrict__ rew, const float* __restrict__ to, const uint8_t* __restrict__ termf,
                                                       int64_t Mn, uint64_t t, float* __restrict__ td_out) {
    constexpr int A = hiv::A;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    float s[hiv::D], ns[hiv::D];
#pragma unroll
    for (int d = 0; d < hiv::D; ++d) { s[d] = from[(int64_t)d * Mn + i]; ns[d] = to[(int64_t)d * Mn + i]; }
    const int a = clamp_action<A>(act[i]);
    const float r = rew[i];
    const bool term = termf[i] != 0;
    HivModel::Feat fs, fn;
    HivModel::features(s, g, fs);
    HivModel::features(ns, g, fn);
    float q_s[A], q_n[A];
    HivModel::q_all(c, i, g, fs, q_s);
    HivModel::q_all(c, i, g, fn, q_n);
    U4 xin = U4{0, 0, 0, 0};
    if (c.alg.kind == ALG_SARSA) xin = draw(c.seed, (uint32_t)(c.env_offset + i), t, BLK_INNER);
    float e;
    const float delta = td_dispatch<A>(c.alg, c.apol, q_s, a, q_n, r, term, xin, e);
    HivModel::update(c, i, g, fs, a, c.alg.lr * e);
    if (td_out) td_out[i] = delta;
}

// The driver loop: n_steps batch-steps per launch, one thread per learner, the hidden state in registers for the launch.  The step order, the
// draws and the statistics are k_train_mem's; HIV never terminates, so an episode ends only at the step cap (truncated, auto-reset to
// Domain::default()).  Q(s,.) is carried from one step to the next: it is Q(s',.) with the updated weights the previous step sampled from (the
// same evaluation k_train_mem repeats at the top of the step).
__global__ __launch_bounds__(kBlock) void k_hiv_train(Common c, BasisGeom g, double* __restrict__ Y, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    constexpr int D = hiv::D, A = hiv::A;
    const int64_t N = c.n_envs;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long n_ep = 0, n_trunc = 0, sum_len = 0;
    double sum_abs = 0.0, sum_r = 0.0;
    if (i < N) {
        const uint32_t gid = (uint32_t)(c.env_offset + i);
        const uint32_t cap = c.max_episode_steps;
        double y[D]; hiv::load(Y, N, i, y);
        float s[D];
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] = c.state[(int64_t)d * N + i];
        int a = c.action[i];
        uint32_t ep = c.ep_step[i];
        HivModel::Feat fs, fn;
        HivModel::features(s, g, fs);
        float q_s[A], q_n[A];
        HivModel::q_all(c, i, g, fs, q_s);
        float facc_abs = 0.0f, facc_r = 0.0f;
        for (int k = 0; k < n_steps; ++k) {
            const uint64_t t = t0 + (uint64_t)k;
            float ns[D];
            const float r = hiv::step(y, ns, a);
            ep += 1;
            const bool trunc = cap > 0 && ep >= cap;
            HivModel::features(ns, g, fn);
            HivModel::q_all(c, i, g, fn, q_n);
            U4 xin = U4{0, 0, 0, 0};
            if (c.alg.kind == ALG_SARSA) xin = draw(c.seed, gid, t, BLK_INNER);
            float e;
            const float delta = td_dispatch<A>(c.alg, c.apol, q_s, a, q_n, r, false, xin, e);
            HivModel::update(c, i, g, fs, a, c.alg.lr * e);
            HivModel::q_all(c, i, g, fn, q_n);                          // UPDATED weights
            const U4 x = draw(c.seed, gid, t, BLK_STEP);
            int na = policy_sample<A>(c.pol, q_n, x);
            facc_abs += fabsf(delta); facc_r += r;
            if (trunc) {
                n_ep += 1; n_trunc += 1; sum_len += ep; ep = 0;
                hiv::reset(y, ns);
                HivModel::features(ns, g, fn);
                HivModel::q_all(c, i, g, fn, q_n);
                const U4 xr = draw(c.seed, gid, t, BLK_RESET);
                na = policy_sample<A>(c.pol, q_n, xr);
            }
#pragma unroll
            for (int d = 0; d < D; ++d) s[d] = ns[d];
            fs = fn;
#pragma unroll
            for (int b = 0; b < A; ++b) q_s[b] = q_n[b];
            a = na;
        }
        sum_abs = (double)facc_abs; sum_r = (double)facc_r;
        hiv::store(Y, N, i, y);
#pragma unroll
        for (int d = 0; d < D; ++d) c.state[(int64_t)d * N + i] = s[d];
        c.action[i] = a;
        c.ep_step[i] = ep;
    }
    if (stats) block_stats_accumulate(stats, n_ep, n_trunc, sum_len, sum_abs, sum_r);
}

// Domain::rollout from a fresh default env per learner (as k_rollout); without a terminal state every rollout runs to step_limit
__global__ __launch_bounds__(kBlock) void k_hiv_rollout(Common c, BasisGeom g, int64_t step_limit, uint32_t* __restrict__ n_states,
                                                        float* __restrict__ total_reward, int64_t Mn, TrajOut tr, RolloutPolicy rp) {
    constexpr int D = hiv::D, A = hiv::A;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    const uint32_t gid = (uint32_t)(c.env_offset + i);
    uint64_t kk = 0;
    double y[D]; float s[D];
    hiv::reset(y, s);
    if (tr.states) {
#pragma unroll
        for (int d = 0; d < D; ++d) tr.states[(int64_t)d * tr.Mn + i] = s[d];
    }
    HivModel::Feat ft; float q[A], tot = 0.0f;
    int64_t steps = 0;
    while (steps < step_limit - 1) {
        HivModel::features(s, g, ft); HivModel::q_all(c, i, g, ft, q);
        const int a = rollout_action<A>(c.pol, rp, q, c.seed, gid, kk++);
        const float r = hiv::step(y, s, a);
        traj_record<D>(tr, i, steps, s, a, r);
        steps += 1; tot += r;
    }
    n_states[i] = (uint32_t)(steps + 1);
    if (total_reward) total_reward[i] = tot;
    if (tr.terminal) tr.terminal[i] = 0;
}

// ---- launchers (launch.hpp)
void launch_hiv_reset(hipStream_t st, const Common& k, const BasisGeom& g, double* Y, uint64_t t) {
    hipLaunchKernelGGL(k_hiv_reset, grid_for(k.n_envs), dim3(kBlock), 0, st, k, g, Y, t);
}
void launch_hiv_domain_step(hipStream_t st, const Common& k, double* Y, const int32_t* act, float* from, float* next, float* rew, uint8_t* term) {
    hipLaunchKernelGGL(k_hiv_domain_step, grid_for(k.n_envs), dim3(kBlock), 0, st, k, Y, act, from, next, rew, term);
}
void launch_hiv_domain_reset(hipStream_t st, const Common& k, double* Y, const uint8_t* mask) {
    hipLaunchKernelGGL(k_hiv_domain_reset, grid_for(k.n_envs), dim3(kBlock), 0, st, k, Y, mask);
}
void launch_hiv_emit(hipStream_t st, double* Y, float* state, int64_t N, bool from_obs) {
    hipLaunchKernelGGL(k_hiv_emit, grid_for(N), dim3(kBlock), 0, st, Y, state, N, from_obs ? 1 : 0);
}
void launch_hiv_qop(hipStream_t st, const Common& k, const BasisGeom& g, int op, const float* states, int64_t Mn, uint64_t call, float* fout, int32_t* iout,
                    const float* fin, const int32_t* iin) {
    hipLaunchKernelGGL(k_hiv_qop, grid_for(Mn), dim3(kBlock), 0, st, k, g, op, states, Mn, call, fout, iout, fin, iin);
}
void launch_hiv_handle(hipStream_t st, const Common& k, const BasisGeom& g, const Transitions& io, uint64_t t) {
    hipLaunchKernelGGL(k_hiv_handle, grid_for(io.M), dim3(kBlock), 0, st, k, g, io.from, io.act, io.rew, io.to, io.term, io.M, t, io.td_out);
}
void launch_hiv_train(hipStream_t st, const Common& k, const BasisGeom& g, double* Y, uint64_t t, int chunk, DevStats* stats) {
    hipLaunchKernelGGL(k_hiv_train, grid_for(k.n_envs), dim3(kBlock), 0, st, k, g, Y, t, chunk, stats);
}
void launch_hiv_rollout(hipStream_t st, const Common& k, const BasisGeom& g, int64_t step_limit, uint32_t* n_states, float* total, int64_t Mn, const TrajOut& tr,
                        const RolloutPolicy& rp) {
    hipLaunchKernelGGL(k_hiv_rollout, grid_for(Mn), dim3(kBlock), 0, st, k, g, step_limit, n_states, total, Mn, tr, rp);
}

}  // namespace rsrl
