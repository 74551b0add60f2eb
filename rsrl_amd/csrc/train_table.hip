// train_table.hip -- every kernel of CliffWalk over the tabular Q (kernels_table.hpp) and their launchers (launch.hpp): the two driver loops,
// Handler::handle, Domain::transition / default, the Q / policy operations and the rollouts.  One-step agents (QLearning, SARSA, ExpectedSARSA, PAL)
// on per-learner f32 tables, W f32[4][60][N].  Kept in a translation unit of its own so that no other kernel's machine code moves.
#include "launch.hpp"
#include "kernels_table.hpp"

namespace rsrl {

using table::A;
using table::D;
using table::Dom;
using table::kEntries;
using table::kLanes;
using table::LdsAcc;
using table::MemAcc;

// the caller's (or the ctx's) state i of Mn as a cell
__device__ __forceinline__ void table_cell(const float* __restrict__ states, int64_t Mn, int64_t i, int& x, int& y) {
    x = Dom::cell(states[i], Dom::kWidth); y = Dom::cell(states[Mn + i], Dom::kHeight);
}

// Domain::default() + initial policy.sample (rsrl_hip_reset), as k_reset
__global__ __launch_bounds__(kBlock) void k_table_reset(Common c, uint64_t t) {
    const int64_t N = c.n_envs;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float q[A];
    MemAcc{c.W + i, N}.row(Dom::row(0, 0), q);
    const U4 x = draw(c.seed, (uint32_t)(c.env_offset + i), t, BLK_INIT);
    c.state[i] = 0.0f; c.state[N + i] = 0.0f;
    c.action[i] = policy_sample<A>(c.pol, q, x);
    c.ep_step[i] = 0;
}

// Domain::transition on the ctx's envs (as k_domain_step): the state before (as the ctx holds it) and after, the reward, the terminal flag
__global__ __launch_bounds__(kBlock) void k_table_domain_step(Common c, const int32_t* __restrict__ actions, float* __restrict__ from_out,
                                                              float* __restrict__ next_out, float* __restrict__ rew_out, uint8_t* __restrict__ term_out) {
    const int64_t N = c.n_envs;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (from_out) { from_out[i] = c.state[i]; from_out[N + i] = c.state[N + i]; }
    const int a = clamp_action<A>(actions ? actions[i] : c.action[i]);
    int x, y; float r;
    table_cell(c.state, N, i, x, y);
    const bool term = Dom::step_cell(x, y, a, r);
    c.state[i] = (float)x; c.state[N + i] = (float)y;
    if (next_out) { next_out[i] = (float)x; next_out[N + i] = (float)y; }
    if (rew_out) rew_out[i] = r;
    if (term_out) term_out[i] = term ? 1 : 0;
}

// Domain::default() for the masked envs (all of them for mask == nullptr); the episode's step count restarts
__global__ __launch_bounds__(kBlock) void k_table_domain_reset(Common c, const uint8_t* __restrict__ mask) {
    const int64_t N = c.n_envs;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (mask && !mask[i]) return;
    c.state[i] = 0.0f; c.state[N + i] = 0.0f;
    c.ep_step[i] = 0;
}

// Function / Enumerable / Policy on caller states, as k_qop: state i against learner i's table
__global__ __launch_bounds__(kBlock) void k_table_qop(Common c, int op, const float* __restrict__ states, int64_t Mn, uint64_t call,
                                                      float* __restrict__ fout, int32_t* __restrict__ iout, const float* __restrict__ fin,
                                                      const int32_t* __restrict__ iin) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    int x, y;
    table_cell(states, Mn, i, x, y);
    float q[A];
    MemAcc{c.W + i, c.n_envs}.row(Dom::row(x, y), q);
    qop_finish<A>(c, op, q, Mn, i, call, fout, iout, fin, iin);
}

// Handler<&Transition>::handle on caller-supplied transitions (as k_handle): transition i is learner i's
__global__ __launch_bounds__(kBlock) void k_table_handle(Common c, const float* __restrict__ from, const int32_t* __restrict__ act,
                                                         const float* __restrict__ rew, const float* __restrict__ to, const uint8_t* __restrict__ termf,
                                                         int64_t Mn, uint64_t t, float* __restrict__ td_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    int x, y, nx, ny;
    table_cell(from, Mn, i, x, y);
    table_cell(to, Mn, i, nx, ny);
    const float delta = table::table_handle(c, MemAcc{c.W + i, c.n_envs}, Dom::row(x, y), clamp_action<A>(act[i]), Dom::row(nx, ny), rew[i], termf[i] != 0,
                                            (uint32_t)(c.env_offset + i), t);
    if (td_out) td_out[i] = delta;
}

// The driver loop with the tables left in memory: n_steps batch-steps per launch, one learner per lane, every row read a gather of four lines
__global__ __launch_bounds__(kLanes) void k_table_train_mem(Common c, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    const int64_t N = c.n_envs;
    const int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    Tally tally;
    if (i < N) {
        table::Learner L; L.load(c, i);
        const MemAcc acc{c.W + i, N};
        for (int k = 0; k < n_steps; ++k) table::table_step(c, acc, L, tally, t0 + (uint64_t)k);
        L.store(c, i);
    }
    tally.hand_over(stats);
}

// The hot path: the same loop out of LDS.  A block is one wave; it stages its 64 learners' whole tables (240 lines of 256 B, each one coalesced
// load and one conflict-free ds_write_b32), runs the launch's batch-steps on the image [entry][lane] and stores the tables back.  A lane only ever
// touches its own column of the image: no barrier.  61 440 B per block -- two blocks per CU.
__global__ __launch_bounds__(kLanes) void k_table_train_lds(Common c, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    __shared__ float image[kEntries * kLanes];
    const int64_t N = c.n_envs;
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kLanes + lane;
    Tally tally;
    if (i < N) {
        float* __restrict__ g = c.W + i;
#pragma unroll 16
        for (int e = 0; e < kEntries; ++e) image[e * kLanes + lane] = g[(int64_t)e * N];
        table::Learner L; L.load(c, i);
        const LdsAcc acc{image + lane, 0};
        for (int k = 0; k < n_steps; ++k) table::table_step(c, acc, L, tally, t0 + (uint64_t)k);
        L.store(c, i);
#pragma unroll 16
        for (int e = 0; e < kEntries; ++e) g[(int64_t)e * N] = image[e * kLanes + lane];
    }
    tally.hand_over(stats);
}

// Domain::rollout from a fresh default env per learner: k_rollout's body (models.hpp) with TrajOut and RolloutPolicy
__global__ __launch_bounds__(kBlock) void k_table_rollout(Common c, int64_t step_limit, uint32_t* __restrict__ n_states, float* __restrict__ total_reward,
                                                          int64_t Mn, TrajOut tr, RolloutPolicy rp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Mn) return;
    const uint32_t gid = (uint32_t)(c.env_offset + i);
    const MemAcc acc{c.W + i, c.n_envs};
    uint64_t kk = 0;
    int x = 0, y = 0;
    float s[D] = {0.0f, 0.0f};
    if (tr.states) { tr.states[i] = 0.0f; tr.states[tr.Mn + i] = 0.0f; }
    float q[A], r, tot = 0.0f;
    acc.row(Dom::row(x, y), q);
    int a = rollout_action<A>(c.pol, rp, q, c.seed, gid, kk++);
    bool term = Dom::step_cell(x, y, a, r);          // the first step is taken eagerly (lib.rs:457-459)
    int64_t steps = 0;
    while (steps < step_limit - 1) {
        s[0] = (float)x; s[1] = (float)y;
        traj_record<D>(tr, i, steps, s, a, r);
        steps += 1; tot += r;
        if (term) break;
        if (steps >= step_limit - 1) break;
        acc.row(Dom::row(x, y), q);
        a = rollout_action<A>(c.pol, rp, q, c.seed, gid, kk++);
        term = Dom::step_cell(x, y, a, r);
    }
    n_states[i] = (uint32_t)(steps + 1);
    if (total_reward) total_reward[i] = tot;
    if (tr.terminal) tr.terminal[i] = (steps > 0 && term) ? 1 : 0;
}

// ---- launchers (launch.hpp)
void launch_table_reset(hipStream_t st, const Common& k, uint64_t t) { hipLaunchKernelGGL(k_table_reset, grid_for(k.n_envs), dim3(kBlock), 0, st, k, t); }
void launch_table_domain_step(hipStream_t st, const Common& k, const int32_t* act, float* from, float* next, float* rew, uint8_t* term) {
    hipLaunchKernelGGL(k_table_domain_step, grid_for(k.n_envs), dim3(kBlock), 0, st, k, act, from, next, rew, term);
}
void launch_table_domain_reset(hipStream_t st, const Common& k, const uint8_t* mask) {
    hipLaunchKernelGGL(k_table_domain_reset, grid_for(k.n_envs), dim3(kBlock), 0, st, k, mask);
}
void launch_table_qop(hipStream_t st, const Common& k, int op, const float* states, int64_t Mn, uint64_t call, float* fout, int32_t* iout, const float* fin,
                      const int32_t* iin) {
    hipLaunchKernelGGL(k_table_qop, grid_for(Mn), dim3(kBlock), 0, st, k, op, states, Mn, call, fout, iout, fin, iin);
}
void launch_table_handle(hipStream_t st, const Common& k, const Transitions& io, uint64_t t) {
    hipLaunchKernelGGL(k_table_handle, grid_for(io.M), dim3(kBlock), 0, st, k, io.from, io.act, io.rew, io.to, io.term, io.M, t, io.td_out);
}
void launch_table_train(hipStream_t st, const Common& k, bool lds, uint64_t t, int chunk, DevStats* stats) {
    if (lds) hipLaunchKernelGGL(k_table_train_lds, grid_for(k.n_envs, kLanes), dim3(kLanes), 0, st, k, t, chunk, stats);
    else hipLaunchKernelGGL(k_table_train_mem, grid_for(k.n_envs, kLanes), dim3(kLanes), 0, st, k, t, chunk, stats);
}
void launch_table_rollout(hipStream_t st, const Common& k, int64_t step_limit, uint32_t* n_states, float* total, int64_t Mn, const TrajOut& tr,
                          const RolloutPolicy& rp) {
    hipLaunchKernelGGL(k_table_rollout, grid_for(Mn), dim3(kBlock), 0, st, k, step_limit, n_states, total, Mn, tr, rp);
}

}  // namespace rsrl
