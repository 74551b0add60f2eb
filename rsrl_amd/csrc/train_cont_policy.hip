// train_cont_policy.hip -- the continuous policies' own kernels on ContinuousMountainCar (cont_policy.hpp), Fourier orders 1-5, for every agent
// that holds the two columns: the policy side on explicit states (sample, mode, params, pdf), reset's initial sample, the mode rollout, and the
// domain's f32 transition with the action clamp (no templates: their one definition is here).
#include "launch.hpp"
#include "cont_policy.hpp"
#include "model_list.hpp"

namespace rsrl {

bool launch_cont_policy(int order, ContPolicy policy, hipStream_t st, const Common& k, const float* w, int op, const float* states, int64_t M, uint64_t t,
                        uint32_t purpose, const float* act_in, float* out0, float* out1, float* keep) {
    return for_cmc_order(order, [&](auto o) { for_cont_policy(policy, [&](auto p) {
        hipLaunchKernelGGL((k_cont_policy<decltype(o)::value, p.value>), dim3(grid_for(M)), dim3(kBlock), 0, st, k, w, op, states, M, t, purpose, act_in, out0, out1, keep);
    }); });
}

bool launch_cont_reset(int order, ContPolicy policy, hipStream_t st, const Common& k, const float* w, uint64_t t, float* action) {
    return for_cmc_order(order, [&](auto o) { for_cont_policy(policy, [&](auto p) {
        hipLaunchKernelGGL((k_cont_reset<decltype(o)::value, p.value>), dim3(grid_for(k.n_envs)), dim3(kBlock), 0, st, k, w, t, action);
    }); });
}

bool launch_cont_rollout_mode(int order, ContPolicy policy, bool map, hipStream_t st, const Common& k, const float* w, int64_t step_limit, uint32_t* n_states,
                              float* total) {
    const dim3 grid(grid_for(k.n_envs)), block(kBlock);
    if (map)        // (2 * mode - 1 is the Beta loops' mapping)
        return policy == ContPolicy::Beta && for_cmc_order(order, [&](auto o) {
            hipLaunchKernelGGL((k_cont_rollout_mode<o.value, ContPolicy::Beta, true>), grid, block, 0, st, k, w, step_limit, n_states, total);
        });
    return for_cmc_order(order, [&](auto o) { for_cont_policy(policy, [&](auto p) {
        hipLaunchKernelGGL((k_cont_rollout_mode<decltype(o)::value, p.value, false>), grid, block, 0, st, k, w, step_limit, n_states, total);
    }); });
}

// Domain::transition on the ctx's envs with f32 actions (k_domain_step's contract): explicit actions are the domain's own, taken literally;
// actions == nullptr steps on the ctx's pending ones -- through the loop's mapping 2a - 1 when map is set
__global__ __launch_bounds__(kBlock) void k_cmc_domain_step(Common c, const float* __restrict__ actions, const float* __restrict__ pending, bool map,
                                                            float* __restrict__ from_out, float* __restrict__ next_out, float* __restrict__ rew_out,
                                                            uint8_t* __restrict__ term_out) {
    using Dom = Domain<kCmc>;
    constexpr int D = Dom::D;
    const int64_t N = c.n_envs;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float s[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        s[d] = c.state[(int64_t)d * N + i];
        if (from_out) from_out[(int64_t)d * N + i] = s[d];
    }
    const float a = actions ? actions[i] : (map ? Cont<ContPolicy::Beta>::domain_action(pending[i]) : pending[i]);
    float r;
    const bool term = Dom::step(s, a, r);
#pragma unroll
    for (int d = 0; d < D; ++d) {
        c.state[(int64_t)d * N + i] = s[d];
        if (next_out) next_out[(int64_t)d * N + i] = s[d];
    }
    if (rew_out) rew_out[i] = r;
    if (term_out) term_out[i] = term ? 1 : 0;
}
// a device array of actions into the action bounds (NaN -> -1), as k_clamp_actions for the index actions
__global__ void k_cmc_clamp_actions(float* __restrict__ a, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = fminf(fmaxf(a[i], -1.0f), 1.0f);
}

void launch_cmc_domain_step(hipStream_t st, const Common& k, const float* act, const float* pending, bool map, float* from, float* next, float* rew,
                            uint8_t* term) {
    hipLaunchKernelGGL(k_cmc_domain_step, grid_for(k.n_envs), dim3(kBlock), 0, st, k, act, pending, map, from, next, rew, term);
}
void launch_cmc_clamp_actions(hipStream_t st, float* a, int64_t n) { hipLaunchKernelGGL(k_cmc_clamp_actions, grid_for(n), dim3(kBlock), 0, st, a, n); }

}  // namespace rsrl
