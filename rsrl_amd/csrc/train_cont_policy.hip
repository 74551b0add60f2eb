// train_cont_policy.hip -- the continuous policies' own kernels on ContinuousMountainCar (cont_policy.hpp), Fourier orders 1-5, for every agent
// that holds the two columns: the policy side on explicit states (sample, mode, params, pdf), reset's initial sample, the mode rollout, and the
// domain's f32 transition with the action clamp (no templates: their one definition is here).
#include "launch.hpp"
#include "cont_policy.hpp"
#include "model_list.hpp"

namespace rsrl {

static inline dim3 grid1(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }
// X(OR, P) for `order` and `policy` given as values; X is the using function's own, defined after this and undefined by it
#define RSRL_CONT_CASE(OR) if (order == OR) { if (policy == ContPolicy::Gaussian) { X(OR, ContPolicy::Gaussian) } else { X(OR, ContPolicy::Beta) } return true; }

bool launch_cont_policy(int order, ContPolicy policy, hipStream_t st, const Common& k, const float* w, int op, const float* states, int64_t M, uint64_t t,
                        uint32_t purpose, const float* act_in, float* out0, float* out1, float* keep) {
#define X(OR, P) hipLaunchKernelGGL((k_cont_policy<OR, P>), grid1(M), dim3(kBlock), 0, st, k, w, op, states, M, t, purpose, act_in, out0, out1, keep);
    RSRL_CMC_ORDERS(RSRL_CONT_CASE)
#undef X
    return false;
}

bool launch_cont_reset(int order, ContPolicy policy, hipStream_t st, const Common& k, const float* w, uint64_t t, float* action) {
#define X(OR, P) hipLaunchKernelGGL((k_cont_reset<OR, P>), grid1(k.n_envs), dim3(kBlock), 0, st, k, w, t, action);
    RSRL_CMC_ORDERS(RSRL_CONT_CASE)
#undef X
    return false;
}

bool launch_cont_rollout_mode(int order, ContPolicy policy, bool map, hipStream_t st, const Common& k, const float* w, int64_t step_limit, uint32_t* n_states,
                              float* total) {
    if (map) {      // (2 * mode - 1 is the Beta loops' mapping)
#define X(OR) if (order == OR && policy == ContPolicy::Beta) { hipLaunchKernelGGL((k_cont_rollout_mode<OR, ContPolicy::Beta, true>), grid1(k.n_envs), dim3(kBlock), 0, st, k, w, step_limit, n_states, total); return true; }
        RSRL_CMC_ORDERS(X)
#undef X
        return false;
    }
#define X(OR, P) hipLaunchKernelGGL((k_cont_rollout_mode<OR, P, false>), grid1(k.n_envs), dim3(kBlock), 0, st, k, w, step_limit, n_states, total);
    RSRL_CMC_ORDERS(RSRL_CONT_CASE)
#undef X
    return false;
}

#undef RSRL_CONT_CASE

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
    hipLaunchKernelGGL(k_cmc_domain_step, grid1(k.n_envs), dim3(kBlock), 0, st, k, act, pending, map, from, next, rew, term);
}
void launch_cmc_clamp_actions(hipStream_t st, float* a, int64_t n) { hipLaunchKernelGGL(k_cmc_clamp_actions, grid1(n), dim3(kBlock), 0, st, a, n); }

}  // namespace rsrl
