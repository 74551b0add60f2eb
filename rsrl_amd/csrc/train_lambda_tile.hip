// eligibility-trace control on tile coding, per-learner tables: one block per learner (kernels_lambda_tile.hpp)
#include "launch.hpp"
#include "kernels_lambda_tile.hpp"
#include "kernels_td_tile.hpp"
#include "model_list.hpp"
namespace rsrl {

// TD / TDLambda on tile coding: io != nullptr -> handle, else the driver loop
bool launch_td_tile(int domain, int n_tilings, bool lambda, hipStream_t st, const Common& k, const BasisGeom& g, const TdParams& tp, uint64_t t, int chunk,
                    DevStats* stats, const Transitions* io) {
    const Transitions x = transitions_or_none(io);
    const int64_t n_blocks = io ? io->M : k.n_envs;
    return for_tile(domain, n_tilings, [&](auto c) {
        hipLaunchKernelGGL((k_td_tile<c.domain, c.n_tilings, 256>), dim3((unsigned)n_blocks), dim3(256), 0, st, k, g, tp, lambda ? 1 : 0, t, chunk, stats, x.from, x.rew,
                           x.to, x.term, x.M, x.td_out);
    });
}
// V(s) of M states into out
bool launch_v_tile(int domain, int n_tilings, hipStream_t st, const Common& k, const BasisGeom& g, const float* states, int64_t M, float* out) {
    return for_tile(domain, n_tilings, [&](auto c) { hipLaunchKernelGGL((k_v_tile<c.domain, c.n_tilings>), dim3(grid_for(M)), dim3(kBlock), 0, st, k, g, states, M, out); });
}

bool launch_lambda_tile(int domain, int n_tilings, hipStream_t st, const Common& k, const BasisGeom& g, const LambdaParams& lp, uint64_t t, int chunk,
                        DevStats* stats, const Transitions* io) {
    const Transitions x = transitions_or_none(io);
    const int64_t n_blocks = io ? io->M : k.n_envs;
    return for_tile(domain, n_tilings, [&](auto c) {
        hipLaunchKernelGGL((k_lambda_tile<c.domain, c.n_tilings, 256>), dim3((unsigned)n_blocks), dim3(256), 0, st, k, g, lp, t, chunk, stats, x.from, x.act, x.rew,
                           x.to, x.term, x.M, x.td_out);
    });
}
}  // namespace rsrl
