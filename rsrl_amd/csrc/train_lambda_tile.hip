// eligibility-trace control on tile coding, per-learner tables: one block per learner (kernels_lambda_tile.hpp)
#include "launch.hpp"
#include "kernels_lambda_tile.hpp"
#include "kernels_td_tile.hpp"
namespace rsrl {

#define RSRL_TT_CASE(DM, TT)                                                                                                              \
    if (domain == DM && n_tilings == TT) {                                                                                                \
        hipLaunchKernelGGL((k_td_tile<DM, TT, 256>), dim3((unsigned)n_blocks), dim3(256), 0, st, k, g, tp, lambda ? 1 : 0, t, chunk, stats, x.from, x.rew, \
                           x.to, x.term, x.M, x.td_out);                                                                                  \
        return true;                                                                                                                      \
    }
// TD / TDLambda on tile coding: io != nullptr -> handle, else the driver loop
bool launch_td_tile(int domain, int n_tilings, bool lambda, hipStream_t st, const Common& k, const BasisGeom& g, const TdParams& tp, uint64_t t, int chunk,
                    DevStats* stats, const Transitions* io) {
    const Transitions x = transitions_or_none(io);
    const int64_t n_blocks = io ? io->M : k.n_envs;
    RSRL_TT_CASE(0, 4) RSRL_TT_CASE(0, 8) RSRL_TT_CASE(0, 16)
    RSRL_TT_CASE(1, 4) RSRL_TT_CASE(1, 8) RSRL_TT_CASE(1, 16)
    RSRL_TT_CASE(2, 4) RSRL_TT_CASE(2, 8) RSRL_TT_CASE(2, 16)
    return false;
}
#define RSRL_VT_CASE(DM, TT)                                                                                                                  \
    if (domain == DM && n_tilings == TT) {                                                                                                    \
        hipLaunchKernelGGL((k_v_tile<DM, TT>), dim3((unsigned)((M + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, k, g, states, M, out);       \
        return true;                                                                                                                          \
    }
// V(s) of M states into out
bool launch_v_tile(int domain, int n_tilings, hipStream_t st, const Common& k, const BasisGeom& g, const float* states, int64_t M, float* out) {
    RSRL_VT_CASE(0, 4) RSRL_VT_CASE(0, 8) RSRL_VT_CASE(0, 16)
    RSRL_VT_CASE(1, 4) RSRL_VT_CASE(1, 8) RSRL_VT_CASE(1, 16)
    RSRL_VT_CASE(2, 4) RSRL_VT_CASE(2, 8) RSRL_VT_CASE(2, 16)
    return false;
}

#define RSRL_LT_CASE(DM, TT)                                                                                                          \
    if (domain == DM && n_tilings == TT) {                                                                                            \
        hipLaunchKernelGGL((k_lambda_tile<DM, TT, 256>), dim3((unsigned)n_blocks), dim3(256), 0, st, k, g, lp, t, chunk, stats, x.from, x.act, x.rew, \
                           x.to, x.term, x.M, x.td_out);                                                                              \
        return true;                                                                                                                  \
    }
bool launch_lambda_tile(int domain, int n_tilings, hipStream_t st, const Common& k, const BasisGeom& g, const LambdaParams& lp, uint64_t t, int chunk,
                        DevStats* stats, const Transitions* io) {
    const Transitions x = transitions_or_none(io);
    const int64_t n_blocks = io ? io->M : k.n_envs;
    RSRL_LT_CASE(0, 4) RSRL_LT_CASE(0, 8) RSRL_LT_CASE(0, 16)
    RSRL_LT_CASE(1, 4) RSRL_LT_CASE(1, 8) RSRL_LT_CASE(1, 16)
    RSRL_LT_CASE(2, 4) RSRL_LT_CASE(2, 8) RSRL_LT_CASE(2, 16)
    return false;
}
}  // namespace rsrl
