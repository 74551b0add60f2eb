// prediction (TD / TDLambda) kernels of the register family
#include "launch.hpp"
#include "kernels_td.hpp"
#include "model_list.hpp"
namespace rsrl {

#define RSRL_TD_CASE(DM, OR)                                                                                        \
    if (domain == DM && order == OR) {                                                                              \
        if (lambda) hipLaunchKernelGGL((k_train_td<DM, OR, true>), grid, block, 0, st, k, tp, t, chunk, stats);     \
        else hipLaunchKernelGGL((k_train_td<DM, OR, false>), grid, block, 0, st, k, tp, t, chunk, stats);           \
        return true;                                                                                                \
    }
#define RSRL_HTD_CASE(DM, OR)                                                                                                 \
    if (domain == DM && order == OR) {                                                                                        \
        hipLaunchKernelGGL((k_handle_td<DM, OR>), grid, block, 0, st, k, tp, lambda ? 1 : 0, io->from, io->rew, io->to, io->term, io->M, io->td_out); \
        return true;                                                                                                          \
    }
bool launch_td(int domain, int order, bool lambda, dim3 grid, dim3 block, hipStream_t st, const Common& k, const TdParams& tp, uint64_t t, int chunk,
               DevStats* stats, const Transitions* io) {
    if (io) {
        RSRL_REG_FOURIER(RSRL_HTD_CASE)
        return false;
    }
    RSRL_REG_FOURIER(RSRL_TD_CASE)
    return false;
}
#define RSRL_VEV_CASE(DM, OR)                                                                            \
    if (domain == DM && order == OR) {                                                                   \
        hipLaunchKernelGGL((k_v_evaluate<DM, OR>), grid, block, 0, st, k, states, Mn, out);              \
        return true;                                                                                     \
    }
bool launch_v_evaluate(int domain, int order, dim3 grid, dim3 block, hipStream_t st, const Common& k, const float* states, int64_t Mn, float* out) {
    RSRL_REG_FOURIER(RSRL_VEV_CASE)
    return false;
}
// TD / TDLambda on the generic Fourier orders: io != nullptr -> handle, else the driver loop
bool launch_td_model(const rsrl_hip_config& cfg, dim3 grid, dim3 block, hipStream_t st, const Common& k, const TdParams& tp, const BasisGeom& g, bool lambda,
                     uint64_t t, int chunk, DevStats* stats, const Transitions* io) {
    if (cfg.basis != RSRL_FOURIER || cfg.order < 1 || cfg.order > 7) return false;
    const Transitions x = transitions_or_none(io);
#define RSRL_TDM_CASE(DM)                                                                                                                            \
    if (cfg.domain == DM) {                                                                                                                          \
        hipLaunchKernelGGL((k_td_mem<FourierGenericModel<DM>>), grid, block, 0, st, k, tp, g, lambda ? 1 : 0, t, chunk, stats, x.from, x.rew, x.to, x.term, x.M, \
                           x.td_out);                                                                                                                \
        return true;                                                                                                                                 \
    }
    RSRL_TDM_CASE(0) RSRL_TDM_CASE(1) RSRL_TDM_CASE(2)
    return false;
}
// V(s) of M states on the generic Fourier orders
bool launch_v_model(const rsrl_hip_config& cfg, dim3 grid, dim3 block, hipStream_t st, const Common& k, const BasisGeom& g, const float* states, int64_t M,
                    float* out) {
    if (cfg.basis != RSRL_FOURIER || cfg.order < 1 || cfg.order > 7) return false;
#define RSRL_VM_CASE(DM)                                                                                                 \
    if (cfg.domain == DM) {                                                                                              \
        hipLaunchKernelGGL((k_v_mem<FourierGenericModel<DM>>), grid, block, 0, st, k, g, states, M, out);                 \
        return true;                                                                                                     \
    }
    RSRL_VM_CASE(0) RSRL_VM_CASE(1) RSRL_VM_CASE(2)
    return false;
}
bool launch_reset_td(int domain, dim3 grid, dim3 block, hipStream_t st, const Common& k, uint64_t t) {
    if (domain == 0) { hipLaunchKernelGGL((k_reset_td<0>), grid, block, 0, st, k, t); return true; }
    if (domain == 1) { hipLaunchKernelGGL((k_reset_td<1>), grid, block, 0, st, k, t); return true; }
    if (domain == 2) { hipLaunchKernelGGL((k_reset_td<2>), grid, block, 0, st, k, t); return true; }
    return false;
}
}  // namespace rsrl
