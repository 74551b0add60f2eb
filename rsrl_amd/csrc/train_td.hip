// prediction (TD / TDLambda) kernels of the register family
#include "launch.hpp"
#include "kernels_td.hpp"
#include "model_list.hpp"
namespace rsrl {

bool launch_td(int domain, int order, bool lambda, dim3 grid, dim3 block, hipStream_t st, const Common& k, const TdParams& tp, uint64_t t, int chunk,
               DevStats* stats, const Transitions* io) {
    if (io)
        return for_reg_fourier(domain, order, [&](auto m) {
            hipLaunchKernelGGL((k_handle_td<m.domain, m.order>), grid, block, 0, st, k, tp, lambda ? 1 : 0, io->from, io->rew, io->to, io->term, io->M, io->td_out);
        });
    return for_reg_fourier(domain, order, [&](auto m) {
        if (lambda) hipLaunchKernelGGL((k_train_td<m.domain, m.order, true>), grid, block, 0, st, k, tp, t, chunk, stats);
        else hipLaunchKernelGGL((k_train_td<m.domain, m.order, false>), grid, block, 0, st, k, tp, t, chunk, stats);
    });
}
bool launch_v_evaluate(int domain, int order, dim3 grid, dim3 block, hipStream_t st, const Common& k, const float* states, int64_t Mn, float* out) {
    return for_reg_fourier(domain, order, [&](auto m) { hipLaunchKernelGGL((k_v_evaluate<m.domain, m.order>), grid, block, 0, st, k, states, Mn, out); });
}
// TD / TDLambda on the generic Fourier orders: io != nullptr -> handle, else the driver loop
bool launch_td_model(const rsrl_hip_config& cfg, dim3 grid, dim3 block, hipStream_t st, const Common& k, const TdParams& tp, const BasisGeom& g, bool lambda,
                     uint64_t t, int chunk, DevStats* stats, const Transitions* io) {
    if (cfg.basis != RSRL_FOURIER || cfg.order < 1 || cfg.order > 7) return false;
    const Transitions x = transitions_or_none(io);
    return for_domain3(cfg.domain, [&](auto d) {
        hipLaunchKernelGGL((k_td_mem<FourierGenericModel<d.value>>), grid, block, 0, st, k, tp, g, lambda ? 1 : 0, t, chunk, stats, x.from, x.rew, x.to, x.term, x.M,
                           x.td_out);
    });
}
// V(s) of M states on the generic Fourier orders
bool launch_v_model(const rsrl_hip_config& cfg, dim3 grid, dim3 block, hipStream_t st, const Common& k, const BasisGeom& g, const float* states, int64_t M,
                    float* out) {
    if (cfg.basis != RSRL_FOURIER || cfg.order < 1 || cfg.order > 7) return false;
    return for_domain3(cfg.domain, [&](auto d) { hipLaunchKernelGGL((k_v_mem<FourierGenericModel<d.value>>), grid, block, 0, st, k, g, states, M, out); });
}
bool launch_reset_td(int domain, dim3 grid, dim3 block, hipStream_t st, const Common& k, uint64_t t) {
    return for_domain3(domain, [&](auto d) { hipLaunchKernelGGL((k_reset_td<d.value>), grid, block, 0, st, k, t); });
}
}  // namespace rsrl
