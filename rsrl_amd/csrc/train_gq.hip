// fused GreedyGQ driver loop + handle for the register family
#include "launch.hpp"
#include "kernels_gq.hpp"
#include "model_list.hpp"
namespace rsrl {

bool launch_gq(int domain, int order, int policy, dim3 grid, dim3 block, hipStream_t st, const Common& k, const GqParams& gp, uint64_t t, int chunk,
               DevStats* stats, const Transitions* io) {
    if (io)
        return for_reg_fourier(domain, order, [&](auto m) {
            hipLaunchKernelGGL((k_handle_gq<m.domain, m.order>), grid, block, 0, st, k, gp, io->from, io->act, io->rew, io->to, io->term, io->M, io->td_out);
        });
    bool found = false;
    for_reg_fourier(domain, order, [&](auto m) { found = for_policy(policy, [&](auto po) {
        hipLaunchKernelGGL((k_train_gq<decltype(m)::domain, decltype(m)::order, po.value>), grid, block, 0, st, k, gp, t, chunk, stats);
    }); });
    return found;
}
// GreedyGQ on the models without a register-family kernel (tile coding, generic Fourier orders)
bool launch_gq_model(const rsrl_hip_config& cfg, dim3 grid, dim3 block, hipStream_t st, const Common& k, const GqParams& gp, const BasisGeom& g, uint64_t t,
                     int chunk, DevStats* stats, const Transitions* io) {
    return for_mem_model(cfg, [&](auto tag) {
        using M = typename decltype(tag)::type;
        if (io) hipLaunchKernelGGL((k_handle_gq_mem<M>), grid, block, 0, st, k, gp, g, io->from, io->act, io->rew, io->to, io->term, io->M, io->td_out);
        else hipLaunchKernelGGL((k_train_gq_mem<M>), grid, block, 0, st, k, gp, g, t, chunk, stats);
    });
}
}  // namespace rsrl
