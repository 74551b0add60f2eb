// fused GreedyGQ driver loop + handle for the register family
#include "launch.hpp"
#include "kernels_gq.hpp"
#include "model_list.hpp"
namespace rsrl {

#define RSRL_GQ_CASE(DM, OR, PO)                                                                        \
    if (domain == DM && order == OR && policy == PO) {                                                  \
        hipLaunchKernelGGL((k_train_gq<DM, OR, PO>), grid, block, 0, st, k, gp, t, chunk, stats);       \
        return true;                                                                                    \
    }
#define RSRL_GQ_POLICIES(DM, OR) RSRL_GQ_CASE(DM, OR, 0) RSRL_GQ_CASE(DM, OR, 1) RSRL_GQ_CASE(DM, OR, 2) RSRL_GQ_CASE(DM, OR, 3)

#define RSRL_HGQ_CASE(DM, OR)                                                                                                   \
    if (domain == DM && order == OR) {                                                                                          \
        hipLaunchKernelGGL((k_handle_gq<DM, OR>), grid, block, 0, st, k, gp, io->from, io->act, io->rew, io->to, io->term, io->M, io->td_out); \
        return true;                                                                                                            \
    }
bool launch_gq(int domain, int order, int policy, dim3 grid, dim3 block, hipStream_t st, const Common& k, const GqParams& gp, uint64_t t, int chunk,
               DevStats* stats, const Transitions* io) {
    if (io) {
        RSRL_REG_FOURIER(RSRL_HGQ_CASE)
        return false;
    }
    RSRL_REG_FOURIER(RSRL_GQ_POLICIES)
    return false;
}
// GreedyGQ on the models without a register-family kernel (tile coding, generic Fourier orders)
bool launch_gq_model(const rsrl_hip_config& cfg, dim3 grid, dim3 block, hipStream_t st, const Common& k, const GqParams& gp, const BasisGeom& g, uint64_t t,
                     int chunk, DevStats* stats, const Transitions* io) {
#define X(TYPE, BS, DM, P)                                                                                                          \
    if (model_match(cfg, BS, DM, P)) {                                                                                               \
        using M = RSRL_UNPAREN TYPE;                                                                                                 \
        if (io) hipLaunchKernelGGL((k_handle_gq_mem<M>), grid, block, 0, st, k, gp, g, io->from, io->act, io->rew, io->to, io->term, io->M, io->td_out); \
        else hipLaunchKernelGGL((k_train_gq_mem<M>), grid, block, 0, st, k, gp, g, t, chunk, stats);                                 \
        return true;                                                                                                                 \
    }
    RSRL_MEM_MODELS(X)
#undef X
    return false;
}
}  // namespace rsrl
