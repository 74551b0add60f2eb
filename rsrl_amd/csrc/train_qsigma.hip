// QSigma kernels (register-family Fourier bases, weights in memory)
#include "launch.hpp"
#include "kernels_qsigma.hpp"
#include "model_list.hpp"
namespace rsrl {
bool launch_qsigma(int domain, int order, dim3 grid, dim3 block, hipStream_t st, const Common& k, const QsParams& qp, const BasisGeom& g, uint64_t t,
                   int chunk, DevStats* stats, const Transitions* io) {
    return for_reg_fourier(domain, order, [&](auto m) {
        using M = typename decltype(m)::type;
        if (io) hipLaunchKernelGGL((k_handle_qsigma<M>), grid, block, 0, st, k, qp, g, io->from, io->act, io->rew, io->to, io->term, io->M, t, io->td_out);
        else hipLaunchKernelGGL((k_train_qsigma<M>), grid, block, 0, st, k, qp, g, t, chunk, stats);
    });
}
// ... and on every other model (tile coding with per-learner tables, the generic Fourier orders): the agent is generic over the
// approximator (q_sigma.rs:80-105), and so are k_train_qsigma / k_handle_qsigma
bool launch_qsigma_model(const rsrl_hip_config& cfg, dim3 grid, dim3 block, hipStream_t st, const Common& k, const QsParams& qp, const BasisGeom& g, uint64_t t,
                         int chunk, DevStats* stats, const Transitions* io) {
    return for_mem_model(cfg, [&](auto tag) {
        using M = typename decltype(tag)::type;
        if (io) hipLaunchKernelGGL((k_handle_qsigma<M>), grid, block, 0, st, k, qp, g, io->from, io->act, io->rew, io->to, io->term, io->M, t, io->td_out);
        else hipLaunchKernelGGL((k_train_qsigma<M>), grid, block, 0, st, k, qp, g, t, chunk, stats);
    });
}
}  // namespace rsrl
