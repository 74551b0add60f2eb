// train_gtd.hip -- GTD2 and TDC (kernels_gtd.hpp) on the register-family Fourier orders: the fused driver loop and Handler::handle.  The value
// side of the other entry points (q_evaluate, get / set_weights) and reset's Random sample run TD's kernels on the one-column W (theta); the
// second column w is the ctx's auxiliary matrix.  Kept in a translation unit of its own so that no other kernel's machine code moves.
#include "launch.hpp"
#include "kernels_gtd.hpp"
#include "model_list.hpp"

namespace rsrl {

bool launch_gtd(int domain, int order, bool tdc, dim3 grid, dim3 block, hipStream_t st, const Common& k, const GtdState& gs, uint64_t t, int chunk,
                DevStats* stats, const Transitions* io) {
    return for_reg_fourier(domain, order, [&](auto m) {
        if (io) hipLaunchKernelGGL((k_handle_gtd<m.domain, m.order>), grid, block, 0, st, k, gs, tdc ? 1 : 0, io->from, io->rew, io->to, io->term, io->M, io->td_out);
        else if (tdc) hipLaunchKernelGGL((k_train_gtd<m.domain, m.order, true>), grid, block, 0, st, k, gs, t, chunk, stats);
        else hipLaunchKernelGGL((k_train_gtd<m.domain, m.order, false>), grid, block, 0, st, k, gs, t, chunk, stats);
    });
}

}  // namespace rsrl
