// fused train kernels, Acrobot, Fourier order 1
#include "launch.hpp"
namespace rsrl {
bool launch_train_reg_d2(int order, int algo, int policy, dim3 grid, dim3 block, hipStream_t st,
                         const Common& k, uint64_t t, int chunk, DevStats* stats, const uint64_t* t_dev) {
    return launch_train_reg_orders<2, 1>(order, algo, policy, grid, block, st, k, t, chunk, stats, t_dev);
}
}  // namespace rsrl
