// train_lstd.hip -- RecursiveLSTD and iLSTD (kernels_lstd.hpp) on the register-family Fourier orders: the fused driver loop, Handler::handle, V(s),
// the driver loop's Random sample and the theta <-> f32 weights.  Kept in a translation unit of its own so that no other kernel's machine code moves.
#include "launch.hpp"
#include "kernels_lstd.hpp"
#include "model_list.hpp"

namespace rsrl {

// (the three kernels below are no templates: defined here, once, and not in kernels_lstd.hpp, which train_tdac_lstd.hip includes too)
// theta <-> f32[F] (get_weights rounds, set_weights widens exactly); set: learners first .. first + count - 1 all receive w
__global__ __launch_bounds__(256) void k_lstd_theta_get(const double* __restrict__ theta, int F, int64_t i, float* __restrict__ w) {
    const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (f < F) w[f] = (float)theta[i * F + f];
}
__global__ __launch_bounds__(256) void k_lstd_theta_set(double* __restrict__ theta, int F, int64_t first, int64_t count, const float* __restrict__ w) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= count * F) return;
    theta[first * F + idx] = (double)w[idx % F];
}

__global__ __launch_bounds__(256) void k_lstd_fill_eye(double* __restrict__ mat, int64_t n, int F, double diag) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int64_t e = idx % ((int64_t)F * F);
    mat[idx] = (e / F == e % F) ? diag : 0.0;
}

bool launch_lstd(int domain, int order, bool incremental, hipStream_t st, const Common& k, const LstdState& ls, uint64_t t, int chunk, DevStats* stats,
                 const Transitions* io) {
    return for_reg_fourier(domain, order, [&](auto m) {
        constexpr int DM = m.domain, OR = m.order;
        const dim3 grid = lstd_grid(io ? io->M : k.n_envs, LstdGroup<FourierReg<DM, OR>::F>::G), block(kBlock);
        if (io) {
            if (incremental) hipLaunchKernelGGL((k_handle_lstd<DM, OR, LSTD_INCREMENTAL>), grid, block, 0, st, ls, io->from, io->rew, io->to, io->term, io->M, io->td_out);
            else hipLaunchKernelGGL((k_handle_lstd<DM, OR, LSTD_RECURSIVE>), grid, block, 0, st, ls, io->from, io->rew, io->to, io->term, io->M, io->td_out);
        } else if (incremental) hipLaunchKernelGGL((k_train_lstd<DM, OR, LSTD_INCREMENTAL>), grid, block, 0, st, k, ls, t, chunk, stats);
        else hipLaunchKernelGGL((k_train_lstd<DM, OR, LSTD_RECURSIVE>), grid, block, 0, st, k, ls, t, chunk, stats);
    });
}

bool launch_lstd_v(int domain, int order, hipStream_t st, const double* theta, const float* states, int64_t M, float* out) {
    return for_reg_fourier(domain, order, [&](auto m) { hipLaunchKernelGGL((k_lstd_v<m.domain, m.order>), dim3(grid_for(M)), dim3(kBlock), 0, st, theta, states, M, out); });
}

void launch_lstd_sample(int domain, hipStream_t st, const Common& k, uint64_t t, uint32_t blk, int32_t* out) {
    const dim3 grid(grid_for(k.n_envs)), block(kBlock);
    if (domain == 0) hipLaunchKernelGGL(k_lstd_sample<0>, grid, block, 0, st, k, t, blk, out);
    else if (domain == 1) hipLaunchKernelGGL(k_lstd_sample<1>, grid, block, 0, st, k, t, blk, out);
    else hipLaunchKernelGGL(k_lstd_sample<2>, grid, block, 0, st, k, t, blk, out);
}

void launch_lstd_theta_get(hipStream_t st, const double* theta, int F, int64_t i, float* w) {
    hipLaunchKernelGGL(k_lstd_theta_get, dim3(grid_for(F)), dim3(kBlock), 0, st, theta, F, i, w);
}
void launch_lstd_theta_set(hipStream_t st, double* theta, int F, int64_t first, int64_t count, const float* w) {
    const int64_t n = count * F;
    hipLaunchKernelGGL(k_lstd_theta_set, dim3(grid_for(n)), dim3(kBlock), 0, st, theta, F, first, count, w);
}

void launch_lstd_fill_eye(hipStream_t st, double* mat, int64_t n, int F, double diag) {
    hipLaunchKernelGGL(k_lstd_fill_eye, dim3(grid_for(n)), dim3(kBlock), 0, st, mat, n, F, diag);
}

}  // namespace rsrl
