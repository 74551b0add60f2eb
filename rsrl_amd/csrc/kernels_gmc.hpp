// kernels_gmc.hpp -- every-visit gradient Monte-Carlo prediction on the register family:
//   GradientMC::handle(&Trajectory)   rsrl/src/prediction/mc.rs:26-58           v_func = ScalarLFA(basis, SGD(lr)), gamma
//   Trajectory's reverse iteration    rsrl_domains/src/lib.rs:289-319            transition k: from = start | steps[k-1].0, reward = steps[k].2
// handle walks the trajectory BACKWARDS, last transition to first, and applies each update as it goes:
//     sum  = r_k + gamma * sum                                                  (sum = 0 before the last transition, bootstrap or not)
//     w   += lr * (sum - <w, phi(s_k)>) * phi(s_k)                              (w as the previous visit left it)
// Only `from` and the reward are read.  One visit is TD's terminal-transition update (kernels_td.hpp: delta = r - V(s), sb = lr * delta,
// w.axpy(sb, phi)) with r := sum: length-1 trajectories leave the bits of a TD ctx's handle with terminal = 1.
// The return runs backwards, so the rule cannot be restated online (REINFORCE's can: kernels_reinforce.hpp): the device keeps every learner's
// OPEN EPISODE, rows 0 .. episode_steps[i]-1 of rec_s f32[cap][D][N] and rec_r f32[cap][N], cap = max_episode_steps -- the layout of
// handle_batch's arguments, so that one function sweeps both.
// gmc_sweep is the ONE update both kernels below run: the driver loop, handle_batch and the trait-granular loop give the same bits.
#pragma once

#include "launch.hpp"
#include "kernels_ac.hpp"

namespace rsrl {

// learner i's rows len-1 .. 0 of states [rows][D][N] and rew [rows][N], w in registers.  ret_out [rows][N] (may be null): sum at each visit.
// Returns the f32 sum of |sum - pred| over the visits, accumulated in visit order.  A per-lane loop: lanes of a wave whose lengths differ
// serialise it (the driver loop's ragged episode ends on CartPole; profiles/gmc_rate.md)
template <class Bas, int D, int F, bool PK>
__device__ __forceinline__ float gmc_sweep(const Common& c, WBuf<1, F, PK>& w, const float* states, const float* rew, int64_t N, int64_t i, int64_t len,
                                           float* __restrict__ ret_out) {
    const float gamma = c.alg.gamma, lr = c.alg.lr;
    float sum = 0.0f, acc = 0.0f;
    // The visits form one dependent chain through w, and a visit's row comes from memory: read when it is needed, every visit waits a whole memory
    // latency with nothing else to run (65 536 learners are one wave per SIMD) -- 3.64 us per batch-step on MountainCar order 3, 1.89 with the
    // rows travelling kRows at a time, the next group's loads in flight under this group's arithmetic (profiles/gmc_rate.md; 16 rows measured the
    // same and cost 48 registers).  The visits' order and arithmetic are what they were.  Rows below 0 of the last group read row 0 (len >= 1: in
    // bounds) and are not visited
    constexpr int kRows = 8;
    float cs[kRows][D], cr[kRows];
    auto load = [&](int64_t k0, float (&bs)[kRows][D], float (&br)[kRows]) {
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const int64_t k = k0 - j > 0 ? k0 - j : 0;
#pragma unroll
            for (int d = 0; d < D; ++d) bs[j][d] = states[(k * D + d) * N + i];
            br[j] = rew[k * N + i];
        }
    };
    if (len > 0) load(len - 1, cs, cr);
    for (int64_t k0 = len - 1; k0 >= 0; k0 -= kRows) {
        float ns[kRows][D], nr[kRows];
        load(k0 - kRows, ns, nr);
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const int64_t k = k0 - j;
            if (k >= 0) {
                sum = cr[j] + gamma * sum;                           // (-ffp-contract=off: a multiply and an add, the reference's f64 restated in f32)
                PhiBuf<F, PK> phi;
                { float ph[F]; Bas::project(cs[j], ph); phi.set(ph); }
                float v[1];
                w.q(phi, v);
                const float err = sum - v[0];
                const float sb[1] = {lr * err};
                w.axpy(sb, phi);
                acc += fabsf(err);
                if (ret_out) ret_out[k * N + i] = sum;
            }
        }
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
#pragma unroll
            for (int d = 0; d < D; ++d) cs[j][d] = ns[j][d];
            cr[j] = nr[j];
        }
    }
    return acc;
}

// the driver loop (Trajectory -> handle, one episode at a time): transition, (from, r) appended to the learner's record, at the episode's end
// (terminal or max_episode_steps: no bootstrap either way) the backward sweep over its rows, then the restart and the Random sample (BLK_STEP;
// BLK_RESET after a cap, its alias) -- the environment side is k_train_td's draw for draw.  w stays in registers for the whole launch and no
// projection happens outside the sweep: Random reads no values.  The statistics' sum |delta| is the sweeps' sum |sum - pred|, booked at the
// step that ended the episode
template <int DOMAIN, int ORDER>
__global__ __launch_bounds__(kBlock) void k_train_gmc(Common c, GmcState gs, uint64_t t0, int n_steps, DevStats* __restrict__ stats) {
    using Dom = Domain<DOMAIN>;
    using Bas = FourierReg<DOMAIN, ORDER>;
    constexpr int D = Dom::D, A = Dom::A, F = Bas::F;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    Tally tally;
    if (i < N) {
        Learner<D> env;
        env.load(c, i);
        PolicyParams pol = c.pol; pol.kind = POL_RANDOM;
        const float q0[A] = {};                        // Random ignores the action values
        constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
        WBuf<1, F, PK> w;
        mat_load<1, F, PK>(w, c.W, N, i);
        const int64_t cap = env.cap;                   // (>= 1: admission)
        for (int k = 0; k < n_steps; ++k) {
            const uint64_t t = t0 + (uint64_t)k;
            Transition<D> tr = env.template step<Dom>();
            const int64_t row = (int64_t)env.ep - 1;
            if (row < cap) {                           // (an episode_steps of cap set from outside: its one step has no row, and ends the episode)
#pragma unroll
                for (int d = 0; d < D; ++d) gs.rec_s[(row * D + d) * N + i] = env.s[d];
                gs.rec_r[row * N + i] = tr.r;
            }
            float delta = 0.0f;
            if (tr.ended()) delta = gmc_sweep<Bas, D, F, PK>(c, w, gs.rec_s, gs.rec_r, N, i, (int64_t)env.ep < cap ? (int64_t)env.ep : cap, nullptr);
            restart_then_sample<Dom>(c, env, tally, tr, delta, t,
                [](const float (&)[D], bool) {},
                [&](const U4& x) { return policy_sample<A>(pol, q0, x); });
        }
        env.store(c, i);
        mat_store<1, F, PK>(w, c.W, N, i);
    }
    tally.hand_over(stats);
}

// Handler<&Trajectory>::handle for every learner: learner i walks rows len[i]-1 .. 0 of its column of the batch (states [T][D][N], rewards [T][N]).
// The ctx's own record is not touched.  ret_out [T][N] (optional): sum at each handled row, NaN in the rows past the learner's length.  A
// learner of length 0 keeps its bytes
template <int DOMAIN, int ORDER>
__global__ __launch_bounds__(kBlock) void k_handle_gmc(Common c, const float* __restrict__ states, const float* __restrict__ rew,
                                                       const uint32_t* __restrict__ len, int64_t T, float* __restrict__ ret_out) {
    using Dom = Domain<DOMAIN>;
    using Bas = FourierReg<DOMAIN, ORDER>;
    constexpr int D = Dom::D, F = Bas::F;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = c.n_envs;
    if (i >= N) return;
    const int64_t L = (int64_t)len[i] < T ? (int64_t)len[i] : T;      // (a device array of lengths is not inspected by the host: clamped here)
    if (ret_out)
        for (int64_t t = L; t < T; ++t) ret_out[t * N + i] = __builtin_nanf("");
    if (L == 0) return;
    constexpr bool PK = (RSRL_PK != 0) && (F % 4 == 0);
    WBuf<1, F, PK> w;
    mat_load<1, F, PK>(w, c.W, N, i);
    gmc_sweep<Bas, D, F, PK>(c, w, states, rew, N, i, L, ret_out);
    mat_store<1, F, PK>(w, c.W, N, i);
}

// the record as the accessors show it: rows at or past episode_steps[i] read NaN.  One thread per (row, learner), learners fastest
__global__ __launch_bounds__(256) void k_gmc_record_get(GmcState gs, const uint32_t* __restrict__ ep_step, int64_t N, int64_t cap, int D,
                                                        float* __restrict__ states, float* __restrict__ rew) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= cap * N) return;
    const int64_t row = idx / N, i = idx % N;
    const bool live = row < (int64_t)ep_step[i];
    const float nan = __builtin_nanf("");
    for (int d = 0; d < D; ++d) states[(row * D + d) * N + i] = live ? gs.rec_s[(row * D + d) * N + i] : nan;
    rew[idx] = live ? gs.rec_r[idx] : nan;
}

}  // namespace rsrl
