// kernels_table.hpp -- CliffWalk (rsrl_domains/src/cliff_walk.rs over grid_world.rs; Domain<5>, device_core.hpp) with the tabular function approximator
// (rsrl/src/fa/tabular/dense.rs, Table<Array2<f64>>): no features and no dot products -- Q(s,.) is a row of a 60 x 4 table, indexed by a value known
// only at run time, and the update adds the error to ONE entry (dense.rs:79-83, :118-127).  Only the kernels of train_table.hip include this header
// (their own translation unit: no other kernel's code moves).
//
// A learner's table lives in the ctx's weight buffer in the Fourier families' layout, W f32[A][F][N] with F = 60 rows, learner fastest: entry
// e = a * 60 + row of learner i at W[e * N + i].  The weight accessors, the checkpoint and the checksum read that layout as it is, and a wave's access to
// one entry of its 64 learners is one contiguous 256-byte line -- which is what the staging copy of k_table_train_lds wants ("CliffWalk").
#pragma once

#include "driver_loop.hpp"
#include "models.hpp"

namespace rsrl {
namespace table {

using Dom = Domain<5>;
constexpr int D = Dom::D, A = Dom::A, F = Dom::kCells, kEntries = A * F;      // 240 entries, 960 B per learner
constexpr int kLanes = 64;                                                    // learners per block of the two driver loops: one wave

// ---- the accessors: where a learner's 240 entries are.  `stride` apart, from the learner's own base: N in memory, 64 in the block's LDS image
// ([entry][lane]: lane l of a 32-lane half reads bank l whatever the row -- ds_read_b32 / ds_write_b32 bank by (address / 4) mod 32 per half)
template <int64_t STRIDE>
struct Acc {
    float* __restrict__ p;      // entry 0 of this learner
    int64_t n;                  // (STRIDE == 0: the run-time stride)
    __device__ __forceinline__ int64_t stride() const { return STRIDE ? STRIDE : n; }
    // Q(s, .) = the row (dense.rs:79-83)
    __device__ __forceinline__ void row(int r, float (&q)[A]) const {
        static_for<0, A>([&](auto B) { constexpr int b = B; q[b] = p[(int64_t)(b * F + r) * stride()]; });
    }
    // Q(s, a): one entry
    __device__ __forceinline__ float at(int r, int a) const { return p[(int64_t)(a * F + r) * stride()]; }
    // Q[row, a] += error (dense.rs:118-127)
    __device__ __forceinline__ void add(int r, int a, float e) const { p[(int64_t)(a * F + r) * stride()] += e; }
};
using MemAcc = Acc<0>;
using LdsAcc = Acc<kLanes>;

// ---- Handler<&Transition>::handle of the four one-step agents on rows: the TD error from Q(s,.) and Q(s',.), then the update of the one entry.
// Table has no optimiser: the reference's agents step with size 1; config.lr scales the error (lr = 1: the literal rule).
// The rules are td_dispatch's (device_core.hpp: td_error_pal as it is; td_error's three bootstraps and its two differences operation for operation),
// except that the two values td_error SELECTS out of a row by a run-time index -- Q(s, a), and SARSA's Q(s', a') -- are GATHERED from the table, which
// is what a table is for.  The same values, hence the same bits; and the select chains, which the compiler turns into an indexed load from a
// stack copy of the row (48 B of scratch in the LDS loop, whose block has no LDS left to promote it to), are gone.
template <class Acc_>
__device__ __forceinline__ float table_handle(const Common& c, const Acc_& acc, int rs, int a, int rn, float r, bool term, uint32_t gid, uint64_t t) {
    const AlgoParams& ap = c.alg;
    float q_n[A], delta, e;
    acc.row(rn, q_n);
    if (ap.kind == ALG_PAL) {
        float q_s[A];
        acc.row(rs, q_s);
        delta = td_error_pal<A>(ap, q_s, q_n, a, r, term, e);
    } else {
        const float qsa = acc.at(rs, a);
        float boot;
        if (ap.kind == ALG_QLEARNING) {
            find_max<A>(q_n, boot);
        } else if (ap.kind == ALG_SARSA) {
            boot = acc.at(rn, policy_sample<A>(c.apol, q_n, draw(c.seed, gid, t, BLK_INNER)));      // the agent's own draw (sarsa.rs:61)
        } else {
            float p[A]; policy_probs<A>(c.apol, q_n, p);
            boot = 0.0f;
#pragma unroll
            for (int i = 0; i < A; ++i) boot = boot + q_n[i] * p[i];                                 // fold(0.0, acc + q*p)
        }
        const float d_term = r - qsa, d_boot = r + ap.gamma * boot - qsa;
        delta = term ? d_term : d_boot;
        e = (ap.kind == ALG_ESARSA) ? ap.alpha * delta : delta;
    }
    acc.add(rs, a, ap.lr * e);
    return delta;
}

// the environment side of a learner as the loops carry it: the cell as integers
struct Learner {
    int x, y, a;
    uint32_t ep, gid, cap;
    __device__ __forceinline__ void load(const Common& c, int64_t i) {
        const int64_t N = c.n_envs;
        gid = (uint32_t)(c.env_offset + i);
        cap = c.max_episode_steps;
        x = Dom::cell(c.state[i], Dom::kWidth); y = Dom::cell(c.state[N + i], Dom::kHeight);
        a = clamp_action<A>(c.action[i]);
        ep = c.ep_step[i];
    }
    __device__ __forceinline__ void store(const Common& c, int64_t i) const {
        const int64_t N = c.n_envs;
        c.state[i] = (float)x; c.state[N + i] = (float)y;
        c.action[i] = a;
        c.ep_step[i] = ep;
    }
};

// ---- THE step body: one batch-step of one learner, k_train_mem's order line for line (models.hpp) -- the transition, a terminal s' replaced by the
// start cell before it is read, the agent's rule against the table as it stands, the behaviour sample at s' from the UPDATED table on BLK_STEP, and
// after a cut the restart and its sample on BLK_RESET
template <class Acc_>
__device__ __forceinline__ void table_step(const Common& c, const Acc_& acc, Learner& L, Tally& tally, uint64_t t) {
    int nx = L.x, ny = L.y;
    float r;
    const bool term = Dom::step_cell(nx, ny, L.a, r);
    L.ep += 1;
    const bool trunc = !term && L.cap > 0 && L.ep >= L.cap;
    if (term) { nx = 0; ny = 0; }
    const float delta = table_handle(c, acc, Dom::row(L.x, L.y), L.a, Dom::row(nx, ny), r, term, L.gid, t);
    float q_n[A];
    acc.row(Dom::row(nx, ny), q_n);                                   // UPDATED table
    int na = policy_sample<A>(c.pol, q_n, draw(c.seed, L.gid, t, BLK_STEP));
    tally.step(delta, r);
    if (term) tally.episode_end(L.ep, false);
    if (trunc) {
        tally.episode_end(L.ep, true);
        nx = 0; ny = 0;
        acc.row(Dom::row(0, 0), q_n);
        na = policy_sample<A>(c.pol, q_n, draw(c.seed, L.gid, t, BLK_RESET));
    }
    L.x = nx; L.y = ny; L.a = na;
}

}  // namespace table
}  // namespace rsrl
