// wave_loop.hpp -- the frame around a wave-per-learner agent rule of the order-7 wave family's memory-sweep kernels (k_wave_lambda, k_wave_aux,
// k_wave_qsigma): driver_loop.hpp's pieces in the wave layout, and the column sweep the three rules share.
//   WaveLearner   Learner with the wave's learner index and lane: the action is wave-uniform, lane 0 stores; given(): Handler::handle's transition
//                 (Given<D> itself does not fit a kernel that is driver loop and handle in one: see given())
//   wave_hand_over      the Tally's hand-over: every thread joins the reduction, only lane 0 of a driver launch contributes
//   sample_then_restart the VALUE agents' episode end (k_wave_lambda, k_wave_aux).  k_wave_qsigma follows restart_then_sample's convention in its own
//                 text: it keeps its loop for its rate and takes the Tally and the column passes (profiles/wave_frame.md)
//   wave_sweep_column   one column of W through a step: load, the rule's update, bf16 rounding, store, <phi(s'), stored column>
//   wave_col_read / wave_col_write   the same column held in registers between two passes (k_wave_qsigma's anchor);   wave_carry
// Everything is __forceinline__ over values the kernel owns, callbacks are inlined at their call.  k_train_wave and k_train_wave_pk are NOT on
// this frame: their digests stamp profiles/isa_mix.json and profiles/pmc_traffic.json, k_train_wave runs through the assembly post-pass and
// both sit at a register count that decides their waves per SIMD -- kernels_wave.hpp therefore does not include this header.
// profiles/wave_frame.md has the tables.
#pragma once

#include "kernels_wave.hpp"
#include "driver_loop.hpp"

namespace rsrl {

template <int D>
struct WaveLearner : Learner<D> {
    using L = Learner<D>;
    using L::s; using L::a; using L::ep; using L::gid; using L::cap;
    int64_t i;             // learner (or caller-supplied transition) of this wave: wave-uniform
    int lane;

    __device__ __forceinline__ WaveLearner() : i((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)), lane(threadIdx.x & 63) {}
    // the driver loop: learner i of the ctx
    __device__ __forceinline__ void load(const Common& c) {
        L::load(c, i);
        a = __builtin_amdgcn_readfirstlane(a);
    }
    // Handler::handle: the learner stands at transition i's s and took its a (clamped; a prediction agent passes no actions)
    template <int A>
    __device__ __forceinline__ void load(const Common& c, const float* __restrict__ from, const int32_t* __restrict__ act, int64_t Mn) {
        gid = (uint32_t)(c.env_offset + i);
        cap = c.max_episode_steps;
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] = from[(int64_t)d * Mn + i];
        a = act ? clamp_action<A>(__builtin_amdgcn_readfirstlane(act[i])) : 0;
        ep = 0;
    }
    // ... and the caller's (s', r, terminal) is the step's transition: no step cap.  Read where the step reads it, not with s (Given<D> holds both
    // from the prologue on: two to three more scalar spills in three instantiations, profiles/wave_frame.md)
    __device__ __forceinline__ Transition<D> given(const float* __restrict__ rew, const float* __restrict__ to, const uint8_t* __restrict__ termf, int64_t Mn) const {
        Transition<D> tr;
#pragma unroll
        for (int d = 0; d < D; ++d) tr.ns[d] = to[(int64_t)d * Mn + i];
        tr.r = rew[i]; tr.term = termf[i] != 0; tr.trunc = false; tr.at_restart = false;
        return tr;
    }
    __device__ __forceinline__ void advance(const Transition<D>& tr, int na) { L::advance(tr, __builtin_amdgcn_readfirstlane(na)); }
    __device__ __forceinline__ void store(const Common& c) const { if (lane == 0) L::store(c, i); }
    // Handler::handle's return value
    __device__ __forceinline__ void report(float* __restrict__ td_out, float delta) const { if (lane == 0 && td_out) td_out[i] = delta; }
};

// Lives OUTSIDE `if (i < N)` like Tally::hand_over.  All 64 lanes of a wave ran the same learner: it is counted once, by lane 0, and a
// Handler::handle launch (driver == false) counts nothing.
__device__ __forceinline__ void wave_hand_over(const Tally& tally, int lane, bool counts, DevStats* __restrict__ stats) {
    Tally mine;
    if (counts && lane == 0) mine = tally;
    mine.hand_over(stats);
}

// ---- the VALUE agents' episode end (driver_loop.hpp states it in words).  The kernel has called terminal_to_restart BEFORE the step's one
// projection and has run the update; q at tr.ns is with the UPDATED weights.  Then: the sample there on BLK_STEP; a truncated episode's s' was
// a live state, so it restarts now, and the restart state is projected, evaluated and sampled again on BLK_RESET.
//   eval(ns)     project and evaluate at ns (a restart state)
//   sample(x)    -> action, from the values the kernel or eval left
template <class Dom, int D, class Eval, class Sample>
__device__ __forceinline__ void sample_then_restart(const Common& c, WaveLearner<D>& env, Tally& tally, Transition<D>& tr, float delta, uint64_t t, Eval&& eval, Sample&& sample) {
    int na;
    [[clang::always_inline]] na = sample(draw(c.seed, env.gid, t, BLK_STEP));
    tally.step(delta, tr.r);
    if (tr.ended()) tally.episode_end(env.ep, tr.trunc);
    if (tr.trunc) {
        Dom::reset(tr.ns);
        [[clang::always_inline]] eval(tr.ns);
        [[clang::always_inline]] na = sample(draw(c.seed, env.gid, t, BLK_RESET));
    }
    env.advance(tr, na);
}

// ---- one column of a learner's W (the family's layout: lane l holds k = j*512 + l*8 + v) through a step, 16 B per lane and chunk:
//   SECOND, xcol    the same column of a SECOND matrix (Z: always f32) that moves with every chunk.  Its chunk is loaded BEFORE W's, so that all of a
//                   chunk's loads are in flight together (one wave per SIMD: nothing else hides their latency; behind W's, k_wave_lambda<bf16> was 15 %
//                   slower), and stored after the update.  A second matrix that moves on a condition (k_wave_aux) stays inside the callback
//   update(j, w8, x8)   the rule on chunk j's eight values of both, in place (x8 is zeros without SECOND)
//   moves == false  a column the step does not touch (GreedyGQ): nothing is rounded or stored, it is read for the dot product only
// bf16: every STORED value of W is rounded once, after the update, with window j*8 + v of the lane's block rnd.  -> the wave total of
// <phi_n, the stored values> in dot()'s order.
__device__ __forceinline__ int64_t wave_off(int lane, int j) { return (int64_t)j * 512 + lane * 8; }

template <class WT, bool SECOND, class Update>
__device__ __forceinline__ float wave_sweep_column(WT* __restrict__ col, float* __restrict__ xcol, int lane, const float (&phi_n)[8][8], const U4& rnd, bool moves,
                                                   Update&& update) {
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float w8[8], x8[8] = {};
        if constexpr (SECOND) WaveIO<float>::load8(xcol, wave_off(lane, j), x8);
        WaveIO<WT>::load8(col, wave_off(lane, j), w8);
        if (moves) {
            [[clang::always_inline]] update(j, w8, x8);
            if constexpr (WaveIO<WT>::kBf16) {
#pragma unroll
                for (int v = 0; v < 8; ++v) w8[v] = round_bf16_sr(w8[v], sr_bits(rnd, j * 8 + v));
            }
            if constexpr (SECOND) WaveIO<float>::store8(xcol, wave_off(lane, j), x8);
            WaveIO<WT>::store8(col, wave_off(lane, j), w8);
        }
#pragma unroll
        for (int v = 0; v < 8; ++v) acc[v & 3] = fmaf(phi_n[j][v], w8[v], acc[v & 3]);
    }
    return wave_sum_uniform((acc[0] + acc[1]) + (acc[2] + acc[3]));
}

// the split form (k_wave_qsigma's anchor): the column is read ONCE and held in 64 registers per lane between its two passes
//   wave_col_read    -> <phi, column> (the wave total), the column left in w
//   wave_col_write   w += scale * phi, bf16 rounding, store -> the LANE's partial of <phi_n, the stored values>: a caller that needs the dot product takes
//                    wave_sum_uniform of it
template <class WT>
__device__ __forceinline__ float wave_col_read(const WT* __restrict__ col, int lane, const float (&phi)[8][8], float (&w)[8][8]) {
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        WaveIO<WT>::load8(col, wave_off(lane, j), w[j]);
#pragma unroll
        for (int v = 0; v < 8; ++v) acc[v & 3] = fmaf(phi[j][v], w[j][v], acc[v & 3]);
    }
    return wave_sum_uniform((acc[0] + acc[1]) + (acc[2] + acc[3]));
}
template <class WT>
__device__ __forceinline__ float wave_col_write(WT* __restrict__ col, int lane, float (&w)[8][8], float scale, const float (&phi)[8][8], const float (&phi_n)[8][8],
                                                const U4& rnd) {
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            float x = fmaf(scale, phi[j][v], w[j][v]);
            if constexpr (WaveIO<WT>::kBf16) x = round_bf16_sr(x, sr_bits(rnd, j * 8 + v));
            w[j][v] = x;
            acc[v & 3] = fmaf(phi_n[j][v], x, acc[v & 3]);
        }
        WaveIO<WT>::store8(col, wave_off(lane, j), w[j]);
    }
    return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// the step's end next to WaveLearner::advance: Q(s',.) and phi(s') of this step are Q(s,.) and phi(s) of the next
template <int A>
__device__ __forceinline__ void wave_carry(float (&q_s)[A], const float (&q_n)[A], float (&phi_s)[8][8], const float (&phi_n)[8][8]) {
#pragma unroll
    for (int b = 0; b < A; ++b) q_s[b] = q_n[b];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int v = 0; v < 8; ++v) phi_s[j][v] = phi_n[j][v];
}

}  // namespace rsrl
