// driver_loop.hpp -- the frame around a thread-per-learner agent rule of the register family: what every k_train_* / k_handle_* of
// kernels_td / _gq / _lambda / _qsigma / _ac / _tdac / _reinforce does that is NOT the agent ("Adding an agent").
//   Learner      the environment side of learner i: s, a, the open episode's step count; one load, one store
//   Transition   t = env.transition(a): s', r, terminal, and the step cap's verdict
//   Tally        the launch's five statistics and their hand-over to block_stats_accumulate
//   restart_then_sample   an episode's end by the Gibbs-actor agents' convention (the value agents' is stated below, in words)
//   ping_pong    the two-buffer step loop;   Given: a caller-supplied transition (Handler::handle);   mat_load / mat_store
// Everything is __forceinline__ over values the kernel owns, and the agent's callbacks are inlined at their call (a closure that is called holds
// the matrices it captured in memory): nothing the register allocator sees as more than locals.  It still numbers registers differently, and
// four loops keep their own text, with the convention they follow named above them: k_train_gq and k_train_lambda (512 registers and scratch
// at orders 4 and 5: any frame piece moves the spills of some instantiation up), k_train_qsigma (a wave per SIMD or scalar spills on Learner;
// it takes the Tally) and k_train_td (2 % slower at order 3).  profiles/driver_frame.md has the tables.
#pragma once

#include "kernels_reg.hpp"

namespace rsrl {

template <int D>
struct Transition {
    float ns[D];           // s' -- or the restart state, once a convention below has put it there
    float r;
    bool term;             // s' is terminal
    bool trunc;            // the episode is cut by max_episode_steps (never together with term)
    bool at_restart;       // ns already is the restart state (terminal_to_restart).  Keep it: resetting twice instead is the same arithmetic, but
                           // k_train_reinforce<0,5,0> then spills six registers (profiles/driver_frame.md, "What broke a condition")
    __device__ __forceinline__ bool ended() const { return term || trunc; }
};

template <int D>
struct Learner {
    float s[D];
    int a;
    uint32_t ep;           // steps of the open episode
    uint32_t gid, cap;     // global learner id (the draws' stream), max_episode_steps (0: none)

    __device__ __forceinline__ void load(const Common& c, int64_t i) {
        const int64_t N = c.n_envs;
        gid = (uint32_t)(c.env_offset + i);
        cap = c.max_episode_steps;
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] = c.state[(int64_t)d * N + i];
        a = c.action[i];
        ep = c.ep_step[i];
    }
    __device__ __forceinline__ void store(const Common& c, int64_t i) const {
        const int64_t N = c.n_envs;
#pragma unroll
        for (int d = 0; d < D; ++d) c.state[(int64_t)d * N + i] = s[d];
        c.action[i] = a;
        c.ep_step[i] = ep;
    }
    // t = env.transition(a) and the step cap
    template <class Dom>
    __device__ __forceinline__ Transition<D> step() {
        Transition<D> tr;
#pragma unroll
        for (int d = 0; d < D; ++d) tr.ns[d] = s[d];
        tr.term = Dom::step(tr.ns, a, tr.r);
        ep += 1;
        tr.trunc = !tr.term && cap > 0 && ep >= cap;
        tr.at_restart = false;
        return tr;
    }
    // the step's end: s <- s' (or the restart state), a <- the sample
    __device__ __forceinline__ void advance(const Transition<D>& tr, int na) {
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] = tr.ns[d];
        a = na;
    }
};

// The sums run in f32 over one launch and are handed over as f64 (block_stats_accumulate adds them to the ctx's f64 totals): the statistics
// of a run are a function of how it is cut into launches, and tests hold them bit for bit.  Lives OUTSIDE `if (i < N)`: every thread of the
// block takes part in the reduction.
struct Tally {
    unsigned long long n_ep = 0, n_trunc = 0, sum_len = 0;
    float abs_delta = 0.0f, reward = 0.0f;

    __device__ __forceinline__ void step(float delta, float r) { abs_delta += fabsf(delta); reward += r; }
    __device__ __forceinline__ void episode_end(uint32_t& ep, bool truncated) {
        n_ep += 1;
        n_trunc += truncated ? 1 : 0;
        sum_len += ep;
        ep = 0;
    }
    __device__ __forceinline__ void hand_over(DevStats* __restrict__ stats) const {
        if (stats) block_stats_accumulate(stats, n_ep, n_trunc, sum_len, (double)abs_delta, (double)reward);
    }
};

// ---- an episode's end.  The reference's drivers run one episode per loop: `let mut a = policy.sample(rng, domain.emit().state())` on a fresh
// domain, then transition / handle / sample until the transition is terminal or the step limit is reached.  Vectorised, a learner's next
// episode begins inside the step that ended the last one.  Either way tr.ns ends as the state the next step starts from.  BLK_RESET is
// BLK_STEP's alias (device_core.hpp): the sample after a restart is the step's one behaviour sample.

// A terminal transition never reads s' (every value agent's target drops it), so s' is replaced by the restart state BEFORE it is projected: the
// step's one projection is then the next episode's phi(s).  The value agents' first move; k_train_ac uses it with restart_then_sample.
template <class Dom, int D>
__device__ __forceinline__ void terminal_to_restart(Transition<D>& tr) {
    if (tr.term) Dom::reset(tr.ns);
    tr.at_restart = tr.term;
}

// VALUE agents (examples/q_learning.rs:47-51, then :37-38 for the next episode) have no function here: k_train_td, k_train_gq and k_train_lambda
// write their convention out, for the reasons given above each.  It is: terminal_to_restart, ONE projection of ns, the update, the values at ns
// with the UPDATED weights and the sample there on BLK_STEP; a truncated episode's s' was a live state, so it restarts after the update, and the
// restart state is projected, evaluated and sampled again on BLK_RESET.

// GIBBS-ACTOR agents (examples/a2c.rs:55-67, tdac.rs): ONE sample per step, after the restart -- on BLK_RESET after a cut, else on BLK_STEP.
// An agent that reads s' of a terminal transition (tdac.rs's TDCritic: V of the terminal state itself) projects tr.ns as it is and leaves
// the restart to this function; one that does not calls terminal_to_restart first.
// Used by k_train_ac, k_train_tdac and k_train_reinforce; k_train_qsigma follows it in its own text.
//   eval(ns, ended)   project and evaluate at ns; ended: ns is a restart state, not the s' the agent has seen
//   sample(x)         -> action
template <class Dom, int D, class Eval, class Sample>
__device__ __forceinline__ void restart_then_sample(const Common& c, Learner<D>& env, Tally& tally, Transition<D>& tr, float delta, uint64_t t, Eval&& eval, Sample&& sample) {
    if (tr.ended()) {
        tally.episode_end(env.ep, tr.trunc);
        if (!tr.at_restart) Dom::reset(tr.ns);
    }
    const uint32_t blk = tr.trunc ? BLK_RESET : BLK_STEP;
    [[clang::always_inline]] eval(tr.ns, tr.ended());
    int na;
    [[clang::always_inline]] na = sample(draw(c.seed, env.gid, t, blk));
    tally.step(delta, tr.r);
    env.advance(tr, na);
}

// ---- n_steps batch-steps from t0 over two feature buffers that swap roles: phi(s') of one step is phi(s) of the next, without a copy
template <class Phi, class Step>
__device__ __forceinline__ void ping_pong(Phi& phi_a, Phi& phi_b, uint64_t t0, int n_steps, Step&& one_step) {
    int k = 0;
    for (; k + 1 < n_steps; k += 2) {
        one_step(phi_a, phi_b, t0 + (uint64_t)k);
        one_step(phi_b, phi_a, t0 + (uint64_t)k + 1);
    }
    if (k < n_steps) one_step(phi_a, phi_b, t0 + (uint64_t)k);
}

// ---- Handler<&Transition>::handle: transition i of a caller-supplied batch of Mn ([D][Mn] states; a prediction agent has no actions)
template <int D>
struct Given {
    float s[D], ns[D];
    int a;
    float r;
    bool term;
    __device__ __forceinline__ void load(const float* __restrict__ from, const float* __restrict__ rew, const float* __restrict__ to,
                                         const uint8_t* __restrict__ termf, int64_t Mn, int64_t i) {
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] = from[(int64_t)d * Mn + i];
#pragma unroll
        for (int d = 0; d < D; ++d) ns[d] = to[(int64_t)d * Mn + i];
        a = 0;
        r = rew[i];
        term = termf[i] != 0;
    }
    template <int A>
    __device__ __forceinline__ void load(const float* __restrict__ from, const int32_t* __restrict__ act, const float* __restrict__ rew,
                                         const float* __restrict__ to, const uint8_t* __restrict__ termf, int64_t Mn, int64_t i) {
        load(from, rew, to, termf, Mn, i);
        a = clamp_action<A>(act[i]);
    }
};

// ---- a learner's A x F matrix between memory ([A][F][N], learner fastest) and registers.  The learner's base address goes through an empty asm
// at every call: the element addresses are then formed next to their access from one VGPR pair and a uniform offset -- otherwise the load's
// addresses are kept for the store and take two VGPRs per weight (the spills of a 2 x 108-weight learner)
template <int A, int F, bool PK>
__device__ __forceinline__ void mat_load(WBuf<A, F, PK>& w, const float* __restrict__ W, int64_t N, int64_t i) {
    const float* p = W + i;
    asm("" : "+v"(p));
#pragma unroll
    for (int b = 0; b < A; ++b)
#pragma unroll
        for (int f = 0; f < F; ++f) w.put(b, f, p[(int64_t)(b * F + f) * N]);
}
template <int A, int F, bool PK>
__device__ __forceinline__ void mat_store(const WBuf<A, F, PK>& w, float* __restrict__ W, int64_t N, int64_t i) {
    float* p = W + i;
    asm("" : "+v"(p));
#pragma unroll
    for (int b = 0; b < A; ++b)
#pragma unroll
        for (int f = 0; f < F; ++f) p[(int64_t)(b * F + f) * N] = w.get(b, f);
}

}  // namespace rsrl
