// kernels_wave_lambda.hpp -- eligibility-trace control (SARSALambda / QLambda, rsrl/src/control/td/sarsa_lambda.rs:53-98,
// q_lambda.rs:56-99; trace rules rsrl/src/traces.rs:188-240) on the WAVE family: Fourier order 7 on a 4-D state space,
// F = 4096 features, one wavefront per learner (kernels_wave.hpp); weights f32, or (round 6) bf16 with stochastic rounding and the trace in f32.
//
// Every entry of W moves at every step (W += alpha * residual * Z), and W + Z are 96 KiB per learner: neither the registers of
// a wave (k_train_wave keeps W alone there, 192 of them) nor its share of the LDS hold both, so this family member is a memory
// sweep like the traces on tile coding (kernels_lambda_tile.hpp): per learner-step
//     Q(s', .) with the pre-update weights       W read once (48 KiB)
//     one fused sweep over (Z, W)                z = rule(rate * z + [b == a] * phi(s));  w += scale * z;  Q_post(s', b) += phi(s') * w
//                                                Z and W read and written once each (192 KiB), 16 B per lane, coalesced
// with the layout of the wave family (f32[N][A][F], internal index k = j*512 + lane*8 + v) for both matrices.  phi(s) and phi(s')
// live in registers (64 + 64 per lane).  Q(s', .) with the UPDATED weights -- what the behaviour policy samples from, and the
// next step's Q(s, .) -- falls out of the sweep: every column's lane partial runs over (j, v) in dot()'s order, four chains,
// then the wave total.  Element by element the operations are project() / dot() / trace_merge() / fmaf of the granular kernels:
// bit-identical to the oracle's wave-order loop (orc_run_train_wave with a lambda agent).
// bf16 weights (WT = bf16_t; the storage format of BASELINE configs[4], here for the trace agents): W is read as bf16, the arithmetic and the
// trace stay f32, and EVERY entry of W -- all of them move -- is rounded back by stochastic rounding with the lane's Philox block 16 + 64 * b + lane
// of the step (column b; the 16-bit window of element e = j * 8 + v as in k_train_wave), so that Q(s', .) of the sweep is the dot product over
// the stored values.  W traffic halves: 4 A F + 2 x 2 A F bytes per learner-step instead of 4 x 4 A F.
#pragma once

#include "wave_loop.hpp"
#include "kernels_lambda.hpp"

namespace rsrl {

// from == nullptr: the driver loop, n_steps batch-steps of the wave's learner.  Otherwise Handler::handle on ONE caller-supplied
// transition per learner (Mn of them).
template <int DOMAIN, class WT = float>
__global__ __launch_bounds__(kBlock) void k_wave_lambda(Common c, LambdaParams lp, WT* __restrict__ Wbase, uint64_t t0, int n_steps,
                                                        DevStats* __restrict__ stats, const float* __restrict__ from, const int32_t* __restrict__ act,
                                                        const float* __restrict__ rew, const float* __restrict__ to, const uint8_t* __restrict__ termf,
                                                        int64_t Mn, float* __restrict__ td_out) {
    using WF = WaveFourier<DOMAIN>;
    using Dom = Domain<DOMAIN>;
    using IO = WaveIO<WT>;
    constexpr int D = WF::D, A = WF::A, F = WF::F;
    const bool driver = from == nullptr;
    WaveLearner<D> env;
    Tally tally;
    if (env.i < (driver ? c.n_envs : Mn)) {
        const int lane = env.lane;
        const bool sarsa = c.alg.kind == ALG_SARSA_LAMBDA;
        AlgoParams alg = c.alg; alg.kind = sarsa ? ALG_SARSA : ALG_QLEARNING;      // the TD target formula
        WT* __restrict__ Wi = Wbase + env.i * (int64_t)(A * F);
        float* __restrict__ Zi = lp.Z + env.i * (int64_t)(A * F);
        if (driver) env.load(c); else env.template load<A>(c, from, act, Mn);
        float phi_s[8][8], q_s[A];
        WF::project(env.s, lane, phi_s);
        WF::template q_from_mem<WT>(Wi, lane, phi_s, q_s);
        // the per-learner epsilon schedule (Common::eps, examples/sarsa_lambda.rs:68): the learner is the wave's, its epsilon wave-uniform
        PolicyParams pol = c.pol;
        learner_eps_load(c, env.i, pol);
        for (int k = 0; k < (driver ? n_steps : 1); ++k) {
            const uint64_t t = t0 + (uint64_t)k;
            Transition<D> tr = driver ? env.template step<Dom>() : env.given(rew, to, termf, Mn);
            if (driver) terminal_to_restart<Dom>(tr);                          // (Handler::handle projects the caller's s' as it is)
            const int a = env.a;
            const bool term = tr.term;
            float phi_n[8][8], q_n[A];
            WF::project(tr.ns, lane, phi_n);
            WF::template q_from_mem<WT>(Wi, lane, phi_n, q_n);              // PRE-update weights
            // ---- trace decay rate: Q(lambda) cuts the trace unless the action taken was argmax_first of Q(s,.)   q_lambda.rs:62-66
            float rate_eff = lp.rate;
            if (!sarsa) rate_eff = (a != argmax_first<A>(q_s)) ? 0.0f : lp.rate;
            U4 xin = U4{0, 0, 0, 0};
            if (sarsa) xin = draw(c.seed, env.gid, t, BLK_INNER);              // the agent's own draw (sarsa_lambda.rs:78)
            float e;
            const float delta = td_error<A>(alg, (c.eps && c.apol_same) ? pol : c.apol, select_a<A>(q_s, a), q_n, tr.r, term, xin, e);
            const float scale = lp.alpha * delta;
            // ---- the fused sweep: trace, weights, and Q(s', .) with the updated weights
#pragma unroll
            for (int b = 0; b < A; ++b) {
                const bool hit = a == b;                                       // wave-uniform
                U4 rnd = U4{0, 0, 0, 0};
                if constexpr (IO::kBf16) rnd = draw(c.seed, env.gid, t, BLK_SR_BASE + 64u * (uint32_t)b + (uint32_t)lane);
                q_n[b] = wave_sweep_column<WT, true>(Wi + (int64_t)b * F, Zi + (int64_t)b * F, lane, phi_n, rnd, true, [&](int j, float (&w8)[8], float (&z8)[8]) {
#pragma unroll
                    for (int v = 0; v < 8; ++v) {
                        const float zz = trace_merge(lp.trace, rate_eff, z8[v], hit ? phi_s[j][v] : 0.0f);
                        w8[v] = fmaf(scale, zz, w8[v]);
                        z8[v] = term ? 0.0f : zz;                              // trace.reset() after a terminal transition
                    }
                });
            }
            if (!driver) { env.report(td_out, delta); break; }
            if (c.eps) learner_eps_step(c, tr.ended(), pol);                   // the episode's last handle is done: its end decays epsilon
            // the VALUE agents' episode end; a step cap does NOT reset the trace
            sample_then_restart<Dom>(c, env, tally, tr, delta, t,
                [&](const float (&ns)[D]) { WF::project(ns, lane, phi_n); WF::template q_from_mem<WT>(Wi, lane, phi_n, q_n); },
                [&](const U4& x) { return policy_sample<A>(pol, q_n, x); });
            wave_carry<A>(q_s, q_n, phi_s, phi_n);
        }
        if (driver) {
            env.store(c);
            if (c.eps && lane == 0) c.eps[env.i] = pol.eps;
        }
    }
    wave_hand_over(tally, env.lane, driver, stats);
}

}  // namespace rsrl
