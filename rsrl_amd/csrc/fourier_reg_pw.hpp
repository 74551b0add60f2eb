// fourier_reg_pw.hpp -- FourierReg's projection as the producer-wave loop uses it (kernels_reg_pw.hpp, the only includer).
//
// At one learner wave per SIMD every instruction of the loop costs one issue slot whatever its class, a register copy and a wait state
// included.  This projection computes what FourierReg::project computes -- every feature by the same operations in the
// same order, in the same half of the same (f, f + 1) pair: bit-identical (tests/test_gpu_reg_producer.py,
// tests/test_gpu_reg_pw_projection.py) -- and differs in two things that are not arithmetic:
//
//   * the register pairs that hold two dimension-1 harmonics side by side are assembled by ONE v_pk_mov_b32 each, where pk_pick takes
//     two v_mov_b32 (the compiler does not select the packed move for this shuffle);
//   * the statements are written in the order the instructions should issue in.  With the loop at the register limit the scheduler
//     keeps much of the order it is given, and a packed fp32 instruction directly in front of a consumer of its result costs an
//     s_nop 0 (the compiler's wait state that the assembly post-pass removes in the other fused units, HISTORY round 4; this unit is
//     not post-processed).  So independent chains alternate: the sine and the cosine polynomial, the two harmonic recurrences, and in
//     each row of products first the multiplies, then the fmas.
//
// The pairs are written into PhiBuf's f2 storage directly and a packed move's result is only ever used as a whole pair: reading .y of
// an f2 inline-asm output element by element is the pattern that ROCm 7.2's clang has miscompiled (HISTORY, round 5; WavePk::close).
// k_train_reg keeps FourierReg::project: its machine code is pinned, and there the packed move alone measured 1 % slower (HISTORY,
// round 4).  profiles/reg_pw_moves.md has this loop's instruction counts and its A/B.
#pragma once

#include "device_core.hpp"

namespace rsrl {
namespace pw {

// {a[SA], b[SB]} as one instruction: D.lo = op_sel[0] ? S0.hi : S0.lo, D.hi = op_sel[1] ? S1.hi : S1.lo.  Not volatile, plain register
// operands: the scheduler may place it like any other VALU instruction.
template <int SA, int SB>
__device__ __forceinline__ f2 pk_pick_mov(f2 a, f2 b) {
    f2 d;
    asm("v_pk_mov_b32 %0, %1, %2 op_sel:[%3,%4]" : "=v"(d) : "v"(a), "v"(b), "n"(SA), "n"(SB));
    return d;
}

// sincospi01_x2 of device_core.hpp with the two Horner chains alternating
__device__ __forceinline__ void sincospi01_x2_alt(f2 x, f2& sn, f2& cs) {
    const f2 x2 = x * splat2(2.0f);
    const f2 q = f2{rintf(x2.x), rintf(x2.y)};
    const f2 r = __builtin_elementwise_fma(q, splat2(-0.5f), x);
    const f2 u = r * r;
    f2 ps = splat2(0.08100174367427826f);
    f2 pc = splat2(0.23132924735546112f);
    ps = __builtin_elementwise_fma(ps, u, splat2(-0.5992020964622498f));
    pc = __builtin_elementwise_fma(pc, u, splat2(-1.335044503211975f));
    ps = __builtin_elementwise_fma(ps, u, splat2(2.5501625537872314f));
    pc = __builtin_elementwise_fma(pc, u, splat2(4.058707237243652f));
    ps = __builtin_elementwise_fma(ps, u, splat2(-5.167712688446045f));
    pc = __builtin_elementwise_fma(pc, u, splat2(-4.934802055358887f));
    ps = __builtin_elementwise_fma(ps, u, splat2(3.1415927410125732f));
    const f2 c = __builtin_elementwise_fma(pc, u, splat2(1.0f));        // cos(pi r)
    const f2 s = ps * r;                                                // sin(pi r)
    float s0, c0, s1, c1;
    quadrant_select((int)q.x, s.x, c.x, s0, c0);
    quadrant_select((int)q.y, s.y, c.y, s1, c1);
    sn = f2{s0, s1}; cs = f2{c0, c1};
}

template <int DOMAIN, int ORDER>
struct FourierRegPw {
    using Base = FourierReg<DOMAIN, ORDER>;
    using Dom = Domain<DOMAIN>;
    static constexpr int D = Base::D, N1 = Base::N1, F = Base::F;
    static_assert(D == 2 && Base::kPairs && N1 % 2 == 0 && N1 >= 4, "two dimensions, rows of an even number of features: every pair starts at an odd harmonic");
    // the harmonic pairs (1, 2), (3, 4), .. of dimension 1; harmonic N1 - 1 is left over.  A row is NP pairs of products and the pair that
    // straddles into the next row
    static constexpr int NP = (N1 - 2) / 2;

    __device__ static __forceinline__ void project(const float (&s)[D], f2 (&phi)[F / 2]) {
        // ---- PairTables::build: ct[n] = (cos n pi x~, cos n pi y~), st[n] the sines
        f2 ct[N1], st[N1];
        {
            constexpr float lo0 = (float)Dom::lo_d(0), hi0 = (float)Dom::hi_d(0), lo1 = (float)Dom::lo_d(1), hi1 = (float)Dom::hi_d(1);
            constexpr float inv0 = 1.0f / (hi0 - lo0), inv1 = 1.0f / (hi1 - lo1);
            const f2 sc = (f2{s[0], s[1]} - f2{lo0, lo1}) * f2{inv0, inv1};
            sincospi01_x2_alt(sc, st[1], ct[1]);
            static_for<2, N1>([&](auto Nn) {
                constexpr int n = Nn;
                const f2 mc = ct[n - 1] * ct[1];
                const f2 ms = st[n - 1] * ct[1];
                ct[n] = __builtin_elementwise_fma(-st[n - 1], st[1], mc);
                st[n] = __builtin_elementwise_fma(ct[n - 1], st[1], ms);
            });
        }
        // ---- (cos_a y, cos_{a+1} y) and (sin_a y, sin_{a+1} y), a = 1, 3, ..: row 0's features themselves, and what every row below multiplies by
        f2 cy[NP], sy[NP];
        static_for<0, NP>([&](auto Ii) {
            constexpr int i = Ii;
            cy[i] = pk_pick_mov<1, 1>(ct[2 * i + 1], ct[2 * i + 2]);
            sy[i] = pk_pick_mov<1, 1>(st[2 * i + 1], st[2 * i + 2]);
        });
        // ---- row 0 (dimension-0 harmonic 0): features k = 1 .. N1 - 1 are the dimension-1 cosines; the last shares its pair with (1, 0) = cos x
        static_for<0, NP>([&](auto Ii) { constexpr int i = Ii; phi[i] = cy[i]; });
        phi[NP] = pk_pick_mov<1, 0>(ct[N1 - 1], ct[1]);
        // ---- rows r >= 1: (r, b) = cos_r x cos_b y - sin_r x sin_b y as fma(-sin_r x, sin_b y, cos_r x * cos_b y), two features per packed
        // instruction; (r, N1 - 1) by the scalar pair of instructions, next to (r + 1, 0) = cos_{r+1} x -- or the constant 1, the last feature
        static_for<1, N1>([&](auto Rr) {
            constexpr int r = Rr, j0 = (r * N1) / 2;
            f2 m[NP];
            static_for<0, NP>([&](auto Ii) { constexpr int i = Ii; m[i] = splat2(ct[r].x) * cy[i]; });
            const float ml = ct[r].x * ct[N1 - 1].y;
            static_for<0, NP>([&](auto Ii) { constexpr int i = Ii; phi[j0 + i] = __builtin_elementwise_fma(splat2(-st[r].x), sy[i], m[i]); });
            const float last = fmaf(-st[r].x, st[N1 - 1].y, ml);
            if constexpr (r + 1 < N1) phi[j0 + NP] = f2{last, ct[r + 1].x};
            else phi[j0 + NP] = f2{last, 1.0f};
        });
        static_assert((N1 - 1) * N1 / 2 + NP == F / 2 - 1, "the last pair is the last row's");
    }
};

}  // namespace pw
}  // namespace rsrl
