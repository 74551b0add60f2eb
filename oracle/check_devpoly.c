/* check_devpoly.c -- TEST INFRASTRUCTURE.  Exhaustive sweep of the HIP path's three hand-written polynomials (rsrl_amd/csrc/device_core.hpp
 * sincospi01, sincos_cw, exp_dev), in the restatement the oracle's f32d instantiation compares the device with bit for bit
 * (oracle/rsrl_oracle_impl.h, ORC_DEVTRIG: the same operations in the same order; included below, not copied), against the f64 library functions:
 *
 *     sincospi  sincospi01(x) against sin(pi x), cos(pi x)      the quadrant taken off exactly in f64 first (sincospi_ref)
 *     sincos    sincos_cw(x)  against sin(x), cos(x)
 *     exp       exp_dev(x)    against exp(x); below -87 the result must be exactly 0, above 88.5 +inf, NaN stays NaN
 *
 *     check_devpoly <sincospi|sincos|exp> <n_threads> <lo> <hi>
 *
 * tries EVERY fp32 x with lo <= x <= hi (both zeros when 0 lies inside) and prints one line with the number of inputs, the largest absolute
 * error and the largest error in units of the last place of the f64 result rounded to fp32 (never less than 2^-149), each with the bit pattern
 * of its argument.  For exp, lo and hi are widened by the program itself with the inputs outside [-87, 88.5] whose result is a rule, not an
 * approximation (-FLT_MAX .. -87, 88.5 .. FLT_MAX, both infinities, every NaN): `rule_bad` counts the ones that break it.  Exit status 0.
 * The caller asserts the figures. */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

/* ---- the functions under test ARE the oracle's: rsrl_oracle.c is compiled into this program (it has no main), so the sweep pins the very code
 * the f32d instantiation compares the device with -- no second copy that could drift */
#include "rsrl_oracle.c"
#define sincospi01_dev sincospi01_dev_f32d
#define sincos_cw_dev sincos_cw_dev_f32d
#define exp_dev exp__f32d

/* sin(pi x), cos(pi x) in f64 without the rounding of pi x: k = rint(2 x) and r = x - k / 2 are exact for an fp32 x, |pi r| <= pi / 4, and the
 * quadrant is applied to the two results -- so sin(pi * 1) is 0 and not the 1.2e-16 that sin(M_PI) is */
static inline void sincospi_ref(double x, double* sn, double* cs) {
    const double k = rint(2.0 * x), r = x - 0.5 * k;
    const double s = sin(M_PI * r), c = cos(M_PI * r);
    const long q = ((long)k) & 3;
    *sn = (q == 0) ? s : ((q == 1) ? c : ((q == 2) ? -s : -c));
    *cs = (q == 0) ? c : ((q == 1) ? -s : ((q == 2) ? -c : s));
}

/* one unit in the last place of fl32(want) */
static inline double ulp32(double want) {
    const float w = fabsf((float)want);
    int e;
    if (!(w >= 1.17549435e-38f)) return ldexp(1.0, -149);
    if (isinf(w)) return ldexp(1.0, 127 - 23);
    e = ilogbf(w);
    return ldexp(1.0, e - 23);
}

enum { F_SINCOSPI, F_SINCOS, F_EXP };
typedef struct {
    int fn, tid, nth; float lo, hi;
    uint64_t seen, rule_bad; uint32_t rule_first;
    double abs_s, abs_c, ulp_s, ulp_c; uint32_t abs_s_at, abs_c_at, ulp_s_at, ulp_c_at;
} job_t;

static inline void keep(double v, uint32_t b, double* best, uint32_t* at) { if (v > *best || v != v) { if (!(*best != *best)) { *best = v; *at = b; } } }

static void* work(void* p) {
    job_t* j = (job_t*)p;
    /* blocks of 2^16 consecutive bit patterns dealt round robin: the inputs of a narrow range are spread over every thread */
    for (uint64_t blk = (uint64_t)j->tid; blk < ((uint64_t)1 << 16); blk += (uint64_t)j->nth)
    for (uint64_t b = blk << 16; b < ((blk + 1) << 16); b++) {
        const float x = u2f((uint32_t)b);
        const int inside = x >= j->lo && x <= j->hi;
        if (j->fn == F_EXP) {
            const float got = exp_dev(x);
            if (isnan(x)) { j->seen++; if (!isnan(got)) { if (!j->rule_bad) j->rule_first = (uint32_t)b; j->rule_bad++; } continue; }
            if (x < -87.0f || x > 88.5f) {
                const int ok = x < -87.0f ? f2u(got) == 0u : f2u(got) == 0x7f800000u;
                j->seen++;
                if (!ok) { if (!j->rule_bad) j->rule_first = (uint32_t)b; j->rule_bad++; }
                continue;
            }
            if (!inside) continue;
            j->seen++;
            { const double want = exp((double)x), e = fabs((double)got - want);
              keep(e, (uint32_t)b, &j->abs_s, &j->abs_s_at); keep(e / ulp32(want), (uint32_t)b, &j->ulp_s, &j->ulp_s_at); }
            continue;
        }
        if (!inside) continue;
        j->seen++;
        {
            float s, c; double ws, wc, es, ec;
            if (j->fn == F_SINCOSPI) { sincospi01_dev(x, &s, &c); sincospi_ref((double)x, &ws, &wc); }
            else { sincos_cw_dev(x, &s, &c); ws = sin((double)x); wc = cos((double)x); }
            es = fabs((double)s - ws); ec = fabs((double)c - wc);
            keep(es, (uint32_t)b, &j->abs_s, &j->abs_s_at); keep(es / ulp32(ws), (uint32_t)b, &j->ulp_s, &j->ulp_s_at);
            keep(ec, (uint32_t)b, &j->abs_c, &j->abs_c_at); keep(ec / ulp32(wc), (uint32_t)b, &j->ulp_c, &j->ulp_c_at);
        }
    }
    return NULL;
}

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: %s <sincospi|sincos|exp> n_threads lo hi\n", argv[0]); return 2; }
    const int fn = !strcmp(argv[1], "sincospi") ? F_SINCOSPI : !strcmp(argv[1], "sincos") ? F_SINCOS : !strcmp(argv[1], "exp") ? F_EXP : -1;
    if (fn < 0) { fprintf(stderr, "unknown function %s\n", argv[1]); return 2; }
    int nth = atoi(argv[2]); if (nth < 1) nth = 1; if (nth > 64) nth = 64;
    const float lo = strtof(argv[3], NULL), hi = strtof(argv[4], NULL);
    pthread_t th[64]; job_t jobs[64];
    for (int t = 0; t < nth; t++) { memset(&jobs[t], 0, sizeof(job_t)); jobs[t].fn = fn; jobs[t].tid = t; jobs[t].nth = nth; jobs[t].lo = lo; jobs[t].hi = hi; pthread_create(&th[t], NULL, work, &jobs[t]); }
    job_t a; memset(&a, 0, sizeof(a));
    for (int t = 0; t < nth; t++) {
        pthread_join(th[t], NULL);
        const job_t* j = &jobs[t];
        a.seen += j->seen;
        if (j->rule_bad && !a.rule_bad) a.rule_first = j->rule_first;
        a.rule_bad += j->rule_bad;
        keep(j->abs_s, j->abs_s_at, &a.abs_s, &a.abs_s_at); keep(j->ulp_s, j->ulp_s_at, &a.ulp_s, &a.ulp_s_at);
        keep(j->abs_c, j->abs_c_at, &a.abs_c, &a.abs_c_at); keep(j->ulp_c, j->ulp_c_at, &a.ulp_c, &a.ulp_c_at);
    }
    if (fn == F_EXP)
        printf("fn=exp lo=%.9g hi=%.9g inputs=%llu rule_bad=%llu rule_first=%08x abs=%.6e abs_at=%08x ulp=%.6f ulp_at=%08x\n", (double)lo, (double)hi,
               (unsigned long long)a.seen, (unsigned long long)a.rule_bad, a.rule_first, a.abs_s, a.abs_s_at, a.ulp_s, a.ulp_s_at);
    else
        printf("fn=%s lo=%.9g hi=%.9g inputs=%llu sin_abs=%.6e sin_abs_at=%08x sin_ulp=%.6f sin_ulp_at=%08x cos_abs=%.6e cos_abs_at=%08x cos_ulp=%.6f cos_ulp_at=%08x\n",
               argv[1], (double)lo, (double)hi, (unsigned long long)a.seen, a.abs_s, a.abs_s_at, a.ulp_s, a.ulp_s_at, a.abs_c, a.abs_c_at, a.ulp_c, a.ulp_c_at);
    return 0;
}
