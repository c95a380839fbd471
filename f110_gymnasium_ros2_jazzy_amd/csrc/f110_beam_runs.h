// f110_beam_runs.h — get_scan's sequential beam index as exact arithmetic progressions (runs).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "f110_math.h"

namespace f110 {

// ------------------------------------------------------ beam index runs --
// get_scan's beam index (laser_models.py:167-184) is a SEQUENTIAL float
// accumulation t_{i+1} = wrap(fl(t_i + inc)).  Inside one binade [2^(e-1), 2^e)
// every t_i is a multiple of u = ulp and fl(t_i + inc) = t_i + RN_u(inc), so the
// sequence is an exact arithmetic progression until it leaves the binade or
// wraps.  A run {start, count, t0, delta} holds t_{start+k} = t0 + k*delta
// (exact in fp64).  Ties (inc exactly half-way on the u grid) round to even:
// once t/u is even the increment is constant again, so an odd start is one
// single step.  t = 0 and t below kRunTMin (where the ulp grid and the tie
// test's half-ulp reach the subnormals) are single-beam runs.  Runs per scan:
// at most two per binade the indices pass through (a tie's odd start), over
// the binades from inc to theta_dis (twice: before and after the one wrap of
// fov < 2*pi), plus the wrapped start's own binade: max_beam_runs() bounds it
// and f110_create rejects a scan configuration whose bound exceeds kMaxSeg.
struct BeamRun {
    int32_t start, count;
    double t0, delta;
};

F110_HD double first_theta_index(double yaw, double fov, int theta_dis) {
    const double td = (double)theta_dis;
    double t = td * (yaw - fov / 2.) / (2. * kPi);  // :167
    t = fmod(t, td);                                // :170
    while (t < 0) t += td;                          // :171-172
    return t;
}

constexpr double kRunTMin = 0x1p-960;

// Upper bound of build_beam_runs' count for any yaw: per part (before and after the wrap)
// two runs per binade from the one holding inc up to theta_dis, one for a start below inc
// and one at the wrap.
inline int max_beam_runs(double inc, int theta_dis) {
    int e_inc, e_td;
    frexp(inc, &e_inc);
    frexp((double)theta_dis, &e_td);
    const int binades = e_td - e_inc + 1;
    return 2 * (2 * binades + 2);
}

// Returns the number of runs written, or -1 if max_runs is too small.
F110_HD int build_beam_runs(double t, double inc, int theta_dis, int B, BeamRun *runs, int max_runs) {
    const double td = (double)theta_dis;
    int i = 0, n = 0;
    while (i < B) {
        if (n >= max_runs) return -1;
        int run = 1;
        double delta = 0.0;
        if (t >= kRunTMin && t < td) {
            int e;
            frexp(t, &e);  // t in [2^(e-1), 2^e)
            double lim = ldexp(1.0, e);
            if (lim > td) lim = td;
            double v = t + inc;
            if (v < lim) {
                delta = v - t;               // exact (same binade)
                double rem = inc - delta;    // exact (|rem| <= u/2, u >= 2^-52)
                double half_u = ldexp(1.0, e - 54);
                bool tie = fabs(rem) == half_u;
                bool even = (((int64_t)ldexp(t, 53 - e)) & 1) == 0;  // t/u (an integer < 2^53) even
                if (!tie || even) {
                    int64_t span_u = (int64_t)ldexp(lim - t, 53 - e);
                    int64_t d_u = (int64_t)ldexp(delta, 53 - e);
                    // kmax = (span_u - 1) / d_u without a 64-bit integer divide:
                    // both < 2^53, the fp64 quotient is within 1 of it, fixed up exactly
                    int64_t kmax = (int64_t)((double)(span_u - 1) / (double)d_u);
                    if (kmax * d_u > span_u - 1) --kmax;
                    else if ((kmax + 1) * d_u <= span_u - 1) ++kmax;
                    int64_t left = (int64_t)(B - i - 1);
                    run = 1 + (int)(kmax < left ? kmax : left);
                }
            }
        }
        runs[n].start = i;
        runs[n].count = run;
        runs[n].t0 = t;
        runs[n].delta = delta;
        ++n;
        double last = t + (double)(run - 1) * delta;
        i += run;
        t = last + inc;               // :180
        while (t >= td) t -= td;      // :183-184
    }
    return n;
}

// build_beam_runs with the same runs (start, count, t0, delta) and a shorter
// dependent chain per run, for k_agents (one thread per car, latency-bound):
// the exponent and the tie test from the bits of t, and the run length
// kmax = max{k : t + k delta < lim} from an approximate quotient fixed up by
// exact sign tests (fma(k, delta, -span) rounds once, so its sign is the exact
// one), instead of 64-bit integer conversions and an IEEE division.  The
// multiples t + k delta (k <= kmax) all lie in t's binade on its ulp grid, as
// in build_beam_runs.  tests/test_host_lib.py checks the two against each
// other over yaws and scan configurations.
F110_HD int build_beam_runs_fast(double t, double inc, int theta_dis, int B, BeamRun *runs, int max_runs) {
    const double td = (double)theta_dis;
    int i = 0, n = 0;
    while (i < B) {
        if (n >= max_runs) return -1;
        int run = 1;
        double delta = 0.0;
        if (t >= kRunTMin && t < td) {
            int e;
            frexp(t, &e);  // t in [2^(e-1), 2^e)
            double lim = ldexp(1.0, e);
            if (lim > td) lim = td;
            const double v = t + inc;
            if (v < lim) {
                delta = v - t;                // exact (same binade)
                const double rem = inc - delta;
                const bool tie = fabs(rem) == ldexp(1.0, e - 54);
                const uint64_t tb = __builtin_bit_cast(uint64_t, t);
                if (!tie || (tb & 1u) == 0) {  // t's last mantissa bit (t normal): even
                    const double span = lim - t;  // exact
#if defined(__HIP_DEVICE_COMPILE__)
                    const double qa = span * __builtin_amdgcn_rcp(delta);
#else
                    const double qa = span / delta;
#endif
                    // (int)qa is kmax - 1, kmax or kmax + 1 (qa within 2^-20 relative of q); a
                    // quotient beyond 2^30 (> B) is clamped there, where kmax > B - i - 1 anyway:
                    // one exact test each way, branch-free
                    int k = (int)(qa < 0x1p30 ? qa : 0x1p30);
                    k -= fma((double)k, delta, -span) >= 0.0 ? 1 : 0;
                    k += fma((double)(k + 1), delta, -span) < 0.0 ? 1 : 0;
                    const int left = B - i - 1;
                    run = 1 + (k < left ? k : left);
                }
            }
        }
        runs[n].start = i;
        runs[n].count = run;
        runs[n].t0 = t;
        runs[n].delta = delta;
        ++n;
        double last = t + (double)(run - 1) * delta;
        i += run;
        t = last + inc;               // :180
        while (t >= td) t -= td;      // :183-184
    }
    return n;
}

// theta index (as get_scan would have it) of beam b, given its runs.
F110_HD double beam_theta_index(const BeamRun *runs, int n, int b) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {  // last run with start <= b
        int mid = (lo + hi + 1) >> 1;
        if (runs[mid].start <= b) lo = mid; else hi = mid - 1;
    }
    return runs[lo].t0 + (double)(b - runs[lo].start) * runs[lo].delta;
}

}  // namespace f110
