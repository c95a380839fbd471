// f110_sincos.h — the trigonometry that has to match the reference's bit for bit: cr_sincos, the
// correctly rounded f64 sin / cos (double-double, with the table of f110_sincos_table.h) and its
// tan / cos pair, and np_sincosf, NumPy's float32 sin / cos.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "f110_math.h"
#include "f110_sincos_table.h"

namespace f110 {

// ------------------------------------------------ correctly rounded sin/cos --
// The reference's np.sin / np.cos (and Numba's libm calls) are glibc's, which
// return the correctly rounded result but in very rare cases; ocml's differ by
// an ulp on a few percent of arguments, which is what left agent ray_cast
// ranges and box vertices inexact.  cr_sincos evaluates sin and cos of x in
// double-double arithmetic and rounds once: the Cody-Waite reduction by a
// three-part pi/2 (the first product exact by fma), then Taylor series of
// sin / cos on |r| <= pi/4 with the terms through r^7 (sin) / r^6 (cos) in
// double-double Horner steps and the rest in double.  The sum before the last
// rounding is within ~2^-70 relative, so the result is the correctly rounded
// value except where the true value lies within that of a rounding midpoint.
// Host and device compute it with the same IEEE operations (no contraction,
// explicit fma): tests/test_host_lib.py checks it against NumPy, equal except
// where glibc is itself one ulp off (< 0.3 % of the sampled arguments; there
// cr_sincos is the correctly rounded value).  That residue is pinned by the
// non-exact budgets (tests/golden/nonexact_beams.json), not by bit-equality.
// |x| >= 2^20 (never a scan or box angle here) falls back to the library call.
struct DD {
    double h, l;
};

F110_HD DD dd_two_sum(double a, double b) {
    const double s = a + b;
    const double bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}

F110_HD DD dd_fast(double a, double b) {  // |a| >= |b|
    const double s = a + b;
    return {s, b - (s - a)};
}

F110_HD DD dd_mul(DD a, DD b) {
    const double p = a.h * b.h;
    double e = fma(a.h, b.h, -p);
    e += a.h * b.l + a.l * b.h;
    return dd_fast(p, e);
}

F110_HD DD dd_add(DD a, DD b) {
    const DD s = dd_two_sum(a.h, b.h);
    return dd_fast(s.h, s.l + (a.l + b.l));
}

// acc = c + z * acc in double-double
F110_HD DD dd_horner(DD c, DD z, DD acc) { return dd_add(c, dd_mul(z, acc)); }

// x - k pi/2 as a double-double, k the nearest quadrant (|x| < 2^20, x != 0).
F110_HD DD sincos_reduce(double x, double &k) {
    const double P1 = 0x1.921fb54442d18p+0, P2 = 0x1.1a62633145c07p-54, P3 = -0x1.f1976b7ed8fbcp-110;
    k = rint(x * 0x1.45f306dc9c883p-1);  // x * 2/pi, nearest quadrant
    const double r1 = fma(-k, P1, x);    // exact: |x| >= pi/4 has ulp >= 2^-53
    const double q2 = k * P2;
    const double q2l = fma(k, P2, -q2);
    const DD s1 = dd_two_sum(r1, -q2);
    return dd_fast(s1.h, s1.l - q2l - k * P3);
}

// sin / cos of the reduced r by the double-double series (the slow, always
// certain path).
F110_HD void sincos_series(DD r, double &s, double &c) {
    const DD z = dd_mul(r, r);
    const double zh = z.h;
    // sin(r) = r (1 - z/3! + z^2/5! - z^3/7! + z^4 ps(z)),  ps = 1/9! - z/11! + ... - z^5/19!
    double ps = 0x1.952c77030ad4ap-49 - zh * 0x1.2f49b46814157p-57;  // 1/17! - z/19!
    ps = 0x1.ae7f3e733b81fp-41 - zh * ps;                             // 1/15!
    ps = 0x1.6124613a86d09p-33 - zh * ps;                             // 1/13!
    ps = 0x1.ae64567f544e4p-26 - zh * ps;                             // 1/11!
    ps = 0x1.71de3a556c734p-19 - zh * ps;                             // 1/9!
    DD as = {ps, 0.0};
    as = dd_horner({-0x1.a01a01a01a01ap-13, -0x1.a01a01a01a01ap-73}, z, as);  // -1/7!
    as = dd_horner({0x1.1111111111111p-7, 0x1.1111111111111p-63}, z, as);    // 1/5!
    as = dd_horner({-0x1.5555555555555p-3, -0x1.5555555555555p-57}, z, as);  // -1/3!
    as = dd_horner({1.0, 0.0}, z, as);
    const DD sr = dd_mul(r, as);
    // cos(r) = 1 - z/2! + z^2/4! - z^3/6! + z^4 pc(z),  pc = 1/8! - z/10! + ... - z^5/18!
    double pc = 0x1.ae7f3e733b81fp-45 - zh * 0x1.6827863b97d97p-53;  // 1/16! - z/18!
    pc = 0x1.93974a8c07c9dp-37 - zh * pc;                            // 1/14!
    pc = 0x1.1eed8eff8d898p-29 - zh * pc;                            // 1/12!
    pc = 0x1.27e4fb7789f5cp-22 - zh * pc;                            // 1/10!
    pc = 0x1.a01a01a01a01ap-16 - zh * pc;                            // 1/8!
    DD ac = {pc, 0.0};
    ac = dd_horner({-0x1.6c16c16c16c17p-10, 0x1.f49f49f49f49fp-65}, z, ac);  // -1/6!
    ac = dd_horner({0x1.5555555555555p-5, 0x1.5555555555555p-59}, z, ac);    // 1/4!
    ac = dd_horner({-0.5, 0.0}, z, ac);
    ac = dd_horner({1.0, 0.0}, z, ac);
    s = sr.h + sr.l;
    c = ac.h + ac.l;
}

// sin(i/64), cos(i/64) as double-doubles, i = 0..52 (scripts/gen_sincos_table.py).
constexpr double kSinCosTab[F110_SINCOS_TAB_N][4] = {F110_SINCOS_TAB_DATA};

// sin / cos of the reduced r by the table: a = |r| = i/64 + t, |t| <= 1/128,
// sin a = S cos t + C sin t, cos a = C cos t - S sin t with (S, C) the table's
// double-doubles and sin t / cos t short series in double with their leading
// products exact.  The sum before the last rounding is within ~2^-68 relative
// of sin a / cos a (the largest term is the rounding of t^3/6 against a result
// >= 1/128 for i >= 1; i = 0 is relative to t itself); a rounding that a 2^-64
// relative error could flip is not certain, and the caller then takes the
// series path (about 0.1 % of the values).  Where it returns true the result
// is the one sincos_series gives (both round the same certain value), which
// tests/test_host_lib.py checks over a few million arguments.
// The table path without a branch: returns whether the rounding is certain (s, c are then the
// correctly rounded values).  |r.h| >= 1 (not a reduced argument) reads entry 0 and returns garbage.
// The table path's double-double sin / cos of |r| (before the rounding) and their rounding bounds.
struct SinCosDD {
    double sh, sl, ch, cl;           // sin |r| = sh + sl, cos |r| = ch + cl (relative error < ~2^-68)
    double s_up, s_dn, c_up, c_dn;   // the roundings at +- the error bound: certain where equal
    bool neg;                        // r < 0
};

F110_HD SinCosDD sincos_table_core(DD r, const double (*tab)[4]) {
    const bool neg = r.h < 0.0;
    const double ah0 = fabs(r.h), al = neg ? -r.l : r.l;
    const double ah = ah0 < 1.0 ? ah0 : 0.0;  // (NaN too) keeps the index in the table
    const int i = (int)rint(ah * 64.0);
    const double *T = tab[i];
    const double th = ah - (double)i * 0.015625;  // exact (Sterbenz)
    const double tl = al;
    const double zh = th * th;
    const double zl = fma(th, th, -zh);
    // sin t = th + slo:  t - t^3/6 + t^5/120 - ...  with the t^2 tl / 2 cross term of t^3 / 6
    const double P = -0x1.5555555555555p-3 +
                     zh * (0x1.1111111111111p-7 + zh * (-0x1.a01a01a01a01ap-13 + zh * 0x1.71de3a556c734p-19));
    const double slo = tl + (th * (zh * P) - (0.5 * zh) * tl);
    // cos t = ch + cl:  1 - t^2/2 + t^4/24 - t^6/720 + t^8/40320
    const double Q = 0x1.5555555555555p-5 + zh * (-0x1.6c16c16c16c17p-10 + zh * 0x1.a01a01a01a01ap-16);
    const double hz = 0.5 * zh;
    const double ch = 1.0 - hz;
    const double cl = ((1.0 - ch) - hz) - ((0.5 * zl + th * tl) - (zh * zh) * Q);
    const double Sh = T[0], Sl = T[1], Ch = T[2], Cl = T[3];
    // sin a = Sh ch + Ch th + (Sh cl + Sl ch + Ch slo + Cl th)
    const double p1 = Sh * ch, e1 = fma(Sh, ch, -p1);
    const double p2 = Ch * th, e2 = fma(Ch, th, -p2);
    const DD sa = dd_two_sum(p1, p2);
    const double sl = sa.l + (e1 + e2) + (((Sh * cl + Sl * ch) + Cl * th) + Ch * slo);
    // cos a = Ch ch - Sh th + (Ch cl + Cl ch - Sh slo - Sl th)
    const double q1 = Ch * ch, f1 = fma(Ch, ch, -q1);
    const double q2 = -(Sh * th), f2 = fma(-Sh, th, -q2);
    const DD ca = dd_two_sum(q1, q2);
    const double cl2 = ca.l + (f1 + f2) + (((Ch * cl + Cl * ch) - Sl * th) - Sh * slo);
    const double es = fabs(sa.h) * 0x1p-64, ec = 0x1p-64;  // |cos a| > 0.7
    const double s_up = sa.h + (sl + es), s_dn = sa.h + (sl - es);
    const double c_up = ca.h + (cl2 + ec), c_dn = ca.h + (cl2 - ec);
    return {sa.h, sl, ca.h, cl2, s_up, s_dn, c_up, c_dn, neg};
}

F110_HD bool sincos_table_nb(DD r, double &s, double &c, const double (*tab)[4]) {
    const SinCosDD v = sincos_table_core(r, tab);
    s = v.neg ? -v.s_up : v.s_up;
    c = v.c_up;
    return (v.s_up == v.s_dn) & (v.c_up == v.c_dn);
}

F110_HD bool sincos_table(DD r, double &s, double &c, const double (*tab)[4] = kSinCosTab) {
    double s2, c2;
    if (!sincos_table_nb(r, s2, c2, tab)) return false;
    s = s2;
    c = c2;
    return true;
}

// cr_sincos's common case without a branch: the reduction, the table path and the quadrant as
// selects, +-0 included.  Returns false where cr_sincos takes another path (|x| >= 2^20, NaN, an
// uncertain rounding); where it returns true sn / cs are cr_sincos's values.  Straight-line code,
// so independent evaluations (and the arithmetic around them) can overlap; the caller runs
// cr_sincos itself on false, after the rest of its work.
F110_HD bool cr_sincos_fast(double x, double &sn, double &cs, const double (*tab)[4] = kSinCosTab) {
    const bool in = fabs(x) < 1048576.0;
    double k;
    const DD r = sincos_reduce(in ? x : 1.0, k);
    double s, c;
    const bool cert = sincos_table_nb(r, s, c, tab);
    const int q = (int)((int64_t)k & 3);
    const double a = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
    const double b = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
    const bool zero = x == 0.0;
    sn = zero ? x : a;
    cs = zero ? 1.0 : b;
    return zero | (cert & in);
}

// tan x and cos x from one table evaluation (the kinematic model's pair, vehicle_dynamics_st).
// cos: cr_sincos's value where ok_c.  tan: sin / cos in double-double, rounded once at a 2^-64
// relative bound -- the correctly rounded tan where ok_t (glibc's tan, which the reference's
// Numba code calls, is correctly rounded on all but ~0.4 % of arguments; the device library's
// differs more often).  Where a flag is false the caller takes cr_cos / the library tan.
F110_HD void tan_cos_fast(double x, const double (*tab)[4], double &t, double &c, bool &ok_t, bool &ok_c) {
    const bool in = fabs(x) < 1048576.0;
    double k;
    const DD r = sincos_reduce(in ? x : 1.0, k);
    const SinCosDD v = sincos_table_core(r, tab);
    const int q = (int)((int64_t)k & 3);
    const double s_r = v.neg ? -v.s_up : v.s_up, c_r = v.c_up;
    const bool s_ok = v.s_up == v.s_dn, c_ok = v.c_up == v.c_dn;
    const bool zero = x == 0.0;
    const double cq = q == 0 ? c_r : q == 1 ? -s_r : q == 2 ? -c_r : s_r;  // cos(r + q pi/2)
    c = zero ? 1.0 : cq;
    ok_c = zero | (in & ((q & 1) ? s_ok : c_ok));
    // tan(r + q pi/2) = sin r / cos r (q even), -cos r / sin r (q odd)
    // (the table path's low parts carry the t^3 / t^2 terms: up to ~2^-22 of the high parts, so both
    // are renormalised before the division, whose correction divides by the high part only)
    const DD Sn = dd_fast(v.neg ? -v.sh : v.sh, v.neg ? -v.sl : v.sl), Cn = dd_fast(v.ch, v.cl);
    const double nh = (q & 1) ? Cn.h : Sn.h, nl = (q & 1) ? Cn.l : Sn.l;
    const double dh = (q & 1) ? Sn.h : Cn.h, dl = (q & 1) ? Sn.l : Cn.l;
    const double q0 = nh / dh;
    const double rr = (fma(-q0, dh, nh) + nl) - q0 * dl;  // N - q0 D (the product's error exact)
#if defined(__HIP_DEVICE_COMPILE__)
    const double q1 = rr * __builtin_amdgcn_rcp(dh);  // a correction below an ulp of q0: a rough quotient
#else
    const double q1 = rr / dh;
#endif
    const double et = fabs(q0) * 0x1p-64;
    const double t_up = q0 + (q1 + et), t_dn = q0 + (q1 - et);
    t = zero ? x : ((q & 1) ? -t_up : t_up);
    ok_t = zero | (in & (t_up == t_dn) & (dh != 0.0));
}

// tab: kSinCosTab or a copy of it (k_agents reads an LDS copy: one short dependent load per call).
// The branch-free common case inline, the rest (library calls, the series) out of line: one copy
// of it per kernel instead of one per call site (k_agents' code is read once per wave from L2).
__host__ __device__ __attribute__((noinline)) inline void cr_sincos_slow(double x, double &sn, double &cs,
                                                                          const double (*tab)[4]);

F110_HD void cr_sincos(double x, double &sn, double &cs, const double (*tab)[4] = kSinCosTab) {
    if (!cr_sincos_fast(x, sn, cs, tab)) cr_sincos_slow(x, sn, cs, tab);
}

__host__ __device__ __attribute__((noinline)) inline void cr_sincos_slow(double x, double &sn, double &cs,
                                                                          const double (*tab)[4]) {
    if (!(fabs(x) < 1048576.0)) {  // NaN, inf, or beyond the exact reduction
        sn = sin(x);
        cs = cos(x);
        return;
    }
    if (x == 0.0) {  // +-0 (keeps the sign of sin(-0.0))
        sn = x;
        cs = 1.0;
        return;
    }
    double k, s, c;
    const DD r = sincos_reduce(x, k);
    if (!sincos_table(r, s, c, tab)) sincos_series(r, s, c);
    switch ((int)((int64_t)k & 3)) {
        case 0: sn = s; cs = c; break;
        case 1: sn = c; cs = -s; break;
        case 2: sn = -s; cs = -c; break;
        default: sn = -c; cs = s; break;
    }
}

// The series path alone (tests: the table path must give the same bits).
F110_HD void cr_sincos_series(double x, double &sn, double &cs) {
    if (!(fabs(x) < 1048576.0) || x == 0.0) {
        cr_sincos(x, sn, cs);
        return;
    }
    double k, s, c;
    sincos_series(sincos_reduce(x, k), s, c);
    switch ((int)((int64_t)k & 3)) {
        case 0: sn = s; cs = c; break;
        case 1: sn = c; cs = -s; break;
        case 2: sn = -s; cs = -c; break;
        default: sn = -c; cs = s; break;
    }
}

F110_HD double cr_sin(double x) {
    double s, c;
    cr_sincos(x, s, c);
    return s;
}

F110_HD double cr_cos(double x, const double (*tab)[4] = kSinCosTab) {
    double s, c;
    cr_sincos(x, s, c, tab);
    return c;
}

// ---------------------------------------------------- NumPy float32 trig --
// np.cos / np.sin on float32 (NumPy 2.2, the x86 SIMD loop of
// umath/loops_trigonometric: Cody-Waite reduction by pi/2 in three fma steps,
// degree-8 cosine / degree-9 sine minimax polynomials on [-pi/4, pi/4],
// quadrant select; |x| beyond 71476.0625 (cos) / 117435.992 (sin) goes to
// libm, here the correctly rounded float of the f64 function).  F110Env.reset
// evaluates start_rot this way when its options are float32
// (f110_env.py:448-451, train_ddpg's dtype).  Bit-exact against the installed
// NumPy on [-pi, pi] and beyond (tests/test_host_lib.py).
F110_HD float np_sincosf(float x, bool cos_op) {
    if (x != x) return x;
    const float ax = x < 0.0f ? -x : x;
    if (ax > (cos_op ? 71476.0625f : 117435.992f)) return (float)(cos_op ? cos((double)x) : sin((double)x));
    const float magic = 0x1.800000p+23f;
    float q = fmaf(x, 0x1.45f306p-1f, magic);  // x * 2/pi, rounded to the nearest integer (one fma)
    q = q - magic;
    float r = fmaf(q, -0x1.921fb0p+00f, x);
    r = fmaf(q, -0x1.5110b4p-22f, r);
    r = fmaf(q, -0x1.846988p-48f, r);
    const float r2 = r * r;
    float c = fmaf(0x1.98e616p-16f, r2, -0x1.6c06dcp-10f);
    c = fmaf(c, r2, 0x1.55553cp-05f);
    c = fmaf(c, r2, -0x1.000000p-01f);
    c = fmaf(c, r2, 0x1.000000p+00f);
    float sn = fmaf(0x1.7d3bbcp-19f, r2, -0x1.a06bbap-13f);
    sn = fmaf(sn, r2, 0x1.11119ap-07f);
    sn = fmaf(sn, r2, -0x1.555556p-03f);
    sn = fmaf(sn, r2, 0.0f);
    sn = fmaf(sn, r, r);
    int iq = (int)q;  // q is integral
    if (cos_op) iq += 1;
    float v = (iq & 1) == 0 ? sn : c;
    if ((iq & 2) == 2) v = 0.0f - v;
    return v;
}

}  // namespace f110
