// ttenv_math.h -- the env kernels' constants and f64 elementary functions: the table of polynomial coefficients and of the RK45
// tableau (KTable, kTable), sin / cos / exp sized for the step, the f32 read-back of an angle, the wrap to [-pi, pi], and the
// counter-based RNG's name and u01.
// Part of csrc/ttenv.hip's translation unit, inside its anonymous namespace.  Needs <hip/hip_runtime.h> and ttphilox.h before it.
#pragma once

constexpr double kPi = 3.14159265358979323846;
constexpr double kDeg = kPi / 180.0;

// numeric constants of the kernel's polynomials and of the RK45 tableau
struct KTable {
    double f[17];     // 1/k!, k = 0..16
    double A[6][5];   // scipy RK45.A
    double B[6];      // scipy RK45.B (5th-order weights)
    double C[6];      // scipy RK45.C
    double two_over_pi, p1, p2, p3, p3t;  // pi/2 in 33-bit pieces (Cody-Waite)
    double inv_2pi, tp_hi, tp_lo;         // 2*pi split
    double log2e, ln2_hi, ln2_lo;
};

constexpr double fact_inv(int k) {
    double r = 1.0;
    for (int i = 2; i <= k; ++i) r /= (double)i;
    return r;
}

constexpr KTable make_table() {
    KTable t{};
    for (int k = 0; k <= 16; ++k) t.f[k] = fact_inv(k);
    constexpr double A[6][5] = {{0, 0, 0, 0, 0},
                                {1.0 / 5, 0, 0, 0, 0},
                                {3.0 / 40, 9.0 / 40, 0, 0, 0},
                                {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
                                {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
                                {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
    constexpr double B[6] = {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
    constexpr double C[6] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0};
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 5; ++j) t.A[i][j] = A[i][j];
        t.B[i] = B[i];
        t.C[i] = C[i];
    }
    t.two_over_pi = 0.6366197723675814;
    t.p1 = 0x1.921fb54400000p+0; t.p2 = 0x1.0b4611a600000p-34; t.p3 = 0x1.3198a2e000000p-69; t.p3t = 0x1.b839a252049c1p-104;
    t.inv_2pi = 0.15915494309189535; t.tp_hi = 0x1.921fb54442000p+2; t.tp_lo = 2.9774189921946493e-12;
    t.log2e = 1.4426950408889634; t.ln2_hi = 0x1.62e42fee00000p-1; t.ln2_lo = 0x1.a39ef35793c76p-33;
    return t;
}

__device__ constexpr KTable kTable = make_table();

// ------------------------------------------------------------------------------------------
// counter-based RNG (csrc/ttphilox.h)
using ttrng::philox4x32;
__device__ inline double u01(uint32_t x) { return ((double)x + 0.5) * (1.0 / 4294967296.0); }

// ------------------------------------------------------------------------------------------
// f64 elementary functions sized for this kernel: branch-free, Taylor coefficients 1/k! shared by all of
// them (sin/cos are written in u = -x^2 so that every coefficient is positive).

// sin and cos of any heading with |x| < 1e6: Cody-Waite reduction by pi/2 split into 33-bit pieces
// (k*P1 and k*P2 are exact for |k| < 2^20), then Taylor on [-pi/4, pi/4] (sin to x^15, cos to x^16: < 5e-17).
__device__ __forceinline__ void tt_sincos(const KTable &T, double x, double &s, double &c) {
    const double k = rint(x * T.two_over_pi);
    double r = fma(-k, T.p1, x);
    r = fma(-k, T.p2, r);
    r = fma(-k, T.p3, r);
    r = fma(-k, T.p3t, r);
    const double u = -(r * r);
    double ps = T.f[15];
    ps = fma(ps, u, T.f[13]);
    ps = fma(ps, u, T.f[11]);
    ps = fma(ps, u, T.f[9]);
    ps = fma(ps, u, T.f[7]);
    ps = fma(ps, u, T.f[5]);
    ps = fma(ps, u, T.f[3]);
    // sin(-0.0) is -0.0 (np.sin; the f32 observation keeps the sign); k = -0 makes the reduction's first fma return +0
    const double sr = x == 0.0 ? x : fma(r * u, ps, r);
    double pc = T.f[16];
    pc = fma(pc, u, T.f[14]);
    pc = fma(pc, u, T.f[12]);
    pc = fma(pc, u, T.f[10]);
    pc = fma(pc, u, T.f[8]);
    pc = fma(pc, u, T.f[6]);
    pc = fma(pc, u, T.f[4]);
    pc = fma(pc, u, T.f[2]);
    const double cr = fma(u, pc, 1.0);
    const int q = (int)(long long)k;
    const double a = (q & 1) ? cr : sr, b = (q & 1) ? sr : cr;
    s = (q & 2) ? -a : a;
    c = ((q + 1) & 2) ? -b : b;
}

// sin and cos of a small angle, no reduction: the heading increments inside one 0.08 s step, bounded by
// dt*|v|/L (0.08 rad for the reference constants; tt_env_create refuses > 0.25).  sin to x^11, cos to x^12:
// truncation 1e-19 at 0.08 rad, 1e-16 at 0.25 rad.
__device__ __forceinline__ void tt_sincos_small(const KTable &T, double x, double &s, double &c) {
    const double u = -(x * x);
    double ps = T.f[11];
    ps = fma(ps, u, T.f[9]);
    ps = fma(ps, u, T.f[7]);
    ps = fma(ps, u, T.f[5]);
    ps = fma(ps, u, T.f[3]);
    s = fma(x * u, ps, x);
    double pc = T.f[12];
    pc = fma(pc, u, T.f[10]);
    pc = fma(pc, u, T.f[8]);
    pc = fma(pc, u, T.f[6]);
    pc = fma(pc, u, T.f[4]);
    pc = fma(pc, u, T.f[2]);
    c = fma(u, pc, 1.0);
}

// exp(y) for y <= 0 (clamped at -100): k = rint(y/ln2), Taylor to r^12 on |r| <= ln2/2 (truncation 2e-16)
__device__ __forceinline__ double tt_exp_neg(const KTable &T, double y) {
    y = fmax(y, -100.0);
    const double k = rint(y * T.log2e);
    double r = fma(-k, T.ln2_hi, y);
    r = fma(-k, T.ln2_lo, r);
    double p = T.f[12];
    p = fma(p, r, T.f[11]);
    p = fma(p, r, T.f[10]);
    p = fma(p, r, T.f[9]);
    p = fma(p, r, T.f[8]);
    p = fma(p, r, T.f[7]);
    p = fma(p, r, T.f[6]);
    p = fma(p, r, T.f[5]);
    p = fma(p, r, T.f[4]);
    p = fma(p, r, T.f[3]);
    p = fma(p, r, T.f[2]);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)k);
}

// The reference reads three angles back through float32: np.arctan2(f32(sin a), f32(cos a)).  Its real value
// is a + e with e = (y*cos a - x*sin a)/(x*cos a + y*sin a) (y, x the f32-rounded sin, cos; |e| ~ 1e-8, the
// first-order form is exact to 1e-21), so the correctly rounded f32 result is (float)(a + e): no atan needed.
// `a` must already be wrapped to [-pi, pi].
__device__ __forceinline__ float tt_atan2_readback(double a, double sa, double ca, float y, float x) {
    const double yd = (double)y, xd = (double)x;
    const double num = yd * ca - xd * sa, den = xd * ca + yd * sa;  // den = 1 - O(1e-8)
    return (float)(a + num * (2.0 - den));
}

__device__ __forceinline__ double tt_wrap_pi(const KTable &T, double a) {
    const double k = rint(a * T.inv_2pi);
    return fma(-k, T.tp_lo, fma(-k, T.tp_hi, a));
}
