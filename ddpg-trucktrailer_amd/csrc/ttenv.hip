// ttenv.hip -- libttenv.so: batched truck-trailer backing environment for MI355X (gfx950).
//
// One thread per env, one fused kernel per vector step:
//   clip -> one Dormand-Prince step of the 6-state kinematic ODE (f64) -> 23-dim observation
//   -> reward_functionv1 reward with its carry -> termination flags -> (optional) in-kernel reset.
//
// Memory layout (DESIGN.md "Data layout"): the per-step state is an array of 64-env TILES, one tile per
// wavefront: 14 rows of 64 x 8 B (6 kinematic f64, 6 reward-carry f64, the start distance, and one row of
// {prev_steer f32, packed counters u32}) = 7168 contiguous bytes that the wave reads and writes with
// 512-byte row accesses at immediate offsets from a single base address.  Attributes that only the reset /
// pose-override path touches (start pose, per-env goal, per-env trailer length) live in separate SoA rows.
// The observation tile of a workgroup is staged through LDS so that each wave stores whole 16-byte vectors
// of the row-major [N,23] f32 matrix instead of 64 words 92 bytes apart.
//
// What is restated from the reference (paths relative to pain7576/ddpg-trucktrailer):
//   kinematic ODE            truck_trailer_sim/simv2.py:269-303
//   observation              truck_trailer_sim/simv2.py:103-181
//   reset / pose override    truck_trailer_sim/simv2.py:459-498, 263-267; DDPG/test.py:96-115
//   step, flags, done        truck_trailer_sim/simv2.py:499-545, 305-345
//   reward + carry           truck_trailer_sim/reward_functionv1.py:6-109, 144-506
//   integrator               scipy RK45 tableau (scipy/integrate/_ivp/rk.py), ONE step of h = dt
//
// Arithmetic shortcuts taken here (the CPU oracle takes none, so the parity tests check them):
//   * only the two headings feed back into the ODE's right-hand side, and they move by < 0.1 rad within a
//     step, so each stage's sin/cos is a small-angle rotation of the step's initial sin/cos (3 full-range
//     sincos per step instead of 18);
//   * the hitch-angle and obs[19..22] sin/cos come from angle-difference identities and (dx, dy)/distance;
//   * the three angles the reward reads back through float32 (np.arctan2 of f32 sin/cos) are reproduced
//     by their exactly-rounded value (float)(a + e), e the first-order effect of the f32 rounding;
//   * tanh(x) = (1 - t)/(1 + t), t = exp(-2|x|); cos(wrap(x)) = cos(x).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "ttenv.h"
#include "tthost.h"
#include "ttphilox.h"

namespace {

constexpr int OBS = TT_OBS_DIM;
#ifndef TT_BLOCK
#define TT_BLOCK 256
#endif
constexpr int BLOCK = TT_BLOCK;  // threads per workgroup (a multiple of the 64-env tile)
constexpr int TILE = 64;
constexpr double kPi = 3.14159265358979323846;
constexpr double kDeg = kPi / 180.0;

// rows of a hot tile [H_ROWS][TILE] (8 bytes per entry)
enum HotRow : int {
    H_PSI1 = 0, H_PSI2, H_X1, H_Y1, H_X2, H_Y2,      // kinematic state
    H_D3, H_D2, H_D1, H_PREV, H_CUM, H_CLOSEST,      // reward carry: distance window, backward sum, closest
    H_DINIT,                                         // |goal - start| (without the 1e-6 of reward_functionv1.py:35)
    H_MISC,                                          // {prev_steer f32, packed counters u32}
    H_ROWS
};
// cold SoA rows [C_ROWS][npad]
enum ColdRow : int { C_SX = 0, C_SY, C_SYAW, C_GX, C_GY, C_GYAW, C_SG, C_CG, C_L2, C_ROWS };

// packed per-env counters: steps [0,12) | max_episode_steps [12,24) | stage latches 2, 3 [24,26) | carry age [26,32)
//   steps      env.episode_steps (simv2.py:523-525): what the exploration tiers, the max-step penalty and the max-steps flag read;
//              a caller may write it (tt_env_set_steps; episode_replay_collectorv2.py:269) WITHOUT touching the reward carry;
//   stages     stages_achieved[1], [2] of the reward carry (reward_functionv1.py:338-367); [0] is written but never read (Q2:
//              the stage-1 bonus is paid on every step inside 5 m), so it is not kept;
//   carry age  step_count_for_backward_tracking of the reward carry (:57-60, :258), saturating at 63 -- only min(1, n / 50) is
//              read (:263) -- and 0 <=> `reward_state is None` (simv2.py:349): the next step builds the carry afresh.
__host__ __device__ inline uint32_t pk_steps(uint32_t p) { return p & 0xFFFu; }
__host__ __device__ inline uint32_t pk_max(uint32_t p) { return (p >> 12) & 0xFFFu; }
__host__ __device__ inline uint32_t pk_stages(uint32_t p) { return (p >> 24) & 0x3u; }
__host__ __device__ inline uint32_t pk_age(uint32_t p) { return p >> 26; }
__host__ __device__ inline uint32_t pk_make(uint32_t steps, uint32_t maxs, uint32_t stages, uint32_t age) {
    return (steps > 0xFFFu ? 0xFFFu : steps) | ((maxs > 0xFFFu ? 0xFFFu : maxs) << 12) | ((stages & 3u) << 24) |
           ((age > 63u ? 63u : age) << 26);
}

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

struct KParams {
    double v, v_over_L1, ho, h;
    double L2;
    double gx, gy, gyaw, sg, cg;
    double minx, maxx, miny, maxy;
    double cx, cy, inv_hx, inv_hy, inv_M;
    double max_steer, pos_thr, ori_thr, step_length, inv_step_length;
    double rlo[3], rhi[3];
    int extra_steps, fixed_max;
    unsigned term_mask;
    int npad;  // envs rounded up to a whole tile: row stride of the cold block
    int stateless;       // simv1.py:435: the reward carries nothing from step to step
    int pool_m;          // > 0: resets draw from pool[pool_m][3] instead of the box rlo..rhi
    int nt;              // 1: obs / reward / done leave as non-temporal stores (set by N: see nt_stores_for)
    const double *pool;
};

__device__ constexpr KTable kTable = make_table();

struct Info {
    double *comp;
    uint8_t *violation;
    uint8_t *flags;
};

struct Bufs {
    double *hot;         // [ntiles][H_ROWS][TILE]
    double *cold;        // [C_ROWS][npad]
    uint32_t *episodes;  // [npad] episode number of each env (keys the reset RNG)
    long long *counter;  // optional caller-owned count of vector steps (tt_env_set_step_counter), advanced by k_step
};

__device__ __forceinline__ double *hot_ptr(double *hot, int i) {
    return hot + (size_t)(i >> 6) * (H_ROWS * TILE) + (i & (TILE - 1));
}
__device__ __forceinline__ const double *hot_ptr(const double *hot, int i) {
    return hot + (size_t)(i >> 6) * (H_ROWS * TILE) + (i & (TILE - 1));
}

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

// ------------------------------------------------------------------------------------------
struct Goal {
    double gx, gy, sg, cg;
};

// 23-dim observation in f64 from the state and the sin/cos the caller already has (simv2.py:103-181).
__device__ __forceinline__ void observe(const KParams &P, const Goal &g, double x1, double y1, double x2, double y2,
                                        double s1, double c1, double s2, double c2, double sd, double cd, double dx,
                                        double dy, double cur, double inv_cur, float *of) {
    const double dxl = dx * c2 + dy * s2, dyl = -dx * s2 + dy * c2;
    of[0] = (float)((x1 - P.cx) * P.inv_hx); of[1] = (float)((y1 - P.cy) * P.inv_hy);
    of[2] = (float)s1; of[3] = (float)c1;
    of[4] = (float)((x2 - P.cx) * P.inv_hx); of[5] = (float)((y2 - P.cy) * P.inv_hy);
    of[6] = (float)s2; of[7] = (float)c2;
    of[8] = (float)(s1 * c2 - c1 * s2); of[9] = (float)(c1 * c2 + s1 * s2);
    of[10] = (float)sd; of[11] = (float)cd;
    of[12] = (float)((g.gx - P.cx) * P.inv_hx); of[13] = (float)((g.gy - P.cy) * P.inv_hy);
    of[14] = (float)g.sg; of[15] = (float)g.cg;
    of[16] = (float)fmin(fmax(cur * P.inv_M, 0.0), 1.0);
    of[17] = (float)fmin(fmax(dxl * P.inv_M, -1.0), 1.0);
    of[18] = (float)fmin(fmax(dyl * P.inv_M, -1.0), 1.0);
    of[19] = (float)(g.sg * c2 - g.cg * s2); of[20] = (float)(g.cg * c2 + g.sg * s2);
    // sin/cos of atan2(dy,dx) - (psi2 + pi); atan2(0,0) = 0
    of[21] = (float)(cur > 0.0 ? -dyl * inv_cur : s2);
    of[22] = (float)(cur > 0.0 ? -dxl * inv_cur : -c2);
}

// Store a workgroup's [nv,23] f32 observation tile, staged through LDS so the global stores are
// contiguous 16-byte vectors.  Every thread of the block must call this (barriers inside).
// nt: non-temporal stores -- at env counts whose per-step traffic is far beyond the caches, the 97 B per env-step that nobody
// re-reads before they are evicted anyway (observation, reward, done: ~half of all written bytes) stop displacing the state
// tiles on their way out: 278 -> 248 us per launch at 4 M envs (0.59 -> 0.66 of 8 TB/s), nothing at 65,536 / 1 M envs, where
// the policy's next launch finds the observations in L2 / the Infinity Cache (profiles/r03_nsweep.md).
__device__ inline void store_obs_tile(float *tile, const float *of, bool valid, float *obs, int block_first, int nv,
                                      const bool nt = false) {
    const int tid = threadIdx.x;
    if (valid) {
#pragma unroll
        for (int j = 0; j < OBS; ++j) tile[tid * OBS + j] = of[j];  // stride 23 words: conflict-free
    }
    __syncthreads();
    float *dst = obs + (size_t)block_first * OBS;
    const int total = nv * OBS;
    if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        const int nvec = total >> 2;
        const float4 *t4 = reinterpret_cast<const float4 *>(tile);
        float4 *d4 = reinterpret_cast<float4 *>(dst);
        if (nt) {
            using v4f = __attribute__((ext_vector_type(4))) float;
            for (int q = tid; q < nvec; q += BLOCK) {
                const float4 t = t4[q];
                __builtin_nontemporal_store(v4f{t.x, t.y, t.z, t.w}, reinterpret_cast<v4f *>(d4 + q));
            }
        } else {
            for (int q = tid; q < nvec; q += BLOCK) d4[q] = t4[q];
        }
        for (int q = (nvec << 2) + tid; q < total; q += BLOCK) dst[q] = tile[q];
    } else {
        for (int q = tid; q < total; q += BLOCK) dst[q] = tile[q];
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------
// one env in registers
struct Env {
    double psi1, psi2, x1, y1, x2, y2;      // kinematic state
    double d3, d2, d1, prev, cum, closest;  // reward carry
    double dinit;
    float psteer;
    uint32_t pk;
    Goal g;
    double gyaw, L2;
};

template <bool PER_ENV>
__device__ __forceinline__ void load_env(const KParams &P, const Bufs &b, int i, Env &e) {
    const double *h = hot_ptr(b.hot, i);
    e.psi1 = h[H_PSI1 * TILE]; e.psi2 = h[H_PSI2 * TILE];
    e.x1 = h[H_X1 * TILE]; e.y1 = h[H_Y1 * TILE]; e.x2 = h[H_X2 * TILE]; e.y2 = h[H_Y2 * TILE];
    e.d3 = h[H_D3 * TILE]; e.d2 = h[H_D2 * TILE]; e.d1 = h[H_D1 * TILE]; e.prev = h[H_PREV * TILE];
    e.cum = h[H_CUM * TILE]; e.closest = h[H_CLOSEST * TILE];
    e.dinit = h[H_DINIT * TILE];
    const uint2 m = *reinterpret_cast<const uint2 *>(h + H_MISC * TILE);
    e.psteer = __uint_as_float(m.x);
    e.pk = m.y;
    if (PER_ENV) {
        const double *c = b.cold + i;
        const size_t S = (size_t)P.npad;
        e.g.gx = c[C_GX * S]; e.g.gy = c[C_GY * S]; e.g.sg = c[C_SG * S]; e.g.cg = c[C_CG * S];
        e.gyaw = c[C_GYAW * S]; e.L2 = c[C_L2 * S];
    } else {
        e.g.gx = P.gx; e.g.gy = P.gy; e.g.sg = P.sg; e.g.cg = P.cg;
        e.gyaw = P.gyaw; e.L2 = P.L2;
    }
}

__device__ __forceinline__ void store_env(const Bufs &b, int i, const Env &e) {
    double *h = hot_ptr(b.hot, i);
    h[H_PSI1 * TILE] = e.psi1; h[H_PSI2 * TILE] = e.psi2;
    h[H_X1 * TILE] = e.x1; h[H_Y1 * TILE] = e.y1; h[H_X2 * TILE] = e.x2; h[H_Y2 * TILE] = e.y2;
    h[H_D3 * TILE] = e.d3; h[H_D2 * TILE] = e.d2; h[H_D1 * TILE] = e.d1; h[H_PREV * TILE] = e.prev;
    h[H_CUM * TILE] = e.cum; h[H_CLOSEST * TILE] = e.closest;
    *reinterpret_cast<uint2 *>(h + H_MISC * TILE) = make_uint2(__float_as_uint(e.psteer), e.pk);
}

// Place an env (in registers) at a start pose (simv2.py:481-496 / DDPG/test.py:96-115): trailer at the pose,
// truck L2 ahead, state rounded to float32 (simv2.py:489), episode cleared.  Writes the cold attributes.
// `of` (may be NULL) receives the first observation (steering 0).
__device__ inline void place_env(const KParams &P, const Bufs &b, int i, Env &e, double sx, double sy, double syaw,
                                 const Goal &g, double gyaw, double L2, float *of) {
    const KTable &T = kTable;
    double ss, cs;
    tt_sincos(T, syaw, ss, cs);
    e.psi1 = e.psi2 = (double)(float)syaw;
    e.x1 = (double)(float)(sx + L2 * cs);
    e.y1 = (double)(float)(sy + L2 * ss);
    e.x2 = (double)(float)sx;
    e.y2 = (double)(float)sy;
    const double ddx = g.gx - sx, ddy = g.gy - sy;
    e.dinit = sqrt(ddx * ddx + ddy * ddy);
    e.g = g; e.gyaw = gyaw; e.L2 = L2;
    const int maxs = P.fixed_max > 0 ? P.fixed_max : (int)(e.dinit / P.step_length) + P.extra_steps;
    e.pk = pk_make(0u, (uint32_t)maxs, 0u, 0u);
    // carry rows are re-initialised by the first step (carry age 0); keep them finite
    e.d3 = e.d2 = e.d1 = e.prev = e.closest = e.dinit; e.cum = 0.0; e.psteer = 0.0f;
    hot_ptr(b.hot, i)[H_DINIT * TILE] = e.dinit;  // read-only for the step kernel: store_env() does not write it
    double *c = b.cold + i;
    const size_t S = (size_t)P.npad;
    c[C_SX * S] = sx; c[C_SY * S] = sy; c[C_SYAW * S] = syaw;
    c[C_GX * S] = g.gx; c[C_GY * S] = g.gy; c[C_GYAW * S] = gyaw; c[C_SG * S] = g.sg; c[C_CG * S] = g.cg;
    c[C_L2 * S] = L2;
    if (of) {
        double sp, cp;
        tt_sincos(T, e.psi1, sp, cp);
        const double dx = g.gx - e.x2, dy = g.gy - e.y2;
        const double cur = sqrt(dx * dx + dy * dy);
        observe(P, g, e.x1, e.y1, e.x2, e.y2, sp, cp, sp, cp, 0.0, 1.0, dx, dy, cur, cur > 0.0 ? 1.0 / cur : 0.0, of);
    }
}

// start pose of episode number `episode` of env `env` under reset seed `seed`: a pure function of the three
__device__ inline void random_pose(const KParams &P, uint64_t seed, uint32_t env, uint32_t episode, double &sx, double &sy,
                                   double &syaw) {
    uint32_t r[4];
    philox4x32(env, episode, 0u, 0x7452u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    if (P.pool_m > 0) {  // pre-filtered poses (simv1's Dubins-feasible starts)
        const double *q = P.pool + 3 * (size_t)(r[3] % (uint32_t)P.pool_m);
        sx = q[0]; sy = q[1]; syaw = q[2];
        return;
    }
    sx = P.rlo[0] + (P.rhi[0] - P.rlo[0]) * u01(r[0]);  // draw order x, y, yaw (simv2.py:331-333)
    sy = P.rlo[1] + (P.rhi[1] - P.rlo[1]) * u01(r[1]);
    syaw = P.rlo[2] + (P.rhi[2] - P.rlo[2]) * u01(r[2]);
}

__device__ __forceinline__ float random_action(uint64_t seed, uint32_t env, uint32_t steps, uint32_t episode) {
    uint32_t r[4];
    philox4x32(env, steps, episode, 0xAC71u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    return (float)((2.0 * u01(r[0]) - 1.0) * (kPi / 4));
}

struct StepOut {
    double total, c_prog, c_head, c_orient, staged, safety, explore, final_bonus, back, c_smooth, budget;
    uint32_t viol, flags;
    bool done;
};

// env.step for one env held in registers (simv2.py:499-545 + reward_functionv1.py:442-506)
__device__ __forceinline__ void step_env(const KParams &P, Env &e, float action, float *of, StepOut &o) {
    const KTable &T = kTable;
    // ---- simv2.py:504-505: clip in f64 against np.radians(45)
    const double delta = fmin(fmax((double)action, -P.max_steer), P.max_steer);
    double sd, cd;
    tt_sincos(T, delta, sd, cd);
    const double w1 = P.v_over_L1 * (sd / cd);  // truck yaw rate, constant over the step

    // ---- one Dormand-Prince step (scipy RK45 tableau).  Positions do not feed back, so they are accumulated
    // straight into their B-weighted sums; every stage's sin/cos is a small rotation of the initial ones.
    const double h = P.h, v = P.v, vL2 = P.v / e.L2, hoL2 = P.ho / e.L2, how1 = P.ho * w1;
    double sp1, cp1, sp2, cp2;
    tt_sincos(T, e.psi1, sp1, cp1);
    tt_sincos(T, e.psi2, sp2, cp2);
    const double beta = h * w1;
    double k2[6];
    double ax1 = 0.0, ay1 = 0.0, ax2 = 0.0, ay2 = 0.0, apsi2 = 0.0;
    double s1 = sp1, c1 = cp1;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        double s2 = sp2, c2 = cp2;
        if (s > 0) {
            double acc = T.A[s][0] * k2[0];
#pragma unroll
            for (int j = 1; j < s; ++j) acc = fma(T.A[s][j], k2[j], acc);
            double sb, cb, sg2, cg2;
            tt_sincos_small(T, T.C[s] * beta, sb, cb);
            tt_sincos_small(T, h * acc, sg2, cg2);
            s1 = sp1 * cb + cp1 * sb; c1 = cp1 * cb - sp1 * sb;
            s2 = sp2 * cg2 + cp2 * sg2; c2 = cp2 * cg2 - sp2 * sg2;
        }
        const double sth = s1 * c2 - c1 * s2, cth = c1 * c2 + s1 * s2;
        const double v2 = v * cth + how1 * sth;
        k2[s] = vL2 * sth - hoL2 * w1 * cth;
        if (s != 1) {  // B[1] = 0
            const double bs = T.B[s];
            apsi2 = fma(bs, k2[s], apsi2);
            ax1 = fma(bs, v * c1, ax1);
            ay1 = fma(bs, v * s1, ay1);
            ax2 = fma(bs, v2 * c2, ax2);
            ay2 = fma(bs, v2 * s2, ay2);
        }
    }
    // stage 6 sits at c = 1: its truck heading IS the new truck heading, so (s1, c1) carry over
    e.psi1 += beta;
    const double dpsi2 = h * apsi2;
    e.psi2 += dpsi2;
    e.x1 = fma(h, ax1, e.x1); e.y1 = fma(h, ay1, e.y1); e.x2 = fma(h, ax2, e.x2); e.y2 = fma(h, ay2, e.y2);
    double s2, c2;
    {
        double sg2, cg2;
        tt_sincos_small(T, dpsi2, sg2, cg2);
        s2 = sp2 * cg2 + cp2 * sg2; c2 = cp2 * cg2 - sp2 * sg2;
    }

    // ---- observation (simv2.py:519), cast to f32 like np.array(..., dtype=float32)
    const double dx = e.g.gx - e.x2, dy = e.g.gy - e.y2;
    const double cur = sqrt(dx * dx + dy * dy);
    const uint32_t pk = e.pk;
    const uint32_t steps = pk_steps(pk) + 1u;  // episode_steps is incremented before the reward (simv2.py:523)
    uint32_t stages = pk_stages(pk);
    const double init = e.dinit + 1e-6;

    // The reward's three tanh -- dynamic weights (:189-238): tanh(7(jp - 0.3)); progress (:144-187):
    // tanh(prev - cur), tanh((hist[0] - cur)/2) -- are (1 - t)/(1 + t), t = exp(-2|x|).  Two of them, 1/cur
    // and 1/init share ONE division through the product of the denominators.
    const bool first = pk_age(pk) == 0u || P.stateless != 0;  // reward_state is None (:40-76)
    const uint32_t age = first ? 1u : pk_age(pk) + 1u;         // step_count_for_backward_tracking after this step (:258)
    const double prev = first ? cur : e.prev, d3 = first ? cur : e.d3, d1 = first ? cur : e.d1;
    const double inst = prev - cur;
    const double net = (d3 - cur) * 0.5;
    const double t_i = tt_exp_neg(T, -2.0 * fabs(inst)), t_n = tt_exp_neg(T, -2.0 * fabs(net));
    const double q_i = 1.0 + t_i, q_n = 1.0 + t_n;
    const double cur_s = cur > 0.0 ? cur : 1.0;
    const double qq = q_i * q_n, ci = cur_s * init;
    const double r_all = 1.0 / (qq * ci);
    const double inv_cur = cur > 0.0 ? r_all * (qq * init) : 0.0;
    const double inv_init = r_all * (qq * cur_s);
    const double th = copysign((1.0 - t_i) * (r_all * (ci * q_n)), inst);
    const double tn = copysign((1.0 - t_n) * (r_all * (ci * q_i)), net);

    observe(P, e.g, e.x1, e.y1, e.x2, e.y2, s1, c1, s2, c2, sd, cd, dx, dy, cur, inv_cur, of);

    // ---- reward (reward_functionv1.py:442-506)
    // int(initial_distance / 0.40096) + 75 (:38): the quotient by one multiplication, and by the real division (what
    // numpy does) only where the two could truncate differently -- next to an integer (wave-uniform, almost never)
    const double rq = init * P.inv_step_length;
    int rmax = (int)rq;
    if (__any(fabs(rq - rint(rq)) <= 1e-11 * rq)) rmax = (int)(init / P.step_length);
    rmax += P.extra_steps;
    const float steer_now = tt_atan2_readback(delta, sd, cd, of[10], of[11]);  // np.arctan2(obs[10], obs[11]) (:37)
    if (first) {
        e.cum = 0.0;
        e.closest = cur;
        e.psteer = steer_now;
        stages = 0u;
    } else if (cur < e.closest) {
        e.closest = cur;
    }
    const double jp = fmin(fmax((init - cur) * inv_init, 0.0), 1.0);
    const double wa = 7.0 * (jp - 0.3);
    const double t_w = tt_exp_neg(T, -2.0 * fabs(wa));
    const double tw = copysign((1.0 - t_w) / (1.0 + t_w), wa);
    const double w_orient = (tw + 1.0) * 0.5;
    const double w_head = 1.0 - w_orient;
    const bool mono = (d1 >= prev) && (prev >= cur);
    const double progress = (inst > 0.0 ? th : th * 0.5) + tn * 0.5 + (mono ? 0.2 : 0.0);
    // heading (:285-309): cos(atan2(dy,dx) - (co + pi)) with co = np.arctan2(obs[6], obs[7]) in f32.
    // co = wrap(psi2) + eps with |eps| ~ 1e-7, so its sin/cos are a rotation of (s2, c2) by eps.
    double heading;
    {
        const double w2 = tt_wrap_pi(T, e.psi2);
        const double eps = (double)tt_atan2_readback(w2, s2, c2, of[6], of[7]) - w2;
        const double half = 1.0 - 0.5 * eps * eps;
        const double sco = s2 * half + c2 * eps, cco = c2 * half - s2 * eps;
        heading = cur > 0.0 ? -(dx * cco + dy * sco) * inv_cur : -cco;
    }
    // orientation (:311-324): f32 * 15.0 stays f32 in numpy
    const float orient15 = of[20] * 15.0f;
    // staged bonuses (:338-367) and success: only within 5 m of the goal (wave-uniform skip otherwise)
    double staged = 0.0;
    bool at_goal = false;
    if (__any(cur <= 5.0)) {
        // |np.arctan2(obs[19], obs[20])| with obs[19], obs[20] = sin, cos(goalyaw - psi2)
        const double oa = tt_wrap_pi(T, e.gyaw - e.psi2);
        const double ori_err = (double)fabsf(tt_atan2_readback(oa, e.g.sg * c2 - e.g.cg * s2, e.g.cg * c2 + e.g.sg * s2,
                                                               of[19], of[20]));
        if (cur <= 5.0) staged += 10.0;   // every step, no latch (Q2)
        if (cur <= 2.0 && ori_err <= 45.0 * kDeg && !(stages & 1u)) { staged += 25.0; stages |= 1u; }
        at_goal = cur <= P.pos_thr && ori_err <= P.ori_thr;
        if (at_goal && !(stages & 2u)) { staged += 100.0; stages |= 2u; }
    }
    // safety (:369-421)
    double safety = 0.0;
    uint32_t viol = TT_V_NONE;
    const double hitch = fabs(e.psi1 - e.psi2);
    if (hitch > 85.0 * kDeg) { safety += -500.0; viol = TT_V_JACKKNIFE; }
    else if (hitch > 70.0 * kDeg) { safety += -50.0; viol = TT_V_JACKKNIFE_WARNING; }
    const double lox = fmin(e.x1, e.x2), hix = fmax(e.x1, e.x2), loy = fmin(e.y1, e.y2), hiy = fmax(e.y1, e.y2);
    const bool outside = lox < P.minx || hix > P.maxx || loy < P.miny || hiy > P.maxy;
    if (lox < P.minx - 2.0 || hix > P.maxx + 2.0 || loy < P.miny - 2.0 || hiy > P.maxy + 2.0) {
        safety += -500.0; viol = TT_V_MAJOR_BOUNDARY;
    } else if (outside) {
        safety += -50.0; viol = TT_V_MINOR_BOUNDARY;
    }
    const bool passed = e.g.gy > e.y2;
    if (passed) { safety += -500.0; viol = TT_V_PAST_THE_GOAL; }
    if ((int)steps >= rmax) { safety += -500.0; viol = TT_V_MAX_STEP; }
    const bool excessive = cur > e.closest + 6.0;  // :120-124
    if (excessive) { safety += -500.0; viol = TT_V_EXCESSIVE_BACKWARD; }
    // exploration (:423-439)
    const double explore = (double)steps < rmax * 0.5 ? 4.0 : ((double)steps < rmax * 0.8 ? 2.0 : 0.0);
    // backward-movement budget (:240-283)
    e.cum += fmax(0.0, cur - prev);
    const double budget = 5.0 * fmin(1.0, (double)age * 0.02);  // step_count_for_backward_tracking (stateless: always 1)
    const double excess = fmax(0.0, e.cum - budget);
    double back = 0.0;
    if (__any(excess > 0.0)) back = excess > 0.0 ? -(excess * sqrt(excess)) * 0.5 : 0.0;
    // smoothness against the episode's FIRST steering (:326-335; previous_steering is never refreshed)
    const double smooth = (double)fabsf(steer_now - e.psteer) * (1.0 / (90.0 * kDeg));
    o.final_bonus = at_goal ? 200.0 : 0.0;

    o.c_prog = progress * 15.0; o.c_head = heading * 15.0 * w_head;
    o.c_orient = (double)orient15 * w_orient; o.c_smooth = smooth * -25.0;
    o.staged = staged; o.safety = safety; o.explore = explore; o.back = back; o.budget = budget;
    o.total = 0.0 + o.c_prog + o.c_head + o.c_orient + staged + safety + explore + back + o.c_smooth + o.final_bonus;

    // ---- flags (simv2.py:528-541)
    uint32_t fl = 0u;
    if (hitch > 90.0 * kDeg) fl |= TT_F_JACKKNIFE;
    if (outside) fl |= TT_F_OUT_OF_MAP;
    if (steps >= pk_max(pk)) fl |= TT_F_MAX_STEPS;
    if (at_goal) fl |= TT_F_GOAL_REACHED | TT_F_SUCCESS;
    if (passed) fl |= TT_F_GOAL_PASSED;
    if (excessive) fl |= TT_F_EXCESSIVE_BACK;
    o.flags = fl; o.viol = viol;
    o.done = (fl & P.term_mask) != 0u;

    // carry for the next step: window [hist1..hist4] <- [hist2, hist3, hist4, cur]
    e.d3 = first ? cur : e.d2; e.d2 = d1; e.d1 = prev; e.prev = cur;
    e.pk = pk_make(steps, pk_max(pk), stages, age);
}

__device__ __forceinline__ void write_info(const Info &info, size_t N, int i, const Env &e, const StepOut &o) {
    if (info.comp) {
        double *c = info.comp + i;
        c[TT_I_TOTAL * N] = o.total; c[TT_I_PROGRESS * N] = o.c_prog; c[TT_I_HEADING * N] = o.c_head;
        c[TT_I_ORIENT * N] = o.c_orient; c[TT_I_STAGED * N] = o.staged; c[TT_I_SAFETY * N] = o.safety;
        c[TT_I_EXPLORE * N] = o.explore; c[TT_I_FINAL * N] = o.final_bonus; c[TT_I_BACKWARD * N] = o.back;
        c[TT_I_SMOOTH * N] = o.c_smooth; c[TT_I_CUMBACK * N] = e.cum; c[TT_I_BUDGET * N] = o.budget;
    }
    if (info.violation) info.violation[i] = (uint8_t)o.viol;
    if (info.flags) info.flags[i] = (uint8_t)o.flags;
}

// ------------------------------------------------------------------------------------------
// the vector step.  RANDOM_POLICY: the action is drawn in-kernel (BASELINE.json config 2), keyed by
// (policy seed, env, step-in-episode, episode number) so that a captured hipGraph replays correctly.
#ifdef TT_STAMPS
#include "ttstamps.h"
__device__ unsigned long long g_stepblk[1024][2];
__device__ TTLog g_log_step;
#endif
// Episode log (tt_env_set_episode_log; DESIGN.md "Episode log"): one device block, laid out as
//   header  [LOG_HDR] u64: the write index, the launch count, the exit ticket and the outcome counters [TT_LOG_NCOUNTS], each
//           group on a 128-byte line of its own (atomics on one line are serialised where they are performed)
//   records ret f64 [cap] | end_step i64 [cap] | len i32 [cap] | lane i32 [cap] | flags u8 [cap] | success u8 [cap] (to 8 B)
//   accumulator f64 [npad]: the return of the running episode of every lane, summed in step order
// so that a checkpoint of the log is one copy of the block.  The kernels get the header, the accumulator and the capacity
// (6 SGPRs, not one pointer per column: the step kernels have none to spare) and find the columns from them.
enum LogHdr : int { LG_WRITTEN = 0, LG_LAUNCHES = 16, LG_TICKET = 32, LG_COUNTS = 48, LOG_HDR = 64 };
static_assert(LG_COUNTS + TT_LOG_NCOUNTS <= LOG_HDR, "episode-log header");

struct EpLog {
    unsigned long long *hdr;
    double *acc;
    unsigned long long capacity;
};
struct LogCols {
    double *ret;
    long long *end_step;
    int32_t *len, *lane;
    uint8_t *flags, *success;
};
__host__ __device__ inline LogCols log_cols(const EpLog &lg) {
    const size_t cap = (size_t)lg.capacity;
    char *p = reinterpret_cast<char *>(lg.hdr + LOG_HDR);
    LogCols c;
    c.ret = reinterpret_cast<double *>(p); p += sizeof(double) * cap;
    c.end_step = reinterpret_cast<long long *>(p); p += sizeof(long long) * cap;
    c.len = reinterpret_cast<int32_t *>(p); p += sizeof(int32_t) * cap;
    c.lane = reinterpret_cast<int32_t *>(p); p += sizeof(int32_t) * cap;
    c.flags = reinterpret_cast<uint8_t *>(p); p += cap;
    c.success = reinterpret_cast<uint8_t *>(p);
    return c;
}
// bytes of the block before the accumulator
__host__ __device__ inline size_t log_records_bytes(unsigned long long cap) {
    return (sizeof(unsigned long long) * LOG_HDR + (2 * sizeof(double) + 2 * sizeof(int32_t) + 2) * (size_t)cap + 7) & ~(size_t)7;
}

// The detailed log (TT_LOG_DETAIL; k_step_tally) extends the same block:
//   header  word LG_DETAIL holds the flags the log was enabled with, so that an exported blob says what it is
//   records after the plain columns: comp f64 [TT_LOG_NCOMP, cap] (the episode's sum of each reward term, TT_I_PROGRESS ..
//           TT_I_SMOOTH) | start f64 [3, cap] (the episode's start pose x, y, yaw)
//   accumulators after the return's row [npad]: the term sums f64 [npad / TILE][TT_LOG_NCOMP][TILE] (tally_acc)
// Nothing of the plain layout moves but the accumulator, which EpLog points at.
constexpr int LG_DETAIL = LG_COUNTS + TT_LOG_NCOUNTS;
static_assert(LG_DETAIL < LOG_HDR, "episode-log header");
static_assert(TT_LOG_NCOMP == TT_I_SMOOTH - TT_I_PROGRESS + 1, "detailed episode log: one sum per reward term");
__host__ __device__ inline size_t tally_records_bytes(unsigned long long cap) {
    return sizeof(double) * (TT_LOG_NCOMP + 3) * (size_t)cap;
}
struct TallyCols {
    double *comp, *start;
};
__host__ __device__ inline TallyCols tally_cols(const EpLog &lg) {
    double *p = reinterpret_cast<double *>(reinterpret_cast<char *>(lg.hdr) + log_records_bytes(lg.capacity));
    return TallyCols{p, p + TT_LOG_NCOMP * (size_t)lg.capacity};
}

__device__ __forceinline__ unsigned long long atomic_add_agent(unsigned long long *p, unsigned long long v) {
    return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The finishers of one wave append their records with ONE atomic on the write index (lane 0: the valid lanes of a wave are a
// prefix, so lane 0 is active whenever any lane is); each finisher's slot is the base plus the number of finishers below it
// (v_mbcnt).  Slots at or past the capacity are not stored, the index keeps counting.  Outcome counters: one integer atomic per
// outcome that has a finisher in the wave.  Called by every active lane of the wave (the ballots need them all) when the wave
// has finishers (fin = __ballot(done) != 0); returns the wave's base slot.
// The record's end_step is the launch number, read in log_write and at the workgroup's exit: both before the workgroup's exit
// ticket (below, TT_STEP_LAUNCH_COUNT), so before the last workgroup of the launch advances it.
__device__ __forceinline__ unsigned long long log_reserve(const EpLog &lg, unsigned long long fin, bool done, uint32_t flags,
                                                          bool succ) {
    const bool lead = __lane_id() == 0;
    unsigned long long base = 0;
    if (lead) base = atomic_add_agent(lg.hdr + LG_WRITTEN, (unsigned long long)__popcll(fin));
    // counters one ballot at a time (nine masks held at once cost 18 SGPRs, and the kernel then spilled)
    if (lead) atomic_add_agent(lg.hdr + LG_COUNTS, (unsigned long long)__popcll(fin));
    const unsigned long long ns = __ballot(succ);
    if (lead && ns) atomic_add_agent(lg.hdr + LG_COUNTS + 1, (unsigned long long)__popcll(ns));
#pragma unroll
    for (int f = 0; f < TT_LOG_NCOUNTS - 2; ++f) {
        const unsigned long long m = __ballot(done && ((flags >> f) & 1u));
        if (lead && m) atomic_add_agent(lg.hdr + LG_COUNTS + 2 + f, (unsigned long long)__popcll(m));
    }
    return ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(base >> 32)) << 32) |
           (unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)base);
}

__device__ __forceinline__ unsigned long long log_slot(unsigned long long base, unsigned long long fin) {
    return base + __builtin_amdgcn_mbcnt_hi((uint32_t)(fin >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fin, 0u));
}

// the plain columns of record `slot` (< capacity)
__device__ __forceinline__ void log_write(const EpLog &lg, unsigned long long slot, int i, uint32_t flags, bool succ,
                                          uint32_t len, double ret) {
    const LogCols c = log_cols(lg);
    c.ret[slot] = ret;
    c.end_step[slot] = (long long)__hip_atomic_load(lg.hdr + LG_LAUNCHES, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c.len[slot] = (int32_t)len;
    c.lane[slot] = i;
    c.flags[slot] = (uint8_t)flags;
    c.success[slot] = succ ? 1 : 0;
}

__device__ __forceinline__ void log_append(const EpLog &lg, int i, bool done, uint32_t flags, bool success, uint32_t len,
                                           double ret) {
    const unsigned long long fin = __ballot(done);
    if (!fin) return;
    const bool succ = done && success;
    const unsigned long long base = log_reserve(lg, fin, done, flags, succ);
    if (done) {
        const unsigned long long slot = log_slot(base, fin);
        if (slot < lg.capacity) log_write(lg, slot, i, flags, succ, len, ret);
    }
}

// ---- the text that k_step, k_step_log and k_step_tally hold word for word, written ONCE ----
// Function-like MACROS, not functions, for the reason csrc/ttlearn_sites.h gives: with k_step's body in a common inlined function
// the register allocation of 8 of its 16 variants changed; as pasted text every variant of the three kernels keeps its .text byte
// for byte (python -m ddpg_trucktrailer_amd.kernel_resources --text before.so after.so: the gate of every change here that is not
// meant to change a kernel).  The pieces use the kernels' argument names (P, n, b, action, action_out, obs, reward, done, info,
// seed, policy_seed, cursor, lg) and the template arguments as they stand; what a piece declares it declares in the scope it is
// pasted into, and the ORDER of the declarations is each kernel's own.  What differs stays written out at the sites: the LDS tile's
// declaration, k_step's TT_STAMPS and TT_DBG_STEP_MEM_ONLY blocks (no #ifdef inside a macro), the load of the running return in
// front of the sched_barrier, step_env, k_step_tally's read of the start pose, and log_append / tally_append.
//
// Head: ring addressing, the lane's index, the count of vector steps.  Declares block_first, i, valid, nv, of.
#define TT_STEP_HEAD()                                                                                                                  \
    if (cursor) { /* tt_env_step_ring: obs / reward / done are the ring's bases, the slots come from the cursor */                      \
        obs += (size_t)cursor[1] * n * OBS;                                                                                             \
        reward += (size_t)cursor[0] * n;                                                                                                \
        done += (size_t)cursor[0] * n;                                                                                                  \
    }                                                                                                                                   \
    const int block_first = blockIdx.x * BLOCK;                                                                                         \
    const int i = block_first + threadIdx.x;                                                                                            \
    const bool valid = i < n;                                                                                                           \
    const int nv = min(BLOCK, n - block_first);                                                                                         \
    float of[OBS];                                                                                                                      \
                                                                                                                                        \
    if (b.counter && i == 0) *b.counter += 1 /* one more vector step stored (read by later launches only) */
// Loads, in front of the site's __builtin_amdgcn_sched_barrier(0).  A lone wave per SIMD hides no latency: every load of the step is
// requested THERE, in one burst (one trip to L2 / the Infinity Cache instead of the four or five the scheduler otherwise spreads
// through the arithmetic by sinking each load next to its first use).  Declares e and a.
#define TT_STEP_LOADS()                                                                                                                 \
    Env e;                                                                                                                              \
    load_env<PER_ENV>(P, b, i, e);                                                                                                      \
    float a = 0.f;                                                                                                                      \
    if (!RANDOM_POLICY) a = action[i]
// Act, behind the sched_barrier: the in-kernel random action
#define TT_STEP_ACT()                                                                                                                   \
    if (RANDOM_POLICY) {                                                                                                                \
        a = random_action(policy_seed, (uint32_t)i, pk_steps(e.pk), b.episodes[i]);                                                     \
        if (action_out) action_out[i] = a;                                                                                              \
    }
// Out: reward, done and the info rows of StepOut o
#define TT_STEP_OUT()                                                                                                                   \
    if (P.nt) {                                                                                                                         \
        __builtin_nontemporal_store((float)o.total, reward + i);                                                                        \
        __builtin_nontemporal_store((uint8_t)(o.done ? 1 : 0), done + i);                                                               \
    } else {                                                                                                                            \
        reward[i] = (float)o.total;                                                                                                     \
        done[i] = o.done ? 1 : 0;                                                                                                       \
    }                                                                                                                                   \
    if (INFO) write_info(info, (size_t)n, i, e, o)
// Reset: a finished lane's next episode, and the env's rows
#define TT_STEP_RESET()                                                                                                                 \
    if (AUTO_RESET && o.done) {                                                                                                         \
        const uint32_t ep = b.episodes[i] + 1u;                                                                                         \
        b.episodes[i] = ep;                                                                                                             \
        double sx, sy, syaw;                                                                                                            \
        random_pose(P, seed, (uint32_t)i, ep, sx, sy, syaw);                                                                            \
        const Goal g0{P.gx, P.gy, P.sg, P.cg};                                                                                          \
        place_env(P, b, i, e, sx, sy, syaw, g0, P.gyaw, e.L2, of);                                                                      \
    }                                                                                                                                   \
    store_env(b, i, e)
// Return (the two log kernels): the lane's running return `ret`, summed in step order.  Declares len (the record is written after
// the reset: fewer registers live across it).
#define TT_STEP_RETURN()                                                                                                                \
    ret += o.total;                                                                                                                     \
    lg.acc[i] = o.done ? 0.0 : ret; /* a finished lane's next episode (auto-reset or not) starts from 0 */                              \
    const uint32_t len = pk_steps(e.pk)
// Launch count (the two log kernels), after store_obs_tile: behind its barrier every wave of this workgroup has read the count (its
// records hold it), so the workgroup's exit ticket follows its reads, and the workgroup that draws the last ticket follows every
// workgroup's.  Nothing waits and nothing is published to other workgroups of this launch, so the atomics are relaxed (an acq_rel
// ticket wrote back and invalidated the L2 in every workgroup: 10 -> 78 us per launch at N = 65536).
#define TT_STEP_LAUNCH_COUNT()                                                                                                          \
    if (threadIdx.x == 0) {                                                                                                             \
        const unsigned long long launch = __hip_atomic_load(lg.hdr + LG_LAUNCHES, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          \
        const unsigned long long t = atomic_add_agent(lg.hdr + LG_TICKET, 1ull);                                                        \
        if (t == gridDim.x - 1u) { /* the last workgroup of the launch; the next launch reads the count */                              \
            __hip_atomic_store(lg.hdr + LG_TICKET, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                                   \
            __hip_atomic_store(lg.hdr + LG_LAUNCHES, launch + 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                        \
        }                                                                                                                               \
    }

template <bool PER_ENV, bool INFO, bool AUTO_RESET, bool RANDOM_POLICY>
__global__ __launch_bounds__(BLOCK) void k_step(const KParams P, const int n, const Bufs b,
                                                const float *__restrict__ action, float *__restrict__ action_out,
                                                float *__restrict__ obs, float *__restrict__ reward,
                                                uint8_t *__restrict__ done, const Info info, const uint64_t seed,
                                                const uint64_t policy_seed, const int *__restrict__ cursor) {
    __shared__ __attribute__((aligned(16))) float tile[BLOCK * OBS];
#ifdef TT_STAMPS      // diagnostic build: wall clock (100 MHz) at the begin and end of every workgroup (tools/step_timeline.py)
    if (threadIdx.x == 0 && blockIdx.x < 1024) g_stepblk[blockIdx.x][0] = wall_clock64();
#endif
    TT_STEP_HEAD();
    if (valid) {
        TT_STEP_LOADS();
        __builtin_amdgcn_sched_barrier(0);
        TT_STEP_ACT();
        StepOut o;
#ifdef TT_DBG_STEP_MEM_ONLY      // diagnostic build (wrong results): the step's memory traffic without its arithmetic
        o = StepOut{};
        o.total = e.psi1 + a; o.done = false;
        e.psi1 += 1e-9; e.psi2 += e.x1 * 1e-12; e.d3 = e.d2; e.d2 = e.d1; e.d1 = e.prev; e.cum += e.closest * 1e-12;
#pragma unroll
        for (int j = 0; j < OBS; ++j) of[j] = (float)(e.x2 + j);
#else
        step_env(P, e, a, of, o);
#endif
        TT_STEP_OUT();
        TT_STEP_RESET();
    }
    store_obs_tile(tile, of, valid, obs, block_first, nv, P.nt != 0);
#ifdef TT_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0 && blockIdx.x < 1024) {
        g_stepblk[blockIdx.x][1] = wall_clock64();
        tt_log_add(g_log_step, g_stepblk[blockIdx.x][0], g_stepblk[blockIdx.x][1]);
    }
#endif
}

// k_step with the episode log on: the same step -- k_step's text, the TT_STEP_* pieces above --, plus the lane's running return
// (loaded in the step's load burst, TT_STEP_RETURN), the append of the finishers' records and the launch count
// (TT_STEP_LAUNCH_COUNT).  A kernel of its own, not a fifth template argument of k_step (that would rename every k_step variant);
// and the shared text is pasted, not called: a common inlined body changed the register allocation of 8 of k_step's 16 variants
// (DESIGN.md "Episode log", section 35).
template <bool PER_ENV, bool INFO, bool AUTO_RESET, bool RANDOM_POLICY>
__global__ __launch_bounds__(BLOCK) void k_step_log(const KParams P, const int n, const Bufs b,
                                                    const float *__restrict__ action, float *__restrict__ action_out,
                                                    float *__restrict__ obs, float *__restrict__ reward,
                                                    uint8_t *__restrict__ done, const Info info, const uint64_t seed,
                                                    const uint64_t policy_seed, const int *__restrict__ cursor,
                                                    const EpLog lg) {
    __shared__ __attribute__((aligned(16))) float tile[BLOCK * OBS];
    TT_STEP_HEAD();
    if (valid) {
        TT_STEP_LOADS();
        double ret = lg.acc[i];
        __builtin_amdgcn_sched_barrier(0);
        TT_STEP_ACT();
        StepOut o;
        step_env(P, e, a, of, o);
        TT_STEP_OUT();
        TT_STEP_RETURN();
        TT_STEP_RESET();
        log_append(lg, i, o.done, o.flags, o.final_bonus > 0.0, len, ret);
    }
    store_obs_tile(tile, of, valid, obs, block_first, nv, P.nt != 0);
    TT_STEP_LAUNCH_COUNT();
}

// The detailed log's part of a step (k_step_tally), called by every active lane after the reset and store_env, as log_append is:
// the nine term sums are added into their accumulators (loaded here, not in the step's load burst: nine f64 held across step_env
// do not fit the register budget) and a finisher's record gets the plain columns, the sums and the start pose (s0, s1, s2), read
// by the kernel before the reset overwrote it.  Each sum is the f64 term added in step order, as the return is, and not contracted
// into the products step_env forms the terms from: a sum equals the host's sum of that info.comp row.
// The term accumulators are tiled like the hot rows, [npad / TILE][TT_LOG_NCOMP][TILE]: a lane's nine rows sit at constant offsets
// (fewer address registers than nine rows of stride npad).
__device__ __forceinline__ double *tally_acc(const EpLog &lg, int npad, int i) {
    return lg.acc + npad + (size_t)(i >> 6) * (TT_LOG_NCOMP * TILE) + (i & (TILE - 1));
}

__device__ __forceinline__ void tally_append(const KParams &P, const EpLog &lg, int i, const StepOut &o, uint32_t len, double ret,
                                             double s0, double s1, double s2) {
#pragma clang fp contract(off)
    double *acc = tally_acc(lg, P.npad, i);
    double sum[TT_LOG_NCOMP];
#pragma unroll
    for (int c = 0; c < TT_LOG_NCOMP; ++c) sum[c] = acc[c * TILE];
    const unsigned long long fin = __ballot(o.done);
    const bool succ = o.done && o.final_bonus > 0.0;
    unsigned long long slot = ~0ull;
    if (fin) {
        const unsigned long long base = log_reserve(lg, fin, o.done, o.flags, succ);
        if (o.done) slot = log_slot(base, fin);
    }
    const double term[TT_LOG_NCOMP] = {o.c_prog, o.c_head, o.c_orient, o.staged, o.safety,
                                       o.explore, o.final_bonus, o.back, o.c_smooth};
#pragma unroll
    for (int c = 0; c < TT_LOG_NCOMP; ++c) {
        sum[c] += term[c];
        acc[c * TILE] = o.done ? 0.0 : sum[c];
    }
    if (o.done && slot < lg.capacity) {
        log_write(lg, slot, i, o.flags, succ, len, ret);
        const TallyCols t = tally_cols(lg);
        const size_t cap = (size_t)lg.capacity;
#pragma unroll
        for (int c = 0; c < TT_LOG_NCOMP; ++c) t.comp[c * cap + slot] = sum[c];
        t.start[slot] = s0;
        t.start[cap + slot] = s1;
        t.start[2 * cap + slot] = s2;
    }
}

// k_step_log with the detailed log on: the same TT_STEP_* pieces in the same order -- the step, the return, the launch count and
// its exit ticket --, with the read of the start pose in front of the reset and tally_append in place of log_append.  Its own
// kernel for the reason k_step_log is: k_step and k_step_log keep their names, their code and their register allocation.
template <bool PER_ENV, bool INFO, bool AUTO_RESET, bool RANDOM_POLICY>
__global__ __launch_bounds__(BLOCK) void k_step_tally(const KParams P, const int n, const Bufs b,
                                                      const float *__restrict__ action, float *__restrict__ action_out,
                                                      float *__restrict__ obs, float *__restrict__ reward,
                                                      uint8_t *__restrict__ done, const Info info, const uint64_t seed,
                                                      const uint64_t policy_seed, const int *__restrict__ cursor,
                                                      const EpLog lg) {
    __shared__ __attribute__((aligned(16))) float tile[BLOCK * OBS];
    TT_STEP_HEAD();
    if (valid) {
        TT_STEP_LOADS();
        double ret = lg.acc[i];
        __builtin_amdgcn_sched_barrier(0);
        TT_STEP_ACT();
        StepOut o;
        step_env(P, e, a, of, o);
        TT_STEP_OUT();
        TT_STEP_RETURN();
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        if (o.done) {           // the finished episode's start pose, before the reset places the next one (k_get_episode's rows)
            const double *cold = b.cold + i;
            const size_t S = (size_t)P.npad;
            s0 = cold[C_SX * S]; s1 = cold[C_SY * S]; s2 = cold[C_SYAW * S];
        }
        TT_STEP_RESET();
        tally_append(P, lg, i, o, len, ret, s0, s1, s2);
    }
    store_obs_tile(tile, of, valid, obs, block_first, nv, P.nt != 0);
    TT_STEP_LAUNCH_COUNT();
}

// K vector steps in ONE launch with the random policy: the env stays in registers, only the last
// observation is stored; per-env reward sums and episode counts are accumulated.
template <bool PER_ENV>
__global__ __launch_bounds__(BLOCK) void k_rollout(const KParams P, const int n, const Bufs b, const int k_steps,
                                                   float *__restrict__ obs, float *__restrict__ reward_sum,
                                                   int32_t *__restrict__ episodes_done, const uint64_t seed,
                                                   const uint64_t policy_seed) {
    __shared__ __attribute__((aligned(16))) float tile[BLOCK * OBS];
    const int block_first = blockIdx.x * BLOCK;
    const int i = block_first + threadIdx.x;
    const bool valid = i < n;
    float of[OBS];
    if (valid) {
        Env e;
        load_env<PER_ENV>(P, b, i, e);
        uint32_t ep = b.episodes[i];
        double rsum = 0.0;
        int ndone = 0;
        for (int t = 0; t < k_steps; ++t) {
            const float a = random_action(policy_seed, (uint32_t)i, pk_steps(e.pk), ep);
            StepOut o;
            step_env(P, e, a, of, o);
            rsum += o.total;
            if (o.done) {
                ep += 1u;
                ndone += 1;
                double sx, sy, syaw;
                random_pose(P, seed, (uint32_t)i, ep, sx, sy, syaw);
                const Goal g0{P.gx, P.gy, P.sg, P.cg};
                place_env(P, b, i, e, sx, sy, syaw, g0, P.gyaw, e.L2, of);
            }
        }
        b.episodes[i] = ep;
        store_env(b, i, e);
        if (reward_sum) reward_sum[i] = (float)rsum;
        if (episodes_done) episodes_done[i] = ndone;
    }
    if (obs) store_obs_tile(tile, of, valid, obs, block_first, min(BLOCK, n - block_first));
}

// ------------------------------------------------------------------------------------------
// Sampling MPC (MPPI; include/ttenv.h: tt_env_mpc_plan has the definition of a decision).
// ONE WORKGROUP PLANS FOR ONE LANE: thread `tid` rolls samples tid, tid + BLOCK, ... through step_env on a copy of the lane's env
// in registers; the env in memory is only read.  The weighted mean needs every u[s, t] again once the largest return is known:
// the noise is counter-based, so the second pass REGENERATES a sample's sequence (S * H Philox blocks, a log and a sincos each:
// a few per cent of the S * H env steps of the first pass) instead of keeping S * H values (256 KB at the limits).  `chunk`
// samples at a time go through an LDS tile [chunk][H | 1] (odd stride: conflict-free both ways), and thread t < H adds column t
// of the tile in sample order.
//
// step_env's three wave votes with a wave that holds different SAMPLES of one lane, some of which have left the horizon loop:
// a vote counts the active lanes only, and each of them only widens what the wave computes -- the quotient by a real division
// gives every lane the value its own test would (the two quotients truncate differently only where the lane itself votes), and
// the staged bonuses and the backward penalty are recomputed under each lane's own comparison inside the voted branch.
constexpr uint32_t MPC_NOISE_TAG = 0x4D50u;     // Philox domain of the MPC's exploration noise
constexpr int MPC_TILE_FLOATS = 12288;          // the second pass's LDS tile: 48 KB

struct MpcK {
    int H, S, chunk;
    float action_scale;
    double sigma, rho, sigma_c;     // sigma_c = sqrt(1 - rho^2) sigma
    double lambda, gamma, k_lat, k_yaw;
    uint64_t seed;
};

// z[s, t]: the recipe of the TD3 smoothing noise (csrc/tttd3.h) with log, sqrt and cos in f64; products only, so that both passes
// get the same bits however they are contracted
__device__ __forceinline__ double mpc_normal(const MpcK &m, uint32_t lane, uint32_t episode, uint32_t steps, int s, int t) {
    uint32_t r[4];
    philox4x32(lane, episode, steps | ((uint32_t)t << 12) | ((uint32_t)s << 18), MPC_NOISE_TAG, (uint32_t)m.seed,
               (uint32_t)(m.seed >> 32), r);
    const float u1 = ((float)(r[0] >> 8) + 0.5f) * (1.f / 16777216.f);
    const float u2 = ((float)(r[1] >> 8) + 0.5f) * (1.f / 16777216.f);
    double sn, cs;
    tt_sincos(kTable, (double)(6.28318530717958647692f * u2), sn, cs);
    return sqrt(-2.0 * log((double)u1)) * cs;
}

// u[s, t] from the AR(1) state `eps` (advanced here) and the plan's entry
__device__ __forceinline__ float mpc_sample(const MpcK &m, uint32_t lane, uint32_t episode, uint32_t steps, int s, int t, float plan_t,
                                            double &eps) {
    if (s > 0) {
        const double z = mpc_normal(m, lane, episode, steps, s, t);
        eps = t == 0 ? m.sigma * z : fma(m.rho, eps, m.sigma_c * z);
    }
    return (float)fmin(fmax((double)plan_t + eps, -1.0), 1.0);
}

// Where a decision of an EXPERT LANE goes (tt_env_mpc_act_ring): the running step's action row of a trajectory ring, found through
// the cursor as k_step finds its rows, and the loop's scaled-action buffer -- the two values the policy launch wrote for the lane.
struct MpcRing {
    const int *cursor;      // [0]: the running step's slot t (left by tt_actor_act_ring)
    float *act;             // the ring's action rows [slots, n_envs]
    float *act_scaled;      // [n_envs]
    int n_envs, slots;
    float high;
};
struct MpcNoRing {};
// Expert lanes [0, expert) as MpcRing, and LABELLED LANES [expert, n) behind them (tt_env_mpc_label_ring): the decision of a
// labelled lane goes to the ring's label row of the running step and nowhere else -- the lane executes what the policy wrote.
struct MpcLabel {
    const int *cursor;      // [0]: the running step's slot t (left by tt_actor_act_ring)
    float *act;             // the ring's action rows [slots, n_envs] (expert lanes only; unused with expert = 0)
    float *act_scaled;      // [n_envs] (expert lanes only)
    float *label;           // the ring's label rows [slots, n_envs]
    int n_envs, slots;
    float high;
    int expert;             // M: workgroup i < M stores as MpcRing, i >= M stores label[t][i]
};

// One planner, three launches: k_mpc_plan (RING = MpcNoRing: mu_out, live, returns_out), k_mpc_act_ring (RING = MpcRing: workgroup
// i < n plans for lane i of the first n lanes, and U'_0 goes to the ring) and k_mpc_label_ring (RING = MpcLabel: the same for lanes
// < ring.expert, U'_0 to the label row for the others).  Everything before the last store is the same text.
template <bool PER_ENV, class RING>
__device__ __forceinline__ void mpc_plan_body(const KParams P, const int n, const Bufs b, const MpcK m, float *plan, float *mu_out,
                                              const uint8_t *live, double *returns_out, const RING ring) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mpc_lds[];
    const int i = blockIdx.x, tid = threadIdx.x;
    if (i >= n || (live && !live[i])) return;       // uniform: a skipped lane keeps every output's bits
    const int H = m.H, S = m.S, HP = H | 1;
    double *G = reinterpret_cast<double *>(mpc_lds);            // [S] returns, then weights
    double *red = G + S;                                        // [BLOCK]
    float *pl = reinterpret_cast<float *>(red + BLOCK);         // [H] the plan as read
    float *tile = pl + ((H + 3) & ~3);                          // [chunk][HP]
    const KTable &T = kTable;

    const uint32_t pk0 = reinterpret_cast<const uint2 *>(hot_ptr(b.hot, i) + H_MISC * TILE)->y;
    const uint32_t steps0 = pk_steps(pk0), ep = b.episodes[i];
    if (tid < H) pl[tid] = steps0 == 0u ? 0.f : plan[(size_t)i * H + tid];
    __syncthreads();

    // ---- pass 1: the returns
    double gmax = -INFINITY;
    for (int s = tid; s < S; s += BLOCK) {
        Env e;
        load_env<PER_ENV>(P, b, i, e);
        double Gs = 0.0, disc = 1.0, eps = 0.0;
        bool open = true;
        float of[OBS];
        for (int t = 0; t < H; ++t) {
            const float u = mpc_sample(m, (uint32_t)i, ep, steps0, s, t, pl[t], eps);
            const float a = u * m.action_scale;
            StepOut o;
            step_env(P, e, a, of, o);
            Gs += disc * o.total;
            disc *= m.gamma;
            if (o.done) { open = false; break; }     // the sample's env stops here: pk's packed fields are not stepped past done
        }
        if (open) {
            const double lat = -(e.x2 - e.g.gx) * e.g.sg + (e.y2 - e.g.gy) * e.g.cg;
            const double dyaw = tt_wrap_pi(T, e.gyaw - e.psi2);
            Gs += disc * -(m.k_lat * (lat * lat) + m.k_yaw * (dyaw * dyaw));
        }
        G[s] = Gs;
        if (returns_out) returns_out[(size_t)i * S + s] = Gs;
        if (isfinite(Gs)) gmax = fmax(gmax, Gs);
    }
    red[tid] = gmax;
    __syncthreads();
    for (int d = BLOCK >> 1; d > 0; d >>= 1) {
        if (tid < d) red[tid] = fmax(red[tid], red[tid + d]);
        __syncthreads();
    }
    gmax = red[0];
    for (int s = tid; s < S; s += BLOCK) {
        const double g = G[s];
        G[s] = isfinite(g) ? tt_exp_neg(T, (g - gmax) / m.lambda) : 0.0;
    }

    // ---- pass 2: the weighted mean, in sample order
    double num = 0.0, den = 0.0;
    for (int s0 = 0; s0 < S; s0 += m.chunk) {
        const int ns = min(m.chunk, S - s0);
        __syncthreads();        // the weights are written (first round); the tile's readers are done (later rounds)
        if (tid < ns) {
            double eps = 0.0;
            for (int t = 0; t < H; ++t) tile[tid * HP + t] = mpc_sample(m, (uint32_t)i, ep, steps0, s0 + tid, t, pl[t], eps);
        }
        __syncthreads();
        if (tid < H)
            for (int q = 0; q < ns; ++q) {
                const double w = G[s0 + q];
                num = fma(w, (double)tile[q * HP + tid], num);
                den += w;
            }
    }
    if (tid < H) {
        const float un = den > 0.0 ? (float)(num / den) : pl[tid];     // no finite sample: the plan shifts unchanged
        float *row = plan + (size_t)i * H;
        if (tid == 0) {
            if constexpr (std::is_same<RING, MpcRing>::value) {
                // ring.act[t][i] = U'_0 (the normalised action: what collect_demonstrations stores) and the env step's input, one
                // f32 product; a cursor outside the ring (never written by a pack launch) stores nothing
                const int t = ring.cursor[0];
                if ((unsigned)t < (unsigned)ring.slots) ring.act[(size_t)t * ring.n_envs + i] = un;
                ring.act_scaled[i] = un * ring.high;
            } else if constexpr (std::is_same<RING, MpcLabel>::value) {
                // an expert lane: MpcRing's two stores; a labelled lane: label[t][i] = U'_0 alone (ring.act[t][i] and act_scaled[i]
                // keep the policy's bits).  i is the workgroup's lane: the branch is uniform
                const int t = ring.cursor[0];
                if (i < ring.expert) {
                    if ((unsigned)t < (unsigned)ring.slots) ring.act[(size_t)t * ring.n_envs + i] = un;
                    ring.act_scaled[i] = un * ring.high;
                } else if ((unsigned)t < (unsigned)ring.slots) {
                    ring.label[(size_t)t * ring.n_envs + i] = un;
                }
            } else {
                mu_out[i] = un;
            }
        } else {
            row[tid - 1] = un;
        }
        if (tid == H - 1) row[tid] = un;
    }
}

template <bool PER_ENV>
__global__ __launch_bounds__(BLOCK) void k_mpc_plan(const KParams P, const int n, const Bufs b, const MpcK m, float *plan,
                                                    float *mu_out, const uint8_t *live, double *returns_out) {
    mpc_plan_body<PER_ENV>(P, n, b, m, plan, mu_out, live, returns_out, MpcNoRing{});
}

// lanes [0, lanes) of the env: grid = lanes; plan is [lanes, H]
template <bool PER_ENV>
__global__ __launch_bounds__(BLOCK) void k_mpc_act_ring(const KParams P, const int lanes, const Bufs b, const MpcK m, float *plan,
                                                        const MpcRing ring) {
    mpc_plan_body<PER_ENV>(P, lanes, b, m, plan, nullptr, nullptr, nullptr, ring);
}

// lanes [0, lanes) of the env, lanes = expert + labelled: grid = lanes; plan is [lanes, H]
template <bool PER_ENV>
__global__ __launch_bounds__(BLOCK) void k_mpc_label_ring(const KParams P, const int lanes, const Bufs b, const MpcK m, float *plan,
                                                          const MpcLabel ring) {
    mpc_plan_body<PER_ENV>(P, lanes, b, m, plan, nullptr, nullptr, nullptr, ring);
}

// ------------------------------------------------------------------------------------------
// reset / pose / state kernels (not hot)
__global__ __launch_bounds__(BLOCK) void k_reset(const KParams P, const int n, const Bufs b, const uint8_t *mask,
                                                 float *obs, const uint64_t seed) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n || (mask && !mask[i])) return;
    // a full reset restarts every env's episode count, so reset(seed) is a pure function of the seed
    // (as np.random.seed is); a masked reset moves the chosen envs on to their next episode
    const uint32_t ep = mask ? b.episodes[i] + 1u : 0u;
    b.episodes[i] = ep;
    double sx, sy, syaw;
    random_pose(P, seed, (uint32_t)i, ep, sx, sy, syaw);
    float of[OBS];
    const Goal g{P.gx, P.gy, P.sg, P.cg};
    Env e;
    place_env(P, b, i, e, sx, sy, syaw, g, P.gyaw, b.cold[C_L2 * (size_t)P.npad + i], obs ? of : nullptr);
    store_env(b, i, e);
    if (obs)
        for (int j = 0; j < OBS; ++j) obs[(size_t)i * OBS + j] = of[j];
}

__global__ __launch_bounds__(BLOCK) void k_init(const KParams P, const Bufs b) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P.npad) return;  // padding lanes of the last tile get a valid env too
    b.episodes[i] = 0u;
    const Goal g{P.gx, P.gy, P.sg, P.cg};
    Env e;
    place_env(P, b, i, e, P.gx, P.gy + 30.0, kPi / 2, g, P.gyaw, P.L2, nullptr);
    store_env(b, i, e);
}

__global__ __launch_bounds__(BLOCK) void k_set_pose(const KParams P, const int n, const Bufs b, const int32_t *idx,
                                                    const int k, const double *start, const double *goal,
                                                    const double *L2, float *obs) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= k) return;
    const int i = idx ? idx[j] : j;
    if (i < 0 || i >= n) return;
    const size_t S = (size_t)P.npad;
    const double *c = b.cold + i;
    Goal g;
    double gyaw;
    if (goal) {
        g.gx = goal[3 * j]; g.gy = goal[3 * j + 1]; gyaw = goal[3 * j + 2];
        tt_sincos(kTable, gyaw, g.sg, g.cg);
    } else {
        g.gx = c[C_GX * S]; g.gy = c[C_GY * S]; gyaw = c[C_GYAW * S]; g.sg = c[C_SG * S]; g.cg = c[C_CG * S];
    }
    const double l2 = L2 ? L2[j] : c[C_L2 * S];
    float of[OBS];
    Env e;
    place_env(P, b, i, e, start[3 * j], start[3 * j + 1], start[3 * j + 2], g, gyaw, l2, obs ? of : nullptr);
    store_env(b, i, e);
    if (obs)
        for (int q = 0; q < OBS; ++q) obs[(size_t)i * OBS + q] = of[q];
}

__global__ __launch_bounds__(BLOCK) void k_set_attrs(const KParams P, const int n, const Bufs b, const int32_t *idx,
                                                     const int k, const double *start, const double *goal,
                                                     const double *L2) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= k) return;
    const int i = idx ? idx[j] : j;
    if (i < 0 || i >= n) return;
    const size_t S = (size_t)P.npad;
    double *c = b.cold + i;
    if (start) {
        c[C_SX * S] = start[3 * j]; c[C_SY * S] = start[3 * j + 1]; c[C_SYAW * S] = start[3 * j + 2];
    }
    if (goal) {
        double sg, cg;
        tt_sincos(kTable, goal[3 * j + 2], sg, cg);
        c[C_GX * S] = goal[3 * j]; c[C_GY * S] = goal[3 * j + 1]; c[C_GYAW * S] = goal[3 * j + 2];
        c[C_SG * S] = sg; c[C_CG * S] = cg;
    }
    if (L2) c[C_L2 * S] = L2[j];
    const double ddx = c[C_GX * S] - c[C_SX * S], ddy = c[C_GY * S] - c[C_SY * S];
    hot_ptr(b.hot, i)[H_DINIT * TILE] = sqrt(ddx * ddx + ddy * ddy);
}

__global__ __launch_bounds__(BLOCK) void k_set_state(const int n, const Bufs b, const int32_t *idx, const int k,
                                                     const double *state) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= k) return;
    const int i = idx ? idx[j] : j;
    if (i < 0 || i >= n) return;
    double *h = hot_ptr(b.hot, i);
    for (int r = 0; r < 6; ++r) h[r * TILE] = state[6 * j + r];
}

__global__ __launch_bounds__(BLOCK) void k_get_state(const int n, const Bufs b, double *out) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double *h = hot_ptr(b.hot, i);
    for (int r = 0; r < 6; ++r) out[r * (size_t)n + i] = h[r * TILE];
}

__global__ __launch_bounds__(BLOCK) void k_set_max_steps(const int n, const Bufs b, const int32_t *idx, const int k,
                                                         const int32_t *maxs) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= k) return;
    const int i = idx ? idx[j] : j;
    if (i < 0 || i >= n) return;
    uint2 *m = reinterpret_cast<uint2 *>(hot_ptr(b.hot, i) + H_MISC * TILE);
    const uint32_t p = m->y;
    m->y = pk_make(pk_steps(p), (uint32_t)(maxs[j] < 0 ? 0 : maxs[j]), pk_stages(p), pk_age(p));
}

// `env.episode_steps = k` (simv2.py:94; episode_replay_collectorv2.py:269): the step counter alone -- the reward carry, its
// age and the stage latches stay (the reference keeps them in reward_state, which such a write does not touch)
__global__ __launch_bounds__(BLOCK) void k_set_steps(const int n, const Bufs b, const int32_t *idx, const int k,
                                                     const int32_t *steps) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= k) return;
    const int i = idx ? idx[j] : j;
    if (i < 0 || i >= n) return;
    uint2 *m = reinterpret_cast<uint2 *>(hot_ptr(b.hot, i) + H_MISC * TILE);
    const uint32_t p = m->y;
    m->y = pk_make((uint32_t)(steps[j] < 0 ? 0 : steps[j]), pk_max(p), pk_stages(p), pk_age(p));
}

__global__ __launch_bounds__(BLOCK) void k_get_episode(const KParams P, const int n, const Bufs b, int32_t *steps,
                                                       int32_t *maxs, double *start, double *goal, double *L2) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = reinterpret_cast<const uint2 *>(hot_ptr(b.hot, i) + H_MISC * TILE)->y;
    if (steps) steps[i] = (int32_t)pk_steps(p);
    if (maxs) maxs[i] = (int32_t)pk_max(p);
    const size_t S = (size_t)P.npad, N = (size_t)n;
    const double *c = b.cold + i;
    if (start) { start[i] = c[C_SX * S]; start[N + i] = c[C_SY * S]; start[2 * N + i] = c[C_SYAW * S]; }
    if (goal) { goal[i] = c[C_GX * S]; goal[N + i] = c[C_GY * S]; goal[2 * N + i] = c[C_GYAW * S]; }
    if (L2) L2[i] = c[C_L2 * S];
}

template <bool PER_ENV>
__global__ __launch_bounds__(BLOCK) void k_observe(const KParams P, const int n, const Bufs b, const float *steering,
                                                   float *obs) {
    __shared__ __attribute__((aligned(16))) float tile[BLOCK * OBS];
    const int block_first = blockIdx.x * BLOCK;
    const int i = block_first + threadIdx.x;
    const bool valid = i < n;
    float of[OBS];
    if (valid) {
        const KTable &T = kTable;
        Env e;
        load_env<PER_ENV>(P, b, i, e);
        double s1, c1, s2, c2, sd = 0.0, cd = 1.0;
        tt_sincos(T, e.psi1, s1, c1);
        tt_sincos(T, e.psi2, s2, c2);
        if (steering) tt_sincos(T, (double)steering[i], sd, cd);
        const double dx = e.g.gx - e.x2, dy = e.g.gy - e.y2;
        const double cur = sqrt(dx * dx + dy * dy);
        observe(P, e.g, e.x1, e.y1, e.x2, e.y2, s1, c1, s2, c2, sd, cd, dx, dy, cur, cur > 0.0 ? 1.0 / cur : 0.0, of);
    }
    store_obs_tile(tile, of, valid, obs, block_first, min(BLOCK, n - block_first));
}

__global__ __launch_bounds__(BLOCK) void k_random_actions(const int n, const uint64_t seed, const uint64_t step,
                                                          float *out) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t r[4];
    philox4x32((uint32_t)i, (uint32_t)step, (uint32_t)(step >> 32), 0xAC71u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    out[i] = (float)((2.0 * u01(r[0]) - 1.0) * (kPi / 4));
}

// the episode log's accumulator of lanes that start a new episode outside the step kernel (tt_env_reset with a mask,
// tt_env_set_pose): entry j < k names lane idx[j] (idx NULL: lane j) and counts when mask is NULL or mask[lane] != 0
__global__ __launch_bounds__(BLOCK) void k_log_zero(const int n, const int k, const uint8_t *mask, const int32_t *idx,
                                                    double *acc) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= k) return;
    const int i = idx ? idx[j] : j;
    if (i < 0 || i >= n || (mask && !mask[i])) return;
    acc[i] = 0.0;
}

// k_log_zero for the detailed log: the lane's return and its nine term sums (tally_acc)
__global__ __launch_bounds__(BLOCK) void k_tally_zero(const int n, const int k, const uint8_t *mask, const int32_t *idx,
                                                      const EpLog lg, const int npad) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= k) return;
    const int i = idx ? idx[j] : j;
    if (i < 0 || i >= n || (mask && !mask[i])) return;
    lg.acc[i] = 0.0;
    double *acc = tally_acc(lg, npad, i);
    for (int c = 0; c < TT_LOG_NCOMP; ++c) acc[c * TILE] = 0.0;
}

// the detailed columns of the first min(written, capacity) records into comp [TT_LOG_NCOMP, capacity] / start [3, capacity]
// (either may be NULL); k_log_drain copies the plain ones
__global__ __launch_bounds__(BLOCK) void k_tally_drain(const EpLog lg, double *comp, double *start) {
    const unsigned long long j = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= min(lg.hdr[LG_WRITTEN], lg.capacity)) return;
    const TallyCols t = tally_cols(lg);
    const size_t cap = (size_t)lg.capacity;
    if (comp)
        for (int c = 0; c < TT_LOG_NCOMP; ++c) comp[c * cap + j] = t.comp[c * cap + j];
    if (start)
        for (int c = 0; c < 3; ++c) start[c * cap + j] = t.start[c * cap + j];
}

__global__ __launch_bounds__(BLOCK) void k_log_drain(const EpLog lg, double *ret, int32_t *len, uint8_t *flags,
                                                     uint8_t *success, int32_t *lane, long long *end_step,
                                                     long long *n_out, unsigned long long *counts_out) {
    const unsigned long long j = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    const unsigned long long written = lg.hdr[LG_WRITTEN];
    if (j < min(written, lg.capacity)) {
        const LogCols c = log_cols(lg);
        if (ret) ret[j] = c.ret[j];
        if (len) len[j] = c.len[j];
        if (flags) flags[j] = c.flags[j];
        if (success) success[j] = c.success[j];
        if (lane) lane[j] = c.lane[j];
        if (end_step) end_step[j] = c.end_step[j];
    }
    if (j == 0) {
        if (n_out) *n_out = (long long)written;
        if (counts_out)
            for (int c = 0; c < TT_LOG_NCOUNTS; ++c) counts_out[c] = lg.hdr[LG_COUNTS + c];
    }
}

// ------------------------------------------------------------------------------------------
// Greedy evaluation (tt_env_set_hold): an env step in which a finished lane HOLDS STILL.  One device block,
//   ret f64 [npad] | end f64 [3][npad] | len i32 [npad] | live u8 [npad] | flags u8 [npad] | success u8 [npad]
// every lane's episode record in the lane's own slot: nothing is appended, no atomics, so an evaluation is bit-reproducible.
// The kernels get the block's base (2 SGPRs) and find the columns from npad.
struct HoldCols {
    double *ret, *end;
    int32_t *len;
    uint8_t *live, *flags, *success;
};
__host__ __device__ inline size_t hold_block_bytes(int npad) { return (4 * sizeof(double) + sizeof(int32_t) + 3) * (size_t)npad; }
__host__ __device__ inline HoldCols hold_cols(void *block, int npad) {
    const size_t S = (size_t)npad;
    HoldCols c;
    c.ret = static_cast<double *>(block);
    c.end = c.ret + S;
    c.len = reinterpret_cast<int32_t *>(c.end + 3 * S);
    c.live = reinterpret_cast<uint8_t *>(c.len + S);
    c.flags = c.live + S;
    c.success = c.flags + S;
    return c;
}

// The workgroup's rows of the observation matrix as they are in memory, into the LDS tile (the mirror of store_obs_tile's second
// half): a held lane's row then passes through store_obs_tile unchanged.  Every thread of the block calls this (barrier inside).
__device__ inline void load_obs_tile(float *tile, const float *obs, int block_first, int nv) {
    const int tid = threadIdx.x;
    const float *src = obs + (size_t)block_first * OBS;
    const int total = nv * OBS;
    if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
        const int nvec = total >> 2;
        const float4 *s4 = reinterpret_cast<const float4 *>(src);
        float4 *t4 = reinterpret_cast<float4 *>(tile);
        for (int q = tid; q < nvec; q += BLOCK) t4[q] = s4[q];
        for (int q = (nvec << 2) + tid; q < total; q += BLOCK) tile[q] = src[q];
    } else {
        for (int q = tid; q < total; q += BLOCK) tile[q] = src[q];
    }
    __syncthreads();
}

// The step of an evaluation: a live lane takes a = mu * action_scale (one f32 multiply, the product torch forms in grid_eval),
// steps with no reset, adds the f64 reward to its return in step order (the episode log's definition) and, on done, writes its
// record and clears its live byte.  A held lane (live == 0) changes nothing of itself: it loads and stores no state, and its
// observation row goes through store_obs_tile's LDS tile as it was read from memory (load_obs_tile; carrying the row in the
// lane's own `of` registers would cost 23 strided loads per held lane, masking it out of the store a test per element of
// vectors that straddle rows).  A workgroup with no live lane returns after one byte load per lane: the barriers of the
// transpose are the whole workgroup's, so the return is taken only where it is uniform.
// A kernel of its own made of k_step's inlined pieces, for k_step_log's reason; b.counter, the episode log and the ring are
// not touched.
template <bool PER_ENV>
__global__ __launch_bounds__(BLOCK) void k_step_hold(const KParams P, const int n, const Bufs b, const float *__restrict__ mu,
                                                     const float action_scale, float *__restrict__ obs, void *const hold) {
    __shared__ __attribute__((aligned(16))) float tile[BLOCK * OBS];
    const int block_first = blockIdx.x * BLOCK;
    const int i = block_first + threadIdx.x;
    const int nv = min(BLOCK, n - block_first);
    const HoldCols h = hold_cols(hold, P.npad);
    const bool live = i < n && h.live[i] != 0;
    const int nlive = __syncthreads_count(live ? 1 : 0);
    if (nlive == 0) return;                             // a held workgroup (uniform)
    if (nlive < nv) load_obs_tile(tile, obs, block_first, nv);      // some lane is held (uniform): its row is kept
    float of[OBS];
    if (live) {
        Env e;
        load_env<PER_ENV>(P, b, i, e);
        float a = mu[i];
        __builtin_amdgcn_sched_barrier(0);     // every load of the step in one burst (k_step)
        a = a * action_scale;
        StepOut o;
        step_env(P, e, a, of, o);
        // (the return is loaded here, not in the burst: held across step_env it cost the PER_ENV = false variant its fourth wave
        // per SIMD -- 129 registers, one of them for spilled SGPRs; now 127 / 122)
        h.ret[i] += o.total;
        store_env(b, i, e);
        if (o.done) {
            const size_t S = (size_t)P.npad;
            h.len[i] = (int32_t)pk_steps(e.pk);
            h.flags[i] = (uint8_t)o.flags;
            h.success[i] = o.final_bonus > 0.0 ? 1 : 0;
            h.end[i] = e.x2; h.end[S + i] = e.y2; h.end[2 * S + i] = e.psi2;
            h.live[i] = 0;
        }
    }
    store_obs_tile(tile, of, live, obs, block_first, nv, P.nt != 0);
}

// every lane < n live, every record zero (lanes n .. npad never live)
__global__ __launch_bounds__(BLOCK) void k_hold_begin(const int n, const int npad, void *const hold) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= npad) return;
    const HoldCols h = hold_cols(hold, npad);
    const size_t S = (size_t)npad;
    h.live[i] = i < n ? 1 : 0;
    h.ret[i] = 0.0;
    h.len[i] = 0;
    h.flags[i] = 0;
    h.success[i] = 0;
    h.end[i] = 0.0; h.end[S + i] = 0.0; h.end[2 * S + i] = 0.0;
}

// The number of live lanes into one device int64: ONE workgroup, each thread sums the live bytes of its stride (four per word;
// npad is a multiple of 64), then a fixed-order tree through LDS.  No atomics.
__global__ __launch_bounds__(BLOCK) void k_hold_live(const int npad, const void *const hold, long long *out) {
    __shared__ long long part[BLOCK];
    const uint32_t *w = reinterpret_cast<const uint32_t *>(hold_cols(const_cast<void *>(hold), npad).live);
    long long s = 0;
    for (int q = threadIdx.x; q < (npad >> 2); q += BLOCK) {
        const uint32_t x = w[q];
        s += (long long)((x & 0xFFu) + ((x >> 8) & 0xFFu) + ((x >> 16) & 0xFFu) + (x >> 24));
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = BLOCK >> 1; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = part[0];
}

// the records into the caller's arrays of n entries (any may be NULL); end is [3][n]
__global__ __launch_bounds__(BLOCK) void k_hold_read(const int n, const int npad, void *const hold, double *ret, int32_t *len,
                                                     uint8_t *flags, uint8_t *success, double *end) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const HoldCols h = hold_cols(hold, npad);
    const size_t S = (size_t)npad, N = (size_t)n;
    if (ret) ret[i] = h.ret[i];
    if (len) len[i] = h.len[i];
    if (flags) flags[i] = h.flags[i];
    if (success) success[i] = h.success[i];
    if (end) { end[i] = h.end[i]; end[N + i] = h.end[S + i]; end[2 * N + i] = h.end[2 * S + i]; }
}

// ------------------------------------------------------------------------------------------
// Start-pose curriculum (tt_env_set_curriculum): a grid of C = nx * ny * nyaw cells over the reset box, cell
// c = (iyaw * ny + iy) * nx + ix, that counts the outcomes of the episodes started in each cell and draws the next start pose by
// weights made from them.  The kernels get ONE pointer, to this descriptor in device memory (2 SGPRs; the step kernels have none to
// spare): only a lane that finishes an episode reads it.  Everything that decides a draw is an integer (q, cum)
// and everything that counts is an integer add, so a run does not depend on the order in which lanes arrive.
struct CurDev {
    uint32_t *cell;                 // [npad] the cell a lane's running episode was drawn from, TT_CURRICULUM_NO_CELL: none
    uint32_t *cum;                  // [C] the inclusive prefix sum of q
    uint32_t *attempts, *successes; // [C] counts since the last update
    int C, nx, ny, nyaw;
    uint32_t *q;                    // [C] draw weight in [1, 65536]
    double *p;                      // [C] running success rate
    unsigned long long *seen;       // [C] episodes ever counted
    int mode, reserved_;
    double alpha, uniform;
    double lo[3], width[3];         // reset_lo and (reset_hi - reset_lo) / bins, formed on the host in f64
    unsigned long long seed;        // the handle's reset seed (k_curriculum_seed): the step kernels read it here, in the path that
                                    // needs it, not from their argument (two SGPRs less across step_env)
};

// The draw: random_pose's Philox words; r[3] picks the cell -- t = (r[3] * cum[C - 1]) >> 32, the smallest c with cum[c] > t --
// and r[0..2] the pose inside it.  f64 with contraction off (as tally_append): a host model equals it bit for bit.  The search
// stays inside [0, C) whatever cum holds.
__device__ __forceinline__ void curriculum_pose(const CurDev *cur, uint64_t seed, uint32_t env, uint32_t episode, double &sx,
                                                double &sy, double &syaw) {
#pragma clang fp contract(off)
    uint32_t r[4];
    philox4x32(env, episode, 0u, 0x7452u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const uint32_t *cum = cur->cum;
    const int C = cur->C;
    const uint32_t t = (uint32_t)(((unsigned long long)r[3] * (unsigned long long)cum[C - 1]) >> 32);
    // the number of cells with cum <= t, by halving steps without a branch (C <= 4096: twelve); t < cum[C - 1] keeps it below C
    uint32_t lo = 0u;
#pragma unroll
    for (uint32_t s = TT_CURRICULUM_MAX_CELLS / 2; s > 0u; s >>= 1) {
        const uint32_t j = lo + s;      // would cells [0, j) all have cum <= t?
        const uint32_t v = cum[min(j, (uint32_t)C) - 1u];
        lo = (j <= (uint32_t)C && v <= t) ? j : lo;
    }
    lo = min(lo, (uint32_t)C - 1u);     // (only a cum that is no prefix sum of positive weights gets here)
    const uint32_t c = lo, nx = (uint32_t)cur->nx, ny = (uint32_t)cur->ny;
    // c / nx and rest / ny as floor((a + 0.5) * rcp(b)) in f32: exact for a < 4096 (the nearest integer boundary is 0.5 / b away, a
    // relative 1.2e-4 at the least, against the 2.4e-7 of the reciprocal and the product), and a tenth of an integer division's code
    const uint32_t rest = (uint32_t)(((float)c + 0.5f) * __builtin_amdgcn_rcpf((float)nx)), ix = c - rest * nx;
    const uint32_t iyaw = (uint32_t)(((float)rest + 0.5f) * __builtin_amdgcn_rcpf((float)ny)), iy = rest - iyaw * ny;
    const double k = 1.0 / 4294967296.0;
    const double u0 = ((double)r[0] + 0.5) * k, u1 = ((double)r[1] + 0.5) * k, u2 = ((double)r[2] + 0.5) * k;
    sx = cur->lo[0] + ((double)ix + u0) * cur->width[0];
    sy = cur->lo[1] + ((double)iy + u1) * cur->width[1];
    syaw = cur->lo[2] + ((double)iyaw + u2) * cur->width[2];
    cur->cell[env] = c;
}

// Head of the curriculum's step kernels, behind TT_STEP_HEAD: the descriptor's address and the address of the lane's episode number
// into VECTOR registers, at the kernel's head (the empty asm pins them there: the compiler neither keeps the scalars nor forms the
// addresses again later).  The step kernels' loop variants sit at their SGPR limit across step_env and have vector registers to
// spare.  With the two held as scalars until the reset, the allocator split the tuple of kernel arguments that holds Bufs and left
// a stack slot behind: 36 B of scratch that no instruction touches, but that every dispatch has to be given.  The descriptor's words
// then arrive by vector loads, in the one path that reads them.  Declares cur and ep_ptr.
#define TT_STEP_CUR()                                                                                                                   \
    uint32_t cur_lo = (uint32_t)reinterpret_cast<uintptr_t>(cur_arg), cur_hi = (uint32_t)(reinterpret_cast<uintptr_t>(cur_arg) >> 32);  \
    asm volatile("" : "+v"(cur_lo), "+v"(cur_hi));                                                                                      \
    const CurDev *cur = reinterpret_cast<const CurDev *>(((uintptr_t)cur_hi << 32) | (uintptr_t)cur_lo);                               \
    uint32_t *ep_ptr = b.episodes + i;                                                                                                  \
    asm volatile("" : "+v"(ep_ptr))
// Reset with the curriculum on (TT_STEP_RESET's place in k_step_cur / k_step_cur_log; auto-reset always): the finished episode is
// counted in the cell it was drawn from -- one relaxed agent-scope u32 add to attempts[cell], one more to successes[cell] on success
// (the episode log's test) -- BEFORE the draw overwrites the lane's cell; a lane whose episode no curriculum draw made (cell outside
// [0, C)) counts nothing.
#define TT_STEP_RESET_CURRICULUM()                                                                                                      \
    /* (tests side by side, not nested: every level of divergent nesting holds an exec mask in two more SGPRs) */                       \
    uint32_t cl = TT_CURRICULUM_NO_CELL, ncell = 0u;                                                                                    \
    if (o.done) {                                                                                                                       \
        cl = cur->cell[i];                                                                                                              \
        ncell = (uint32_t)cur->C;                                                                                                       \
    }                                                                                                                                   \
    if (cl < ncell) __hip_atomic_fetch_add(cur->attempts + cl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                         \
    if (cl < ncell && o.final_bonus > 0.0) __hip_atomic_fetch_add(cur->successes + cl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
    if (o.done) {                                                                                                                       \
        const uint32_t ep = *ep_ptr + 1u;                                                                                               \
        *ep_ptr = ep;                                                                                                                   \
        double sx, sy, syaw;                                                                                                            \
        curriculum_pose(cur, cur->seed, (uint32_t)i, ep, sx, sy, syaw);                                                                 \
        const Goal g0{P.gx, P.gy, P.sg, P.cg};                                                                                          \
        place_env(P, b, i, e, sx, sy, syaw, g0, P.gyaw, e.L2, of);                                                                      \
    }                                                                                                                                   \
    store_env(b, i, e)

// k_step with the curriculum on: k_step's text with the curriculum's reset piece.  A kernel of its own for k_step_log's reason (a
// fifth template argument would rename every k_step variant); the curriculum's pointer travels in this kernel's last argument, and
// KParams and Bufs keep their layout.
template <bool PER_ENV, bool INFO, bool RANDOM_POLICY>
__global__ __launch_bounds__(BLOCK) void k_step_cur(const KParams P, const int n, const Bufs b,
                                                    const float *__restrict__ action, float *__restrict__ action_out,
                                                    float *__restrict__ obs, float *__restrict__ reward,
                                                    uint8_t *__restrict__ done, const Info info, const uint64_t seed,
                                                    const uint64_t policy_seed, const int *__restrict__ cursor,
                                                    const CurDev *cur_arg) {
    __shared__ __attribute__((aligned(16))) float tile[BLOCK * OBS];
    TT_STEP_HEAD();
    TT_STEP_CUR();
    if (valid) {
        TT_STEP_LOADS();
        __builtin_amdgcn_sched_barrier(0);
        TT_STEP_ACT();
        StepOut o;
        step_env(P, e, a, of, o);
        TT_STEP_OUT();
        TT_STEP_RESET_CURRICULUM();
    }
    store_obs_tile(tile, of, valid, obs, block_first, nv, P.nt != 0);
}

// ... and k_step_log with the curriculum on: the same pieces in k_step_log's order
template <bool PER_ENV, bool INFO, bool RANDOM_POLICY>
__global__ __launch_bounds__(BLOCK) void k_step_cur_log(const KParams P, const int n, const Bufs b,
                                                        const float *__restrict__ action, float *__restrict__ action_out,
                                                        float *__restrict__ obs, float *__restrict__ reward,
                                                        uint8_t *__restrict__ done, const Info info, const uint64_t seed,
                                                        const uint64_t policy_seed, const int *__restrict__ cursor,
                                                        const EpLog lg, const CurDev *cur_arg) {
    __shared__ __attribute__((aligned(16))) float tile[BLOCK * OBS];
    TT_STEP_HEAD();
    TT_STEP_CUR();
    if (valid) {
        TT_STEP_LOADS();
        double ret = lg.acc[i];
        __builtin_amdgcn_sched_barrier(0);
        TT_STEP_ACT();
        StepOut o;
        step_env(P, e, a, of, o);
        TT_STEP_OUT();
        TT_STEP_RETURN();
        TT_STEP_RESET_CURRICULUM();
        log_append(lg, i, o.done, o.flags, o.final_bonus > 0.0, len, ret);
    }
    store_obs_tile(tile, of, valid, obs, block_first, nv, P.nt != 0);
    TT_STEP_LAUNCH_COUNT();
}

// k_reset with the curriculum on (k_reset keeps its text): the same reset, the pose from the curriculum's draw
__global__ __launch_bounds__(BLOCK) void k_reset_curriculum(const KParams P, const int n, const Bufs b, const uint8_t *mask,
                                                            float *obs, const uint64_t seed, const CurDev *cur) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n || (mask && !mask[i])) return;
    const uint32_t ep = mask ? b.episodes[i] + 1u : 0u;
    b.episodes[i] = ep;
    double sx, sy, syaw;
    curriculum_pose(cur, seed, (uint32_t)i, ep, sx, sy, syaw);
    float of[OBS];
    const Goal g{P.gx, P.gy, P.sg, P.cg};
    Env e;
    place_env(P, b, i, e, sx, sy, syaw, g, P.gyaw, b.cold[C_L2 * (size_t)P.npad + i], obs ? of : nullptr);
    store_env(b, i, e);
    if (obs)
        for (int j = 0; j < OBS; ++j) obs[(size_t)i * OBS + j] = of[j];
}

// the reset seed into the descriptor (tt_env_reset, tt_env_import; one thread)
__global__ void k_curriculum_seed(CurDev *cur, const uint64_t seed) { cur->seed = seed; }

// lanes placed from outside (tt_env_set_pose, tt_env_set_state): their episode is no curriculum draw's.  Entry j < k names lane
// idx[j] (idx NULL: lane j), as k_log_zero's
__global__ __launch_bounds__(BLOCK) void k_curriculum_unset(const int n, const int k, const int32_t *idx, uint32_t *cell) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= k) return;
    const int i = idx ? idx[j] : j;
    if (i < 0 || i >= n) return;
    cell[i] = TT_CURRICULUM_NO_CELL;
}

// The update (tt_env_curriculum_update): ONE workgroup, thread t owns the cells [t * per, (t + 1) * per), per = ceil(C / BLOCK) <=
// 16.  Per cell with n = attempts > 0: p <- (1 - alpha) p + alpha (s / n), seen += n, both counters 0.  Then for every cell
// f = 4 p (1 - p) (frontier) or 1 - p (hard), w = u + (1 - u) f, q = min(65536, 1 + floor(65535 w)), and cum = the inclusive scan of
// q: each thread's sum, a scan of the BLOCK sums through LDS, each thread's cells again.  f64 elementwise with contraction off, the
// scan in integers (C * 65536 <= 2^28): a pure function of its inputs.
__global__ __launch_bounds__(BLOCK) void k_curriculum_update(const CurDev *cur) {
#pragma clang fp contract(off)
    __shared__ uint32_t part[BLOCK];
    const int C = cur->C, tid = threadIdx.x;
    const int per = (C + BLOCK - 1) / BLOCK;
    const int first = min(C, tid * per), last = min(C, first + per);
    const double alpha = cur->alpha, u = cur->uniform;
    const bool hard = cur->mode == TT_CURRICULUM_HARD;
    uint32_t sum = 0u;
    for (int c = first; c < last; ++c) {
        double p = cur->p[c];
        const uint32_t na = cur->attempts[c];
        if (na > 0u) {
            const uint32_t s = cur->successes[c];
            p = (1.0 - alpha) * p + alpha * ((double)s / (double)na);
            cur->p[c] = p;
            cur->seen[c] += (unsigned long long)na;
            cur->attempts[c] = 0u;
            cur->successes[c] = 0u;
        }
        const double f = hard ? 1.0 - p : 4.0 * p * (1.0 - p);
        const double w = u + (1.0 - u) * f;
        const double x = floor(w * 65535.0);
        const uint32_t q = x >= 65535.0 ? 65536u : (x >= 1.0 ? 1u + (uint32_t)x : 1u);       // (also for a p outside [0, 1] or NaN)
        cur->q[c] = q;
        sum += q;
    }
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < BLOCK; d <<= 1) {
        const uint32_t v = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t run = part[tid] - sum;
    for (int c = first; c < last; ++c) {
        run += cur->q[c];
        cur->cum[c] = run;
    }
}

char g_err[tthost::ERR_BYTES] = "";

}  // namespace

// ==========================================================================================
// host side
struct tt_env {
    int n = 0, npad = 0, device = 0;
    tt_params params{};
    KParams kp{};
    Bufs b{nullptr, nullptr, nullptr, nullptr};
    bool per_env = false;
    uint64_t seed = 0;
    // optional per-launch timing of the step kernel (tt_env_profile): event pairs bound to the dispatch
    bool profiling = false;
    std::vector<hipEvent_t> ev_start, ev_stop;
    size_t ev_used = 0;
    double prof_ms = 0.0;
    long prof_launches = 0;
    // episode log (tt_env_set_episode_log): one device block, EpLog's pointers into it; log_bytes == 0 <=> off
    void *log_block = nullptr;
    size_t log_bytes = 0;
    EpLog log{};
    uint32_t log_flags = 0;     // TT_LOG_DETAIL: the detailed log (k_step_tally)
    void *hold_block = nullptr; // evaluation block (tt_env_set_hold; hold_cols), nullptr <=> off
    // start-pose curriculum (tt_env_set_curriculum): the descriptor in device memory (followed, in the same block, by the arrays
    // the handle owns) and its host copy; cur_dev == nullptr <=> off
    void *cur_block = nullptr;
    CurDev *cur_dev = nullptr;
    CurDev cur{};
    char err[tthost::ERR_BYTES] = "";
};

namespace {

__attribute__((format(printf, 3, 4))) int fail(tt_env *e, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    tthost::vfail(e ? e->err : g_err, code, fmt, ap);
    va_end(ap);
    return code;
}

// a refusal that reads the handle, left where both tt_last_error(env) and tt_last_error(NULL) find it (tthost::fail's message)
__attribute__((format(printf, 3, 4))) int fail_both(tt_env *e, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    tthost::vfail(g_err, code, fmt, ap);
    va_end(ap);
    if (e) std::memcpy(e->err, g_err, tthost::ERR_BYTES);
    return code;
}

// The opening the handle entry points share: a NULL handle is refused in the entry point's own name (an extern "C" function's
// __func__ is its symbol), and TT_ENTER then makes the handle's device current.  Entry points with refusals or an early TT_OK
// between the two keep them there, and those that word the refusal differently ("NULL argument") keep their own.
#define TT_HANDLE(env)                                                                       \
    do {                                                                                     \
        if (!(env)) return fail(nullptr, TT_EINVAL, "%s: NULL handle", __func__);            \
    } while (0)
#define TT_ENTER(env)                                                                        \
    do {                                                                                     \
        TT_HANDLE(env);                                                                      \
        TT_HIP(env, hipSetDevice(env->device));                                              \
    } while (0)

#define TT_HIP(e, call)                                                                      \
    do {                                                                                     \
        hipError_t err_ = (call);                                                            \
        if (err_ != hipSuccess) return fail((e), TT_EHIP, "%s: %s", #call, hipGetErrorString(err_)); \
    } while (0)

// Non-temporal obs / reward / done stores from this many envs on: a step then writes > 200 MB, past every cache level
// (TT_NT_ENVS overrides: 0 = never, 1 = always).
inline int nt_stores_for(int npad) {
    static const long long thr = [] {
        const char *e = std::getenv("TT_NT_ENVS");
        return e ? std::atoll(e) : 2097152ll;
    }();
    return thr > 0 && npad >= thr ? 1 : 0;
}

KParams make_kparams(const tt_params &p, int npad) {
    KParams k{};
    k.v = p.v1x;
    k.v_over_L1 = p.v1x / p.L1;
    k.ho = p.hitch_offset;
    k.h = p.dt;
    k.L2 = p.L2;
    k.gx = p.goal[0]; k.gy = p.goal[1]; k.gyaw = p.goal[2];
    k.sg = std::sin(p.goal[2]); k.cg = std::cos(p.goal[2]);
    k.minx = p.map_min_x; k.maxx = p.map_max_x; k.miny = p.map_min_y; k.maxy = p.map_max_y;
    const double w = p.map_max_x - p.map_min_x, hgt = p.map_max_y - p.map_min_y;
    k.cx = (p.map_max_x + p.map_min_x) / 2; k.cy = (p.map_max_y + p.map_min_y) / 2;
    k.inv_hx = 1.0 / (w / 2); k.inv_hy = 1.0 / (hgt / 2);
    k.inv_M = 1.0 / std::sqrt(w * w + hgt * hgt);
    k.max_steer = p.max_steer;
    k.pos_thr = p.position_threshold; k.ori_thr = p.orientation_threshold;
    k.step_length = p.step_length;
    k.inv_step_length = 1.0 / p.step_length;
    for (int i = 0; i < 3; ++i) { k.rlo[i] = p.reset_lo[i]; k.rhi[i] = p.reset_hi[i]; }
    k.extra_steps = p.extra_steps; k.fixed_max = p.fixed_max_steps;
    k.term_mask = p.term_mask;
    k.npad = npad;
    k.stateless = p.stateless_reward;
    k.pool_m = 0;
    k.pool = nullptr;
    k.nt = nt_stores_for(npad);
    return k;
}

inline int grid_for(int n) { return (n + BLOCK - 1) / BLOCK; }

// the kernels' PER_ENV template argument from the handle: f(std::true_type{}) when envs carry goals / trailer lengths of their own
template <class F>
void by_per_env(const tt_env *env, F &&f) {
    if (env->per_env) f(std::true_type{});
    else f(std::false_type{});
}

template <bool PER_ENV, bool INFO, bool RANDOM_POLICY>
void launch_step(tt_env *e, bool auto_reset, const float *action, float *action_out, float *obs, float *reward,
                 uint8_t *done, const Info &info, uint64_t policy_seed, hipStream_t s, const int *cursor = nullptr) {
    const dim3 g(grid_for(e->n)), b(BLOCK);
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (e->profiling && e->ev_used < e->ev_start.size()) {
        t0 = e->ev_start[e->ev_used];
        t1 = e->ev_stop[e->ev_used];
        e->ev_used += 1;
    }
    // hipExtLaunchKernelGGL with null events is a plain launch; with events they time this dispatch alone.  The argument list is
    // stated once: `kernel` is the chosen instantiation, `log` the trailing EpLog of the two log kernels (nothing for k_step)
    const auto launch = [&](auto kernel, const auto &...log) {
        hipExtLaunchKernelGGL(kernel, g, b, 0, s, t0, t1, 0, e->kp, e->n, e->b, action, action_out, obs, reward, done, info, e->seed,
                              policy_seed, cursor, log...);
    };
    if (e->cur_dev && auto_reset) {     // the curriculum counts and draws where the step resets (never with the detailed log)
        const CurDev *cur = e->cur_dev;
        if (e->log_bytes) launch(k_step_cur_log<PER_ENV, INFO, RANDOM_POLICY>, e->log, cur);
        else launch(k_step_cur<PER_ENV, INFO, RANDOM_POLICY>, cur);
    } else if (e->log_flags & TT_LOG_DETAIL) {
        if (auto_reset) launch(k_step_tally<PER_ENV, INFO, true, RANDOM_POLICY>, e->log);
        else launch(k_step_tally<PER_ENV, INFO, false, RANDOM_POLICY>, e->log);
    } else if (e->log_bytes) {
        if (auto_reset) launch(k_step_log<PER_ENV, INFO, true, RANDOM_POLICY>, e->log);
        else launch(k_step_log<PER_ENV, INFO, false, RANDOM_POLICY>, e->log);
    } else if (auto_reset)
        launch(k_step<PER_ENV, INFO, true, RANDOM_POLICY>);
    else
        launch(k_step<PER_ENV, INFO, false, RANDOM_POLICY>);
}

template <bool RANDOM_POLICY>
int step_common(tt_env *env, const float *action, float *action_out, float *obs, float *reward, uint8_t *done,
                const tt_info *info, int auto_reset, uint64_t policy_seed, hipStream_t stream, const int *cursor = nullptr) {
    Info ki{nullptr, nullptr, nullptr};
    bool want_info = false;
    if (info) {
        ki.comp = info->comp; ki.violation = info->violation; ki.flags = info->flags;
        want_info = ki.comp || ki.violation || ki.flags;
    }
    const auto launch = [&](auto per_env, auto with_info) {
        launch_step<decltype(per_env)::value, decltype(with_info)::value, RANDOM_POLICY>(env, auto_reset != 0, action, action_out, obs,
                                                                                         reward, done, ki, policy_seed, stream, cursor);
    };
    by_per_env(env, [&](auto per_env) {
        if (want_info) launch(per_env, std::true_type{});
        else launch(per_env, std::false_type{});
    });
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(env, TT_EHIP, "tt_env_step launch: %s", hipGetErrorString(err));
    return TT_OK;
}

constexpr long long kLogMaxCapacity = 1ll << 28;
// the accumulator rows of the log: the return's, and with TT_LOG_DETAIL one per reward term
inline int log_acc_rows(uint32_t flags) { return (flags & TT_LOG_DETAIL) ? 1 + TT_LOG_NCOMP : 1; }
size_t log_acc_offset(long long cap, uint32_t flags) {
    return log_records_bytes((unsigned long long)cap) + ((flags & TT_LOG_DETAIL) ? tally_records_bytes((unsigned long long)cap) : 0);
}
size_t log_block_bytes(long long cap, int npad, uint32_t flags) {
    return log_acc_offset(cap, flags) + sizeof(double) * (size_t)log_acc_rows(flags) * (size_t)npad;
}
const char *log_kind(uint64_t flags) { return (flags & TT_LOG_DETAIL) ? "detailed" : "plain"; }

// a lane set starts new episodes outside the step kernel: entry j < k names lane idx[j] (idx NULL: lane j), counted where mask
// is NULL or mask[lane] != 0
int log_restart(tt_env *env, int k, const uint8_t *mask, const int32_t *idx, hipStream_t stream) {
    if (env->log_flags & TT_LOG_DETAIL)
        hipLaunchKernelGGL(k_tally_zero, dim3(grid_for(k)), dim3(BLOCK), 0, stream, env->n, k, mask, idx, env->log, env->npad);
    else
        hipLaunchKernelGGL(k_log_zero, dim3(grid_for(k)), dim3(BLOCK), 0, stream, env->n, k, mask, idx, env->log.acc);
    TT_HIP(env, hipGetLastError());
    return TT_OK;
}

// The packed counters hold 12 bits: tt_env_set_max_steps and tt_env_set_steps refuse what they cannot represent instead of
// clamping (setters, not hot calls).  `values` [k] is device memory; `fn` and `what` name the entry point and its array.
int check_counter_range(tt_env *env, const int32_t *values, int k, hipStream_t stream, const char *fn, const char *what) {
    std::vector<int32_t> host((size_t)k);
    TT_HIP(env, hipMemcpyAsync(host.data(), values, sizeof(int32_t) * (size_t)k, hipMemcpyDeviceToHost, stream));
    TT_HIP(env, hipStreamSynchronize(stream));
    for (int j = 0; j < k; ++j)
        if (host[(size_t)j] < 0 || host[(size_t)j] > TT_MAX_EPISODE_STEPS)
            return fail(env, TT_EINVAL, "%s: %s[%d] = %d outside [0, %d]", fn, what, j, host[(size_t)j], TT_MAX_EPISODE_STEPS);
    return TT_OK;
}

int set_episode_log(tt_env *env, int64_t capacity, uint32_t flags, hipStream_t stream, const char *fn) {
    if (capacity < 0 || capacity > kLogMaxCapacity)
        return fail(env, TT_EINVAL, "%s: capacity %lld outside [0, %lld]", fn, (long long)capacity, kLogMaxCapacity);
    if ((flags & TT_LOG_DETAIL) && capacity > 0 && env->cur_dev)
        return fail_both(env, TT_EINVAL, "%s: the detailed episode log with a curriculum is not supported (the curriculum's step kernels "
                                         "carry the plain log only); tt_env_set_curriculum(env, NULL, ...) first", fn);
    TT_HIP(env, hipSetDevice(env->device));
    if (env->log_block) {       // launches in flight may still write the old block
        TT_HIP(env, hipStreamSynchronize(stream));
        TT_HIP(env, hipDeviceSynchronize());
        TT_HIP(env, hipFree(env->log_block));
        env->log_block = nullptr;
        env->log_bytes = 0;
        env->log = EpLog{};
        env->log_flags = 0;
    }
    if (capacity == 0) return TT_OK;
    const size_t cap = (size_t)capacity, bytes = log_block_bytes(capacity, env->npad, flags);
    void *blk = nullptr;
    hipError_t err = hipMalloc(&blk, bytes);
    if (err != hipSuccess)
        return fail(env, err == hipErrorOutOfMemory ? TT_ENOMEM : TT_EHIP, "%s: %s", fn, hipGetErrorString(err));
    EpLog lg{};
    lg.hdr = static_cast<unsigned long long *>(blk);
    lg.acc = reinterpret_cast<double *>(static_cast<char *>(blk) + log_acc_offset(capacity, flags));
    lg.capacity = (unsigned long long)cap;
    env->log_block = blk;
    env->log_bytes = bytes;
    env->log = lg;
    env->log_flags = flags;
    TT_HIP(env, hipMemsetAsync(blk, 0, bytes, stream));
    if (flags) TT_HIP(env, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(lg.hdr + LG_DETAIL), (int)flags, 1, stream));
    return TT_OK;
}

// lanes placed from outside (entry j < k names lane idx[j], idx NULL: lane j): no curriculum draw made their episode
int curriculum_unset(tt_env *env, int k, const int32_t *idx, hipStream_t stream) {
    if (!env->cur_dev) return TT_OK;
    hipLaunchKernelGGL(k_curriculum_unset, dim3(grid_for(k)), dim3(BLOCK), 0, stream, env->n, k, idx, env->cur.cell);
    TT_HIP(env, hipGetLastError());
    return TT_OK;
}

int drain_episode_log(tt_env *env, double *ret, int32_t *len, uint8_t *flags, uint8_t *success, int32_t *lane, int64_t *end_step,
                      double *comp, double *start, int64_t *n_out, uint64_t *counts_out, hipStream_t stream, const char *fn) {
    if (!env) return fail(nullptr, TT_EINVAL, "%s: NULL handle", fn);
    if (!env->log_bytes) return fail(env, TT_EINVAL, "%s: the episode log is off", fn);
    if ((comp || start) && !(env->log_flags & TT_LOG_DETAIL))
        return fail(env, TT_EINVAL, "%s: comp / start asked of a plain episode log (enable it with TT_LOG_DETAIL)", fn);
    TT_HIP(env, hipSetDevice(env->device));
    const dim3 g(grid_for((int)env->log.capacity));
    hipLaunchKernelGGL(k_log_drain, g, dim3(BLOCK), 0, stream, env->log, ret, len, flags, success, lane,
                       reinterpret_cast<long long *>(end_step), reinterpret_cast<long long *>(n_out),
                       reinterpret_cast<unsigned long long *>(counts_out));
    TT_HIP(env, hipGetLastError());
    if (comp || start) {
        hipLaunchKernelGGL(k_tally_drain, g, dim3(BLOCK), 0, stream, env->log, comp, start);
        TT_HIP(env, hipGetLastError());
    }
    TT_HIP(env, hipMemsetAsync(env->log.hdr + LG_WRITTEN, 0, sizeof(unsigned long long), stream));
    return TT_OK;
}

}  // namespace

extern "C" {

int tt_version(void) { return TT_VERSION; }
#ifdef TT_STAMPS
int tt_debug_log_step(unsigned long long *out, int reset) {      // out: 1 + 2 * TT_LOG_CAP words (count, then begin / end pairs) or NULL
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_log_step), sizeof(TTLog)) != hipSuccess) return -3;
    if (reset) { const unsigned long long z = 0; if (hipMemcpyToSymbol(HIP_SYMBOL(g_log_step), &z, sizeof(z)) != hipSuccess) return -3; }
    return 0;
}
int tt_debug_step_blocks(unsigned long long *out2048) {
    return hipMemcpyFromSymbol(out2048, HIP_SYMBOL(g_stepblk), sizeof(unsigned long long) * 2048) == hipSuccess ? 0 : -3;
}
#endif

const char *tt_last_error(const tt_env *env) { return env ? env->err : g_err; }

int tt_params_default(int variant, tt_params *out) {
    if (!out || (variant != 0 && variant != 1)) return fail(nullptr, TT_EINVAL, "tt_params_default: bad argument");
    std::memset(out, 0, sizeof(*out));
    out->L1 = variant ? 5.74 : 5.0;
    out->L2 = variant ? 10.192 : 7.0;
    out->hitch_offset = 0.0;
    out->v1x = -5.012;
    out->dt = 0.08;
    out->map_min_x = out->map_min_y = -40.0;
    out->map_max_x = out->map_max_y = 40.0;
    out->max_steer = 45.0 * kDeg;
    out->position_threshold = 0.5;
    out->orientation_threshold = 15.0 * kDeg;
    out->step_length = 0.40096;
    out->extra_steps = 75;
    out->fixed_max_steps = variant ? 300 : 0;
    out->term_mask = variant ? TT_TERM_SIMV1 : TT_TERM_SIMV2;
    out->variant = variant;
    out->stateless_reward = variant ? 1 : 0;
    out->goal[0] = 0.0; out->goal[1] = -30.0; out->goal[2] = 90.0 * kDeg;
    out->reset_lo[0] = -27.0; out->reset_hi[0] = 27.0;
    out->reset_lo[1] = 0.0; out->reset_hi[1] = 27.0;
    out->reset_lo[2] = 45.0 * kDeg; out->reset_hi[2] = 120.0 * kDeg;
    return TT_OK;
}

int tt_env_create(int n_envs, int device, const tt_params *params, tt_env **out) {
    if (!out) return fail(nullptr, TT_EINVAL, "tt_env_create: out is NULL");
    *out = nullptr;
    if (n_envs <= 0) return fail(nullptr, TT_EINVAL, "tt_env_create: n_envs must be positive (got %d)", n_envs);
    tt_params p;
    if (params) p = *params;
    else tt_params_default(0, &p);
    if (!(p.L1 > 0.0) || !(p.L2 > 0.0) || !(p.dt > 0.0) || !(p.step_length > 0.0) || !(p.map_max_x > p.map_min_x) ||
        !(p.map_max_y > p.map_min_y))
        return fail(nullptr, TT_EINVAL, "tt_env_create: non-physical parameters");
    // the in-step heading increments must stay small-angle (tt_sincos_small): dt*|v|*tan(max_steer)/L1 and dt*|v|/L2
    const double turn = std::fabs(p.dt * p.v1x) * std::fmax(std::tan(std::fabs(p.max_steer)) / p.L1, 1.0 / p.L2);
    if (!(turn <= 0.25) || !(std::fabs(p.max_steer) < 1.5))
        return fail(nullptr, TT_EINVAL, "tt_env_create: dt*|v|/L = %.3f rad per step exceeds the 0.25 rad the integrator's "
                                        "small-angle stage rotations are sized for", turn);
    {   // episode lengths must fit the 12-bit packed counters (steps | max_episode_steps)
        const double w = p.map_max_x - p.map_min_x, hgt = p.map_max_y - p.map_min_y;
        const double longest = p.fixed_max_steps > 0 ? (double)p.fixed_max_steps
                                                     : std::sqrt(w * w + hgt * hgt) * 1.5 / p.step_length + p.extra_steps;
        if (p.fixed_max_steps < 0 || p.extra_steps < 0 || !(longest <= (double)TT_MAX_EPISODE_STEPS))
            return fail(nullptr, TT_EINVAL, "tt_env_create: episodes of up to %.0f steps exceed the %d the packed counters hold",
                        longest, TT_MAX_EPISODE_STEPS);
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(nullptr, TT_ENODEV, "tt_env_create: no HIP device visible");
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) device = 0;
    }
    if (device >= count) return fail(nullptr, TT_ENODEV, "tt_env_create: device %d of %d", device, count);
    tt_env *e = new (std::nothrow) tt_env;
    if (!e) return fail(nullptr, TT_ENOMEM, "tt_env_create: host allocation failed");
    e->n = n_envs;
    e->npad = (n_envs + TILE - 1) / TILE * TILE;
    e->device = device;
    e->params = p;
    e->kp = make_kparams(p, e->npad);
    const size_t npad = (size_t)e->npad;
    hipError_t err = hipSetDevice(device);
    if (err == hipSuccess) err = hipMalloc(&e->b.hot, sizeof(double) * H_ROWS * npad);
    if (err == hipSuccess) err = hipMalloc(&e->b.cold, sizeof(double) * C_ROWS * npad);
    if (err == hipSuccess) err = hipMalloc(&e->b.episodes, sizeof(uint32_t) * npad);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(k_init, dim3(grid_for(e->npad)), dim3(BLOCK), 0, nullptr, e->kp, e->b);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipStreamSynchronize(nullptr);
    if (err != hipSuccess) {
        const int code = err == hipErrorOutOfMemory ? TT_ENOMEM : TT_EHIP;
        fail(nullptr, code, "tt_env_create: %s", hipGetErrorString(err));
        tt_env_destroy(e);
        return code;
    }
    *out = e;
    return TT_OK;
}

int tt_env_destroy(tt_env *env) {
    if (!env) return TT_OK;
    (void)hipSetDevice(env->device);
    if (env->b.hot) (void)hipFree(env->b.hot);
    if (env->b.cold) (void)hipFree(env->b.cold);
    if (env->b.episodes) (void)hipFree(env->b.episodes);
    if (env->log_block) (void)hipFree(env->log_block);
    if (env->hold_block) (void)hipFree(env->hold_block);
    if (env->cur_block) (void)hipFree(env->cur_block);
    for (hipEvent_t ev : env->ev_start) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : env->ev_stop) (void)hipEventDestroy(ev);
    delete env;
    return TT_OK;
}

int tt_env_num_envs(const tt_env *env) { return env ? env->n : TT_EINVAL; }

int tt_env_reset(tt_env *env, const uint8_t *mask, uint64_t seed, float *obs_out, tt_stream_t stream) {
    TT_ENTER(env);
    env->seed = seed;
    if (env->cur_dev) {
        hipLaunchKernelGGL(k_curriculum_seed, dim3(1), dim3(1), 0, stream, env->cur_dev, env->seed);
        hipLaunchKernelGGL(k_reset_curriculum, dim3(grid_for(env->n)), dim3(BLOCK), 0, stream, env->kp, env->n, env->b, mask, obs_out,
                           env->seed, (const CurDev *)env->cur_dev);
    } else
        hipLaunchKernelGGL(k_reset, dim3(grid_for(env->n)), dim3(BLOCK), 0, stream, env->kp, env->n, env->b, mask, obs_out,
                           env->seed);
    TT_HIP(env, hipGetLastError());
    if (env->log_bytes) {       // the reset lanes' episodes start from a zero return (and zero term sums)
        if (mask)
            return log_restart(env, env->n, mask, nullptr, stream);
        TT_HIP(env, hipMemsetAsync(env->log.acc, 0, sizeof(double) * (size_t)log_acc_rows(env->log_flags) * (size_t)env->npad,
                                   stream));
    }
    return TT_OK;
}

int tt_env_set_reset_pool(tt_env *env, const double *pool, int m) {
    TT_HANDLE(env);
    if (m < 0) return fail(env, TT_EINVAL, "tt_env_set_reset_pool: m=%d", m);
    if (pool && m > 0 && env->cur_dev)
        return fail_both(env, TT_EINVAL, "tt_env_set_reset_pool: a reset pool with a curriculum is not supported (the curriculum draws "
                                         "from the reset box); tt_env_set_curriculum(env, NULL, ...) first");
    env->kp.pool_m = pool ? m : 0;
    env->kp.pool = env->kp.pool_m > 0 ? pool : nullptr;
    return TT_OK;
}

int tt_env_set_pose(tt_env *env, const int32_t *idx, int k, const double *start, const double *goal, const double *L2,
                    float *obs_out, tt_stream_t stream) {
    TT_HANDLE(env);
    if (k < 0 || k > env->n || (k > 0 && !start))
        return fail(env, TT_EINVAL, "tt_env_set_pose: k=%d outside [0,%d] or start NULL", k, env->n);
    if (k == 0) return TT_OK;
    TT_HIP(env, hipSetDevice(env->device));
    if (goal || L2) env->per_env = true;
    hipLaunchKernelGGL(k_set_pose, dim3(grid_for(k)), dim3(BLOCK), 0, stream, env->kp, env->n, env->b, idx, k, start, goal,
                       L2, obs_out);
    TT_HIP(env, hipGetLastError());
    if (const int rc = curriculum_unset(env, k, idx, stream)) return rc;
    if (env->log_bytes) return log_restart(env, k, nullptr, idx, stream);
    return TT_OK;
}

int tt_env_set_attrs(tt_env *env, const int32_t *idx, int k, const double *start, const double *goal, const double *L2,
                     tt_stream_t stream) {
    TT_HANDLE(env);
    if (k < 0 || k > env->n) return fail(env, TT_EINVAL, "tt_env_set_attrs: k=%d outside [0,%d]", k, env->n);
    if (k == 0 || (!start && !goal && !L2)) return TT_OK;
    TT_HIP(env, hipSetDevice(env->device));
    if (goal || L2) env->per_env = true;
    hipLaunchKernelGGL(k_set_attrs, dim3(grid_for(k)), dim3(BLOCK), 0, stream, env->kp, env->n, env->b, idx, k, start, goal,
                       L2);
    TT_HIP(env, hipGetLastError());
    return TT_OK;
}

int tt_env_set_state(tt_env *env, const int32_t *idx, int k, const double *state, tt_stream_t stream) {
    TT_HANDLE(env);
    if (k < 0 || k > env->n || (k > 0 && !state))
        return fail(env, TT_EINVAL, "tt_env_set_state: k=%d outside [0,%d] or state NULL", k, env->n);
    if (k == 0) return TT_OK;
    TT_HIP(env, hipSetDevice(env->device));
    hipLaunchKernelGGL(k_set_state, dim3(grid_for(k)), dim3(BLOCK), 0, stream, env->n, env->b, idx, k, state);
    TT_HIP(env, hipGetLastError());
    return curriculum_unset(env, k, idx, stream);
}

int tt_env_get_state(tt_env *env, double *state_out, tt_stream_t stream) {
    if (!env || !state_out) return fail(env, TT_EINVAL, "tt_env_get_state: NULL argument");
    TT_HIP(env, hipSetDevice(env->device));
    hipLaunchKernelGGL(k_get_state, dim3(grid_for(env->n)), dim3(BLOCK), 0, stream, env->n, env->b, state_out);
    TT_HIP(env, hipGetLastError());
    return TT_OK;
}

int tt_env_set_max_steps(tt_env *env, const int32_t *idx, int k, const int32_t *max_steps, tt_stream_t stream) {
    TT_HANDLE(env);
    if (k < 0 || k > env->n || (k > 0 && !max_steps))
        return fail(env, TT_EINVAL, "tt_env_set_max_steps: k=%d outside [0,%d] or max_steps NULL", k, env->n);
    if (k == 0) return TT_OK;
    TT_HIP(env, hipSetDevice(env->device));
    if (const int rc = check_counter_range(env, max_steps, k, stream, __func__, "max_steps")) return rc;
    hipLaunchKernelGGL(k_set_max_steps, dim3(grid_for(k)), dim3(BLOCK), 0, stream, env->n, env->b, idx, k, max_steps);
    TT_HIP(env, hipGetLastError());
    return TT_OK;
}

int tt_env_set_steps(tt_env *env, const int32_t *idx, int k, const int32_t *steps, tt_stream_t stream) {
    TT_HANDLE(env);
    if (k < 0 || k > env->n || (k > 0 && !steps))
        return fail(env, TT_EINVAL, "tt_env_set_steps: k=%d outside [0,%d] or steps NULL", k, env->n);
    if (k == 0) return TT_OK;
    TT_HIP(env, hipSetDevice(env->device));
    if (const int rc = check_counter_range(env, steps, k, stream, __func__, "steps")) return rc;
    hipLaunchKernelGGL(k_set_steps, dim3(grid_for(k)), dim3(BLOCK), 0, stream, env->n, env->b, idx, k, steps);
    TT_HIP(env, hipGetLastError());
    return TT_OK;
}

int tt_env_get_episode(tt_env *env, int32_t *steps, int32_t *max_steps, double *start, double *goal, double *L2,
                       tt_stream_t stream) {
    TT_HANDLE(env);
    if (!steps && !max_steps && !start && !goal && !L2) return TT_OK;
    TT_HIP(env, hipSetDevice(env->device));
    hipLaunchKernelGGL(k_get_episode, dim3(grid_for(env->n)), dim3(BLOCK), 0, stream, env->kp, env->n, env->b, steps,
                       max_steps, start, goal, L2);
    TT_HIP(env, hipGetLastError());
    return TT_OK;
}

int tt_env_observe(tt_env *env, const float *steering, float *obs_out, tt_stream_t stream) {
    if (!env || !obs_out) return fail(env, TT_EINVAL, "tt_env_observe: NULL argument");
    TT_HIP(env, hipSetDevice(env->device));
    by_per_env(env, [&](auto per_env) {
        hipLaunchKernelGGL(k_observe<decltype(per_env)::value>, dim3(grid_for(env->n)), dim3(BLOCK), 0, stream, env->kp, env->n, env->b,
                           steering, obs_out);
    });
    TT_HIP(env, hipGetLastError());
    return TT_OK;
}

int tt_env_set_step_counter(tt_env *env, int64_t *counter) {
    TT_HANDLE(env);
    env->b.counter = reinterpret_cast<long long *>(counter);
    return TT_OK;
}

int tt_env_step(tt_env *env, const float *action, float *obs, float *reward, uint8_t *done, const tt_info *info,
                int auto_reset, tt_stream_t stream) {
    TT_HANDLE(env);
    if (!action || !obs || !reward || !done)
        return fail(env, TT_EINVAL, "tt_env_step: action, obs, reward and done are required");
    TT_HIP(env, hipSetDevice(env->device));
    return step_common<false>(env, action, nullptr, obs, reward, done, info, auto_reset, 0, stream);
}

int tt_env_step_ring(tt_env *env, const float *action, const tt_ring_view *ring, int auto_reset, tt_stream_t stream) {
    TT_HANDLE(env);
    if (!action || !ring || !ring->cursor || !ring->obs || !ring->rew || !ring->done || ring->n_envs != env->n)
        return fail(env, TT_EINVAL, "tt_env_step_ring: action and a ring view of this handle's %d envs are required", env->n);
    TT_HIP(env, hipSetDevice(env->device));
    return step_common<false>(env, action, nullptr, ring->obs, ring->rew, ring->done, nullptr, auto_reset, 0, stream, ring->cursor);
}

int tt_env_step_random(tt_env *env, uint64_t policy_seed, float *action_out, float *obs, float *reward, uint8_t *done,
                       const tt_info *info, int auto_reset, tt_stream_t stream) {
    TT_HANDLE(env);
    if (!obs || !reward || !done) return fail(env, TT_EINVAL, "tt_env_step_random: obs, reward and done are required");
    TT_HIP(env, hipSetDevice(env->device));
    return step_common<true>(env, nullptr, action_out, obs, reward, done, info, auto_reset, policy_seed, stream);
}

size_t tt_env_state_bytes(const tt_env *env) {
    if (!env) return 0;
    const size_t npad = (size_t)env->npad;
    return sizeof(double) * (H_ROWS + C_ROWS) * npad + sizeof(uint32_t) * npad;
}

int tt_env_export(tt_env *env, void *blob, uint64_t meta[4], tt_stream_t stream) {
    if (!env || !blob || !meta) return fail(env, TT_EINVAL, "tt_env_export: NULL argument");
    TT_HIP(env, hipSetDevice(env->device));
    const size_t npad = (size_t)env->npad, hb = sizeof(double) * H_ROWS * npad, cb = sizeof(double) * C_ROWS * npad;
    char *dst = static_cast<char *>(blob);
    TT_HIP(env, hipMemcpyAsync(dst, env->b.hot, hb, hipMemcpyDeviceToDevice, stream));
    TT_HIP(env, hipMemcpyAsync(dst + hb, env->b.cold, cb, hipMemcpyDeviceToDevice, stream));
    TT_HIP(env, hipMemcpyAsync(dst + hb + cb, env->b.episodes, sizeof(uint32_t) * npad, hipMemcpyDeviceToDevice, stream));
    meta[0] = env->per_env ? 1 : 0; meta[1] = env->seed; meta[2] = (uint64_t)env->n; meta[3] = TT_VERSION;
    return TT_OK;
}

int tt_env_import(tt_env *env, const void *blob, const uint64_t meta[4], tt_stream_t stream) {
    if (!env || !blob || !meta) return fail(env, TT_EINVAL, "tt_env_import: NULL argument");
    if (meta[2] != (uint64_t)env->n || meta[3] != TT_VERSION)
        return fail(env, TT_EINVAL, "tt_env_import: blob is for %llu envs (version %llu), handle has %d (version %d)",
                    (unsigned long long)meta[2], (unsigned long long)meta[3], env->n, TT_VERSION);
    TT_HIP(env, hipSetDevice(env->device));
    const size_t npad = (size_t)env->npad, hb = sizeof(double) * H_ROWS * npad, cb = sizeof(double) * C_ROWS * npad;
    const char *src = static_cast<const char *>(blob);
    TT_HIP(env, hipMemcpyAsync(env->b.hot, src, hb, hipMemcpyDeviceToDevice, stream));
    TT_HIP(env, hipMemcpyAsync(env->b.cold, src + hb, cb, hipMemcpyDeviceToDevice, stream));
    TT_HIP(env, hipMemcpyAsync(env->b.episodes, src + hb + cb, sizeof(uint32_t) * npad, hipMemcpyDeviceToDevice, stream));
    env->per_env = meta[0] != 0;
    env->seed = meta[1];
    if (env->cur_dev) {
        hipLaunchKernelGGL(k_curriculum_seed, dim3(1), dim3(1), 0, stream, env->cur_dev, env->seed);
        TT_HIP(env, hipGetLastError());
    }
    return TT_OK;
}

int tt_env_set_episode_log(tt_env *env, int64_t capacity, tt_stream_t stream) {
    TT_HANDLE(env);
    return set_episode_log(env, capacity, 0u, stream, "tt_env_set_episode_log");
}

int tt_env_set_episode_log2(tt_env *env, int64_t capacity, uint32_t flags, tt_stream_t stream) {
    if (flags & ~(uint32_t)TT_LOG_DETAIL)
        return fail(env, TT_EINVAL, "tt_env_set_episode_log2: unknown flag bits 0x%x", flags & ~(uint32_t)TT_LOG_DETAIL);
    TT_HANDLE(env);
    return set_episode_log(env, capacity, flags, stream, "tt_env_set_episode_log2");
}

int tt_env_drain_episode_log(tt_env *env, double *ret, int32_t *len, uint8_t *flags, uint8_t *success, int32_t *lane,
                             int64_t *end_step, int64_t *n_out, uint64_t *counts_out, tt_stream_t stream) {
    return drain_episode_log(env, ret, len, flags, success, lane, end_step, nullptr, nullptr, n_out, counts_out, stream,
                             "tt_env_drain_episode_log");
}

int tt_env_drain_episode_log2(tt_env *env, double *ret, int32_t *len, uint8_t *flags, uint8_t *success, int32_t *lane,
                              int64_t *end_step, double *comp, double *start, int64_t *n_out, uint64_t *counts_out,
                              tt_stream_t stream) {
    return drain_episode_log(env, ret, len, flags, success, lane, end_step, comp, start, n_out, counts_out, stream,
                             "tt_env_drain_episode_log2");
}

size_t tt_env_episode_log_bytes(const tt_env *env) { return env ? env->log_bytes : 0; }

int tt_env_export_episode_log(tt_env *env, void *blob, uint64_t meta[2], tt_stream_t stream) {
    if (!env || !blob || !meta) return fail(env, TT_EINVAL, "tt_env_export_episode_log: NULL argument");
    if (!env->log_bytes) return fail(env, TT_EINVAL, "tt_env_export_episode_log: the episode log is off");
    TT_HIP(env, hipSetDevice(env->device));
    TT_HIP(env, hipMemcpyAsync(blob, env->log_block, env->log_bytes, hipMemcpyDeviceToDevice, stream));
    meta[0] = env->log.capacity; meta[1] = (uint64_t)env->n;
    return TT_OK;
}

int tt_env_import_episode_log(tt_env *env, const void *blob, const uint64_t meta[2], tt_stream_t stream) {
    if (!env || !blob || !meta) return fail(env, TT_EINVAL, "tt_env_import_episode_log: NULL argument");
    if (!env->log_bytes || meta[0] != env->log.capacity || meta[1] != (uint64_t)env->n)
        return fail(env, TT_EINVAL, "tt_env_import_episode_log: blob is for capacity %llu and %llu envs, the handle's log has "
                                    "capacity %llu (0 = off) and %d envs", (unsigned long long)meta[0],
                    (unsigned long long)meta[1], env->log.capacity, env->n);
    TT_HIP(env, hipSetDevice(env->device));
    // the blob's own header says which kind of log wrote it (a plain blob is shorter than a detailed log's block)
    uint64_t kind = 0;
    TT_HIP(env, hipMemcpyAsync(&kind, static_cast<const unsigned long long *>(blob) + LG_DETAIL, sizeof(kind),
                               hipMemcpyDeviceToHost, stream));
    TT_HIP(env, hipStreamSynchronize(stream));
    if (kind != env->log_flags)
        return fail(env, TT_EINVAL, "tt_env_import_episode_log: the blob is of a %s episode log, the handle's log is %s",
                    log_kind(kind), log_kind(env->log_flags));
    TT_HIP(env, hipMemcpyAsync(env->log_block, blob, env->log_bytes, hipMemcpyDeviceToDevice, stream));
    return TT_OK;
}

int tt_env_set_hold(tt_env *env, int on, tt_stream_t stream) {
    TT_ENTER(env);
    if (env->hold_block) {      // launches in flight may still write the old block
        TT_HIP(env, hipStreamSynchronize(stream));
        TT_HIP(env, hipDeviceSynchronize());
        TT_HIP(env, hipFree(env->hold_block));
        env->hold_block = nullptr;
    }
    if (!on) return TT_OK;
    const size_t bytes = hold_block_bytes(env->npad);
    void *blk = nullptr;
    hipError_t err = hipMalloc(&blk, bytes);
    if (err != hipSuccess)
        return fail(env, err == hipErrorOutOfMemory ? TT_ENOMEM : TT_EHIP, "tt_env_set_hold: %s", hipGetErrorString(err));
    env->hold_block = blk;
    TT_HIP(env, hipMemsetAsync(blk, 0, bytes, stream));     // nothing live until tt_env_hold_begin
    return TT_OK;
}

int tt_env_hold_begin(tt_env *env, tt_stream_t stream) {
    TT_HANDLE(env);
    if (!env->hold_block) return fail(env, TT_EINVAL, "tt_env_hold_begin: hold is not enabled (tt_env_set_hold)");
    TT_HIP(env, hipSetDevice(env->device));
    hipLaunchKernelGGL(k_hold_begin, dim3(grid_for(env->npad)), dim3(BLOCK), 0, stream, env->n, env->npad, env->hold_block);
    TT_HIP(env, hipGetLastError());
    return TT_OK;
}

int tt_env_step_hold(tt_env *env, const float *mu, float action_scale, float *obs, tt_stream_t stream) {
    TT_HANDLE(env);
    // (before the handle is read: these hold for any handle)
    if (!mu || !obs) return tthost::fail(TT_EINVAL, "tt_env_step_hold: mu and obs are required");
    if (!std::isfinite(action_scale)) return tthost::fail(TT_EINVAL, "tt_env_step_hold: action_scale is not finite");
    if (!env->hold_block) return fail(env, TT_EINVAL, "tt_env_step_hold: hold is not enabled (tt_env_set_hold)");
    TT_HIP(env, hipSetDevice(env->device));
    by_per_env(env, [&](auto per_env) {
        hipLaunchKernelGGL(k_step_hold<decltype(per_env)::value>, dim3(grid_for(env->n)), dim3(BLOCK), 0, stream, env->kp, env->n,
                           env->b, mu, action_scale, obs, env->hold_block);
    });
    TT_HIP(env, hipGetLastError());
    return TT_OK;
}

int tt_env_hold_read(tt_env *env, double *ret, int32_t *len, uint8_t *flags, uint8_t *success, double *end, int64_t *live_out,
                     tt_stream_t stream) {
    TT_HANDLE(env);
    if (!env->hold_block) return fail(env, TT_EINVAL, "tt_env_hold_read: hold is not enabled (tt_env_set_hold)");
    TT_HIP(env, hipSetDevice(env->device));
    if (ret || len || flags || success || end) {
        hipLaunchKernelGGL(k_hold_read, dim3(grid_for(env->n)), dim3(BLOCK), 0, stream, env->n, env->npad, env->hold_block, ret, len,
                           flags, success, end);
        TT_HIP(env, hipGetLastError());
    }
    if (live_out) {
        hipLaunchKernelGGL(k_hold_live, dim3(1), dim3(BLOCK), 0, stream, env->npad, env->hold_block,
                           reinterpret_cast<long long *>(live_out));
        TT_HIP(env, hipGetLastError());
    }
    return TT_OK;
}

int tt_env_rollout_random(tt_env *env, int k_steps, uint64_t policy_seed, float *obs_out, float *reward_sum,
                          int32_t *episodes_done, tt_stream_t stream) {
    TT_HANDLE(env);
    if (k_steps < 0) return fail(env, TT_EINVAL, "tt_env_rollout_random: k_steps=%d", k_steps);
    if (env->log_bytes) return fail(env, TT_EINVAL, "tt_env_rollout_random: the episode log does not follow k_rollout; disable it first");
    if (env->cur_dev) return fail(env, TT_EINVAL, "tt_env_rollout_random: the curriculum does not follow k_rollout; turn it off first");
    if (k_steps == 0) return TT_OK;
    TT_HIP(env, hipSetDevice(env->device));
    by_per_env(env, [&](auto per_env) {
        hipLaunchKernelGGL(k_rollout<decltype(per_env)::value>, dim3(grid_for(env->n)), dim3(BLOCK), 0, stream, env->kp, env->n, env->b,
                           k_steps, obs_out, reward_sum, episodes_done, env->seed, policy_seed);
    });
    TT_HIP(env, hipGetLastError());
    return TT_OK;
}

// what both planning entry points refuse of a tt_mpc_args (TT_EINVAL with "<who>: <reason>", no handle read, no HIP call), and the
// kernel's constants and dynamic LDS bytes of one that passes
static int mpc_constants(const char *who, const tt_mpc_args &a, MpcK &m, size_t &lds) {
    static_assert(TT_MPC_MAX_HORIZON <= BLOCK && TT_MPC_MAX_HORIZON <= 64 && TT_MPC_MAX_SAMPLES <= 1024,
                  "k_mpc_plan: a thread per plan entry; 6 bits of t and 10 bits of s in the noise counter");
    if (a.horizon < 1 || a.horizon > TT_MPC_MAX_HORIZON)
        return tthost::fail(TT_EINVAL, "%s: horizon %d outside [1, %d]", who, a.horizon, TT_MPC_MAX_HORIZON);
    if (a.samples < 1 || a.samples > TT_MPC_MAX_SAMPLES)
        return tthost::fail(TT_EINVAL, "%s: samples %d outside [1, %d]", who, a.samples, TT_MPC_MAX_SAMPLES);
    if (!std::isfinite(a.sigma) || a.sigma < 0.f) return tthost::fail(TT_EINVAL, "%s: sigma is negative or not finite", who);
    if (!std::isfinite(a.k_lat) || a.k_lat < 0.f) return tthost::fail(TT_EINVAL, "%s: k_lat is negative or not finite", who);
    if (!std::isfinite(a.k_yaw) || a.k_yaw < 0.f) return tthost::fail(TT_EINVAL, "%s: k_yaw is negative or not finite", who);
    if (!(a.rho >= 0.f && a.rho < 1.f)) return tthost::fail(TT_EINVAL, "%s: rho is outside [0, 1)", who);
    if (!std::isfinite(a.lambda) || !(a.lambda > 0.f)) return tthost::fail(TT_EINVAL, "%s: lambda is not finite or <= 0", who);
    if (!(a.gamma > 0.f && a.gamma <= 1.f)) return tthost::fail(TT_EINVAL, "%s: gamma is outside (0, 1]", who);
    if (!std::isfinite(a.action_scale) || !(a.action_scale > 0.f))
        return tthost::fail(TT_EINVAL, "%s: action_scale is not finite or <= 0", who);
    m = MpcK{};
    m.H = a.horizon; m.S = a.samples;
    const int hp = m.H | 1;
    m.chunk = MPC_TILE_FLOATS / hp < BLOCK ? MPC_TILE_FLOATS / hp : BLOCK;
    m.action_scale = a.action_scale;
    m.sigma = (double)a.sigma; m.rho = (double)a.rho;
    m.sigma_c = std::sqrt(1.0 - m.rho * m.rho) * m.sigma;
    m.lambda = (double)a.lambda; m.gamma = (double)a.gamma; m.k_lat = (double)a.k_lat; m.k_yaw = (double)a.k_yaw;
    m.seed = a.seed;
    lds = sizeof(double) * ((size_t)m.S + BLOCK) + sizeof(float) * ((size_t)((m.H + 3) & ~3) + (size_t)m.chunk * hp);
    return TT_OK;
}

int tt_env_mpc_plan(tt_env *env, const tt_mpc_args *args, float *plan, float *mu_out, const uint8_t *live, double *returns_out,
                    tt_stream_t stream) {
    TT_HANDLE(env);
    // (before the handle is read: these hold for any handle)
    if (!args || !plan || !mu_out) return tthost::fail(TT_EINVAL, "tt_env_mpc_plan: args, plan and mu_out are required");
    MpcK m;
    size_t lds;
    if (const int rc = mpc_constants("tt_env_mpc_plan", *args, m, lds)) return rc;
    TT_HIP(env, hipSetDevice(env->device));
    by_per_env(env, [&](auto per_env) {
        hipLaunchKernelGGL(k_mpc_plan<decltype(per_env)::value>, dim3(env->n), dim3(BLOCK), lds, stream, env->kp, env->n, env->b, m,
                           plan, mu_out, live, returns_out);
    });
    TT_HIP(env, hipGetLastError());
    return TT_OK;
}

int tt_env_mpc_act_ring(tt_env *env, const tt_mpc_args *args, float *plan, int32_t lanes, const tt_ring_view *ring, float high,
                        float *act_scaled, tt_stream_t stream) {
    const char *const who = "tt_env_mpc_act_ring";
    TT_HANDLE(env);
    // (before the handle is read: these hold for any handle)
    if (!args || !plan || !ring || !act_scaled) return tthost::fail(TT_EINVAL, "%s: args, plan, ring and act_scaled are required", who);
    if (!ring->cursor || !ring->act) return tthost::fail(TT_EINVAL, "%s: ring->cursor and ring->act are required", who);
    if (ring->slots < 1) return tthost::fail(TT_EINVAL, "%s: a ring of %d slots", who, ring->slots);
    if (lanes < 1 || lanes > ring->n_envs)
        return tthost::fail(TT_EINVAL, "%s: lanes %d outside [1, n_envs = %d]", who, lanes, ring->n_envs);
    if (!std::isfinite(high) || !(high > 0.f)) return tthost::fail(TT_EINVAL, "%s: high is not finite or <= 0", who);
    MpcK m;
    size_t lds;
    if (const int rc = mpc_constants(who, *args, m, lds)) return rc;
    if (ring->n_envs != env->n) return tthost::fail(TT_EINVAL, "%s: the ring view has %d envs, this handle %d", who, ring->n_envs, env->n);
    const MpcRing r{ring->cursor, ring->act, act_scaled, ring->n_envs, ring->slots, high};
    TT_HIP(env, hipSetDevice(env->device));
    by_per_env(env, [&](auto per_env) {
        hipLaunchKernelGGL(k_mpc_act_ring<decltype(per_env)::value>, dim3(lanes), dim3(BLOCK), lds, stream, env->kp, (int)lanes, env->b, m,
                           plan, r);
    });
    TT_HIP(env, hipGetLastError());
    return TT_OK;
}

int tt_env_mpc_label_ring(tt_env *env, const tt_mpc_args *args, float *plan, int32_t expert_lanes, int32_t label_lanes,
                          const tt_ring_view *ring, float *label, float high, float *act_scaled, tt_stream_t stream) {
    const char *const who = "tt_env_mpc_label_ring";
    TT_HANDLE(env);
    // (before the handle is read: these hold for any handle)
    if (!args || !plan || !ring || !label) return tthost::fail(TT_EINVAL, "%s: args, plan, ring and label are required", who);
    if (expert_lanes < 0) return tthost::fail(TT_EINVAL, "%s: expert_lanes = %d is negative", who, (int)expert_lanes);
    if (label_lanes < 1) return tthost::fail(TT_EINVAL, "%s: label_lanes = %d, not >= 1", who, (int)label_lanes);
    if (!ring->cursor) return tthost::fail(TT_EINVAL, "%s: ring->cursor is required", who);
    if (expert_lanes > 0 && (!ring->act || !act_scaled))
        return tthost::fail(TT_EINVAL, "%s: ring->act and act_scaled are required with expert_lanes > 0", who);
    if (ring->slots < 1) return tthost::fail(TT_EINVAL, "%s: a ring of %d slots", who, ring->slots);
    if ((int64_t)expert_lanes + (int64_t)label_lanes > (int64_t)ring->n_envs)
        return tthost::fail(TT_EINVAL, "%s: expert_lanes + label_lanes = %d + %d is more than n_envs = %d", who, (int)expert_lanes,
                            (int)label_lanes, ring->n_envs);
    if (!std::isfinite(high) || !(high > 0.f)) return tthost::fail(TT_EINVAL, "%s: high is not finite or <= 0", who);
    MpcK m;
    size_t lds;
    if (const int rc = mpc_constants(who, *args, m, lds)) return rc;
    if (ring->n_envs != env->n) return tthost::fail(TT_EINVAL, "%s: the ring view has %d envs, this handle %d", who, ring->n_envs, env->n);
    const int lanes = (int)(expert_lanes + label_lanes);
    const MpcLabel r{ring->cursor, ring->act, act_scaled, label, ring->n_envs, ring->slots, high, (int)expert_lanes};
    TT_HIP(env, hipSetDevice(env->device));
    by_per_env(env, [&](auto per_env) {
        hipLaunchKernelGGL(k_mpc_label_ring<decltype(per_env)::value>, dim3(lanes), dim3(BLOCK), lds, stream, env->kp, lanes, env->b, m,
                           plan, r);
    });
    TT_HIP(env, hipGetLastError());
    return TT_OK;
}

// ---- start-pose curriculum (include/ttenv.h: tt_env_set_curriculum)
static size_t cur_align(size_t x) { return (x + 255) & ~(size_t)255; }

int tt_env_set_curriculum(tt_env *env, const tt_curriculum *cfg, const tt_curriculum_arrays *place, tt_stream_t stream) {
    const char *const who = "tt_env_set_curriculum";
    TT_HANDLE(env);
    long long C = 0;
    if (cfg) {      // (before the handle is read: these hold for any handle)
        if (cfg->nx < 1 || cfg->ny < 1 || cfg->nyaw < 1)
            return tthost::fail(TT_EINVAL, "%s: bins (%d, %d, %d): a bin count below 1", who, cfg->nx, cfg->ny, cfg->nyaw);
        C = (long long)cfg->nx * cfg->ny * cfg->nyaw;
        if (C > TT_CURRICULUM_MAX_CELLS)
            return tthost::fail(TT_EINVAL, "%s: bins (%d, %d, %d) make %lld cells, outside [1, %d]", who, cfg->nx, cfg->ny, cfg->nyaw, C,
                                TT_CURRICULUM_MAX_CELLS);
        if (cfg->mode != TT_CURRICULUM_FRONTIER && cfg->mode != TT_CURRICULUM_HARD)
            return tthost::fail(TT_EINVAL, "%s: unknown mode %d", who, cfg->mode);
        if (!(cfg->alpha > 0.0 && cfg->alpha <= 1.0)) return tthost::fail(TT_EINVAL, "%s: alpha is outside (0, 1]", who);
        if (!std::isfinite(cfg->uniform) || !(cfg->uniform >= 0.0 && cfg->uniform <= 1.0))
            return tthost::fail(TT_EINVAL, "%s: uniform is outside [0, 1] or not finite", who);
        if (place && (!place->p || !place->seen || !place->attempts || !place->successes || !place->q || !place->cum || !place->cell))
            return tthost::fail(TT_EINVAL, "%s: place names every array or is NULL", who);
        if (env->kp.pool_m > 0)
            return fail_both(env, TT_EINVAL, "%s: a curriculum with a reset pool is not supported (the curriculum draws from the reset "
                                             "box); tt_env_set_reset_pool(env, NULL, 0) first", who);
        if (env->log_flags & TT_LOG_DETAIL)
            return fail_both(env, TT_EINVAL, "%s: a curriculum with the detailed episode log is not supported (the curriculum's step "
                                             "kernels carry the plain log only)", who);
        for (int d = 0; d < 3; ++d)
            if (!(env->params.reset_hi[d] >= env->params.reset_lo[d]))
                return fail_both(env, TT_EINVAL, "%s: the reset box has reset_hi[%d] < reset_lo[%d]", who, d, d);
    }
    TT_HIP(env, hipSetDevice(env->device));
    if (env->cur_block) {       // launches in flight may still read and write the old block
        TT_HIP(env, hipStreamSynchronize(stream));
        TT_HIP(env, hipDeviceSynchronize());
        TT_HIP(env, hipFree(env->cur_block));
        env->cur_block = nullptr;
        env->cur_dev = nullptr;
        env->cur = CurDev{};
    }
    if (!cfg) return TT_OK;
    const size_t c = (size_t)C, npad = (size_t)env->npad;
    // the block: the descriptor, then (without `place`) p | seen | attempts | successes | q | cum | cell, each 256-byte aligned
    const size_t sizes[7] = {sizeof(double) * c, sizeof(unsigned long long) * c, sizeof(uint32_t) * c, sizeof(uint32_t) * c,
                             sizeof(uint32_t) * c, sizeof(uint32_t) * c, sizeof(uint32_t) * npad};
    size_t bytes = cur_align(sizeof(CurDev));
    size_t off[7];
    for (int a = 0; a < 7; ++a) {
        off[a] = bytes;
        if (!place) bytes += cur_align(sizes[a]);
    }
    void *blk = nullptr;
    hipError_t err = hipMalloc(&blk, bytes);
    if (err != hipSuccess) return fail(env, err == hipErrorOutOfMemory ? TT_ENOMEM : TT_EHIP, "%s: %s", who, hipGetErrorString(err));
    char *base = static_cast<char *>(blk);
    CurDev d{};
    if (place) {
        d.p = place->p; d.seen = reinterpret_cast<unsigned long long *>(place->seen);
        d.attempts = place->attempts; d.successes = place->successes; d.q = place->q; d.cum = place->cum; d.cell = place->cell;
    } else {
        d.p = reinterpret_cast<double *>(base + off[0]);
        d.seen = reinterpret_cast<unsigned long long *>(base + off[1]);
        d.attempts = reinterpret_cast<uint32_t *>(base + off[2]);
        d.successes = reinterpret_cast<uint32_t *>(base + off[3]);
        d.q = reinterpret_cast<uint32_t *>(base + off[4]);
        d.cum = reinterpret_cast<uint32_t *>(base + off[5]);
        d.cell = reinterpret_cast<uint32_t *>(base + off[6]);
    }
    d.nx = cfg->nx; d.ny = cfg->ny; d.nyaw = cfg->nyaw; d.C = (int)C;
    d.mode = cfg->mode;
    d.alpha = cfg->alpha; d.uniform = cfg->uniform;
    d.seed = env->seed;
    const int bins[3] = {cfg->nx, cfg->ny, cfg->nyaw};
    for (int k = 0; k < 3; ++k) {
        d.lo[k] = env->params.reset_lo[k];
        d.width[k] = (env->params.reset_hi[k] - env->params.reset_lo[k]) / (double)bins[k];
    }
    env->cur_block = blk;
    env->cur = d;
    // a fresh curriculum: p = 0.5 everywhere, nothing seen or counted, no lane's episode drawn by it; q and cum by the update
    // itself (no counts: it forms the weights only)
    const std::vector<double> half(c, 0.5);
    TT_HIP(env, hipMemcpyAsync(blk, &d, sizeof(d), hipMemcpyHostToDevice, stream));
    TT_HIP(env, hipMemcpyAsync(d.p, half.data(), sizes[0], hipMemcpyHostToDevice, stream));
    TT_HIP(env, hipMemsetAsync(d.seen, 0, sizes[1], stream));
    TT_HIP(env, hipMemsetAsync(d.attempts, 0, sizes[2], stream));
    TT_HIP(env, hipMemsetAsync(d.successes, 0, sizes[3], stream));
    TT_HIP(env, hipMemsetAsync(d.cell, 0xFF, sizes[6], stream));
    hipLaunchKernelGGL(k_curriculum_update, dim3(1), dim3(BLOCK), 0, stream, (const CurDev *)blk);
    TT_HIP(env, hipGetLastError());
    TT_HIP(env, hipStreamSynchronize(stream));      // `d` and `half` are temporaries
    env->cur_dev = static_cast<CurDev *>(blk);
    return TT_OK;
}

int tt_env_curriculum_update(tt_env *env, tt_stream_t stream) {
    TT_HANDLE(env);
    if (!env->cur_dev) return fail_both(env, TT_EINVAL, "tt_env_curriculum_update: the curriculum is off (tt_env_set_curriculum)");
    TT_HIP(env, hipSetDevice(env->device));
    hipLaunchKernelGGL(k_curriculum_update, dim3(1), dim3(BLOCK), 0, stream, (const CurDev *)env->cur_dev);
    TT_HIP(env, hipGetLastError());
    return TT_OK;
}

// tt_env_curriculum_read (to_caller) and tt_env_curriculum_write: device-to-device copies of the arrays the caller names
static int curriculum_copy(tt_env *env, const tt_curriculum_arrays *a, bool to_caller, hipStream_t stream, const char *who) {
    if (!env) return tthost::fail(TT_EINVAL, "%s: NULL handle", who);
    if (!a) return tthost::fail(TT_EINVAL, "%s: NULL argument", who);
    if (!env->cur_dev) return fail_both(env, TT_EINVAL, "%s: the curriculum is off (tt_env_set_curriculum)", who);
    TT_HIP(env, hipSetDevice(env->device));
    const CurDev &d = env->cur;
    const size_t c = (size_t)d.C;
    void *mine[7] = {d.p, d.seen, d.attempts, d.successes, d.q, d.cum, d.cell};
    void *theirs[7] = {a->p, a->seen, a->attempts, a->successes, a->q, a->cum, a->cell};
    const size_t sizes[7] = {sizeof(double) * c, sizeof(uint64_t) * c, sizeof(uint32_t) * c, sizeof(uint32_t) * c, sizeof(uint32_t) * c,
                             sizeof(uint32_t) * c, sizeof(uint32_t) * (size_t)env->n};
    for (int k = 0; k < 7; ++k)
        if (theirs[k])
            TT_HIP(env, hipMemcpyAsync(to_caller ? theirs[k] : mine[k], to_caller ? mine[k] : theirs[k], sizes[k], hipMemcpyDeviceToDevice,
                                       stream));
    return TT_OK;
}

int tt_env_curriculum_read(tt_env *env, const tt_curriculum_arrays *out, tt_stream_t stream) {
    return curriculum_copy(env, out, true, stream, "tt_env_curriculum_read");
}

int tt_env_curriculum_write(tt_env *env, const tt_curriculum_arrays *in, tt_stream_t stream) {
    return curriculum_copy(env, in, false, stream, "tt_env_curriculum_write");
}

int tt_env_profile(tt_env *env, int max_launches) {
    TT_ENTER(env);
    env->profiling = max_launches > 0;
    env->ev_used = 0;
    env->prof_ms = 0.0;
    env->prof_launches = 0;
    while ((long)env->ev_start.size() < (long)max_launches) {
        hipEvent_t a, b;
        TT_HIP(env, hipEventCreate(&a));
        TT_HIP(env, hipEventCreate(&b));
        env->ev_start.push_back(a);
        env->ev_stop.push_back(b);
    }
    return TT_OK;
}

int tt_env_profile_read(tt_env *env, double *total_ms, int64_t *launches) {
    TT_ENTER(env);
    for (size_t i = 0; i < env->ev_used; ++i) {
        TT_HIP(env, hipEventSynchronize(env->ev_stop[i]));
        float ms = 0.f;
        TT_HIP(env, hipEventElapsedTime(&ms, env->ev_start[i], env->ev_stop[i]));
        env->prof_ms += ms;
        env->prof_launches += 1;
    }
    env->ev_used = 0;
    if (total_ms) *total_ms = env->prof_ms;
    if (launches) *launches = env->prof_launches;
    return TT_OK;
}

int tt_random_actions(int n, uint64_t seed, uint64_t step, float *out, tt_stream_t stream) {
    if (n < 0 || (n > 0 && !out)) return fail(nullptr, TT_EINVAL, "tt_random_actions: bad argument");
    if (n == 0) return TT_OK;
    hipLaunchKernelGGL(k_random_actions, dim3(grid_for(n)), dim3(BLOCK), 0, stream, n, seed, step, out);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(nullptr, TT_EHIP, "tt_random_actions: %s", hipGetErrorString(err));
    return TT_OK;
}

}  // extern "C"

// the refusals of the other sources (csrc/tthost.h): the library's message (tt_last_error(NULL))
namespace tthost {
int vfail(char *dst, int code, const char *fmt, va_list ap) {
    vsnprintf(dst, ERR_BYTES, fmt, ap);
    return code;
}
int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfail(g_err, code, fmt, ap);
    va_end(ap);
    return code;
}
int refuse_nstep(const char *who, int n_step, float gamma) {
    if (n_step < 1 || n_step > TT_NSTEP_MAX) return fail(TT_EINVAL, "%s: n_step %d is outside 1 .. %d", who, n_step, TT_NSTEP_MAX);
    if (!(gamma > 0.f && gamma < 1.f)) return fail(TT_EINVAL, "%s: gamma is outside (0, 1)", who);
    return TT_OK;
}
int refuse_nstep_window(const char *who, int n_step, int slots, int reserve) {
    if (slots >= 3 + reserve + (n_step - 1)) return TT_OK;
    return fail(TT_EINVAL, "%s: a ring of %d slots has no window for n_step %d with this reserve", who, slots, n_step);
}
}  // namespace tthost
