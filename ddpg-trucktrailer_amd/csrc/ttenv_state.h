// ttenv_state.h -- the env's memory and one env in registers: the hot tile's and the cold block's rows, the packed counters
// (pk_*), KParams, Bufs, Goal, Env, the observation and its LDS-staged store, load_env / store_env / place_env, and the reset's
// and the random policy's draws.
// Part of csrc/ttenv.hip's translation unit, inside its anonymous namespace.  Needs ttenv.h (TT_OBS_DIM) and ttenv_math.h before it.
#pragma once

constexpr int OBS = TT_OBS_DIM;
#ifndef TT_BLOCK
#define TT_BLOCK 256
#endif
constexpr int BLOCK = TT_BLOCK;  // threads per workgroup (a multiple of the 64-env tile)
constexpr int TILE = 64;

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

// The prologue of the kernels that work on a LANE SET (the setters of ttenv_pose.h, k_log_zero / k_tally_zero, k_curriculum_unset):
// entry j < k names lane idx[j] (idx NULL: lane j), into i.  False where the thread has no entry (j >= k) or its entry names no lane
// of [0, n): it then returns.
__device__ __forceinline__ bool lane_of_entry(const int32_t *idx, int k, int n, int j, int &i) {
    if (j >= k) return false;
    i = idx ? idx[j] : j;
    return i >= 0 && i < n;
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
