// ttenv_curriculum.h -- the start-pose curriculum: its descriptor (CurDev), the draw, the curriculum's reset piece and its two
// step kernels, the reset with a curriculum draw, and the small kernels that seed, unset and update it.
// Part of csrc/ttenv.hip's translation unit, inside its anonymous namespace.  Needs ttenv.h (TT_CURRICULUM_*), ttenv_state.h,
// ttenv_step.h, ttenv_log.h (EpLog, log_append) and the TT_STEP_* pieces of csrc/ttenv.hip before it.  Non-template kernels: the
// unit's last, behind ttenv_hold.h's.
#pragma once

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

// k_reset with the curriculum on (k_reset keeps its code): the same reset (reset_lane, ttenv_pose.h), the pose from the curriculum's
// draw
__global__ __launch_bounds__(BLOCK) void k_reset_curriculum(const KParams P, const int n, const Bufs b, const uint8_t *mask,
                                                            float *obs, const uint64_t seed, const CurDev *cur) {
    reset_lane(P, n, b, mask, obs, [&](uint32_t env, uint32_t episode, double &sx, double &sy, double &syaw) {
        curriculum_pose(cur, seed, env, episode, sx, sy, syaw);
    });
}

// the reset seed into the descriptor (tt_env_reset, tt_env_import; one thread)
__global__ void k_curriculum_seed(CurDev *cur, const uint64_t seed) { cur->seed = seed; }

// lanes placed from outside (tt_env_set_pose, tt_env_set_state): their episode is no curriculum draw's.  Entry j < k names lane
// idx[j] (idx NULL: lane j), as k_log_zero's
__global__ __launch_bounds__(BLOCK) void k_curriculum_unset(const int n, const int k, const int32_t *idx, uint32_t *cell) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    int i;
    if (!lane_of_entry(idx, k, n, j, i)) return;
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
