// ttenv_task.h -- the task curriculum: its descriptor (TaskDev), the draw of an episode's goal and trailer length by the weights of a
// grid of cells over the randomisation's ranges, the reset piece that counts and draws, its two step kernels and the reset with
// the draw.  Part of csrc/ttenv.hip's translation unit, inside its anonymous namespace.  Needs ttenv_curriculum.h (CurDev,
// TT_CURRICULUM_*, k_curriculum_update / _unset, which run on this descriptor's arrays as they are) and ttenv_randomize.h (RndDev,
// randomized_start, k_rnd_seed) before it.  Non-template kernels: the unit's last, behind ttenv_randomize.h's.
#pragma once

// ------------------------------------------------------------------------------------------
// Task curriculum (tt_env_set_task_curriculum): a grid of C = ngx * ngy * ngyaw * nl2 cells over the ranges of
// episode randomisation, cell c = ((il2 * ngyaw + igyaw) * ngy + igy) * ngx + igx, that counts the outcomes of the episodes drawn in
// each cell and draws the next task by weights made from them.  The kernels get ONE pointer, to this descriptor in device memory,
// as the curriculum's and the randomised kernels do.  It STARTS with a CurDev: the arrays, C, mode, alpha and uniform are what
// k_curriculum_update reads, so the update and k_curriculum_unset run on it unchanged (the CurDev's own bins, box and seed are not
// used).  Then an RndDev: the ranges' lower bounds, the seed (k_rnd_seed), and the start box and pool that randomized_start reads --
// state kept twice, as RndDev's own comment says, and kept current by the same entry points.
struct TaskDev {
    CurDev cur;
    RndDev rnd;
    double cw[4];       // the cell widths (hi - lo) / bins of goal x, y, yaw and L2, formed on the host in f64
    int bins[4];        // ngx, ngy, ngyaw, nl2
};
static_assert(offsetof(TaskDev, cur) == 0, "k_curriculum_update takes the descriptor's address as a CurDev's");

// The draw.  The task's words are plain randomisation's (third counter word 1); the cell comes from words of its own (third counter
// word 2, which nothing else uses): t = (s[0] * cum[C - 1]) >> 32, the smallest c with cum[c] > t, by curriculum_pose's search, which
// stays inside [0, C) whatever cum holds.  c -> (igx, igy, igyaw, il2) by curriculum_pose's f32-reciprocal step, exact below 4096.
// f64 with contraction off: a host model equals it bit for bit; with one bin (0 + u) * (w / 1) is w * u, plain randomisation's
// product, and a width of 0 gives exactly lo.  Writes the lane's cell.
__device__ __forceinline__ void task_draw(const TaskDev *tk, uint64_t seed, uint32_t env, uint32_t episode, Goal &g, double &gyaw,
                                          double &L2) {
#pragma clang fp contract(off)
    uint32_t r[4], s[4];
    philox4x32(env, episode, 1u, 0x7452u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    philox4x32(env, episode, 2u, 0x7452u, (uint32_t)seed, (uint32_t)(seed >> 32), s);
    const uint32_t *cum = tk->cur.cum;
    const int C = tk->cur.C;
    const uint32_t t = (uint32_t)(((unsigned long long)s[0] * (unsigned long long)cum[C - 1]) >> 32);
    uint32_t lo = 0u;
#pragma unroll
    for (uint32_t h = TT_CURRICULUM_MAX_CELLS / 2; h > 0u; h >>= 1) {
        const uint32_t j = lo + h;      // would cells [0, j) all have cum <= t?
        const uint32_t v = cum[min(j, (uint32_t)C) - 1u];
        lo = (j <= (uint32_t)C && v <= t) ? j : lo;
    }
    const uint32_t c = min(lo, (uint32_t)C - 1u);
    const uint32_t ngx = (uint32_t)tk->bins[0], ngy = (uint32_t)tk->bins[1], ngyaw = (uint32_t)tk->bins[2];
    const uint32_t r1 = (uint32_t)(((float)c + 0.5f) * __builtin_amdgcn_rcpf((float)ngx)), igx = c - r1 * ngx;
    const uint32_t r2 = (uint32_t)(((float)r1 + 0.5f) * __builtin_amdgcn_rcpf((float)ngy)), igy = r1 - r2 * ngy;
    const uint32_t il2 = (uint32_t)(((float)r2 + 0.5f) * __builtin_amdgcn_rcpf((float)ngyaw)), igyaw = r2 - il2 * ngyaw;
    g.gx = tk->rnd.glo[0] + ((double)igx + u01(r[0])) * tk->cw[0];
    g.gy = tk->rnd.glo[1] + ((double)igy + u01(r[1])) * tk->cw[1];
    gyaw = tk->rnd.glo[2] + ((double)igyaw + u01(r[2])) * tk->cw[2];
    L2 = tk->rnd.l2lo + ((double)il2 + u01(r[3])) * tk->cw[3];
    tt_sincos(kTable, gyaw, g.sg, g.cg);
    tk->cur.cell[env] = c;
}

// Head of the task curriculum's step kernels, behind TT_STEP_HEAD: TT_STEP_CUR's cure (ttenv_curriculum.h) -- the descriptor's address
// and the address of the lane's episode number into VECTOR registers at the kernel's head.  Declares tk and ep_ptr.
#define TT_STEP_TASK()                                                                                                                  \
    uint32_t tk_lo = (uint32_t)reinterpret_cast<uintptr_t>(tk_arg), tk_hi = (uint32_t)(reinterpret_cast<uintptr_t>(tk_arg) >> 32);      \
    asm volatile("" : "+v"(tk_lo), "+v"(tk_hi));                                                                                        \
    const TaskDev *tk = reinterpret_cast<const TaskDev *>(((uintptr_t)tk_hi << 32) | (uintptr_t)tk_lo);                                \
    uint32_t *ep_ptr = b.episodes + i;                                                                                                  \
    asm volatile("" : "+v"(ep_ptr))
// Reset with the task curriculum on (TT_STEP_RESET's place; auto-reset always): the finished episode is counted in the cell its task
// was drawn in, as TT_STEP_RESET_CURRICULUM counts -- relaxed agent-scope u32 adds, the tests side by side -- BEFORE the draw
// overwrites the lane's cell; then TT_STEP_RESET_RANDOMIZED's reset with the weighted draw in the uniform one's place.
#define TT_STEP_RESET_TASK()                                                                                                            \
    uint32_t cl = TT_CURRICULUM_NO_CELL, ncell = 0u;                                                                                    \
    if (o.done) {                                                                                                                       \
        cl = tk->cur.cell[i];                                                                                                           \
        ncell = (uint32_t)tk->cur.C;                                                                                                    \
    }                                                                                                                                   \
    if (cl < ncell) __hip_atomic_fetch_add(tk->cur.attempts + cl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                      \
    if (cl < ncell && o.final_bonus > 0.0)                                                                                              \
        __hip_atomic_fetch_add(tk->cur.successes + cl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                                 \
    if (o.done) {                                                                                                                       \
        const uint32_t ep = *ep_ptr + 1u;                                                                                               \
        *ep_ptr = ep;                                                                                                                   \
        const uint64_t rseed = tk->rnd.seed;                                                                                            \
        double sx, sy, syaw, gyaw, l2;                                                                                                  \
        randomized_start(&tk->rnd, rseed, (uint32_t)i, ep, sx, sy, syaw);                                                               \
        Goal g1;                                                                                                                        \
        task_draw(tk, rseed, (uint32_t)i, ep, g1, gyaw, l2);                                                                            \
        place_env(P, b, i, e, sx, sy, syaw, g1, gyaw, l2, of);                                                                          \
    }                                                                                                                                   \
    store_env(b, i, e)

// k_step with the task curriculum on: k_step's text with the task curriculum's reset piece; per-env attributes and auto-reset are
// always on, as in k_step_rnd
template <bool INFO, bool RANDOM_POLICY>
__global__ __launch_bounds__(BLOCK) void k_step_task(const KParams P, const int n, const Bufs b,
                                                     const float *__restrict__ action, float *__restrict__ action_out,
                                                     float *__restrict__ obs, float *__restrict__ reward,
                                                     uint8_t *__restrict__ done, const Info info, const uint64_t seed,
                                                     const uint64_t policy_seed, const int *__restrict__ cursor,
                                                     const TaskDev *tk_arg) {
    constexpr bool PER_ENV = true;
    __shared__ __attribute__((aligned(16))) float tile[BLOCK * OBS];
    TT_STEP_HEAD();
    TT_STEP_TASK();
    if (valid) {
        TT_STEP_LOADS();
        __builtin_amdgcn_sched_barrier(0);
        TT_STEP_ACT();
        StepOut o;
        step_env(P, e, a, of, o);
        TT_STEP_OUT();
        TT_STEP_RESET_TASK();
    }
    store_obs_tile(tile, of, valid, obs, block_first, nv, P.nt != 0);
}

// ... and k_step_log with the task curriculum on: the same pieces in k_step_log's order
template <bool INFO, bool RANDOM_POLICY>
__global__ __launch_bounds__(BLOCK) void k_step_task_log(const KParams P, const int n, const Bufs b,
                                                         const float *__restrict__ action, float *__restrict__ action_out,
                                                         float *__restrict__ obs, float *__restrict__ reward,
                                                         uint8_t *__restrict__ done, const Info info, const uint64_t seed,
                                                         const uint64_t policy_seed, const int *__restrict__ cursor,
                                                         const EpLog lg, const TaskDev *tk_arg) {
    constexpr bool PER_ENV = true;
    __shared__ __attribute__((aligned(16))) float tile[BLOCK * OBS];
    TT_STEP_HEAD();
    TT_STEP_TASK();
    if (valid) {
        TT_STEP_LOADS();
        double ret = lg.acc[i];
        __builtin_amdgcn_sched_barrier(0);
        TT_STEP_ACT();
        StepOut o;
        step_env(P, e, a, of, o);
        TT_STEP_OUT();
        TT_STEP_RETURN();
        TT_STEP_RESET_TASK();
        log_append(lg, i, o.done, o.flags, o.final_bonus > 0.0, len, ret);
    }
    store_obs_tile(tile, of, valid, obs, block_first, nv, P.nt != 0);
    TT_STEP_LAUNCH_COUNT();
}

// k_reset with the task curriculum on: the same reset (reset_lane, ttenv_pose.h), the task from the weighted draw
__global__ __launch_bounds__(BLOCK) void k_reset_task(const KParams P, const int n, const Bufs b, const uint8_t *mask, float *obs,
                                                      const uint64_t seed, const TaskDev *tk) {
    reset_lane(
        P, n, b, mask, obs,
        [&](uint32_t env, uint32_t episode, double &sx, double &sy, double &syaw) { random_pose(P, seed, env, episode, sx, sy, syaw); },
        [&](uint32_t env, uint32_t episode, Goal &g, double &gyaw, double &L2) { task_draw(tk, seed, env, episode, g, gyaw, L2); });
}
