// ttenv_randomize.h -- episode randomisation: its descriptor (RndDev), the draw of an episode's goal and trailer length, the
// randomised reset piece and its two step kernels, the reset with the draw, and the small kernel that seeds the descriptor.
// Part of csrc/ttenv.hip's translation unit, inside its anonymous namespace.  Needs ttenv_math.h, ttenv_state.h, ttenv_step.h,
// ttenv_pose.h (reset_lane), ttenv_log.h (EpLog, log_append) and the TT_STEP_* pieces of csrc/ttenv.hip before it.  Non-template
// kernels: the unit's last, behind ttenv_curriculum.h's.
#pragma once

// ------------------------------------------------------------------------------------------
// Episode randomisation (tt_env_set_randomization): at every reset of a lane the goal (x, y, yaw) and the
// trailer length L2 of the new episode are drawn uniformly from configured ranges, as a pure function of (reset seed, lane, episode
// number).  The kernels get ONE pointer, to this descriptor in device memory, as the curriculum's do (CurDev, ttenv_curriculum.h):
// only a lane that finishes an episode reads it.
struct RndDev {
    double glo[3], gw[3];       // goal_lo and goal_hi - goal_lo, formed on the host in f64
    double l2lo, l2w;           // L2_lo and L2_hi - L2_lo
    unsigned long long seed;    // the handle's reset seed (k_rnd_seed): the step kernels read it here, in the path that needs it
    // The start pose's box and pool, as KParams has them (the host keeps the two equal: tt_env_set_randomization,
    // tt_env_set_reset_pool).  The step kernels read them HERE, by vector loads in the reset path: random_pose on the kernel's own
    // KParams keeps fourteen more scalars live across step_env, and the loop's variants are at their SGPR limit there -- the
    // allocator then spills scalars and, in one variant, leaves the stack slot TT_STEP_CUR's comment describes.
    double rlo[3], rhi[3];
    const double *pool;
    int pool_m, reserved_;
};

// The draw: the reset's Philox domain with third counter word 1 (the start pose's draw has 0 there and keeps its words); r[0..2] the
// goal's x, y and yaw, r[3] the trailer length.  f64 with contraction off (as curriculum_pose): a host model equals it bit for bit,
// and a width of 0 gives exactly lo.  The Goal as k_set_pose forms it.
__device__ __forceinline__ void randomized_task(const RndDev *rnd, uint64_t seed, uint32_t env, uint32_t episode, Goal &g, double &gyaw,
                                                double &L2) {
#pragma clang fp contract(off)
    uint32_t r[4];
    philox4x32(env, episode, 1u, 0x7452u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    g.gx = rnd->glo[0] + rnd->gw[0] * u01(r[0]);
    g.gy = rnd->glo[1] + rnd->gw[1] * u01(r[1]);
    gyaw = rnd->glo[2] + rnd->gw[2] * u01(r[2]);
    L2 = rnd->l2lo + rnd->l2w * u01(r[3]);
    tt_sincos(kTable, gyaw, g.sg, g.cg);
}

// random_pose on the descriptor's copy of the box and the pool: the same function on the same values, so the same start pose, bit
// for bit, as random_pose(P, ...) gives
__device__ __forceinline__ void randomized_start(const RndDev *rnd, uint64_t seed, uint32_t env, uint32_t episode, double &sx,
                                                 double &sy, double &syaw) {
    KParams Q{};
    Q.pool_m = rnd->pool_m;
    Q.pool = rnd->pool;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        Q.rlo[k] = rnd->rlo[k];
        Q.rhi[k] = rnd->rhi[k];
    }
    random_pose(Q, seed, env, episode, sx, sy, syaw);
}

// Head of the randomised step kernels, behind TT_STEP_HEAD: TT_STEP_CUR's cure (ttenv_curriculum.h) for the same stack slot -- the
// descriptor's address and the address of the lane's episode number into VECTOR registers at the kernel's head, the descriptor's
// words by vector loads in the one path that reads them.  Declares rnd and ep_ptr.
#define TT_STEP_RND()                                                                                                                   \
    uint32_t rnd_lo = (uint32_t)reinterpret_cast<uintptr_t>(rnd_arg), rnd_hi = (uint32_t)(reinterpret_cast<uintptr_t>(rnd_arg) >> 32);  \
    asm volatile("" : "+v"(rnd_lo), "+v"(rnd_hi));                                                                                      \
    const RndDev *rnd = reinterpret_cast<const RndDev *>(((uintptr_t)rnd_hi << 32) | (uintptr_t)rnd_lo);                               \
    uint32_t *ep_ptr = b.episodes + i;                                                                                                  \
    asm volatile("" : "+v"(ep_ptr))
// Reset with randomisation on (TT_STEP_RESET's place in k_step_rnd / k_step_rnd_log; auto-reset always): the start pose is
// random_pose's (box or pool, the words of a plain env), the goal and the trailer length are the draw's, and place_env does the
// rest -- dinit, max_steps from the drawn goal, the cold rows.  One test: only a finished lane does more than a plain step.
// (random_pose's `pool_m > 0` test sits INSIDE that test and acts on a vector-loaded value here, where TT_STEP_RESET's acts on a
// scalar kernel argument: one level of possibly divergent nesting, two more SGPRs for its exec mask.  The variants have room for it
// today -- no spill; a change that brings SGPR pressure back should look here first and hoist the test out,
// side by side, as TT_STEP_RESET_CURRICULUM does.)
#define TT_STEP_RESET_RANDOMIZED()                                                                                                      \
    if (o.done) {                                                                                                                       \
        const uint32_t ep = *ep_ptr + 1u;                                                                                               \
        *ep_ptr = ep;                                                                                                                   \
        const uint64_t rseed = rnd->seed;                                                                                               \
        double sx, sy, syaw, gyaw, l2;                                                                                                  \
        randomized_start(rnd, rseed, (uint32_t)i, ep, sx, sy, syaw);                                                                    \
        Goal g1;                                                                                                                        \
        randomized_task(rnd, rseed, (uint32_t)i, ep, g1, gyaw, l2);                                                                     \
        place_env(P, b, i, e, sx, sy, syaw, g1, gyaw, l2, of);                                                                          \
    }                                                                                                                                   \
    store_env(b, i, e)

// k_step with randomisation on: k_step's text with the randomised reset piece.  Per-env attributes and auto-reset are always on
// (a randomised handle is a per-env handle), so two template arguments remain; a kernel of its own for k_step_cur's reason.
template <bool INFO, bool RANDOM_POLICY>
__global__ __launch_bounds__(BLOCK) void k_step_rnd(const KParams P, const int n, const Bufs b,
                                                    const float *__restrict__ action, float *__restrict__ action_out,
                                                    float *__restrict__ obs, float *__restrict__ reward,
                                                    uint8_t *__restrict__ done, const Info info, const uint64_t seed,
                                                    const uint64_t policy_seed, const int *__restrict__ cursor,
                                                    const RndDev *rnd_arg) {
    constexpr bool PER_ENV = true;
    __shared__ __attribute__((aligned(16))) float tile[BLOCK * OBS];
    TT_STEP_HEAD();
    TT_STEP_RND();
    if (valid) {
        TT_STEP_LOADS();
        __builtin_amdgcn_sched_barrier(0);
        TT_STEP_ACT();
        StepOut o;
        step_env(P, e, a, of, o);
        TT_STEP_OUT();
        TT_STEP_RESET_RANDOMIZED();
    }
    store_obs_tile(tile, of, valid, obs, block_first, nv, P.nt != 0);
}

// ... and k_step_log with randomisation on: the same pieces in k_step_log's order
template <bool INFO, bool RANDOM_POLICY>
__global__ __launch_bounds__(BLOCK) void k_step_rnd_log(const KParams P, const int n, const Bufs b,
                                                        const float *__restrict__ action, float *__restrict__ action_out,
                                                        float *__restrict__ obs, float *__restrict__ reward,
                                                        uint8_t *__restrict__ done, const Info info, const uint64_t seed,
                                                        const uint64_t policy_seed, const int *__restrict__ cursor,
                                                        const EpLog lg, const RndDev *rnd_arg) {
    constexpr bool PER_ENV = true;
    __shared__ __attribute__((aligned(16))) float tile[BLOCK * OBS];
    TT_STEP_HEAD();
    TT_STEP_RND();
    if (valid) {
        TT_STEP_LOADS();
        double ret = lg.acc[i];
        __builtin_amdgcn_sched_barrier(0);
        TT_STEP_ACT();
        StepOut o;
        step_env(P, e, a, of, o);
        TT_STEP_OUT();
        TT_STEP_RETURN();
        TT_STEP_RESET_RANDOMIZED();
        log_append(lg, i, o.done, o.flags, o.final_bonus > 0.0, len, ret);
    }
    store_obs_tile(tile, of, valid, obs, block_first, nv, P.nt != 0);
    TT_STEP_LAUNCH_COUNT();
}

// k_reset with randomisation on (k_reset keeps its code): the same reset (reset_lane, ttenv_pose.h) with the drawn goal and length
__global__ __launch_bounds__(BLOCK) void k_reset_rnd(const KParams P, const int n, const Bufs b, const uint8_t *mask, float *obs,
                                                     const uint64_t seed, const RndDev *rnd) {
    reset_lane(
        P, n, b, mask, obs,
        [&](uint32_t env, uint32_t episode, double &sx, double &sy, double &syaw) { random_pose(P, seed, env, episode, sx, sy, syaw); },
        [&](uint32_t env, uint32_t episode, Goal &g, double &gyaw, double &L2) { randomized_task(rnd, seed, env, episode, g, gyaw, L2); });
}

// the reset seed into the descriptor (tt_env_reset, tt_env_import; one thread)
__global__ void k_rnd_seed(RndDev *rnd, const uint64_t seed) { rnd->seed = seed; }
