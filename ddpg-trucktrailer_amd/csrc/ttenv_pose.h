// ttenv_pose.h -- the kernels that place envs and read or write their state outside a step: reset, init, the pose / attribute /
// state / counter setters and getters, the observation of the stored state, and the stand-alone random actions.
// Part of csrc/ttenv.hip's translation unit, inside its anonymous namespace.  Needs ttenv_math.h and ttenv_state.h before it.
// The non-template kernels of the unit keep their relative order: this file's come first.
#pragma once

// ------------------------------------------------------------------------------------------
// reset / pose / state kernels (not hot)
// The reset of the thread's lane, written once for k_reset and k_reset_curriculum (ttenv_curriculum.h), which differ in the draw
// alone: pose(env, episode, sx, sy, syaw) gives the start pose of the lane's next episode.  k_reset_rnd (ttenv_randomize.h) also
// draws the episode's task: task(env, episode, g, gyaw, L2) gives its goal and trailer length; without one they are the
// parameters' goal and the lane's stored length.
struct ResetTaskStored {};
template <class POSE, class TASK = ResetTaskStored>
__device__ __forceinline__ void reset_lane(const KParams &P, const int n, const Bufs &b, const uint8_t *mask, float *obs,
                                           const POSE pose, const TASK task = TASK{}) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n || (mask && !mask[i])) return;
    // a full reset restarts every env's episode count, so reset(seed) is a pure function of the seed
    // (as np.random.seed is); a masked reset moves the chosen envs on to their next episode
    const uint32_t ep = mask ? b.episodes[i] + 1u : 0u;
    b.episodes[i] = ep;
    double sx, sy, syaw;
    pose((uint32_t)i, ep, sx, sy, syaw);
    float of[OBS];
    Env e;
    if constexpr (std::is_same<TASK, ResetTaskStored>::value) {
        const Goal g{P.gx, P.gy, P.sg, P.cg};
        place_env(P, b, i, e, sx, sy, syaw, g, P.gyaw, b.cold[C_L2 * (size_t)P.npad + i], obs ? of : nullptr);
    } else {
        Goal g;
        double gyaw, L2;
        task((uint32_t)i, ep, g, gyaw, L2);
        place_env(P, b, i, e, sx, sy, syaw, g, gyaw, L2, of);      // (always observed: `of` then stays in registers, no stack)
    }
    store_env(b, i, e);
    if constexpr (std::is_same<TASK, ResetTaskStored>::value) {
        if (obs)
            for (int j = 0; j < OBS; ++j) obs[(size_t)i * OBS + j] = of[j];
    } else if (obs) {       // (unrolled: the observation stays in registers)
#pragma unroll
        for (int j = 0; j < OBS; ++j) obs[(size_t)i * OBS + j] = of[j];
    }
}

__global__ __launch_bounds__(BLOCK) void k_reset(const KParams P, const int n, const Bufs b, const uint8_t *mask,
                                                 float *obs, const uint64_t seed) {
    reset_lane(P, n, b, mask, obs, [&](uint32_t env, uint32_t episode, double &sx, double &sy, double &syaw) {
        random_pose(P, seed, env, episode, sx, sy, syaw);
    });
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
    int i;
    if (!lane_of_entry(idx, k, n, j, i)) return;
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
    int i;
    if (!lane_of_entry(idx, k, n, j, i)) return;
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
    int i;
    if (!lane_of_entry(idx, k, n, j, i)) return;
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
    int i;
    if (!lane_of_entry(idx, k, n, j, i)) return;
    uint2 *m = reinterpret_cast<uint2 *>(hot_ptr(b.hot, i) + H_MISC * TILE);
    const uint32_t p = m->y;
    m->y = pk_make(pk_steps(p), (uint32_t)(maxs[j] < 0 ? 0 : maxs[j]), pk_stages(p), pk_age(p));
}

// `env.episode_steps = k` (simv2.py:94; episode_replay_collectorv2.py:269): the step counter alone -- the reward carry, its
// age and the stage latches stay (the reference keeps them in reward_state, which such a write does not touch)
__global__ __launch_bounds__(BLOCK) void k_set_steps(const int n, const Bufs b, const int32_t *idx, const int k,
                                                     const int32_t *steps) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    int i;
    if (!lane_of_entry(idx, k, n, j, i)) return;
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
