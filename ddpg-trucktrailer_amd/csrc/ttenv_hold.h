// ttenv_hold.h -- greedy evaluation on held lanes: the evaluation block's layout (HoldCols), the step in which a finished lane
// holds still (k_step_hold) and the kernels that begin an evaluation, count its live lanes and read its records.
// Part of csrc/ttenv.hip's translation unit, inside its anonymous namespace.  Needs ttenv_state.h and ttenv_step.h before it.
// Non-template kernels: behind ttenv_log.h's, in front of ttenv_curriculum.h's.
#pragma once

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
