// ttenv_harvest.h -- success replay (include/ttenv.h: tt_ring_harvest, tt_env_harvest): the transitions of the
// successful episodes the episode log names, copied from the trajectory ring into a region of the ring's side buffer.  Two kernels,
// launched between the vector steps: k_harvest_plan (which rows, where) and k_harvest_copy (the rows).
// Part of csrc/ttenv.hip's translation unit, inside its anonymous namespace, behind every other topic header (its kernels are the
// last non-template ones).  Needs ttenv_state.h (BLOCK, OBS) and ttenv_log.h (atomic_add_agent; the host side uses log_cols).
#pragma once

// the record columns of a harvest: the env's own log (log_cols) or the caller's arrays
struct HarvestRecs {
    const int32_t *lane;
    const long long *end_step;
    const int32_t *len;
    const uint8_t *success;
    const unsigned long long *written;
    long long capacity;
};
// tt_harvest + the ring, as the kernels take them
struct HarvestK {
    long long *state;
    float *obs, *act, *rew, *obs2;
    uint8_t *done;
    int capacity, tail;
    long long step_base;
    int32_t *work;
    const float *r_obs, *r_act, *r_rew;
    const uint8_t *r_done;
    int n_envs, slots;
    const long long *k_dev;
};
enum HarvestState : int { HV_MARK = 0, HV_ROWS = 1, HV_EPISODES = 2, HV_CUT = 3, HV_EXPIRED = 4, HV_TICKET = 7 };

// the window of records and of ring steps of this harvest: records [mark, m), ring steps [lo, k)
struct HarvestWindow {
    long long mark, m, k, lo;
};
__device__ __forceinline__ HarvestWindow harvest_window(const HarvestK &h, const HarvestRecs &rc, long long mark) {
    HarvestWindow w;
    const unsigned long long written = *rc.written;
    w.m = written < (unsigned long long)rc.capacity ? (long long)written : rc.capacity;
    w.mark = mark < 0 ? 0 : (mark > w.m ? w.m : mark);
    const long long k = *h.k_dev;
    w.k = k > 0 ? k : 0;
    w.lo = w.k - (w.k < h.slots - 1 ? w.k : h.slots - 1);
    return w;
}

// What record j is to this harvest.  rows > 0: eligible, with its key (s - lo) * n_envs + lane, ascending in (s, lane), the absolute
// step s of its done transition and the rows cut off its front; rows == 0: expired (expired = true) or nothing
struct HarvestRec {
    long long key, s;
    int rows, cut, lane;
    bool expired;
};
__device__ __forceinline__ HarvestRec harvest_record(const HarvestK &h, const HarvestRecs &rc, const HarvestWindow &w, long long j) {
    HarvestRec r{-1, 0, 0, 0, 0, false};
    if (!rc.success[j]) return r;
    const int e = rc.lane[j], L = rc.len[j];
    const long long s = rc.end_step[j] + h.step_base;
    if (e < 0 || e >= h.n_envs || L < 1 || s >= w.k) return r;          // not a record of this ring
    if (s < w.lo) { r.expired = true; return r; }
    const long long want = h.tail > 0 && L > h.tail ? h.tail : L;
    const long long first = s - want + 1 > w.lo ? s - want + 1 : w.lo;
    r.s = s;
    r.lane = e;
    r.rows = (int)(s - first + 1);                                      // 1 .. slots - 1
    r.cut = (int)(want - (s - first + 1));
    r.key = (s - w.lo) * h.n_envs + e;
    return r;
}

// Plan.  Thread j owns record j; work[j] = 0 for a record that is not eligible (or not in the window), else the rows from its first
// row to the END of the harvest: the sum of rows over the eligible records with a key >= its own (itself included), found by
// counting against every record of the window, which the workgroup streams through LDS in tiles of BLOCK.  Row i of the record
// (oldest first) is then d = work[j] - i rows before the end: stored iff d <= capacity, at row (written_rows' - d) % capacity, where
// written_rows' is the count AFTER this harvest -- so the copy launch needs nothing of the state before it.  The workgroup that
// draws the last exit ticket (every other one has read the state by then) adds the harvest's totals and moves the mark.
__global__ __launch_bounds__(BLOCK) void k_harvest_plan(const HarvestK h, const HarvestRecs rc) {
    __shared__ long long s_key[BLOCK];
    __shared__ int s_rows[BLOCK];
    __shared__ unsigned long long s_tot[4];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    const long long j = (long long)blockIdx.x * BLOCK + tid;
    const HarvestWindow w = harvest_window(h, rc, h.state[HV_MARK]);
    const long long block_first = (long long)blockIdx.x * BLOCK;
    if (block_first < w.m && block_first + BLOCK > w.mark) {            // (uniform) a workgroup with records of the window
        HarvestRec mine{-1, 0, 0, 0, 0, false};
        if (j >= w.mark && j < w.m) mine = harvest_record(h, rc, w, j);
        int acc = 0;
        // (uniform) a workgroup without an eligible record has nothing to count: a log of failures costs one pass over itself
        const long long tiles_end = __syncthreads_or(mine.rows > 0) ? w.m : 0;
        for (long long tile = w.mark - w.mark % BLOCK; tile < tiles_end; tile += BLOCK) {
            const long long q = tile + tid;
            HarvestRec o{-1, 0, 0, 0, 0, false};
            if (q >= w.mark && q < w.m) o = harvest_record(h, rc, w, q);
            s_key[tid] = o.key;
            s_rows[tid] = o.rows;
            __syncthreads();
            if (mine.rows > 0)
                for (int t = 0; t < BLOCK; ++t)
                    if (s_key[t] >= mine.key) acc += s_rows[t];
            __syncthreads();
        }
        if (j < rc.capacity) h.work[j] = mine.rows > 0 ? acc : 0;
    } else if (j < rc.capacity)
        h.work[j] = 0;
    if (tid < 4) s_tot[tid] = 0ull;
    __syncthreads();
    if (tid == 0) {
        const unsigned long long t = __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(h.state + HV_TICKET), 1ull,
                                                            __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == gridDim.x - 1u;
    }
    __syncthreads();
    if (!s_last) return;
    unsigned long long rows = 0, episodes = 0, cut = 0, expired = 0;
    for (long long q = w.mark + tid; q < w.m; q += BLOCK) {
        const HarvestRec o = harvest_record(h, rc, w, q);
        rows += (unsigned long long)o.rows;
        episodes += o.rows > 0;
        cut += (unsigned long long)o.cut;
        expired += o.expired;
    }
    if (rows) atomicAdd(&s_tot[0], rows);
    if (episodes) atomicAdd(&s_tot[1], episodes);
    if (cut) atomicAdd(&s_tot[2], cut);
    if (expired) atomicAdd(&s_tot[3], expired);
    __syncthreads();
    if (tid == 0) {
        h.state[HV_MARK] = w.m;
        h.state[HV_ROWS] += (long long)s_tot[0];
        h.state[HV_EPISODES] += (long long)s_tot[1];
        h.state[HV_CUT] += (long long)s_tot[2];
        h.state[HV_EXPIRED] += (long long)s_tot[3];
        h.state[5] = 0;
        h.state[6] = 0;
        h.state[HV_TICKET] = 0;
    }
}

// Copy.  Wave v of the launch's V looks at records v + (64 c + lane) V, c = 0, 1, ... (neighbouring records, which a window holds,
// go to different waves) and moves the rows of each eligible one in turn: lanes 0..22 the observation, 32..54 the next one, 63 the
// scalars, as ring_sample_row does.  The launch follows the plan on its stream: state[HV_ROWS] is the count after this harvest and
// the mark is the window's end.
__global__ __launch_bounds__(BLOCK) void k_harvest_copy(const HarvestK h, const HarvestRecs rc) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), waves = (long long)gridDim.x * (BLOCK / 64);
    const HarvestWindow w = harvest_window(h, rc, 0);
    const long long written = h.state[HV_ROWS];
    const long long cap = h.capacity;
    for (long long base = wave; base < w.m; base += 64 * waves) {
        const long long mine = base + (long long)lane * waves;
        const int d_mine = mine < w.m ? h.work[mine] : 0;
        unsigned long long todo = __ballot(d_mine > 0);
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const long long j = base + (long long)src * waves;
            const int d0 = __shfl(d_mine, src);
            const HarvestRec r = harvest_record(h, rc, w, j);           // (the plan's own classification: rows > 0)
            const long long first = r.s - r.rows + 1;
            for (int i = 0; i < r.rows; ++i) {
                const long long d = (long long)d0 - i;
                if (d > cap || d < 1) continue;                         // a harvest larger than the region keeps its last rows
                const long long g = written - d;
                const size_t row = (size_t)(((g % cap) + cap) % cap);
                const long long step = first + i;
                const size_t t = (size_t)(step % h.slots), t1 = (size_t)((step + 1) % h.slots);
                const size_t at = t * h.n_envs + r.lane, at1 = t1 * h.n_envs + r.lane;
                if (lane < OBS) h.obs[row * OBS + lane] = h.r_obs[at * OBS + lane];
                else if (lane >= 32 && lane < 32 + OBS) h.obs2[row * OBS + lane - 32] = h.r_obs[at1 * OBS + lane - 32];
                if (lane == 63) {
                    h.act[row] = h.r_act[at];
                    h.rew[row] = h.r_rew[at];
                    h.done[row] = h.r_done[at];
                }
            }
        }
    }
}
