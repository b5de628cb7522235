// ttenv_log.h -- the episode log, plain and detailed: the block's layout (EpLog, LogCols, TallyCols), the wave-level append the
// log's step kernels call (log_append, tally_append) and the four small kernels that zero a lane's accumulators and drain the
// records.  The step kernels themselves (k_step_log, k_step_tally) are in csrc/ttenv.hip with the TT_STEP_* pieces.
// Part of csrc/ttenv.hip's translation unit, inside its anonymous namespace.  Needs ttenv.h (TT_LOG_*, TT_I_*), ttenv_state.h and
// ttenv_step.h (StepOut) before it.  Non-template kernels: behind ttenv_pose.h's, in front of ttenv_hold.h's.
#pragma once

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
// ticket (csrc/ttenv.hip, TT_STEP_LAUNCH_COUNT), so before the last workgroup of the launch advances it.
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

// the episode log's accumulator of lanes that start a new episode outside the step kernel (tt_env_reset with a mask,
// tt_env_set_pose): entry j < k names lane idx[j] (idx NULL: lane j) and counts when mask is NULL or mask[lane] != 0
__global__ __launch_bounds__(BLOCK) void k_log_zero(const int n, const int k, const uint8_t *mask, const int32_t *idx,
                                                    double *acc) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    int i;
    if (!lane_of_entry(idx, k, n, j, i) || (mask && !mask[i])) return;
    acc[i] = 0.0;
}

// k_log_zero for the detailed log: the lane's return and its nine term sums (tally_acc)
__global__ __launch_bounds__(BLOCK) void k_tally_zero(const int n, const int k, const uint8_t *mask, const int32_t *idx,
                                                      const EpLog lg, const int npad) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    int i;
    if (!lane_of_entry(idx, k, n, j, i) || (mask && !mask[i])) return;
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
