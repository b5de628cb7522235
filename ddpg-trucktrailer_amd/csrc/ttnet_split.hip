// ttnet_split.hip -- the N-env forward of the reference's actor / critic MLPs (DDPG/networks.py:55-68, 138-147) on the
// 16-bit MFMA of gfx950 at f32 accuracy ("split-f16").
//
// Why: the f32-input MFMA runs at 1/16 of the f16/bf16 rate (155 TFLOP/s vs ~2.5 PFLOP/s dense), and fc2 (400 -> 300)
// is 93 % of the network's arithmetic.  An f32 number x (24 significand bits) is, to within its own rounding error, the
// sum of TWO f16 numbers when both conversions round to nearest: h = rn16(x) leaves |x - h| <= 2^-12 |x| and
// m = rn16(x - h) leaves |x - h - m| <= 2^-24 |x| (11 + 1 + 11 + 1 bits; the remainder x - h is exact in f32).  A
// product of two f16 numbers is exact in f32 (22 bits), so
//     x*w = h*h' + (h*m' + m*h') + [m*m' + (x - h - m)*w + x*(w - h' - m')]
// where every term of the bracket is below 2^-24 |x*w|: three f16 MFMAs with f32 accumulation reproduce the f32 product
// to within ~3 of its own rounding errors, at 3/16 of the f32 MFMA's cycles (the round-1 kernel used three bf16 pieces
// and six MFMAs per product block).  f16 has 5 exponent bits, so both operands are scaled by powers of two (exact) to
// keep their `m` pieces normal: activations by 2^4, weights by 2^6; the accumulator is scaled back by 2^-10 (exact)
// where the bias is added.  Ranges: |activation| < 4094, |weight| < 1023 (a piece becomes inf from 16 |x| >= 65520 and
// 64 |w| >= 65520: 4095 and 1023.75) -- beyond them a piece becomes inf and the row's output NaN (loud, not silently wrong:
// the `poison` term of the epilogue; a weight beyond the range does that to EVERY row); a NaN or inf observation or action
// likewise gives a NaN row, as in the torch modules, and leaves every other row's bits alone (tests/test_gpu_policy_edges.py).
// Pieces below the normal range carry an absolute error <= 2^-25 / scale.
//
// Orientation: everything is computed TRANSPOSED (neurons on the MFMA's M axis, envs on N), with
// v_mfma_f32_32x32x16_f16.  Its 32x32 result has the env on the lane (lane & 31) and 16 neurons in the lane's
// registers, which is exactly the B-operand layout of the next product that sums over neurons: the layer-1 result
// goes through LayerNorm + ReLU in registers and feeds layer 2 with no LDS round trip and no lane movement
// (the k order inside a step is permuted; the packed weights are laid out to match).  Both LayerNorms and the
// 300 -> 1 head reduce over registers plus ONE cross-lane exchange (lane ^ 32).
//
//   workgroup = 4 waves = 128 envs (32 per wave); per wave: h1 = 13 tiles x 16 registers (f32), layer-2
//   accumulators 10 tiles x 16 registers; fc2 is streamed once per workgroup, as pre-split f16 planes in MFMA
//   fragment order, through a 7-slot LDS ring shared by the four waves (20 KB per k16 step), filled by LDS-DMA five
//   steps ahead of its use.
//   Layer 1 (K = 23 + the bias as a 24th input that is always 1) runs on the same three-product scheme from pre-split
//   fc1 fragments, also brought into LDS by DMA.
//   EVERY request of the tile loop is issued behind an MFMA (the matrix pipe hides most of a piece's issue cost; between
//   vector phases a piece costs 100-185 cycles): the schedule is the table above l2_job below, the counted waits follow from it.
#include "ttnet_common.h"
#include "ttnet_pack.h"
#include "ttstamps.h"

namespace ttnet {
namespace {

#ifdef TT_STAMPS   // diagnostic build only: clocks of thread 0 of every workgroup at the phase boundaries
__device__ unsigned long long g_nstamps[16];
__device__ unsigned long long g_bstamps[4096 * 8];      // [block][phase] wall clock (100 MHz); [block][7] = XCC id
#define NSTAMP(i) do { if (threadIdx.x == 0) { const unsigned long long w_ = wall_clock64();                                \
        if (blockIdx.x < 4096) { g_bstamps[blockIdx.x * 8 + (i)] = w_;                                                      \
            if ((i) == 0) g_bstamps[blockIdx.x * 8 + 7] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)); }     \
        if (blockIdx.x == 0) { g_nstamps[i] = w_; g_nstamps[8 + i] = clock64(); } } } while (0)
// begin / end of every tile a workgroup takes: [block][round of the tile loop][2] (tools/step_timeline.py)
__device__ unsigned long long g_tile[512][4][2];
__device__ TTLog g_log_tile;
#define TSTAMP(round, e) do { if (threadIdx.x == 0 && blockIdx.x < 512 && (round) < 4) g_tile[blockIdx.x][round][e] = wall_clock64(); } while (0)
#else
#define NSTAMP(i) do { } while (0)
#define TSTAMP(round, e) do { } while (0)
#endif

__global__ __launch_bounds__(256) void k_split_pack(const Weights W, const bool critic, unsigned char *__restrict__ ws,
                                                    unsigned char *__restrict__ ws_alt, long long *__restrict__ bump,
                                                    const RingCursor cur) {
    split_pack_body(W, critic, ws, ws_alt, bump, cur, blockIdx.x * 256 + threadIdx.x);
    publish_image(cur, PACK_BLOCKS);
}

// What opens a pipelined vector step, in ONE launch (two small kernels would each cost their ~4 us of launch and a
// dependency gap on the loop's critical path): the policy's image from the actor's current weights, and the first batch of
// this step's learn() -- or all of its batches, one per update (RingSample.draws) -- from the replay ring (four sampled
// transitions per 256-thread workgroup).
__global__ __launch_bounds__(256) void k_pack_and_sample(const Weights W, const bool critic, unsigned char *__restrict__ ws,
                                                         unsigned char *__restrict__ ws_alt, const RingSample R,
                                                         const RingCursor cur) {
    if ((int)blockIdx.x < PACK_BLOCKS) {
        split_pack_body(W, critic, ws, ws_alt, nullptr, cur, blockIdx.x * 256 + threadIdx.x);
        publish_image(cur, PACK_BLOCKS);
        return;
    }
    const int b = ((int)blockIdx.x - PACK_BLOCKS) * 4 + (threadIdx.x >> 6);
    if (b < R.batch * R.draws) ring_sample_row(R, b, threadIdx.x & 63);
}

// ---- Where a wave issues its LDS-DMA pieces inside the tile loop, and what the counted waits may leave in flight.
// Ring slot of k16 step s: s % RING.  At a tile's top the ring holds packed fc1 in slots 4..6 (W1_OFF) and -- from the second
// tile of a workgroup on -- steps 0, 1 in slots 0, 1.
//   layer 1, behind the third MFMA of product q = 2 t + s (26 products):
//     q 0..9   steps 0, 1 -> slots 0, 1     FIRST tile only (later tiles got them from the previous tile's tail)
//     q 10..19 steps 2, 3 -> slots 2, 3     held steps 23, 24 of the previous tile: every wave is past the tile's top barrier,
//                                           which it reaches after its last fragment read of the previous tile
//   layer 2, behind the third MFMA of tile u of step s (l2_job):
//     s = 0           steps 4 (u < 5), 5 (u >= 5) -> slots 4, 5   held fc1: every wave is past the barrier in front of layer 2,
//     s = 1, u < 5    step 6 -> slot 6                            which it reaches after its layer 1
//     s = 1..18, u >= 5   step s + 6 -> the slot of step s - 1    every wave is past the mid-step barrier of step s, i.e. past
//                                                                 tile 4 of step s: its reads of step s - 1 ended in step s - 1
//     s = 19..21, u >= 5  the NEXT tile's fc1 pieces 5 (s - 19) + u - 5 < 13 -> slots 4, 5, 6 = the slots of steps 18, 19, 20:
//                         the slot of step s - 1 again, by the same barrier
//     s = 22, 23, u >= 5  the NEXT tile's steps 0, 1 -> slots 0, 1 = the slots of steps 21, 22: likewise
// In EVERY layer-2 row the rule is the same: behind the mid-step barrier of step s a piece may overwrite the slot of step
// s - 1 (static_asserts below).  The tail requests are unconditional -- the image is the same for every tile -- so the counts
// are compile-time; a workgroup's last tile fetches 23 pieces per wave that nobody reads and drains them before it ends.
constexpr int JOB_NONE = -1, JOB_FC1 = 100, JOB_NEXT = 200;      // a job: fc2 step 0..24 of this tile | fc1 piece | next tile's step
constexpr int TAIL0 = STEPS - (RING - 1);                         // 19: the first step whose u >= 5 slots carry no fc2 step
constexpr int l2_job(const int s, const int u) {
    if (s == 0) return AHEAD - 1 + u / 5;
    if (s == 1 && u < 5) return RING - 1;
    if (u < 5) return JOB_NONE;
    if (s < TAIL0) return s + RING - 1;
    const int i = 5 * (s - TAIL0) + u - 5;
    if (i < W1_WAVE_PIECES) return JOB_FC1 + i;
    if (s == TAIL0 + 3 || s == TAIL0 + 4) return JOB_NEXT + s - (TAIL0 + 3);
    return JOB_NONE;
}
constexpr int l2_piece(const int u) { return u % 5; }             // which of the wave's five pieces of a step
// the ring slot a job of layer 2 writes (fc1 piece i of every wave lies in row i of W1_OFF: 5 rows per slot)
constexpr int job_slot(const int j) { return j >= JOB_NEXT ? j - JOB_NEXT : (j >= JOB_FC1 ? W1_OFF / CHUNK_BYTES + (j - JOB_FC1) / 5 : j % RING); }
constexpr bool l2_slots_free() {
    for (int s = 0; s < STEPS; ++s)
        for (int u = 0; u < T2; ++u) {
            const int j = l2_job(s, u);
            if (j == JOB_NONE) continue;
            if (s == 0 || (s == 1 && u < 5)) { if (job_slot(j) < W1_OFF / CHUNK_BYTES) return false; }      // fc1's slots only
            else if (u < 5 || job_slot(j) != (s - 1) % RING) return false;
        }
    return true;
}
static_assert(l2_slots_free(), "a piece of layer 2 overwrites a slot that may still be read");
// Pieces a wave has issued before the mid-step barrier of step s that are YOUNGER than its pieces of step s + 1: what the
// s_waitcnt there may leave in flight (pieces retire in issue order; nothing else is outstanding inside a tile: the top of the
// tile waits for 0).  Counted over the order of issue: layer 1's steps 2, 3 (steps 0, 1 are older in either form of the tile),
// then l2_job row by row.
constexpr int mid_allowed(const int s) {
    int n = 10, after = s + 1 == 2 ? 5 : (s + 1 == 3 ? 10 : -1000);
    for (int ss = 0; ss < STEPS; ++ss)
        for (int u = 0; u < T2; ++u) {
            if (ss == s && u == T2 / 2) return n - after;
            const int j = l2_job(ss, u);
            if (j != JOB_NONE) { ++n; if (j == s + 1) after = n; }
        }
    return -1;
}
// steps 1..21: four younger steps, or the rest of them plus the next tile's fc1 so far (15 + 5, 10 + 10): 20.  Steps 22, 23:
// step 24 (5) + fc1 (13), fc1 (13) + the next tile's step 0 (5): 18.  Steps 0 and 24 wait for nothing (see the loop).
constexpr bool mid_counts_ok() {
    for (int s = 1; s + 1 < STEPS; ++s) if (mid_allowed(s) != (s < TAIL0 + 3 ? 20 : 18)) return false;
    return true;
}
static_assert(mid_counts_ok(), "the counted waits of layer 2 do not match the issue schedule");
// (tables: the kernel's unrolled loops index them with constants)
struct L2Schedule {
    int job[STEPS][T2], mid[STEPS];
};
constexpr L2Schedule make_l2_schedule() {
    L2Schedule t{};
    for (int s = 0; s < STEPS; ++s) {
        t.mid[s] = mid_allowed(s);
        for (int u = 0; u < T2; ++u) t.job[s][u] = l2_job(s, u);
    }
    return t;
}
constexpr L2Schedule L2S = make_l2_schedule();

// LDS reads through laundered address-space-3 bases.  The ring + vectors span 152 KB and a ds_read's immediate offset reaches
// 64 KB, so three byte bases (0, 64 KB, 128 KB; + this lane's 16 bytes) cover every fragment with an immediate; the bases pass
// through an empty asm at the top of every tile so that the compiler can neither hoist the ~300 fragment addresses of a tile out
// of the tile loop nor keep them live across it (the loop form spilled ~400 registers that way).
using lds_b = const __attribute__((address_space(3))) unsigned char;
using v4u = __attribute__((ext_vector_type(4))) unsigned;
struct LdsBases {
    lds_b *b0, *b1, *b2;
};
__device__ __forceinline__ uint4 lds_frag(const LdsBases &L, const int off) {      // off: compile-time byte offset (+ lane * 16)
    lds_b *p = (off >> 16) == 0 ? L.b0 : ((off >> 16) == 1 ? L.b1 : L.b2);
    const v4u t = *(const __attribute__((address_space(3))) v4u *)(p + (off & 0xFFFF));
    return make_uint4(t[0], t[1], t[2], t[3]);
}

// One workgroup = 4 waves = 128 envs per TILE; a workgroup takes the tiles tile0 + blockIdx.x, + gridDim.x, ... < tile_end in
// turn.  From the second tile on, the tile's packed fc1 and the first two k16 steps of fc2 are requested under the last steps
// of the PREVIOUS tile's layer 2 and its observations before that tile's epilogue; the per-neuron vectors stay in LDS.
template <bool CRITIC>
__global__ __launch_bounds__(256, 1) void k_mlp_split(const int n, const int tile0, const int tile_end,
                                                      int *__restrict__ cursor_e, const long long *__restrict__ step_e,
                                                      const float *__restrict__ obs,
                                                      const unsigned char *__restrict__ ws,
                                                      const unsigned char *__restrict__ ws_alt,
                                                      const float *__restrict__ action, float *__restrict__ out,
                                                      const ActArgs act) {
    // The first 16 dwords of the arguments reach the wave in SGPRs (kernarg preload, build.py): n .. action.  cursor_e / step_e
    // repeat act.cursor / act.step_dev there, so that the launch's first loads -- the step counter and the image epochs --
    // leave before the rest of the argument segment (the struct) has been fetched.
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const float *p1_s = reinterpret_cast<const float *>(lds_raw + RING_BYTES);              // g1' | be1'       [2][416]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    // this lane's view of the per-neuron vectors, its address held in a register: the region lies beyond the 64 KB a
    // ds_read's immediate offset reaches from address 0, and left to itself the compiler forms every address with an add
    using lds_f = const __attribute__((address_space(3))) float;
    using v4 = __attribute__((ext_vector_type(4))) float;
    auto lds4 = [](lds_f *q) -> float4 {
        const v4 t = *(const __attribute__((address_space(3))) v4 *)q;
        return make_float4(t[0], t[1], t[2], t[3]);
    };
    lds_f *pv1_0 = (lds_f *)(p1_s + 4 * h);
    LdsBases LB0;
    LB0.b0 = (lds_b *)lds_raw + lane * 16;
    LB0.b1 = LB0.b0 + 65536;
    LB0.b2 = LB0.b0 + 131072;
    // ring addressing: the running step's slots follow from the ring's step counter (the same numbers the opening pack launch
    // leaves in the cursor buffer); the first workgroup leaves them where the env step reads them.  The IMAGE of this step
    // (that of the step's parity: the other one may be being written for the next step) comes from the opening pack launch,
    // which need not be ordered before this launch: await_image (ttnet_common.h) -- behind the first tile's observation loads,
    // which do not depend on it.
    const EpochPair epochs = await_image_early(cursor_e);        // (requested beside the step counter, not behind it)
    const long long kstep = cursor_e ? *step_e : 0;
    const bool odd = act.cursor && (kstep & 1);
    const bool local = act.cursor && act.ring_slots > 0;
    // (the 64-bit modulo is a software loop in front of every launch's observation loads: 32 bits while the counter fits)
    const int slot_t = !local ? 0 : ((unsigned long long)kstep >> 32) == 0ull ? (int)((unsigned)kstep % (unsigned)act.ring_slots)
                                                                             : (int)(kstep % act.ring_slots);
    const float *obs_base = local ? obs + (size_t)slot_t * act.ring_n * IN : obs;      // (re-read from the cursor below when !local)
    // LDS is filled by LDS-DMA (global_load_lds_dwordx4: 64 lanes x 16 B = one 1 KB piece per wave-instruction, no
    // staging registers).  The statements are inline asm, so hipcc neither counts them nor drains them at a barrier:
    // each wave retires its own pieces with an s_waitcnt vmcnt before the barrier that precedes their first read.
    // A piece = global bytes [base + voff .. + 1 KB) -> LDS [lds_wave + dst_const .. + 1 KB).  The global side is ONE SGPR base
    // (the image) plus a per-lane VGPR offset that carries everything else (lane * 16, the wave's share, the piece), the LDS side
    // a per-wave SGPR plus a constant added INSIDE the asm: no scalar address arithmetic is left to the compiler, which forms
    // 64-bit scalar adds on the vector ALU when SCC is live and then cannot feed them to an "s" operand.
    const unsigned lds_base0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)lds_raw;
    auto dma_piece = [&](const unsigned char *base, const unsigned voff, const unsigned lds_wave, const unsigned dst_const)
                         __attribute__((always_inline)) {
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_add_u32 m0, %3, %4\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff), "s"(base), "s"(lds_wave), "s"(dst_const) : "memory", "scc");
    };
    const unsigned voff_w2 = lane * 16 + wave * 5120 + WS_W2;                              // this wave's 5 pieces of a k16 step
    const unsigned voff_w1 = lane * 16 + wave * 1024 + WS_W1;                              // ... 13 pieces of packed fc1: 4 i + wave
    const unsigned voff_vec = lane * 16 + wave * (VEC_PIECES / 4) * 1024 + WS_VEC;         // ... 3 pieces of the vectors
    const unsigned ldsw_w2_0 = lds_base0 + wave * 5120, ldsw_w1_0 = lds_base0 + W1_OFF + wave * 1024;
    // this wave's share of packed fc1 (13 pieces) / of k16 step s of fc2 (5 pieces), from image `w`
    auto issue_fc1_piece = [&](const unsigned char *w, const unsigned ldsw_w1, const int i) __attribute__((always_inline)) {
        dma_piece(w, voff_w1 + i * 4096, ldsw_w1, i * 4096);
    };
    auto issue_step_piece = [&](const unsigned char *w, const unsigned ldsw_w2, const int s, const int i) __attribute__((always_inline)) {
        dma_piece(w, voff_w2 + s * CHUNK_BYTES + i * 1024, ldsw_w2, (s % RING) * CHUNK_BYTES + i * 1024);
    };
    // unconditional loads from clamped (always valid) addresses, selected afterwards: 16 loads in flight at once
    // instead of 16 exec-masked round trips
    float xo[S1][8];                                                          // obs^T as the B operand: input 16 s + 8 h + j
    // choose_action's noise inputs of the tile's rows -- the OU state and the previous step's done flag (DDPG_agent.py:36-49,
    // noise.py:13-17, trainv2.py:492) -- are requested WITH the observations: read where the head's output is known (finish_row)
    // they were two dependent round trips to memory at the very end of every tile, with nothing left to hide them behind
    float ou_pre = 0.f;
    unsigned dp_pre = 0u;
    const bool with_noise = !CRITIC && act.ou != nullptr;                     // (uniform over the launch)
    const uint8_t *dprev = act.done_prev;                                    // the done flags that restart a row's noise, or nullptr
    float *araw = act.act_raw;
    auto load_obs = [&](const int tile) __attribute__((always_inline)) {
        const int row = tile * ROWS + wave * WROWS + r;
        const int rowc = row < n ? row : n - 1;
        const float *orow = obs_base + (size_t)rowc * IN;
#pragma unroll
        for (int s = 0; s < S1; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 16 * s + 8 * h + j;
                xo[s][j] = orow[k < IN ? k : IN - 1];
            }
        if (with_noise) {
            ou_pre = act.ou[rowc];
            dp_pre = dprev ? (unsigned)dprev[rowc] : 0u;
        }
    };

    NSTAMP(0);
    // ---- prologue of the FIRST tile: this lane's observation features first (ordinary loads: the compiler waits for them on
    // its own count), then packed fc1 + the per-neuron vectors by DMA; fc2 steps 0 and 1 are not needed before layer 2 and are
    // requested inside layer 1
    int tile = tile0 + (int)blockIdx.x;
    if (tile >= tile_end) return;
    if (local) {                          // the ring's slots of this step follow from the step counter: no look at the cursor
        const int sl = act.ring_slots;
        const int slot_prev = slot_t == 0 ? sl - 1 : slot_t - 1;          // (one 64-bit modulo per launch, not three)
        dprev = kstep > 0 ? act.done_prev + (size_t)slot_prev * act.ring_n : nullptr;
        araw = act.act_raw + (size_t)slot_t * act.ring_n;
    }
    if (!act.cursor || local) load_obs(tile);
    await_image(act.cursor, act.step_dev, epochs);
    const unsigned char *wsl = (odd && ws_alt) ? ws_alt : ws;
    if (act.cursor && !local) {          // (a caller that gave no slot count: the cursor the pack launch wrote)
        obs_base = resolve_obs(act, obs);
        const int *c = cursor_of(act);
        dprev = c[3] ? act.done_prev + (size_t)c[2] * act.ring_n : nullptr;
        araw = act.act_raw + (size_t)c[0] * act.ring_n;
        load_obs(tile);
    }
    const unsigned long long noise_step = act.step + (act.step_dev ? (unsigned long long)*act.step_dev : 0ull);
    if (act.cursor && tile0 == 0 && blockIdx.x == 0 && tid == 0)      // this launch has begun: the step chain is at step kstep
        __hip_atomic_store(act.cursor + CUR_PROGRESS, (int)(kstep + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (act.cursor && tile0 == 0 && blockIdx.x == 0 && tid < 4) {
        const int sl = act.ring_slots;
        act.cursor[tid] = !local ? cursor_of(act)[tid]
                                 : (tid == 0 ? slot_t : tid == 1 ? (slot_t + 1 == sl ? 0 : slot_t + 1)
                                                      : tid == 2 ? (slot_t == 0 ? sl - 1 : slot_t - 1) : (kstep > 0 ? 1 : 0));
    }
#pragma unroll
    for (int i = 0; i < W1_WAVE_PIECES; ++i) issue_fc1_piece(wsl, ldsw_w1_0, i);
#pragma unroll
    for (int i = 0; i < VEC_PIECES / 4; ++i)
        dma_piece(wsl, voff_vec + i * 1024, lds_base0 + RING_BYTES + wave * (VEC_PIECES / 4) * 1024, i * 1024);
    bool first = true;
#ifdef TT_STAMPS
    int round = 0;
    if (threadIdx.x == 0 && blockIdx.x < 512) for (int q = 0; q < 4; ++q) g_tile[blockIdx.x][q][0] = g_tile[blockIdx.x][q][1] = 0ull;
    if (threadIdx.x == 0 && blockIdx.x < 512) g_tile[blockIdx.x][0][0] = wall_clock64();
#endif

#pragma unroll 1
    for (;;) {
        // tile-invariant addresses, opaque per tile (see LdsBases)
        const unsigned char *wsl_cur = wsl;
        unsigned ldsw_w2 = ldsw_w2_0, ldsw_w1 = ldsw_w1_0;
        LdsBases LB = LB0;
        lds_f *pv1 = pv1_0;
        asm volatile("" : "+s"(wsl_cur), "+s"(ldsw_w2), "+s"(ldsw_w1), "+v"(LB.b0), "+v"(LB.b1), "+v"(LB.b2), "+v"(pv1));
        lds_f *pv2 = pv1 + 2 * H1P;
        const int row = tile * ROWS + wave * WROWS + r;                       // this lane's env (lanes r and r+32 share it)
#pragma unroll
        for (int s = 0; s < S1; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 16 * s + 8 * h + j;
                xo[s][j] = k < IN ? (row < n ? xo[s][j] : 0.f) : (k == IN ? 1.f : 0.f);
            }
        // this row's noise for the step (independent of the network: see load_obs), from the values requested a tile ago
        float ou_next = 0.f;
        if (with_noise) ou_next = ou_advance(row < n ? row : n - 1, ou_pre, dp_pre != 0u, act, noise_step);
        uint4 xb[S1][2];                                                      // the observation's h and m pieces
#pragma unroll
        for (int s = 0; s < S1; ++s) {
            uint32_t ph[4], pm[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) split2(xo[s][2 * p] * SX, xo[s][2 * p + 1] * SX, ph[p], pm[p]);
            xb[s][0] = make_uint4(ph[0], ph[1], ph[2], ph[3]);
            xb[s][1] = make_uint4(pm[0], pm[1], pm[2], pm[3]);
        }
        // Nothing younger than this tile's operands is in flight.  First tile: fc1 + the vectors, nothing requested after them.
        // Later tiles: fc1 and fc2 steps 0, 1 were requested under the previous tile's layer 2, before its observation loads
        // and its epilogue's stores; stores and loads retire in no fixed order, so nothing short of 0 tells that the DMA
        // pieces have landed -- and nothing of this tile has been requested yet that 0 would wait for in vain.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // publishes fc1 (and steps 0, 1); every wave is past the previous tile's layer 2: slots 2, 3 are free
        __builtin_amdgcn_s_barrier();
        if (first) NSTAMP(1);

        // ---- layer 1: acc1[t][v] = SX*SW * (pre-activation + bias) of neuron 32t + 8(v>>2) + 4h + (v&3), env `row`
        // The same pinned issue order as layer 2 below: behind the three MFMAs of product q = (tile t, step s) go the two
        // fragment reads of product q + 2 and one LDS-DMA piece (l1 rows of the schedule above).
#define SB __builtin_amdgcn_sched_barrier(0)
        f32x16 acc1[T1];
        {
            auto w1_frag = [&](const int q, const int plane) __attribute__((always_inline)) {
                return lds_frag(LB, W1_OFF + (((q % S1) * T1 + q / S1) * 2 + plane) * 1024);
            };
            // (the image base opaque once more for this layer, as layer 2 does per step: the layer's piece addresses are formed here.
            // It costs the critic variant two SGPRs, 96 as before this schedule; every other entry of the kernels' resource table is
            // what it was -- tests/golden/kernel_resources_main.json)
            const unsigned char *wsl_1 = wsl_cur;
            asm volatile("" : "+s"(wsl_1));
            uint4 a0h = w1_frag(0, 0), a0m = w1_frag(0, 1), a1h = w1_frag(1, 0), a1m = w1_frag(1, 1), a2h = a0h, a2m = a0m;
            SB;
#pragma unroll
            for (int q = 0; q < S1 * T1; ++q) {
                const int t = q / S1, s = q % S1;
                if (s == 0) {
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc1[t][v] = 0.f;
                }
                acc1[t] = mfma_f16(a0m, xb[s][0], acc1[t]); SB;                // small terms first
                if (q + 2 < S1 * T1) a2h = w1_frag(q + 2, 0);
                SB;
                acc1[t] = mfma_f16(a0h, xb[s][1], acc1[t]); SB;
                if (q + 2 < S1 * T1) a2m = w1_frag(q + 2, 1);
                SB;
                acc1[t] = mfma_f16(a0h, xb[s][0], acc1[t]); SB;
                if (q < 10) { if (first) issue_step_piece(wsl_1, ldsw_w2, q / 5, q % 5); }
                else if (q < 20) issue_step_piece(wsl_1, ldsw_w2, 2 + (q - 10) / 5, q % 5);
                SB;
                a0h = a1h; a0m = a1m; a1h = a2h; a1m = a2m;
            }
        }
        if (first) NSTAMP(2);
        // (no barrier and no request here: fc1's slots are written again only behind the barrier in front of layer 2)
        uint32_t hb[STEPS][4], mb[STEPS][4];
        // LayerNorm(400) (biased variance, eps 1e-5) on the SCALED pre-activations: mean and deviations scale with them,
        // 1/sigma absorbs the scale; then gamma*SX, beta*SX and ReLU give the layer-2 operand already scaled by SX.
        // Tile 12 holds neurons 384..399 in v < 8.
        // Only the two statistics passes stand between the layers.  The third pass -- normalise, ReLU, split into the two f16
        // pieces layer 2 multiplies with -- needs nothing but mean and 1/sigma and produces the B operand of ONE k16 step from
        // 16 accumulator registers, so it runs INSIDE layer 2 (round 4), two steps ahead of the step that multiplies with it, in
        // the issue slots the matrix pipe leaves free (ln_chunk below).  hb[s] / mb[s] are the B fragments (h, m planes) of k16
        // step s -- element j of lane half h is neuron 16 s + 8 (j >> 2) + 4 h + (j & 3), i.e. registers 8 (s & 1) .. + 7 of tile
        // s >> 1, the order the packed fc2 fragments are laid out in.
        f32x2 nmean, rstdp;
        {
            f32x2 sp = pk(0.f, 0.f);
#pragma unroll
            for (int t = 0; t < T1; ++t)
#pragma unroll
                for (int v = 0; v < (t == T1 - 1 ? 8 : 16); v += 4)
                    sp += pk(acc1[t][v], acc1[t][v + 1]) + pk(acc1[t][v + 2], acc1[t][v + 3]);
            const float s = sp[0] + sp[1];
            const float mean = (s + __shfl_xor(s, 32)) * (1.f / H1);
            nmean = pk(-mean, -mean);
            f32x2 ssp = pk(0.f, 0.f);
#pragma unroll
            for (int t = 0; t < T1; ++t)
#pragma unroll
                for (int v = 0; v < (t == T1 - 1 ? 8 : 16); v += 2) {
                    const f32x2 d = pk(acc1[t][v], acc1[t][v + 1]) + nmean;   // (formed again where it is used: same operation, same bits)
                    ssp = pk_fma(d, d, ssp);
                }
            const float ss = ssp[0] + ssp[1];
            const float var = (ss + __shfl_xor(ss, 32)) * (1.f / H1) * (UNSCALE * UNSCALE);
            const float rstd = rsqrtf(var + 1e-5f) * UNSCALE;
            rstdp = pk(rstd, rstd);
        }
        // One GROUP = four neurons of this lane (registers 4i .. 4i+3 of tile t; group number G = 4t + i = 2 * step + half), in
        // five chunks of 3-4 vector instructions; a chunk fits in the shadow of one MFMA.  gamma/beta of group G + 1 are read
        // from LDS in chunk 2 of group G (three tiles of MFMAs before their use).
        constexpr int GROUPS = 2 * STEPS;                                     // 50: tile 12 has groups 48, 49 only
        float4 gq[2], bq[2];
        f32x2 ya, yb;
        float y0, y1, y2, y3;
        auto ln_read = [&](const int G) __attribute__((always_inline)) {
            gq[G & 1] = lds4(pv1 + 8 * G);                                    // 32 t + 8 i
            bq[G & 1] = lds4(pv1 + H1P + 8 * G);
        };
        auto ln_chunk = [&](const int G, const int k) __attribute__((always_inline)) {
            const int t = G >> 2, i = G & 3, st = G >> 1, e = 2 * (G & 1);
            const float4 g = gq[G & 1], be = bq[G & 1];
            if (k == 0) ya = pk_fma((pk(acc1[t][4 * i], acc1[t][4 * i + 1]) + nmean) * rstdp, pk(g.x, g.y), pk(be.x, be.y));
            if (k == 1) yb = pk_fma((pk(acc1[t][4 * i + 2], acc1[t][4 * i + 3]) + nmean) * rstdp, pk(g.z, g.w), pk(be.z, be.w));
            if (k == 2) {
                y0 = fmaxf(ya[0], 0.f); y1 = fmaxf(ya[1], 0.f); y2 = fmaxf(yb[0], 0.f); y3 = fmaxf(yb[1], 0.f);
                if (G + 1 < GROUPS) ln_read(G + 1);
            }
            if (k == 3) split2(y0, y1, hb[st][e], mb[st][e]);
            if (k == 4) split2(y2, y3, hb[st][e + 1], mb[st][e + 1]);
        };
        // steps 0 and 1 (groups 0..3) before the first MFMA
        ln_read(0);
#pragma unroll
        for (int G = 0; G < 4; ++G)
#pragma unroll
            for (int k = 0; k < 5; ++k) ln_chunk(G, k);

        if (first) NSTAMP(3);
        // ---- layer 2: 25 k16 steps x 10 neuron tiles x 3 f16 MFMAs; the h1 registers are the B operand
        f32x16 acc2[T2];
#pragma unroll
        for (int u = 0; u < T2; ++u)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc2[u][v] = 0.f;
        // Hand-pipelined issue order, pinned with sched_barrier(0) between every pair of instruction groups: each of the
        // three MFMAs of a tile is followed by one small job that issues while the matrix pipe is busy (an MFMA holds the
        // wave's issue port for 8 of its 32 cycles) -- the two fragment reads of the tile two ahead, and in tiles 5..9 one
        // LDS-DMA piece of step s + 6 -- and, behind the first MFMA of every tile, one chunk of LayerNorm 1's last pass for the B
        // operand of step s + 2 (a tenth of a step's worth: 3-4 vector instructions).
        // One barrier per step, in the middle (before tile 5): it publishes step s + 1 (every wave has waited for its own
        // pieces of it with a COUNTED vmcnt that leaves the younger pieces in flight: mid_allowed) and tells that every wave is
        // past step s - 1, whose slot the pieces behind it overwrite (l2_job).  Fragments are read TWO tiles ahead
        // (tiles 0, 1 of step s + 1 during tiles 8, 9 of step s, after that barrier), so a read has six MFMAs to land.
        // Step 0 has no such barrier: step 1 is published by the barrier in front of the loop and its pieces go to fc1's
        // slots.  Step 24 has none either: nothing is read after it and nothing is issued in it.
        asm volatile("s_waitcnt vmcnt(10)" ::: "memory");      // steps 0 and 1 (this wave's pieces); 2 and 3 (layer 1) may still fly
        // publishes steps 0, 1; every wave is past its layer 1: fc1's slots 4..6 are free for steps 4, 5, 6
        __builtin_amdgcn_s_barrier();
        // A fragments (h, m) of three consecutive tiles: the current one, the next, and the one being read (two ahead);
        // rotated by renaming at the end of every tile (the loops are fully unrolled: no moves)
        uint4 c0h = lds_frag(LB, 0), c0m = lds_frag(LB, 1024), c1h = lds_frag(LB, 2048), c1m = lds_frag(LB, 3072), c2h = c0h, c2m = c0m;
        SB;
        auto l2_step = [&](const int s) __attribute__((always_inline)) {
            const uint4 vh = make_uint4(hb[s][0], hb[s][1], hb[s][2], hb[s][3]), vm = make_uint4(mb[s][0], mb[s][1], mb[s][2], mb[s][3]);
            const int slot = (s % RING) * CHUNK_BYTES, nslot = ((s + 1) % RING) * CHUNK_BYTES;
            // (per step, so that the step's five DMA addresses are formed here and not all 125 at the top of the tile)
            const unsigned char *wsl_s = wsl_cur;
            unsigned lds_s = ldsw_w2, lds1_s = ldsw_w1;
            asm volatile("" : "+s"(wsl_s), "+s"(lds_s));
            if (s >= TAIL0 && s < TAIL0 + 3) asm volatile("" : "+s"(lds1_s));
#pragma unroll
            for (int u = 0; u < T2; ++u) {
                if (u == T2 / 2 && s >= 1 && s + 1 < STEPS) {
                    // step s + 1 must have landed; the pieces issued after it may still be in flight (mid_counts_ok: 20 or 18)
                    switch (L2S.mid[s]) {
                        case 20: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); break;
                        default: asm volatile("s_waitcnt vmcnt(18)" ::: "memory"); break;
                    }
                    __builtin_amdgcn_s_barrier();
                    SB;
                }
                const bool more = u + 2 < T2 || s + 1 < STEPS;                // is there a tile two ahead to prefetch
                const int nx = u + 2 < T2 ? slot + (u + 2) * 2048 : nslot + (u + 2 - T2) * 2048;
                acc2[u] = mfma_f16(c0h, vm, acc2[u]); SB;      // small terms first
                if (more) c2h = lds_frag(LB, nx);
                if (s + 2 < STEPS) ln_chunk(2 * (s + 2) + u / 5, u % 5);      // LayerNorm 1's last pass for step s + 2
                SB;
                acc2[u] = mfma_f16(c0m, vh, acc2[u]); SB;
                if (more) c2m = lds_frag(LB, nx + 1024);
                SB;
                acc2[u] = mfma_f16(c0h, vh, acc2[u]); SB;
                {
                    // (one request statement, its operands selected by the job: all constants once s and u are)
                    const int j = L2S.job[s][u];
                    const bool f1 = j >= JOB_FC1 && j < JOB_NEXT;
                    const int st = j >= JOB_NEXT ? j - JOB_NEXT : j, i1 = j - JOB_FC1;
                    if (j != JOB_NONE)
                        dma_piece(wsl_s, f1 ? voff_w1 + i1 * 4096 : voff_w2 + st * CHUNK_BYTES + l2_piece(u) * 1024, f1 ? lds1_s : lds_s,
                                  f1 ? i1 * 4096 : (st % RING) * CHUNK_BYTES + l2_piece(u) * 1024);
                }
                SB;
                c0h = c1h; c0m = c1m; c1h = c2h; c1m = c2m;
            }
        };
        // (three loops, not one: the unroller takes a loop only up to a size, and it sizes the body before s is a constant)
#pragma unroll
        for (int s = 0; s < 2; ++s) l2_step(s);
#pragma unroll
        for (int s = 2; s < TAIL0; ++s) l2_step(s);
#pragma unroll
        for (int s = TAIL0; s < STEPS; ++s) l2_step(s);
#undef SB

        if (first) NSTAMP(4);
        // ---- the next tile of this workgroup: its packed fc1 and fc2 steps 0, 1 are on their way (layer 2's tail); its
        // observations are requested NOW and land behind the epilogue below (they go to registers: no barrier)
        const int next = tile + (int)gridDim.x;
        const bool more_tiles = next < tile_end;
        if (more_tiles) load_obs(next);
        // ---- epilogue: scale back + bias, LayerNorm(300), (critic: + action_value(a)), ReLU, head; acc2[u][v] is neuron
        // 32u + 8(v>>2) + 4h + (v&3); 300 = 9*32 + 12, so groups of four are all real or all padding
        // (the per-neuron vectors are read from LDS one tile ahead of their use, as in LayerNorm 1)
        f32x2 s2p = pk(0.f, 0.f);
        {
            float4 bq[2][4];
            auto ldb = [&](const int u, float4 (&b)[4]) {
#pragma unroll
                for (int i = 0; i < 4; ++i) b[i] = lds4(pv2 + 32 * u + 8 * i);   // zero beyond 300
            };
            ldb(0, bq[0]);
#pragma unroll
            for (int u = 0; u < T2; ++u) {
                if (u + 1 < T2) ldb(u + 1, bq[(u + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float4 b = bq[u & 1][i];
                    const f32x2 xa = pk_fma(pk(acc2[u][4 * i], acc2[u][4 * i + 1]), pk(UNSCALE, UNSCALE), pk(b.x, b.y));
                    const f32x2 xb2 = pk_fma(pk(acc2[u][4 * i + 2], acc2[u][4 * i + 3]), pk(UNSCALE, UNSCALE), pk(b.z, b.w));
                    acc2[u][4 * i] = xa[0]; acc2[u][4 * i + 1] = xa[1]; acc2[u][4 * i + 2] = xb2[0]; acc2[u][4 * i + 3] = xb2[1];
                    s2p += xa + xb2;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        const float s2 = s2p[0] + s2p[1];
        const float mean2 = (s2 + __shfl_xor(s2, 32)) * (1.f / H2);
        const f32x2 nmean2 = pk(-mean2, -mean2);
        // deviations in place (the last pass needs nothing else of the pre-activations); padding groups do not count
        f32x2 ss2p = pk(0.f, 0.f);
#pragma unroll
        for (int u = 0; u < T2; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool real = 32 * u + 8 * i + 4 * h < H2;
                const f32x2 keep = real ? pk(1.f, 1.f) : pk(0.f, 0.f);
#pragma unroll
                for (int j = 0; j < 4; j += 2) {
                    const f32x2 d = pk(acc2[u][4 * i + j], acc2[u][4 * i + j + 1]) + nmean2;
                    acc2[u][4 * i + j] = d[0]; acc2[u][4 * i + j + 1] = d[1];
                    const f32x2 dk = (32 * u + 8 * i + 4 < H2) ? d : d * keep;      // only the last tiles can hold padding
                    ss2p = pk_fma(dk, dk, ss2p);
                }
            }
        const float ss2 = ss2p[0] + ss2p[1];
        const float rstd2 = rsqrtf((ss2 + __shfl_xor(ss2, 32)) * (1.f / H2) + 1e-5f);
        const f32x2 rstd2p = pk(rstd2, rstd2);
        const float av = (CRITIC && row < n) ? action[row] : 0.f;
        f32x2 dotp = pk(0.f, 0.f);
        {
            constexpr int NV = CRITIC ? 5 : 3;                  // gamma2, beta2, w3 (, wa, ba)
            float4 vq[2][4][NV];
            auto ldv = [&](const int u, float4 (&v)[4][NV]) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int q = 0; q < NV; ++q) v[i][q] = lds4(pv2 + (q + 1) * H2P + 32 * u + 8 * i);
            };
            ldv(0, vq[0]);
#pragma unroll
            for (int u = 0; u < T2; ++u) {
                if (u + 1 < T2) ldv(u + 1, vq[(u + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float4 g = vq[u & 1][i][0], be = vq[u & 1][i][1], w3 = vq[u & 1][i][2];
                    f32x2 ya = pk_fma(pk(acc2[u][4 * i], acc2[u][4 * i + 1]) * rstd2p, pk(g.x, g.y), pk(be.x, be.y));
                    f32x2 yb = pk_fma(pk(acc2[u][4 * i + 2], acc2[u][4 * i + 3]) * rstd2p, pk(g.z, g.w), pk(be.z, be.w));
                    if (CRITIC) {
                        const float4 wa = vq[u & 1][i][NV - 2], ba = vq[u & 1][i][NV - 1];
                        ya += pk_fma(pk(av, av), pk(wa.x, wa.y), pk(ba.x, ba.y));
                        yb += pk_fma(pk(av, av), pk(wa.z, wa.w), pk(ba.z, ba.w));
                    }
                    dotp = pk_fma(pk(fmaxf(ya[0], 0.f), fmaxf(ya[1], 0.f)), pk(w3.x, w3.y), dotp);      // w3 = 0 on padding
                    dotp = pk_fma(pk(fmaxf(yb[0], 0.f), fmaxf(yb[1], 0.f)), pk(w3.z, w3.w), dotp);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        const float dot = dotp[0] + dotp[1];
        // A row with a NaN or inf pre-activation in either layer has a NaN 1/sigma there, but fmaxf(NaN, 0) = 0 would hand on zeros
        // and the row would end as the finite tanh(b3) / b3.  The row's two 1/sigma (critic: and its action) go into the head value
        // through a term that is exactly -0 for finite inputs (v + -0 = v for every v, -0 included) and NaN otherwise: one
        // multiply-add per ROW, and the torch modules' result (F.relu propagates NaN).
        float poison = rstdp[0] * (rstd2 * -0.f);
        if (CRITIC) poison = fmaf(fabsf(av), -0.f, poison);
        const float v = dot + __shfl_xor(dot, 32) + lds4(pv1 - 4 * h + VEC_FLOATS).x + poison;
        if (h == 0 && row < n) {
            if (with_noise) finish_row_noise(row, v, out, act, ou_next, araw);
            else finish_row<CRITIC>(row, v, out, act);
        }
        if (first) NSTAMP(5);
#ifdef TT_STAMPS
        TSTAMP(round, 1);
        if (threadIdx.x == 0 && blockIdx.x < 512 && round < 4) tt_log_add(g_log_tile, g_tile[blockIdx.x][round][0], g_tile[blockIdx.x][round][1]);
        ++round;
        if (more_tiles) TSTAMP(round, 0);
#endif
        if (!more_tiles) break;
        tile = next;
        first = false;
    }
    // the last tile's tail requested a next tile's operands like every other: no piece may be in flight when the wave ends
    // (the LDS goes to another workgroup).  They were issued an epilogue ago: the wait is over before it begins.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace

#ifdef TT_STAMPS
int split_debug_stamps(unsigned long long *out16) {
    return hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_nstamps), sizeof(unsigned long long) * 16) == hipSuccess ? 0 : -3;
}
int split_debug_tiles(unsigned long long *out4096) {
    return hipMemcpyFromSymbol(out4096, HIP_SYMBOL(g_tile), sizeof(unsigned long long) * 512 * 4 * 2) == hipSuccess ? 0 : -3;
}
int split_debug_log(unsigned long long *out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_log_tile), sizeof(TTLog)) != hipSuccess) return -3;
    if (reset) { const unsigned long long z = 0; if (hipMemcpyToSymbol(HIP_SYMBOL(g_log_tile), &z, sizeof(z)) != hipSuccess) return -3; }
    return 0;
}
int split_debug_poll(unsigned long long *out4) {
    return hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_poll), sizeof(unsigned long long) * 4) == hipSuccess ? 0 : -3;
}
int split_debug_block_stamps(unsigned long long *out, int nblocks) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bstamps), sizeof(unsigned long long) * 8 * (nblocks < 4096 ? nblocks : 4096)) == hipSuccess ? 0 : -3;
}
#endif

size_t split_ws_bytes() { return (size_t)WS_BYTES; }

int split_pack(const tt_mlp_weights *w, bool critic, void *ws, long long *bump, const RingCursor &cur, hipStream_t stream) {
    // (the second image takes part only when the caller packs into the struct's own workspace)
    unsigned char *alt = ws == w->split_ws ? reinterpret_cast<unsigned char *>(w->split_ws_alt) : nullptr;
    hipLaunchKernelGGL(k_split_pack, dim3(PACK_BLOCKS), dim3(256), 0, stream, to_weights(w), critic,
                       reinterpret_cast<unsigned char *>(ws), alt, bump, cur);
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

int split_pack_and_sample(const tt_mlp_weights *w, bool critic, void *ws, const RingSample &R, const RingCursor &cur,
                          hipStream_t stream) {
    unsigned char *alt = ws == w->split_ws ? reinterpret_cast<unsigned char *>(w->split_ws_alt) : nullptr;
    hipLaunchKernelGGL(k_pack_and_sample, dim3(PACK_BLOCKS + (R.batch * R.draws + 3) / 4), dim3(256), 0, stream, to_weights(w), critic,
                       reinterpret_cast<unsigned char *>(ws), alt, R, cur);
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

template <bool CRITIC>
static int launch_split(int n, const float *obs, const float *action, const tt_mlp_weights *w, float *out,
                        const ActArgs &act, hipStream_t stream) {
    static bool attr[64] = {};      // per device: a function attribute set on one device says nothing about another
    static int cus[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return TT_EHIP;
    if (!attr[dev]) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mlp_split<CRITIC>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess)
            return TT_EHIP;
        int c = 0;
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
        cus[dev] = c;
        attr[dev] = true;
    }
    // One workgroup per CU is resident (LDS), and a workgroup takes its tiles in turn (tile, tile + grid, ...).
    // max_workgroups > 0: never more than that many CUs are busy with this forward (the rest stay free for launches on other
    // streams): the tiles are shared out in rounds of at most that many, ONE launch of the equal share (512 tiles, limit 192 ->
    // 171 workgroups x 3 tiles).  capped_grids > 0: only that many rounds are capped -- what the cap makes room for is over by
    // then -- and the rest of the tiles go out in a second launch over the whole chip.  0: one launch over the whole chip.
    const int ntiles = (n + ROWS - 1) / ROWS;
    const int chip = cus[dev];
    int capped = 0;
    if (w->max_workgroups > 0) {
        const int limit = w->max_workgroups;
        capped = ntiles;
        if (w->capped_grids > 0 && (long long)w->capped_grids * limit < ntiles) capped = w->capped_grids * limit;
        const int rounds = (capped + limit - 1) / limit, g = (capped + rounds - 1) / rounds;
        hipLaunchKernelGGL((k_mlp_split<CRITIC>), dim3(g), dim3(256), LDS_BYTES, stream, n, 0, capped, act.cursor, act.step_dev, obs,
                           reinterpret_cast<const unsigned char *>(w->split_ws),
                           reinterpret_cast<const unsigned char *>(w->split_ws_alt), action, out, act);
    }
    if (capped < ntiles) {
        const int rest = ntiles - capped, rounds = (rest + chip - 1) / chip, g = (rest + rounds - 1) / rounds;
        hipLaunchKernelGGL((k_mlp_split<CRITIC>), dim3(g), dim3(256), LDS_BYTES, stream, n, capped, ntiles, act.cursor, act.step_dev, obs,
                           reinterpret_cast<const unsigned char *>(w->split_ws),
                           reinterpret_cast<const unsigned char *>(w->split_ws_alt), action, out, act);
    }
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

int split_forward(bool critic, int n, const float *obs, const float *action, const tt_mlp_weights *w, float *out,
                  const ActArgs &act, hipStream_t stream) {
    return critic ? launch_split<true>(n, obs, action, w, out, act, stream)
                  : launch_split<false>(n, obs, action, w, out, act, stream);
}

}  // namespace ttnet
