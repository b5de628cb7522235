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

// The device side by concern.  ONE translation unit: the order of these includes, and of the two further
// down, is the order that keeps every kernel's code -- the non-template kernels stay in the order k_reset .. k_random_actions
// (pose), k_log_zero .. k_log_drain (log), k_hold_* (hold), k_reset_curriculum .. k_curriculum_update (curriculum), k_reset_rnd,
// k_rnd_seed (randomize), k_reset_task (task), k_harvest_plan, k_harvest_copy (harvest), and the template kernels are instantiated in the order the host side below first names them.
#include "ttenv_math.h"        // KTable, tt_sincos*, tt_exp_neg, tt_atan2_readback, tt_wrap_pi, u01
#include "ttenv_state.h"       // rows, pk_*, KParams, Bufs, Goal, Env, observe, store_obs_tile, load / store / place_env, draws
#include "ttenv_step.h"        // StepOut, Info, step_env, write_info
#include "ttenv_pose.h"        // k_reset .. k_random_actions, k_observe
#include "ttenv_log.h"         // EpLog, log_append, tally_append, k_log_zero .. k_log_drain
#include "ttenv_hold.h"        // HoldCols, k_step_hold, k_hold_begin / live / read

// ------------------------------------------------------------------------------------------
// the vector step.  RANDOM_POLICY: the action is drawn in-kernel (BASELINE.json config 2), keyed by
// (policy seed, env, step-in-episode, episode number) so that a captured hipGraph replays correctly.
#ifdef TT_STAMPS
#include "ttstamps.h"
__device__ unsigned long long g_stepblk[1024][2];
__device__ TTLog g_log_step;
#endif
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

// behind the TT_STEP_* pieces, which the curriculum's and the randomised step kernels paste
#include "ttenv_mpc.h"         // MpcK, mpc_plan_body, k_mpc_plan / act_ring / label_ring
#include "ttenv_curriculum.h"  // CurDev, k_step_cur, k_step_cur_log, k_reset_curriculum .. k_curriculum_update
#include "ttenv_randomize.h"   // RndDev, randomized_task, k_step_rnd, k_step_rnd_log, k_reset_rnd, k_rnd_seed
#include "ttenv_task.h"        // TaskDev, task_draw, k_step_task, k_step_task_log, k_reset_task
#include "ttenv_harvest.h"     // HarvestK, HarvestRecs, k_harvest_plan, k_harvest_copy

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
    // episode randomisation (tt_env_set_randomization): the descriptor in device memory and the ranges as given; rnd_dev == nullptr
    // <=> off
    RndDev *rnd_dev = nullptr;
    tt_randomization rnd{};
    // task curriculum (tt_env_set_task_curriculum): the descriptor in device memory (followed, in the same block, by the arrays the
    // handle owns), its host copy and the option as given; task_dev == nullptr <=> off.  On only while rnd_dev is.
    void *task_block = nullptr;
    TaskDev *task_dev = nullptr;
    TaskDev task{};
    tt_task_curriculum task_cfg{};
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

// The close the launching entry points share, written once: TT_LAUNCH is a launch (hipLaunchKernelGGL, or by_per_env around one:
// the variadic tail takes its commas) and the launch's error; TT_RUN is the whole tail behind an entry point's refusals -- the
// handle's device made current, the launch, its error, TT_OK.  Macros like TT_HIP, which returns from the entry point.
#define TT_LAUNCH(env, ...)                                                                  \
    do {                                                                                     \
        __VA_ARGS__;                                                                         \
        TT_HIP(env, hipGetLastError());                                                      \
    } while (0)
#define TT_RUN(env, ...)                                                                     \
    do {                                                                                     \
        TT_HIP(env, hipSetDevice(env->device));                                              \
        TT_LAUNCH(env, __VA_ARGS__);                                                         \
        return TT_OK;                                                                        \
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
    if (e->task_dev && auto_reset) {    // the task curriculum counts and draws where the step resets (randomisation is on with it)
        const TaskDev *tk = e->task_dev;
        if (e->log_bytes) launch(k_step_task_log<INFO, RANDOM_POLICY>, e->log, tk);
        else launch(k_step_task<INFO, RANDOM_POLICY>, tk);
    } else if (e->rnd_dev && auto_reset) {     // the task is drawn where the step resets (a per-env handle; never with the detailed log)
        const RndDev *rnd = e->rnd_dev;
        if (e->log_bytes) launch(k_step_rnd_log<INFO, RANDOM_POLICY>, e->log, rnd);
        else launch(k_step_rnd<INFO, RANDOM_POLICY>, rnd);
    } else if (e->cur_dev && auto_reset) {     // the curriculum counts and draws where the step resets (never with the detailed log)
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
        TT_LAUNCH(env, hipLaunchKernelGGL(k_tally_zero, dim3(grid_for(k)), dim3(BLOCK), 0, stream, env->n, k, mask, idx, env->log,
                                          env->npad));
    else
        TT_LAUNCH(env, hipLaunchKernelGGL(k_log_zero, dim3(grid_for(k)), dim3(BLOCK), 0, stream, env->n, k, mask, idx, env->log.acc));
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
    if ((flags & TT_LOG_DETAIL) && capacity > 0 && env->rnd_dev)
        return fail_both(env, TT_EINVAL, "%s: the detailed episode log with episode randomisation is not supported (the randomised step "
                                         "kernels carry the plain log only); tt_env_set_randomization(env, NULL, ...) first", fn);
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

// lanes placed from outside (entry j < k names lane idx[j], idx NULL: lane j): no curriculum draw made their episode, neither the
// start-pose curriculum's nor the task curriculum's
int curriculum_unset(tt_env *env, int k, const int32_t *idx, hipStream_t stream) {
    for (uint32_t *cell : {env->cur_dev ? env->cur.cell : nullptr, env->task_dev ? env->task.cur.cell : nullptr})
        if (cell) TT_LAUNCH(env, hipLaunchKernelGGL(k_curriculum_unset, dim3(grid_for(k)), dim3(BLOCK), 0, stream, env->n, k, idx, cell));
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
    TT_LAUNCH(env, hipLaunchKernelGGL(k_log_drain, g, dim3(BLOCK), 0, stream, env->log, ret, len, flags, success, lane,
                                      reinterpret_cast<long long *>(end_step), reinterpret_cast<long long *>(n_out),
                                      reinterpret_cast<unsigned long long *>(counts_out)));
    if (comp || start) TT_LAUNCH(env, hipLaunchKernelGGL(k_tally_drain, g, dim3(BLOCK), 0, stream, env->log, comp, start));
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
    if (env->rnd_dev) (void)hipFree(env->rnd_dev);
    if (env->task_block) (void)hipFree(env->task_block);
    for (hipEvent_t ev : env->ev_start) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : env->ev_stop) (void)hipEventDestroy(ev);
    delete env;
    return TT_OK;
}

int tt_env_num_envs(const tt_env *env) { return env ? env->n : TT_EINVAL; }

int tt_env_reset(tt_env *env, const uint8_t *mask, uint64_t seed, float *obs_out, tt_stream_t stream) {
    TT_ENTER(env);
    env->seed = seed;
    if (env->task_dev) {        // (randomisation is on with it: both descriptors get the seed)
        hipLaunchKernelGGL(k_rnd_seed, dim3(1), dim3(1), 0, stream, env->rnd_dev, env->seed);
        hipLaunchKernelGGL(k_rnd_seed, dim3(1), dim3(1), 0, stream, &env->task_dev->rnd, env->seed);
        hipLaunchKernelGGL(k_reset_task, dim3(grid_for(env->n)), dim3(BLOCK), 0, stream, env->kp, env->n, env->b, mask, obs_out,
                           env->seed, (const TaskDev *)env->task_dev);
    } else if (env->rnd_dev) {
        hipLaunchKernelGGL(k_rnd_seed, dim3(1), dim3(1), 0, stream, env->rnd_dev, env->seed);
        hipLaunchKernelGGL(k_reset_rnd, dim3(grid_for(env->n)), dim3(BLOCK), 0, stream, env->kp, env->n, env->b, mask, obs_out,
                           env->seed, (const RndDev *)env->rnd_dev);
    } else if (env->cur_dev) {
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
    if (env->rnd_dev) {         // the randomised step kernels read the pool from the descriptor (RndDev); a setter, not a hot call
        TT_HIP(env, hipSetDevice(env->device));
        TT_HIP(env, hipDeviceSynchronize());
        TT_HIP(env, hipMemcpy(&env->rnd_dev->pool, &env->kp.pool, sizeof(env->kp.pool), hipMemcpyHostToDevice));
        TT_HIP(env, hipMemcpy(&env->rnd_dev->pool_m, &env->kp.pool_m, sizeof(env->kp.pool_m), hipMemcpyHostToDevice));
        if (env->task_dev) {    // ... and so do the task curriculum's, from theirs
            TT_HIP(env, hipMemcpy(&env->task_dev->rnd.pool, &env->kp.pool, sizeof(env->kp.pool), hipMemcpyHostToDevice));
            TT_HIP(env, hipMemcpy(&env->task_dev->rnd.pool_m, &env->kp.pool_m, sizeof(env->kp.pool_m), hipMemcpyHostToDevice));
        }
    }
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
    TT_LAUNCH(env, hipLaunchKernelGGL(k_set_pose, dim3(grid_for(k)), dim3(BLOCK), 0, stream, env->kp, env->n, env->b, idx, k, start,
                                      goal, L2, obs_out));
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
    TT_LAUNCH(env, hipLaunchKernelGGL(k_set_attrs, dim3(grid_for(k)), dim3(BLOCK), 0, stream, env->kp, env->n, env->b, idx, k, start,
                                      goal, L2));
    return TT_OK;
}

int tt_env_set_state(tt_env *env, const int32_t *idx, int k, const double *state, tt_stream_t stream) {
    TT_HANDLE(env);
    if (k < 0 || k > env->n || (k > 0 && !state))
        return fail(env, TT_EINVAL, "tt_env_set_state: k=%d outside [0,%d] or state NULL", k, env->n);
    if (k == 0) return TT_OK;
    TT_HIP(env, hipSetDevice(env->device));
    TT_LAUNCH(env, hipLaunchKernelGGL(k_set_state, dim3(grid_for(k)), dim3(BLOCK), 0, stream, env->n, env->b, idx, k, state));
    return curriculum_unset(env, k, idx, stream);
}

int tt_env_get_state(tt_env *env, double *state_out, tt_stream_t stream) {
    if (!env || !state_out) return fail(env, TT_EINVAL, "tt_env_get_state: NULL argument");
    TT_RUN(env, hipLaunchKernelGGL(k_get_state, dim3(grid_for(env->n)), dim3(BLOCK), 0, stream, env->n, env->b, state_out));
}

int tt_env_set_max_steps(tt_env *env, const int32_t *idx, int k, const int32_t *max_steps, tt_stream_t stream) {
    TT_HANDLE(env);
    if (k < 0 || k > env->n || (k > 0 && !max_steps))
        return fail(env, TT_EINVAL, "tt_env_set_max_steps: k=%d outside [0,%d] or max_steps NULL", k, env->n);
    if (k == 0) return TT_OK;
    TT_HIP(env, hipSetDevice(env->device));
    if (const int rc = check_counter_range(env, max_steps, k, stream, __func__, "max_steps")) return rc;
    TT_LAUNCH(env, hipLaunchKernelGGL(k_set_max_steps, dim3(grid_for(k)), dim3(BLOCK), 0, stream, env->n, env->b, idx, k, max_steps));
    return TT_OK;
}

int tt_env_set_steps(tt_env *env, const int32_t *idx, int k, const int32_t *steps, tt_stream_t stream) {
    TT_HANDLE(env);
    if (k < 0 || k > env->n || (k > 0 && !steps))
        return fail(env, TT_EINVAL, "tt_env_set_steps: k=%d outside [0,%d] or steps NULL", k, env->n);
    if (k == 0) return TT_OK;
    TT_HIP(env, hipSetDevice(env->device));
    if (const int rc = check_counter_range(env, steps, k, stream, __func__, "steps")) return rc;
    TT_LAUNCH(env, hipLaunchKernelGGL(k_set_steps, dim3(grid_for(k)), dim3(BLOCK), 0, stream, env->n, env->b, idx, k, steps));
    return TT_OK;
}

int tt_env_get_episode(tt_env *env, int32_t *steps, int32_t *max_steps, double *start, double *goal, double *L2,
                       tt_stream_t stream) {
    TT_HANDLE(env);
    if (!steps && !max_steps && !start && !goal && !L2) return TT_OK;
    TT_RUN(env, hipLaunchKernelGGL(k_get_episode, dim3(grid_for(env->n)), dim3(BLOCK), 0, stream, env->kp, env->n, env->b, steps,
                                   max_steps, start, goal, L2));
}

int tt_env_observe(tt_env *env, const float *steering, float *obs_out, tt_stream_t stream) {
    if (!env || !obs_out) return fail(env, TT_EINVAL, "tt_env_observe: NULL argument");
    TT_RUN(env, by_per_env(env, [&](auto per_env) {
        hipLaunchKernelGGL(k_observe<decltype(per_env)::value>, dim3(grid_for(env->n)), dim3(BLOCK), 0, stream, env->kp, env->n, env->b,
                           steering, obs_out);
    }));
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
    env->per_env = meta[0] != 0 || env->rnd_dev;      // (a randomised handle stays a per-env handle: every blob has the rows)
    env->seed = meta[1];
    if (env->rnd_dev) TT_LAUNCH(env, hipLaunchKernelGGL(k_rnd_seed, dim3(1), dim3(1), 0, stream, env->rnd_dev, env->seed));
    if (env->task_dev) TT_LAUNCH(env, hipLaunchKernelGGL(k_rnd_seed, dim3(1), dim3(1), 0, stream, &env->task_dev->rnd, env->seed));
    if (env->cur_dev) TT_LAUNCH(env, hipLaunchKernelGGL(k_curriculum_seed, dim3(1), dim3(1), 0, stream, env->cur_dev, env->seed));
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
    TT_RUN(env, hipLaunchKernelGGL(k_hold_begin, dim3(grid_for(env->npad)), dim3(BLOCK), 0, stream, env->n, env->npad, env->hold_block));
}

int tt_env_step_hold(tt_env *env, const float *mu, float action_scale, float *obs, tt_stream_t stream) {
    TT_HANDLE(env);
    // (before the handle is read: these hold for any handle)
    if (!mu || !obs) return tthost::fail(TT_EINVAL, "tt_env_step_hold: mu and obs are required");
    if (!std::isfinite(action_scale)) return tthost::fail(TT_EINVAL, "tt_env_step_hold: action_scale is not finite");
    if (!env->hold_block) return fail(env, TT_EINVAL, "tt_env_step_hold: hold is not enabled (tt_env_set_hold)");
    TT_RUN(env, by_per_env(env, [&](auto per_env) {
        hipLaunchKernelGGL(k_step_hold<decltype(per_env)::value>, dim3(grid_for(env->n)), dim3(BLOCK), 0, stream, env->kp, env->n,
                           env->b, mu, action_scale, obs, env->hold_block);
    }));
}

int tt_env_hold_read(tt_env *env, double *ret, int32_t *len, uint8_t *flags, uint8_t *success, double *end, int64_t *live_out,
                     tt_stream_t stream) {
    TT_HANDLE(env);
    if (!env->hold_block) return fail(env, TT_EINVAL, "tt_env_hold_read: hold is not enabled (tt_env_set_hold)");
    TT_HIP(env, hipSetDevice(env->device));
    if (ret || len || flags || success || end)
        TT_LAUNCH(env, hipLaunchKernelGGL(k_hold_read, dim3(grid_for(env->n)), dim3(BLOCK), 0, stream, env->n, env->npad,
                                          env->hold_block, ret, len, flags, success, end));
    if (live_out)
        TT_LAUNCH(env, hipLaunchKernelGGL(k_hold_live, dim3(1), dim3(BLOCK), 0, stream, env->npad, env->hold_block,
                                          reinterpret_cast<long long *>(live_out)));
    return TT_OK;
}

int tt_env_rollout_random(tt_env *env, int k_steps, uint64_t policy_seed, float *obs_out, float *reward_sum,
                          int32_t *episodes_done, tt_stream_t stream) {
    TT_HANDLE(env);
    if (k_steps < 0) return fail(env, TT_EINVAL, "tt_env_rollout_random: k_steps=%d", k_steps);
    if (env->log_bytes) return fail(env, TT_EINVAL, "tt_env_rollout_random: the episode log does not follow k_rollout; disable it first");
    if (env->cur_dev) return fail(env, TT_EINVAL, "tt_env_rollout_random: the curriculum does not follow k_rollout; turn it off first");
    if (env->rnd_dev)
        return fail_both(env, TT_EINVAL, "tt_env_rollout_random: episode randomisation does not follow k_rollout; turn it off first");
    if (k_steps == 0) return TT_OK;
    TT_RUN(env, by_per_env(env, [&](auto per_env) {
        hipLaunchKernelGGL(k_rollout<decltype(per_env)::value>, dim3(grid_for(env->n)), dim3(BLOCK), 0, stream, env->kp, env->n, env->b,
                           k_steps, obs_out, reward_sum, episodes_done, env->seed, policy_seed);
    }));
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
    TT_RUN(env, by_per_env(env, [&](auto per_env) {
        hipLaunchKernelGGL(k_mpc_plan<decltype(per_env)::value>, dim3(env->n), dim3(BLOCK), lds, stream, env->kp, env->n, env->b, m,
                           plan, mu_out, live, returns_out);
    }));
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
    TT_RUN(env, by_per_env(env, [&](auto per_env) {
        hipLaunchKernelGGL(k_mpc_act_ring<decltype(per_env)::value>, dim3(lanes), dim3(BLOCK), lds, stream, env->kp, (int)lanes, env->b, m,
                           plan, r);
    }));
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
    TT_RUN(env, by_per_env(env, [&](auto per_env) {
        hipLaunchKernelGGL(k_mpc_label_ring<decltype(per_env)::value>, dim3(lanes), dim3(BLOCK), lds, stream, env->kp, lanes, env->b, m,
                           plan, r);
    }));
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
        if (env->rnd_dev)
            return fail_both(env, TT_EINVAL, "%s: a curriculum with episode randomisation is not supported (the two have step kernels "
                                             "of their own, and the cells would be counted under a moving goal); "
                                             "tt_env_set_randomization(env, NULL, ...) first", who);
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
    TT_LAUNCH(env, hipLaunchKernelGGL(k_curriculum_update, dim3(1), dim3(BLOCK), 0, stream, (const CurDev *)blk));
    TT_HIP(env, hipStreamSynchronize(stream));      // `d` and `half` are temporaries
    env->cur_dev = static_cast<CurDev *>(blk);
    return TT_OK;
}

int tt_env_curriculum_update(tt_env *env, tt_stream_t stream) {
    TT_HANDLE(env);
    if (!env->cur_dev) return fail_both(env, TT_EINVAL, "tt_env_curriculum_update: the curriculum is off (tt_env_set_curriculum)");
    TT_RUN(env, hipLaunchKernelGGL(k_curriculum_update, dim3(1), dim3(BLOCK), 0, stream, (const CurDev *)env->cur_dev));
}

// tt_env_curriculum_read (to_caller) and tt_env_curriculum_write: device-to-device copies of the arrays the caller names
// (task: the task curriculum's arrays, tt_env_task_curriculum_read / _write)
static int curriculum_copy(tt_env *env, const tt_curriculum_arrays *a, bool to_caller, hipStream_t stream, const char *who,
                           bool task = false) {
    if (!env) return tthost::fail(TT_EINVAL, "%s: NULL handle", who);
    if (!a) return tthost::fail(TT_EINVAL, "%s: NULL argument", who);
    if (task && !env->task_dev) return fail_both(env, TT_EINVAL, "%s: the task curriculum is off (tt_env_set_task_curriculum)", who);
    if (!task && !env->cur_dev) return fail_both(env, TT_EINVAL, "%s: the curriculum is off (tt_env_set_curriculum)", who);
    TT_HIP(env, hipSetDevice(env->device));
    const CurDev &d = task ? env->task.cur : env->cur;
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

// ---- episode randomisation (include/ttenv.h: tt_env_set_randomization)
int tt_env_set_randomization(tt_env *env, const tt_randomization *cfg, tt_stream_t stream) {
    const char *const who = "tt_env_set_randomization";
    TT_HANDLE(env);
    if (cfg) {      // (before the handle is read: these hold for any handle)
        static const char *const axis[3] = {"x", "y", "yaw"};
        for (int d = 0; d < 3; ++d) {
            if (!std::isfinite(cfg->goal_lo[d]) || !std::isfinite(cfg->goal_hi[d]))
                return tthost::fail(TT_EINVAL, "%s: the goal %s range has a bound that is not finite", who, axis[d]);
            if (cfg->goal_lo[d] > cfg->goal_hi[d])
                return tthost::fail(TT_EINVAL, "%s: the goal %s range has lo = %g > hi = %g", who, axis[d], cfg->goal_lo[d], cfg->goal_hi[d]);
        }
        if (!std::isfinite(cfg->L2_lo) || !std::isfinite(cfg->L2_hi))
            return tthost::fail(TT_EINVAL, "%s: the L2 range has a bound that is not finite", who);
        if (cfg->L2_lo > cfg->L2_hi) return tthost::fail(TT_EINVAL, "%s: the L2 range has lo = %g > hi = %g", who, cfg->L2_lo, cfg->L2_hi);
        if (!(cfg->L2_lo > 0.0)) return tthost::fail(TT_EINVAL, "%s: L2_lo = %g is not > 0", who, cfg->L2_lo);
        const tt_params &p = env->params;
        if (cfg->goal_lo[0] < p.map_min_x || cfg->goal_hi[0] > p.map_max_x || cfg->goal_lo[1] < p.map_min_y || cfg->goal_hi[1] > p.map_max_y)
            return fail_both(env, TT_EINVAL, "%s: the goal range x [%g, %g], y [%g, %g] leaves the map x [%g, %g], y [%g, %g]", who,
                             cfg->goal_lo[0], cfg->goal_hi[0], cfg->goal_lo[1], cfg->goal_hi[1], p.map_min_x, p.map_max_x, p.map_min_y,
                             p.map_max_y);
        const double turn = std::fabs(p.dt * p.v1x) / cfg->L2_lo;      // (tt_env_create's test, for the shortest trailer)
        if (!(turn <= 0.25))
            return fail_both(env, TT_EINVAL, "%s: with L2_lo = %g, dt*|v|/L2 = %.3f rad per step exceeds the 0.25 rad the integrator's "
                                             "small-angle stage rotations are sized for", who, cfg->L2_lo, turn);
        if (env->cur_dev)
            return fail_both(env, TT_EINVAL, "%s: episode randomisation with a curriculum is not supported (the two have step kernels "
                                             "of their own, and the cells would be counted under a moving goal); "
                                             "tt_env_set_curriculum(env, NULL, ...) first", who);
        if (env->log_flags & TT_LOG_DETAIL)
            return fail_both(env, TT_EINVAL, "%s: episode randomisation with the detailed episode log is not supported (the randomised "
                                             "step kernels carry the plain log only)", who);
    }
    if (env->task_dev)          // (its cells lie on these ranges)
        return fail_both(env, TT_EINVAL, "%s: turn the task curriculum off first (tt_env_set_task_curriculum(env, NULL, ...))", who);
    TT_HIP(env, hipSetDevice(env->device));
    if (env->rnd_dev) {         // launches in flight may still read the old descriptor
        TT_HIP(env, hipStreamSynchronize(stream));
        TT_HIP(env, hipDeviceSynchronize());
        TT_HIP(env, hipFree(env->rnd_dev));
        env->rnd_dev = nullptr;
        env->rnd = tt_randomization{};
    }
    if (!cfg) return TT_OK;
    void *blk = nullptr;
    hipError_t err = hipMalloc(&blk, sizeof(RndDev));
    if (err != hipSuccess) return fail(env, err == hipErrorOutOfMemory ? TT_ENOMEM : TT_EHIP, "%s: %s", who, hipGetErrorString(err));
    RndDev d{};
    for (int k = 0; k < 3; ++k) {
        d.glo[k] = cfg->goal_lo[k];
        d.gw[k] = cfg->goal_hi[k] - cfg->goal_lo[k];
    }
    d.l2lo = cfg->L2_lo;
    d.l2w = cfg->L2_hi - cfg->L2_lo;
    d.seed = env->seed;
    for (int k = 0; k < 3; ++k) { d.rlo[k] = env->kp.rlo[k]; d.rhi[k] = env->kp.rhi[k]; }
    d.pool = env->kp.pool;
    d.pool_m = env->kp.pool_m;
    err = hipMemcpyAsync(blk, &d, sizeof(d), hipMemcpyHostToDevice, stream);
    if (err == hipSuccess) err = hipStreamSynchronize(stream);      // `d` is a temporary
    if (err != hipSuccess) {
        (void)hipFree(blk);
        return fail(env, TT_EHIP, "%s: %s", who, hipGetErrorString(err));
    }
    env->rnd_dev = static_cast<RndDev *>(blk);
    env->rnd = *cfg;
    env->per_env = true;
    return TT_OK;
}

int tt_env_randomization(const tt_env *env, tt_randomization *out) {
    TT_HANDLE(env);
    if (!env->rnd_dev) return 0;
    if (out) *out = env->rnd;
    return 1;
}

// ---- task curriculum (include/ttenv.h: tt_env_set_task_curriculum)
int tt_env_set_task_curriculum(tt_env *env, const tt_task_curriculum *cfg, const tt_curriculum_arrays *place, tt_stream_t stream) {
    const char *const who = "tt_env_set_task_curriculum";
    TT_HANDLE(env);
    long long C = 1;
    if (cfg) {      // (before the handle is read: these hold for any handle)
        const int *const n = cfg->bins;
        for (int k = 0; k < 4; ++k) {
            if (n[k] < 1) return tthost::fail(TT_EINVAL, "%s: bins (%d, %d, %d, %d): a bin count below 1", who, n[0], n[1], n[2], n[3]);
            C = std::min<long long>(C * n[k], (long long)TT_CURRICULUM_MAX_CELLS + 1);      // (no overflow)
        }
        if (C > TT_CURRICULUM_MAX_CELLS)
            return tthost::fail(TT_EINVAL, "%s: bins (%d, %d, %d, %d) make more than %d cells", who, n[0], n[1], n[2], n[3],
                                TT_CURRICULUM_MAX_CELLS);
        if (cfg->mode != TT_CURRICULUM_FRONTIER && cfg->mode != TT_CURRICULUM_HARD)
            return tthost::fail(TT_EINVAL, "%s: unknown mode %d", who, cfg->mode);
        if (!(cfg->alpha > 0.0 && cfg->alpha <= 1.0)) return tthost::fail(TT_EINVAL, "%s: alpha is outside (0, 1]", who);
        if (!std::isfinite(cfg->uniform) || !(cfg->uniform >= 0.0 && cfg->uniform <= 1.0))
            return tthost::fail(TT_EINVAL, "%s: uniform is outside [0, 1] or not finite", who);
        if (place && (!place->p || !place->seen || !place->attempts || !place->successes || !place->q || !place->cum || !place->cell))
            return tthost::fail(TT_EINVAL, "%s: place names every array or is NULL", who);
        if (!env->rnd_dev)
            return fail_both(env, TT_EINVAL, "%s: episode randomisation is not on: there is no range to put cells on "
                                             "(tt_env_set_randomization first)", who);
        static const char *const axis[4] = {"goal x", "goal y", "goal yaw", "L2"};
        const double lo[4] = {env->rnd.goal_lo[0], env->rnd.goal_lo[1], env->rnd.goal_lo[2], env->rnd.L2_lo};
        const double hi[4] = {env->rnd.goal_hi[0], env->rnd.goal_hi[1], env->rnd.goal_hi[2], env->rnd.L2_hi};
        for (int k = 0; k < 4; ++k)
            if (n[k] > 1 && !(hi[k] - lo[k] > 0.0))
                return fail_both(env, TT_EINVAL, "%s: %d bins on the %s range, which has width 0 (its cells could not be told apart)", who,
                                 n[k], axis[k]);
    }
    TT_HIP(env, hipSetDevice(env->device));
    if (env->task_block) {      // launches in flight may still read and write the old block
        TT_HIP(env, hipStreamSynchronize(stream));
        TT_HIP(env, hipDeviceSynchronize());
        TT_HIP(env, hipFree(env->task_block));
        env->task_block = nullptr;
        env->task_dev = nullptr;
        env->task = TaskDev{};
        env->task_cfg = tt_task_curriculum{};
    }
    if (!cfg) return TT_OK;
    const size_t c = (size_t)C, npad = (size_t)env->npad;
    // the block: the descriptor, then (without `place`) p | seen | attempts | successes | q | cum | cell, each 256-byte aligned
    const size_t sizes[7] = {sizeof(double) * c, sizeof(unsigned long long) * c, sizeof(uint32_t) * c, sizeof(uint32_t) * c,
                             sizeof(uint32_t) * c, sizeof(uint32_t) * c, sizeof(uint32_t) * npad};
    size_t bytes = cur_align(sizeof(TaskDev));
    size_t off[7];
    for (int a = 0; a < 7; ++a) {
        off[a] = bytes;
        if (!place) bytes += cur_align(sizes[a]);
    }
    void *blk = nullptr;
    hipError_t err = hipMalloc(&blk, bytes);
    if (err != hipSuccess) return fail(env, err == hipErrorOutOfMemory ? TT_ENOMEM : TT_EHIP, "%s: %s", who, hipGetErrorString(err));
    char *base = static_cast<char *>(blk);
    TaskDev d{};
    if (place) {
        d.cur.p = place->p; d.cur.seen = reinterpret_cast<unsigned long long *>(place->seen);
        d.cur.attempts = place->attempts; d.cur.successes = place->successes; d.cur.q = place->q; d.cur.cum = place->cum;
        d.cur.cell = place->cell;
    } else {
        d.cur.p = reinterpret_cast<double *>(base + off[0]);
        d.cur.seen = reinterpret_cast<unsigned long long *>(base + off[1]);
        d.cur.attempts = reinterpret_cast<uint32_t *>(base + off[2]);
        d.cur.successes = reinterpret_cast<uint32_t *>(base + off[3]);
        d.cur.q = reinterpret_cast<uint32_t *>(base + off[4]);
        d.cur.cum = reinterpret_cast<uint32_t *>(base + off[5]);
        d.cur.cell = reinterpret_cast<uint32_t *>(base + off[6]);
    }
    d.cur.C = (int)C;
    d.cur.mode = cfg->mode;
    d.cur.alpha = cfg->alpha; d.cur.uniform = cfg->uniform;
    d.cur.seed = env->seed;
    // the RndDev as tt_env_set_randomization forms it, and the cell widths
    const tt_randomization &r = env->rnd;
    for (int k = 0; k < 3; ++k) {
        d.rnd.glo[k] = r.goal_lo[k];
        d.rnd.gw[k] = r.goal_hi[k] - r.goal_lo[k];
        d.cw[k] = (r.goal_hi[k] - r.goal_lo[k]) / (double)cfg->bins[k];
        d.rnd.rlo[k] = env->kp.rlo[k]; d.rnd.rhi[k] = env->kp.rhi[k];
    }
    d.rnd.l2lo = r.L2_lo;
    d.rnd.l2w = r.L2_hi - r.L2_lo;
    d.cw[3] = (r.L2_hi - r.L2_lo) / (double)cfg->bins[3];
    d.rnd.seed = env->seed;
    d.rnd.pool = env->kp.pool;
    d.rnd.pool_m = env->kp.pool_m;
    for (int k = 0; k < 4; ++k) d.bins[k] = cfg->bins[k];
    env->task_block = blk;
    env->task = d;
    // fresh, as tt_env_set_curriculum starts: p = 0.5 everywhere, nothing seen or counted, no lane's episode drawn by it; q and cum
    // by the update itself
    const std::vector<double> half(c, 0.5);
    TT_HIP(env, hipMemcpyAsync(blk, &d, sizeof(d), hipMemcpyHostToDevice, stream));
    TT_HIP(env, hipMemcpyAsync(d.cur.p, half.data(), sizes[0], hipMemcpyHostToDevice, stream));
    TT_HIP(env, hipMemsetAsync(d.cur.seen, 0, sizes[1], stream));
    TT_HIP(env, hipMemsetAsync(d.cur.attempts, 0, sizes[2], stream));
    TT_HIP(env, hipMemsetAsync(d.cur.successes, 0, sizes[3], stream));
    TT_HIP(env, hipMemsetAsync(d.cur.cell, 0xFF, sizes[6], stream));
    TT_LAUNCH(env, hipLaunchKernelGGL(k_curriculum_update, dim3(1), dim3(BLOCK), 0, stream, (const CurDev *)blk));
    TT_HIP(env, hipStreamSynchronize(stream));      // `d` and `half` are temporaries
    env->task_dev = static_cast<TaskDev *>(blk);
    env->task_cfg = *cfg;
    return TT_OK;
}

int tt_env_task_curriculum_update(tt_env *env, tt_stream_t stream) {
    TT_HANDLE(env);
    if (!env->task_dev)
        return fail_both(env, TT_EINVAL, "tt_env_task_curriculum_update: the task curriculum is off (tt_env_set_task_curriculum)");
    // the curriculum's update on the descriptor's leading CurDev: it reads C, the arrays, mode, alpha and uniform only
    TT_RUN(env, hipLaunchKernelGGL(k_curriculum_update, dim3(1), dim3(BLOCK), 0, stream, (const CurDev *)&env->task_dev->cur));
}

int tt_env_task_curriculum_read(tt_env *env, const tt_curriculum_arrays *out, tt_stream_t stream) {
    return curriculum_copy(env, out, true, stream, "tt_env_task_curriculum_read", true);
}

int tt_env_task_curriculum_write(tt_env *env, const tt_curriculum_arrays *in, tt_stream_t stream) {
    return curriculum_copy(env, in, false, stream, "tt_env_task_curriculum_write", true);
}

int tt_env_task_curriculum(const tt_env *env, tt_task_curriculum *out) {
    TT_HANDLE(env);
    if (!env->task_dev) return 0;
    if (out) *out = env->task_cfg;
    return 1;
}

}  // extern "C"

namespace {

// the refusals and the two launches of a harvest (include/ttenv.h: tt_ring_harvest); `env` (may be NULL: the current device) takes
// the message, and its device is made current behind the refusals
int ring_harvest(tt_env *env, const char *who, const tt_harvest *h, const tt_ring_view *ring, const int64_t *k_dev,
                 const HarvestRecs &rc, hipStream_t stream) {
    if (!h || !ring || !k_dev) return fail_both(env, TT_EINVAL, "%s: h, ring and k_dev are required", who);
    if (!h->state || !h->obs || !h->act || !h->rew || !h->obs2 || !h->done || !h->work)
        return fail_both(env, TT_EINVAL, "%s: a NULL pointer in tt_harvest (state, obs, act, rew, obs2, done and work are required)", who);
    if (!ring->obs || !ring->act || !ring->rew || !ring->done)
        return fail_both(env, TT_EINVAL, "%s: a NULL pointer in the ring view (obs, act, rew and done are required)", who);
    if (!rc.lane || !rc.end_step || !rc.len || !rc.success || !rc.written)
        return fail_both(env, TT_EINVAL, "%s: a NULL record column (lane, end_step, len, success and written_dev are required)", who);
    if (h->capacity < 1 || h->tail < 0)
        return fail_both(env, TT_EINVAL, "%s: capacity = %d is below 1 or tail = %d is negative", who, h->capacity, h->tail);
    if (rc.capacity < 1) return fail_both(env, TT_EINVAL, "%s: record_capacity = %lld is below 1", who, rc.capacity);
    if (ring->slots < 3 || ring->n_envs < 1)
        return fail_both(env, TT_EINVAL, "%s: a ring of %d slots and %d envs (slots >= 3 and n_envs >= 1 are required)", who, ring->slots,
                         ring->n_envs);
    if (rc.capacity * (long long)(ring->slots - 1) > 2147483647ll)
        return fail_both(env, TT_EINVAL, "%s: record_capacity = %lld with %d slots: work[] holds 32-bit row counts", who, rc.capacity,
                         ring->slots);
    const HarvestK k{reinterpret_cast<long long *>(h->state), h->obs, h->act, h->rew, h->obs2, h->done, h->capacity, h->tail,
                     (long long)h->step_base, h->work, ring->obs, ring->act, ring->rew, ring->done, ring->n_envs, ring->slots,
                     reinterpret_cast<const long long *>(k_dev)};
    const long long groups = (rc.capacity + BLOCK - 1) / BLOCK;
    if (env) TT_HIP(env, hipSetDevice(env->device));
    TT_LAUNCH(env, hipLaunchKernelGGL(k_harvest_plan, dim3((unsigned)groups), dim3(BLOCK), 0, stream, k, rc));
    TT_LAUNCH(env, hipLaunchKernelGGL(k_harvest_copy, dim3((unsigned)(groups < 4096 ? groups : 4096)), dim3(BLOCK), 0, stream, k, rc));
    return TT_OK;
}

}  // namespace

extern "C" {

int tt_ring_harvest(const tt_harvest *h, const tt_ring_view *ring, const int64_t *k_dev, const int32_t *lane, const int64_t *end_step,
                    const int32_t *len, const uint8_t *success, const uint64_t *written_dev, int64_t record_capacity,
                    tt_stream_t stream) {
    const HarvestRecs rc{lane, reinterpret_cast<const long long *>(end_step), len, success,
                         reinterpret_cast<const unsigned long long *>(written_dev), (long long)record_capacity};
    return ring_harvest(nullptr, "tt_ring_harvest", h, ring, k_dev, rc, stream);
}

int tt_env_harvest(tt_env *env, const tt_harvest *h, const tt_ring_view *ring, const int64_t *k_dev, tt_stream_t stream) {
    TT_HANDLE(env);
    if (!env->log_bytes) return fail_both(env, TT_EINVAL, "tt_env_harvest: the episode log is off (tt_env_set_episode_log)");
    if (ring && ring->n_envs != env->n)
        return fail_both(env, TT_EINVAL, "tt_env_harvest: the ring view has %d envs, this handle %d", ring->n_envs, env->n);
    const LogCols c = log_cols(env->log);
    const HarvestRecs rc{c.lane, c.end_step, c.len, c.success, env->log.hdr + LG_WRITTEN, (long long)env->log.capacity};
    return ring_harvest(env, "tt_env_harvest", h, ring, k_dev, rc, stream);
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
