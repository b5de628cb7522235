// ttenv_mpc.h -- the sampling MPC planner on the device: its constants (MpcK), its noise, the three places a decision goes (plan,
// expert lanes of a ring, labelled lanes of a ring) and the one planner body under the three kernels.
// Part of csrc/ttenv.hip's translation unit, inside its anonymous namespace.  Needs <type_traits>, ttenv_math.h, ttenv_state.h and
// ttenv_step.h before it.  Template kernels only: they are instantiated in the order the host entry points name them.
#pragma once

// ------------------------------------------------------------------------------------------
// Sampling MPC (MPPI; include/ttenv.h: tt_env_mpc_plan has the definition of a decision).
// ONE WORKGROUP PLANS FOR ONE LANE: thread `tid` rolls samples tid, tid + BLOCK, ... through step_env on a copy of the lane's env
// in registers; the env in memory is only read.  The weighted mean needs every u[s, t] again once the largest return is known:
// the noise is counter-based, so the second pass REGENERATES a sample's sequence (S * H Philox blocks, a log and a sincos each:
// a few per cent of the S * H env steps of the first pass) instead of keeping S * H values (256 KB at the limits).  `chunk`
// samples at a time go through an LDS tile [chunk][H | 1] (odd stride: conflict-free both ways), and thread t < H adds column t
// of the tile in sample order.
//
// step_env's three wave votes with a wave that holds different SAMPLES of one lane, some of which have left the horizon loop:
// a vote counts the active lanes only, and each of them only widens what the wave computes -- the quotient by a real division
// gives every lane the value its own test would (the two quotients truncate differently only where the lane itself votes), and
// the staged bonuses and the backward penalty are recomputed under each lane's own comparison inside the voted branch.
constexpr uint32_t MPC_NOISE_TAG = 0x4D50u;     // Philox domain of the MPC's exploration noise
constexpr int MPC_TILE_FLOATS = 12288;          // the second pass's LDS tile: 48 KB

struct MpcK {
    int H, S, chunk;
    float action_scale;
    double sigma, rho, sigma_c;     // sigma_c = sqrt(1 - rho^2) sigma
    double lambda, gamma, k_lat, k_yaw;
    uint64_t seed;
};

// z[s, t]: the recipe of the TD3 smoothing noise (csrc/tttd3.h) with log, sqrt and cos in f64; products only, so that both passes
// get the same bits however they are contracted
__device__ __forceinline__ double mpc_normal(const MpcK &m, uint32_t lane, uint32_t episode, uint32_t steps, int s, int t) {
    uint32_t r[4];
    philox4x32(lane, episode, steps | ((uint32_t)t << 12) | ((uint32_t)s << 18), MPC_NOISE_TAG, (uint32_t)m.seed,
               (uint32_t)(m.seed >> 32), r);
    const float u1 = ((float)(r[0] >> 8) + 0.5f) * (1.f / 16777216.f);
    const float u2 = ((float)(r[1] >> 8) + 0.5f) * (1.f / 16777216.f);
    double sn, cs;
    tt_sincos(kTable, (double)(6.28318530717958647692f * u2), sn, cs);
    return sqrt(-2.0 * log((double)u1)) * cs;
}

// u[s, t] from the AR(1) state `eps` (advanced here) and the plan's entry
__device__ __forceinline__ float mpc_sample(const MpcK &m, uint32_t lane, uint32_t episode, uint32_t steps, int s, int t, float plan_t,
                                            double &eps) {
    if (s > 0) {
        const double z = mpc_normal(m, lane, episode, steps, s, t);
        eps = t == 0 ? m.sigma * z : fma(m.rho, eps, m.sigma_c * z);
    }
    return (float)fmin(fmax((double)plan_t + eps, -1.0), 1.0);
}

// Where a decision of an EXPERT LANE goes (tt_env_mpc_act_ring): the running step's action row of a trajectory ring, found through
// the cursor as k_step finds its rows, and the loop's scaled-action buffer -- the two values the policy launch wrote for the lane.
struct MpcRing {
    const int *cursor;      // [0]: the running step's slot t (left by tt_actor_act_ring)
    float *act;             // the ring's action rows [slots, n_envs]
    float *act_scaled;      // [n_envs]
    int n_envs, slots;
    float high;
};
struct MpcNoRing {};
// Expert lanes [0, expert) as MpcRing, and LABELLED LANES [expert, n) behind them (tt_env_mpc_label_ring): the decision of a
// labelled lane goes to the ring's label row of the running step and nowhere else -- the lane executes what the policy wrote.
struct MpcLabel {
    const int *cursor;      // [0]: the running step's slot t (left by tt_actor_act_ring)
    float *act;             // the ring's action rows [slots, n_envs] (expert lanes only; unused with expert = 0)
    float *act_scaled;      // [n_envs] (expert lanes only)
    float *label;           // the ring's label rows [slots, n_envs]
    int n_envs, slots;
    float high;
    int expert;             // M: workgroup i < M stores as MpcRing, i >= M stores label[t][i]
};

// One planner, three launches: k_mpc_plan (RING = MpcNoRing: mu_out, live, returns_out), k_mpc_act_ring (RING = MpcRing: workgroup
// i < n plans for lane i of the first n lanes, and U'_0 goes to the ring) and k_mpc_label_ring (RING = MpcLabel: the same for lanes
// < ring.expert, U'_0 to the label row for the others).  Everything before the last store is the same text.
template <bool PER_ENV, class RING>
__device__ __forceinline__ void mpc_plan_body(const KParams P, const int n, const Bufs b, const MpcK m, float *plan, float *mu_out,
                                              const uint8_t *live, double *returns_out, const RING ring) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mpc_lds[];
    const int i = blockIdx.x, tid = threadIdx.x;
    if (i >= n || (live && !live[i])) return;       // uniform: a skipped lane keeps every output's bits
    const int H = m.H, S = m.S, HP = H | 1;
    double *G = reinterpret_cast<double *>(mpc_lds);            // [S] returns, then weights
    double *red = G + S;                                        // [BLOCK]
    float *pl = reinterpret_cast<float *>(red + BLOCK);         // [H] the plan as read
    float *tile = pl + ((H + 3) & ~3);                          // [chunk][HP]
    const KTable &T = kTable;

    const uint32_t pk0 = reinterpret_cast<const uint2 *>(hot_ptr(b.hot, i) + H_MISC * TILE)->y;
    const uint32_t steps0 = pk_steps(pk0), ep = b.episodes[i];
    if (tid < H) pl[tid] = steps0 == 0u ? 0.f : plan[(size_t)i * H + tid];
    __syncthreads();

    // ---- pass 1: the returns
    double gmax = -INFINITY;
    for (int s = tid; s < S; s += BLOCK) {
        Env e;
        load_env<PER_ENV>(P, b, i, e);
        double Gs = 0.0, disc = 1.0, eps = 0.0;
        bool open = true;
        float of[OBS];
        for (int t = 0; t < H; ++t) {
            const float u = mpc_sample(m, (uint32_t)i, ep, steps0, s, t, pl[t], eps);
            const float a = u * m.action_scale;
            StepOut o;
            step_env(P, e, a, of, o);
            Gs += disc * o.total;
            disc *= m.gamma;
            if (o.done) { open = false; break; }     // the sample's env stops here: pk's packed fields are not stepped past done
        }
        if (open) {
            const double lat = -(e.x2 - e.g.gx) * e.g.sg + (e.y2 - e.g.gy) * e.g.cg;
            const double dyaw = tt_wrap_pi(T, e.gyaw - e.psi2);
            Gs += disc * -(m.k_lat * (lat * lat) + m.k_yaw * (dyaw * dyaw));
        }
        G[s] = Gs;
        if (returns_out) returns_out[(size_t)i * S + s] = Gs;
        if (isfinite(Gs)) gmax = fmax(gmax, Gs);
    }
    red[tid] = gmax;
    __syncthreads();
    for (int d = BLOCK >> 1; d > 0; d >>= 1) {
        if (tid < d) red[tid] = fmax(red[tid], red[tid + d]);
        __syncthreads();
    }
    gmax = red[0];
    for (int s = tid; s < S; s += BLOCK) {
        const double g = G[s];
        G[s] = isfinite(g) ? tt_exp_neg(T, (g - gmax) / m.lambda) : 0.0;
    }

    // ---- pass 2: the weighted mean, in sample order
    double num = 0.0, den = 0.0;
    for (int s0 = 0; s0 < S; s0 += m.chunk) {
        const int ns = min(m.chunk, S - s0);
        __syncthreads();        // the weights are written (first round); the tile's readers are done (later rounds)
        if (tid < ns) {
            double eps = 0.0;
            for (int t = 0; t < H; ++t) tile[tid * HP + t] = mpc_sample(m, (uint32_t)i, ep, steps0, s0 + tid, t, pl[t], eps);
        }
        __syncthreads();
        if (tid < H)
            for (int q = 0; q < ns; ++q) {
                const double w = G[s0 + q];
                num = fma(w, (double)tile[q * HP + tid], num);
                den += w;
            }
    }
    if (tid < H) {
        const float un = den > 0.0 ? (float)(num / den) : pl[tid];     // no finite sample: the plan shifts unchanged
        float *row = plan + (size_t)i * H;
        if (tid == 0) {
            if constexpr (std::is_same<RING, MpcRing>::value) {
                // ring.act[t][i] = U'_0 (the normalised action: what collect_demonstrations stores) and the env step's input, one
                // f32 product; a cursor outside the ring (never written by a pack launch) stores nothing
                const int t = ring.cursor[0];
                if ((unsigned)t < (unsigned)ring.slots) ring.act[(size_t)t * ring.n_envs + i] = un;
                ring.act_scaled[i] = un * ring.high;
            } else if constexpr (std::is_same<RING, MpcLabel>::value) {
                // an expert lane: MpcRing's two stores; a labelled lane: label[t][i] = U'_0 alone (ring.act[t][i] and act_scaled[i]
                // keep the policy's bits).  i is the workgroup's lane: the branch is uniform
                const int t = ring.cursor[0];
                if (i < ring.expert) {
                    if ((unsigned)t < (unsigned)ring.slots) ring.act[(size_t)t * ring.n_envs + i] = un;
                    ring.act_scaled[i] = un * ring.high;
                } else if ((unsigned)t < (unsigned)ring.slots) {
                    ring.label[(size_t)t * ring.n_envs + i] = un;
                }
            } else {
                mu_out[i] = un;
            }
        } else {
            row[tid - 1] = un;
        }
        if (tid == H - 1) row[tid] = un;
    }
}

template <bool PER_ENV>
__global__ __launch_bounds__(BLOCK) void k_mpc_plan(const KParams P, const int n, const Bufs b, const MpcK m, float *plan,
                                                    float *mu_out, const uint8_t *live, double *returns_out) {
    mpc_plan_body<PER_ENV>(P, n, b, m, plan, mu_out, live, returns_out, MpcNoRing{});
}

// lanes [0, lanes) of the env: grid = lanes; plan is [lanes, H]
template <bool PER_ENV>
__global__ __launch_bounds__(BLOCK) void k_mpc_act_ring(const KParams P, const int lanes, const Bufs b, const MpcK m, float *plan,
                                                        const MpcRing ring) {
    mpc_plan_body<PER_ENV>(P, lanes, b, m, plan, nullptr, nullptr, nullptr, ring);
}

// lanes [0, lanes) of the env, lanes = expert + labelled: grid = lanes; plan is [lanes, H]
template <bool PER_ENV>
__global__ __launch_bounds__(BLOCK) void k_mpc_label_ring(const KParams P, const int lanes, const Bufs b, const MpcK m, float *plan,
                                                          const MpcLabel ring) {
    mpc_plan_body<PER_ENV>(P, lanes, b, m, plan, nullptr, nullptr, nullptr, ring);
}
