// tttd3.hip -- TD3 (Fujimoto et al., 2018) in the fused learner: twin critics, target-policy smoothing, delayed actor and target
// updates, in the launch shapes of one agent's learn() (MI355X, gfx950).
//
// One update u of a vector step, with t = the critic updates done before it:
//
//   k_td3_fwd_multi            five or six forwards in one launch, job-major as k_fwd_multi, on the launch's own replay draw (seed +
//                              u * seed_stride): target actor on s', the state branches of both target critics on s', Q1(s, a) and
//                              Q2(s, a) saved, and -- full updates only -- mu(s) saved.  Workgroup 0 leaves a snapshot of t.
//   k_td3_bwd_rows             [0, nb) critic 1, [nb, 2 nb) critic 2, full updates: [2 nb, 3 nb) the actor's unit backward; the last
//                              workgroup ticks the counters.  A critic workgroup first runs the TD3 prologue for its 16 rows --
//                              eps = clip(sigma N, -c, c) with N from Philox + Box-Muller keyed by (row, t, TD3_NOISE_TAG, noise seed),
//                              a' = clip(mu' + eps, -1, 1), both target heads on a', y = r + gamma min(q1', q2') (y = r where done)
//                              -- and then bwd_rows_body<true, true> with that y given.
//   k_td3_bwd_weights          2 x 210 workgroups, critic-major: each critic's weight gradients + Adam + fc2 image patches; on a
//                              critic-only update through the descriptor's tau = 0 variant, which leaves the target's bits alone:
//                              fmaf(0, p - t, t) is t for every finite p - t -- except that a target element -0.0 can become +0.0 (equal
//                              as a number; its image pieces change sign with it) and an overflowing p - t would make it NaN.
//   k_td3_actor_tail           full updates only: k_actor_tail through the UPDATED critic 1, the actor's Adam on its OWN step count
//                              (ticked by k_td3_bwd_rows on full updates only) and the actor's soft update.
//
// The bodies are those of ttlearn_bodies.h.  The per-agent arguments live in device memory (Td3Agent), filled once at
// tt_td3_create and read through the constant address space as ttpop.h's agent_of does: a launch takes (descriptor, u, full) and is
// graph-capturable.  With critic 2 a copy of critic 1, sigma = 0 and every update full, an update leaves the bits of the lone
// learn() with the tail in one grid (tests/test_gpu_td3.py).
#include "tthost.h"
#include "ttlearn_bodies.h"

#include <cmath>
#include <cstdio>

using tthost::fail;

namespace {

constexpr uint32_t TD3_NOISE_TAG = 0x7D3Eu;      // Philox domain of the target-smoothing noise (0x0A5E: OU noise, 0x5A3D: replay draws)

struct Td3Agent {
    int n;
    // k_td3_fwd_multi
    FwdJob j[6];
    ttnet::RingSample R;                 // R.seed: the key of update 0; update u adds u * R.seed_stride
    int write_s, write_s2;
    long long *step_dev, *step_snap;     // the critics' step count (= t before the tick) and this update's snapshot of it
    // k_td3_bwd_rows
    float scale_c;                       // 2 / B
    const float *q_out[2], *mu_out;      // Q1(s, a), Q2(s, a), mu(s) of the forwards
    Weights Wc[2], Wa;
    Saved sv_c[2], sv_a;
    BwdOut o_c[2], o_a;
    const float *z_state[2], *mu_t, *r;  // the TD3 prologue: both target critics' state branches on s', mu'(s'), the draw's r, done
    const uint8_t *done;
    const float *twa[2], *tba[2], *tw3[2], *tb3[2];      // the target critics' action branches and heads
    float gamma, sigma, clip;
    unsigned long long noise_seed;
    float *y_out[2], *qt_out[2], *eps_out;
    TdIn tick_c, tick_a;                 // clock_tick()'s fields only: {step_dev, bc_out, beta1, beta2} of the critics / the actor
    // k_td3_bwd_weights and the weight workgroups of k_td3_actor_tail
    const float *s, *a;
    Grads Gc[2], Ga;
    AdamFused Ac[2][2], Aa;              // Ac[c][0]: with tau (full updates), Ac[c][1]: tau = 0 (critic-only updates)
    RowScale RSa;
    float *q_pi, *dq_da;
    TailSync ts;                         // the tail's own words; its epoch is the ACTOR's step count
};

__device__ __forceinline__ const Td3Agent &td3_of(const Td3Agent *D) {
    return *(const Td3Agent *)((const __attribute__((address_space(4))) Td3Agent *)D);
}

// grid: (full ? 6 : 5) x nb, job-major as k_fwd_multi (the sampled prologue is k_pop_fwd_multi's)
__global__ __launch_bounds__(64 * NW) void k_td3_fwd_multi(const Td3Agent *__restrict__ D, const int u, const int full) {
    __shared__ __attribute__((aligned(16))) float h1_s[H1S_FLOATS];
    __shared__ __attribute__((aligned(16))) float z_s[TR * DS];
    __shared__ __attribute__((aligned(16))) float w1_s[H1 * IN];
    const Td3Agent &P = td3_of(D);
    const int n = P.n, nb = (n + TR - 1) / TR, job = (int)blockIdx.x / nb;
    if (job >= (full ? 6 : 5)) return;
    const int row0 = ((int)blockIdx.x - job * nb) * TR;
    if (blockIdx.x == 0 && threadIdx.x == 0) *P.step_snap = *P.step_dev;      // (the next launch ticks step_dev)
    const FwdJob &q = P.j[job];
    ttnet::RingSample R = P.R;
    R.seed += (unsigned long long)u * R.seed_stride;
    static_assert(TR / NW == 2, "two rows per wave");
    const int tid = threadIdx.x, wave = tid >> 6, l15 = tid & 15;
    const bool from_s = q.obs == R.s_out;
    const float *orow;
    {
        const ttnet::RingPick p = ttnet::ring_sample_index(R, min(row0 + l15, n - 1));
        orow = from_s ? ttnet::ring_pick_s(R, p) : ttnet::ring_pick_s2(R, p);
    }
    bool have_act = false;
    float act_r0 = 0.f, act_r1 = 0.f;
    if (q.critic && q.action) {
        act_r0 = ttnet::ring_pick_a(R, ttnet::ring_sample_index(R, min(row0 + wave * 2, n - 1)));
        act_r1 = ttnet::ring_pick_a(R, ttnet::ring_sample_index(R, min(row0 + wave * 2 + 1, n - 1)));
        have_act = true;
    }
    if (job == P.write_s || job == P.write_s2) {        // the batch rows of this workgroup for the later launches
        const int lr = tid / ttnet::IN, c = tid - lr * ttnet::IN, b = row0 + lr;
        if (lr < TR && b < n) {
            const ttnet::RingPick p = ttnet::ring_sample_index(R, b);
            if (job == P.write_s) {
                R.s_out[(size_t)b * ttnet::IN + c] = ttnet::ring_pick_s(R, p)[c];
                if (c == 0) {
                    R.a_out[b] = ttnet::ring_pick_a(R, p);
                    if (R.idx_out) { R.idx_out[2 * b] = p.side ? -1 : p.t; R.idx_out[2 * b + 1] = p.side ? p.j : p.e; }
                }
            }
            if (job == P.write_s2) {
                R.s2_out[(size_t)b * ttnet::IN + c] = ttnet::ring_pick_s2(R, p)[c];
                if (c == 0) { R.r_out[b] = ttnet::ring_pick_r(R, p); R.d_out[b] = ttnet::ring_pick_d(R, p); }
            }
        }
    }
    if (q.critic)
        fwd_small_body<true>(n, q.obs, q.action, q.W, q.out, q.sv, q.dq_da, q.z_state, h1_s, z_s, w1_s, row0, orow, have_act, act_r0, act_r1);
    else
        fwd_small_body<false>(n, q.obs, q.action, q.W, q.out, q.sv, nullptr, nullptr, h1_s, z_s, w1_s, row0, orow);
}

// The TD3 prologue for the two rows of this wave: y[rr] of row row0 + 2 wave + rr.  The two dot products have the fma order and the
// wave_sum64 of the TD prologue inside bwd_rows_body, so that with eps = 0 and equal critics y has the lone learn()'s bits.
// `c`: the critic this workgroup serves -- it leaves y_out[c]; critic 1's workgroups also leave q1', q2' and eps.
__device__ __forceinline__ void td3_prologue(const Td3Agent &P, const int c, const int row0, float (&y)[TR / NW]) {
    constexpr int RPW = TR / NW;
    const int n = P.n, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float4 wat[2][RV], bat[2][RV], w3t[2][RV], zt[2][RPW][RV];
    float b3t[2], mut[RPW], rt[RPW];
    bool dt[RPW];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
        for (int i = 0; i < RV; ++i) {
            const int col = rv_col(lane, i), cc = col < H2 ? col : 0;
            wat[k][i] = f4_ldu(P.twa[k] + cc); bat[k][i] = f4_ldu(P.tba[k] + cc); w3t[k][i] = f4_ldu(P.tw3[k] + cc);
        }
        b3t[k] = P.tb3[k][0];
    }
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
        const int rowc = min(row0 + wave * RPW + rr, n - 1);
        mut[rr] = P.mu_t[rowc]; rt[rr] = P.r[rowc]; dt[rr] = P.done[rowc] != 0;
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int i = 0; i < RV; ++i) {
                const int col = rv_col(lane, i);
                zt[k][rr][i] = f4_ldu(P.z_state[k] + (size_t)rowc * H2 + (col < H2 ? col : 0));
            }
    }
    const unsigned long long t = (unsigned long long)*P.step_snap;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int i = 0; i < RV; ++i)                           // the dot products run over every lane's columns: none beyond 299
            if (!(rv_col(lane, i) < H2)) w3t[k][i] = f4_zero();
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
        const int row = row0 + wave * RPW + rr;
        // N(0, 1) as ou_advance (csrc/ttnet_common.h) makes it, keyed by (row, t) in this noise's own Philox domain
        uint32_t rnd[4];
        ttrng::philox4x32((uint32_t)row, (uint32_t)t, (uint32_t)(t >> 32), TD3_NOISE_TAG, (uint32_t)P.noise_seed,
                          (uint32_t)(P.noise_seed >> 32), rnd);
        const float u1 = ((float)(rnd[0] >> 8) + 0.5f) * (1.f / 16777216.f);
        const float u2 = ((float)(rnd[1] >> 8) + 0.5f) * (1.f / 16777216.f);
        const float nrm = sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
        const float eps = fminf(fmaxf(P.sigma * nrm, -P.clip), P.clip);
        const float a2 = fminf(fmaxf(mut[rr] + eps, -1.f), 1.f);
        float qk[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            float dot = 0.f;
#pragma unroll
            for (int i = 0; i < RV; ++i) {
                dot = fmaf(fmaxf(zt[k][rr][i].x + fmaf(a2, wat[k][i].x, bat[k][i].x), 0.f), w3t[k][i].x, dot);
                dot = fmaf(fmaxf(zt[k][rr][i].y + fmaf(a2, wat[k][i].y, bat[k][i].y), 0.f), w3t[k][i].y, dot);
                dot = fmaf(fmaxf(zt[k][rr][i].z + fmaf(a2, wat[k][i].z, bat[k][i].z), 0.f), w3t[k][i].z, dot);
                dot = fmaf(fmaxf(zt[k][rr][i].w + fmaf(a2, wat[k][i].w, bat[k][i].w), 0.f), w3t[k][i].w, dot);
            }
            qk[k] = wave_sum64(dot) + b3t[k];
        }
        y[rr] = dt[rr] ? rt[rr] : fmaf(P.gamma, fminf(qk[0], qk[1]), rt[rr]);
        if (row < n && lane == 0) {
            P.y_out[c][row] = y[rr];
            if (c == 0) { P.qt_out[0][row] = qk[0]; P.qt_out[1][row] = qk[1]; P.eps_out[row] = eps; }
        }
    }
}

// grid: (full ? 3 : 2) x nb + 1: critic 1's rows, critic 2's rows, [the actor's unit rows,] the counter workgroup
__global__ __launch_bounds__(64 * NW) void k_td3_bwd_rows(const Td3Agent *__restrict__ D, const int u, const int full) {
    __shared__ __attribute__((aligned(16))) float dx2_s[DXS_FLOATS];
    __shared__ float red[2 * NW * TR];
    __shared__ float rsc_s[TR];
    const Td3Agent &P = td3_of(D);
    const int n = P.n, nb = (n + TR - 1) / TR, lb = (int)blockIdx.x, groups = full ? 3 : 2;
    if (lb >= groups * nb) {
        if (lb == groups * nb && threadIdx.x == 0) {
            clock_tick(P.tick_c);
            if (full) clock_tick(P.tick_a);
        }
        return;
    }
    if (lb < 2 * nb) {
        const int c = lb / nb, row0 = (lb - c * nb) * TR;
        float y[TR / NW];
        td3_prologue(P, c, row0, y);
        bwd_rows_body<true, true>(n, P.scale_c, P.q_out[c], P.Wc[c], P.sv_c[c], P.o_c[c], TdIn{}, dx2_s, red, rsc_s, row0, y);
    } else {
        bwd_rows_body<false>(n, 0.f, nullptr, P.Wa, P.sv_a, P.o_a, TdIn{}, dx2_s, red, rsc_s, (lb - 2 * nb) * TR);
    }
}

// grid: 2 x 210, critic-major: a critic's weight gradients with its optimizer step (k_pop_bwd_weights<false> per critic)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k_td3_bwd_weights(const Td3Agent *__restrict__ D, const int u,
                                                                                             const int full) {
    __shared__ __attribute__((aligned(16))) float part[4][4][256];
    __shared__ float f_s[1];
    __shared__ __attribute__((aligned(16))) _Float16 stage_s[4 * 1024];
    const int c = (int)blockIdx.x / WG_CRITIC_WEIGHTS;
    if (c >= 2) return;
    const Td3Agent &P = td3_of(D);
    bwd_weights_body<false, false>((int)blockIdx.x - c * WG_CRITIC_WEIGHTS, P.n, 1, P.s, P.a, P.sv_c[c], P.o_c[c], P.Gc[c],
                                   P.Ac[c][full ? 0 : 1], RowScale{nullptr, nullptr, 1.f}, part, f_s,
                                   TailSync{nullptr, nullptr, 0, nullptr}, 0, stage_s);
}

// grid: nb row workgroups first, then 200 weight workgroups (k_pop_actor_tail for one agent): Q1(s, mu(s)) and dQ/da through the
// updated critic 1, then the actor's weight gradients + Adam + soft update.  The epoch is the actor's own step count.
__global__ __launch_bounds__(64 * NW) void k_td3_actor_tail(const Td3Agent *__restrict__ D, const int u, const int full) {
    __shared__ __attribute__((aligned(16))) float lds[H1S_FLOATS + TR * DS + H1 * IN];
    const Td3Agent &P = td3_of(D);
    const int n = P.n, nb = (n + TR - 1) / TR;
    const long long epoch = *P.Aa.step_dev;
    if ((int)blockIdx.x < nb) {
        const int lb = (int)blockIdx.x;
        const Saved none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        fwd_small_body<true>(n, P.s, P.mu_out, P.Wc[0], P.q_pi, none, P.dq_da, nullptr, lds, lds + H1S_FLOATS,
                             lds + H1S_FLOATS + TR * DS, lb * TR, nullptr, false, 0.f, 0.f, P.ts.rows, (unsigned)epoch);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every wave: its rows' words have been sent
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(P.ts.hints + lb, (int)epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const int blk = (int)blockIdx.x - nb;
    if (threadIdx.x >= 256 || blk >= WG_ACTOR_WEIGHTS) return;
    float (&part)[4][4][256] = *reinterpret_cast<float (*)[4][4][256]>(lds);
    bwd_weights_body<true, true>(blk, n, 0, P.s, nullptr, P.sv_a, P.o_a, P.Ga, P.Aa, P.RSa, part, lds + 4 * 4 * 256, P.ts, epoch,
                                 reinterpret_cast<_Float16 *>(lds + 4 * 4 * 256 + MAXB));
}

bool finite_nonneg(const float x) { return std::isfinite(x) && x >= 0.f; }

// tt_td3_agent -> Td3Agent (host checks only: no HIP call)
int to_td3_agent(const tt_td3_agent &g, const int n, Td3Agent &P) {
    P = Td3Agent{};
    P.n = n;
    if (!finite_nonneg(g.target_noise)) return fail(TT_EINVAL, "tt_td3_create: target_noise = %g is negative or not finite", (double)g.target_noise);
    if (!finite_nonneg(g.noise_clip)) return fail(TT_EINVAL, "tt_td3_create: noise_clip = %g is negative or not finite", (double)g.noise_clip);
    const tt_sample_args *smp = g.sample;
    if (!smp) return fail(TT_EINVAL, "tt_td3_create: sample (tt_sample_args) is NULL");
    if (smp->batch != n) return fail(TT_EINVAL, "tt_td3_create: the sample draws batches of %d rows, not batch = %d", smp->batch, n);
    if (smp->step_progress || smp->draws > 1) return fail(TT_EINVAL, "tt_td3_create: step_progress / draws > 1 in the sample are not supported");
    if (smp->side && smp->side->count > 0) return fail(TT_EINVAL, "tt_td3_create: the sample has a side buffer (not supported)");
    if (ttnet::make_ring_sample(smp, P.R) != TT_OK) return fail(TT_EINVAL, "tt_td3_create: bad tt_sample_args");
    P.R.seed_stride = smp->seed_stride;
    const tt_fwd_job *jobs = g.jobs;
    if (!jobs) return fail(TT_EINVAL, "tt_td3_create: jobs is NULL");
    // the six forwards, in their order: target actor on s', both target critics' state branches on s', Q1(s, a), Q2(s, a), mu(s)
    bool shape = !jobs[0].critic && jobs[0].obs == smp->s2_out && !jobs[5].critic && jobs[5].obs == smp->s_out && jobs[5].saved;
    for (int i = 1; i <= 2; ++i) shape = shape && jobs[i].critic && jobs[i].obs == smp->s2_out && jobs[i].z_state;
    for (int i = 3; i <= 4; ++i) shape = shape && jobs[i].critic && jobs[i].obs == smp->s_out && jobs[i].action == smp->a_out && jobs[i].saved;
    if (!shape) return fail(TT_EINVAL, "tt_td3_create: the jobs are not TD3's six forwards on the draw");
    P.write_s = P.write_s2 = -1;
    for (int i = 0; i < 6; ++i) {
        FwdJobs one{};
        one.write_s = one.write_s2 = 0;
        if (!to_fwd_job(jobs[i], 0, smp, one))
            return fail(TT_EINVAL, "tt_td3_create: forward job %d is incomplete or has an action other than the draw's a on s", i);
        P.j[i] = one.j[0];
        if (jobs[i].obs == smp->s_out && P.write_s < 0) P.write_s = i;
        if (jobs[i].obs == smp->s2_out && P.write_s2 < 0) P.write_s2 = i;
    }
    if (!jobs[0].out || !jobs[3].out || !jobs[4].out || !jobs[5].out)
        return fail(TT_EINVAL, "tt_td3_create: mu'(s'), Q1(s, a), Q2(s, a) and mu(s) need outputs");
    P.scale_c = (float)(2.0 / n);
    P.q_out[0] = jobs[3].out; P.q_out[1] = jobs[4].out; P.mu_out = jobs[5].out;
    P.Wc[0] = P.j[3].W; P.Wc[1] = P.j[4].W; P.Wa = P.j[5].W;
    P.sv_c[0] = P.j[3].sv; P.sv_c[1] = P.j[4].sv; P.sv_a = P.j[5].sv;
    const tt_td_input *tdi = g.td;
    TdIn td{};
    if (!to_td(tdi, td) || !tdi->step_dev || !tdi->q_out || !tdi->bias_corr_out)
        return fail(TT_EINVAL, "tt_td3_create: bad tt_td_input (arrays, q_out, a step counter and bias_corr_out are required)");
    if (tdi->window_dev) return fail(TT_EINVAL, "tt_td3_create: window_dev is set (the pipelined order is not supported)");
    if (!g.z_state_2 || !ok_shape(g.target_critic_2, true)) return fail(TT_EINVAL, "tt_td3_create: z_state_2 or target_critic_2 is missing");
    if (!g.eps_out || !g.y2_out || !g.q2t_out) return fail(TT_EINVAL, "tt_td3_create: eps_out, y2_out and q2t_out are required");
    if (!g.step_snapshot || !g.actor_step_dev || !g.actor_bias_corr_out)
        return fail(TT_EINVAL, "tt_td3_create: step_snapshot, actor_step_dev and actor_bias_corr_out are required");
    if (!g.q_pi || !g.dq_da || !g.tail_words) return fail(TT_EINVAL, "tt_td3_create: q_pi, dq_da and tail_words are required");
    // the parts of the description belong together: the prologue reads what the forwards and the draw of the SAME update leave
    if (tdi->z_state != jobs[1].z_state || g.z_state_2 != jobs[2].z_state)
        return fail(TT_EINVAL, "tt_td3_create: td->z_state / z_state_2 are not the z_state outputs of forward jobs 1 and 2");
    if (tdi->mu_target != jobs[0].out) return fail(TT_EINVAL, "tt_td3_create: td->mu_target is not the output of forward job 0 (the target actor)");
    if (tdi->reward != smp->r_out || tdi->done != smp->d_out)
        return fail(TT_EINVAL, "tt_td3_create: td->reward / td->done are not the draw's r_out / d_out");
    if (tdi->target_critic != jobs[1].w || g.target_critic_2 != jobs[2].w)
        return fail(TT_EINVAL, "tt_td3_create: td->target_critic / target_critic_2 are not the networks of forward jobs 1 and 2");
    const tt_mlp_weights &t2 = *g.target_critic_2;
    P.step_dev = td.step_dev;
    P.step_snap = reinterpret_cast<long long *>(g.step_snapshot);
    P.z_state[0] = td.z_state; P.z_state[1] = g.z_state_2;
    P.mu_t = td.mu_t; P.r = td.r; P.done = td.done;
    P.twa[0] = td.wa; P.tba[0] = td.ba; P.tw3[0] = td.w3; P.tb3[0] = td.b3;
    P.twa[1] = t2.wa; P.tba[1] = t2.ba; P.tw3[1] = t2.w3; P.tb3[1] = t2.b3;
    P.gamma = td.gamma; P.sigma = g.target_noise; P.clip = g.noise_clip; P.noise_seed = g.noise_seed;
    P.y_out[0] = td.y_out; P.y_out[1] = g.y2_out; P.qt_out[0] = td.q_out; P.qt_out[1] = g.q2t_out; P.eps_out = g.eps_out;
    P.tick_c = TdIn{};
    P.tick_c.step_dev = td.step_dev; P.tick_c.bc_out = td.bc_out; P.tick_c.beta1 = td.beta1; P.tick_c.beta2 = td.beta2;
    P.tick_a = TdIn{};
    P.tick_a.step_dev = reinterpret_cast<long long *>(g.actor_step_dev); P.tick_a.bc_out = g.actor_bias_corr_out;
    P.tick_a.beta1 = g.actor.beta1; P.tick_a.beta2 = g.actor.beta2;
    P.s = smp->s_out; P.a = smp->a_out;
    if (!to_bwd_out(g.critic.ws, P.o_c[0]) || !to_bwd_out(g.critic_2.ws, P.o_c[1]) || !to_bwd_out(g.actor.ws, P.o_a))
        return fail(TT_EINVAL, "tt_td3_create: a per-row workspace (tt_mlp_bwd_ws) is incomplete");
    if (P.o_c[0].dx2 == P.o_c[1].dx2 || P.o_c[0].dx2 == P.o_a.dx2 || P.o_c[1].dx2 == P.o_a.dx2)
        return fail(TT_EINVAL, "tt_td3_create: two networks share a per-row workspace");
    for (int net = 0; net < 3; ++net) {
        const tt_pop_net &t = net == 0 ? g.critic : net == 1 ? g.critic_2 : g.actor;
        const bool critic = net < 2;
        if (!ok_shape(t.grads, critic)) return fail(TT_EINVAL, "tt_td3_create: network %d has no gradient buffers", net);
        if (critic) {
            for (int v = 0; v < 2; ++v)
                if (!to_adam(true, t.count, t.params, t.exp_avg, t.exp_avg_sq, t.targets, tdi->step_dev, t.lr, t.beta1, t.beta2, t.eps,
                             t.weight_decay, v == 0 ? t.tau : 0.f, t.images, tdi->bias_corr_out, P.Ac[net][v]))
                    return fail(TT_EINVAL, "tt_td3_create: network %d has an incomplete optimizer step", net);
            P.Gc[net] = to_grads(t.grads);
        } else {
            if (!to_adam(false, t.count, t.params, t.exp_avg, t.exp_avg_sq, t.targets, g.actor_step_dev, t.lr, t.beta1, t.beta2, t.eps,
                         t.weight_decay, t.tau, t.images, g.actor_bias_corr_out, P.Aa))
                return fail(TT_EINVAL, "tt_td3_create: network %d has an incomplete optimizer step", net);
            P.Ga = to_grads(t.grads);
        }
    }
    if (g.critic.grads->w1 == g.critic_2.grads->w1) return fail(TT_EINVAL, "tt_td3_create: the two critics share a gradient buffer");
    P.q_pi = g.q_pi;
    P.dq_da = g.dq_da;
    P.RSa = RowScale{g.dq_da, P.mu_out, (float)(-1.0 / n)};
    P.ts = TailSync{g.tail_words, reinterpret_cast<unsigned long long *>(g.tail_words + 64), (n + TR - 1) / TR, g.gave_up_host};
    return TT_OK;
}

}  // namespace

struct tt_td3 {
    int n = 0;
    Td3Agent *dev = nullptr;
};

extern "C" {

int tt_td3_create(int batch, const tt_td3_agent *agent, tt_td3 **out) {
    if (!out) return fail(TT_EINVAL, "tt_td3_create: out is NULL");
    *out = nullptr;
    if (batch < 1 || batch > MAXB) return fail(TT_EINVAL, "tt_td3_create: batch = %d rows, not in [1, %d]", batch, MAXB);
    if (!agent) return fail(TT_EINVAL, "tt_td3_create: agent is NULL");
    Td3Agent host;
    const int rc = to_td3_agent(*agent, batch, host);
    if (rc != TT_OK) return rc;
    Td3Agent *dev = nullptr;
    if (hipMalloc(&dev, sizeof(Td3Agent)) != hipSuccess) return fail(TT_ENOMEM, "tt_td3_create: hipMalloc");
    if (hipMemcpy(dev, &host, sizeof(Td3Agent), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(dev);
        return fail(TT_EHIP, "tt_td3_create: hipMemcpy");
    }
    *out = new tt_td3{batch, dev};
    return TT_OK;
}

int tt_td3_update(tt_td3 *h, const tt_td3_agent *agent) {
    if (!h) return fail(TT_EINVAL, "tt_td3_update: handle is NULL");
    if (!agent) return fail(TT_EINVAL, "tt_td3_update: agent is NULL");
    Td3Agent host;
    const int rc = to_td3_agent(*agent, h->n, host);
    if (rc != TT_OK) return rc;
    if (hipDeviceSynchronize() != hipSuccess) return fail(TT_EHIP, "tt_td3_update: hipDeviceSynchronize");
    if (hipMemcpy(h->dev, &host, sizeof(Td3Agent), hipMemcpyHostToDevice) != hipSuccess) return fail(TT_EHIP, "tt_td3_update: hipMemcpy");
    return TT_OK;
}

int tt_td3_learn(tt_td3 *h, int update, int full, tt_stream_t stream) {
    if (!h) return fail(TT_EINVAL, "tt_td3_learn: handle is NULL");
    if (update < 0) return fail(TT_EINVAL, "tt_td3_learn: update = %d < 0", update);
    const int nb = (h->n + TR - 1) / TR, f = full ? 1 : 0;
    hipLaunchKernelGGL(k_td3_fwd_multi, dim3((f ? 6 : 5) * nb), dim3(64 * NW), 0, stream, h->dev, update, f);
    hipLaunchKernelGGL(k_td3_bwd_rows, dim3((f ? 3 : 2) * nb + 1), dim3(64 * NW), 0, stream, h->dev, update, f);
    hipLaunchKernelGGL(k_td3_bwd_weights, dim3(2 * WG_CRITIC_WEIGHTS), dim3(256), 0, stream, h->dev, update, f);
    if (f) hipLaunchKernelGGL(k_td3_actor_tail, dim3(nb + WG_ACTOR_WEIGHTS), dim3(64 * NW), 0, stream, h->dev, update, f);
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

int tt_td3_destroy(tt_td3 *h) {
    if (!h) return TT_OK;
    const hipError_t e = hipFree(h->dev);
    delete h;
    return e == hipSuccess ? TT_OK : TT_EHIP;
}

}  // extern "C"
