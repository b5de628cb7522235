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
#include "tttd3.h"

namespace {

// grid: (full ? 6 : 5) x nb, job-major as k_fwd_multi (the sampled prologue is TT_SAMPLED_ROWS of csrc/ttlearn_sites.h)
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
    const float *orow;
    bool have_act = false;
    float act_r0 = 0.f, act_r1 = 0.f;
    TT_SAMPLED_ROWS(R, n, row0, q, job, P.write_s, P.write_s2, orow, have_act, act_r0, act_r1);
    if (q.critic)
        fwd_small_body<true>(n, q.obs, q.action, q.W, q.out, q.sv, q.dq_da, q.z_state, h1_s, z_s, w1_s, row0, orow, have_act, act_r0, act_r1);
    else
        fwd_small_body<false>(n, q.obs, q.action, q.W, q.out, q.sv, nullptr, nullptr, h1_s, z_s, w1_s, row0, orow);
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
        TT_ACTOR_TAIL_ROWS(n, P.s, P.mu_out, P.Wc[0], P.q_pi, P.dq_da, lds, P.ts, lb, epoch);
        return;
    }
    const int blk = (int)blockIdx.x - nb;
    if (threadIdx.x >= 256 || blk >= WG_ACTOR_WEIGHTS) return;
    TT_ACTOR_TAIL_WEIGHTS(blk, n, P.s, P.sv_a, P.o_a, P.Ga, P.Aa, P.RSa, lds, P.ts, epoch);
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
    const int rc = to_td3_agent(*agent, -1, batch, host);
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
    const int rc = to_td3_agent(*agent, -1, h->n, host);
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
