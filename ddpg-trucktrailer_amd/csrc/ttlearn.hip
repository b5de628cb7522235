// ttlearn.hip -- hand-fused DDPG learn() for the reference-shaped networks (23 -> 400 -> LN -> ReLU -> 300 -> LN ...),
// exact f32, MI355X (gfx950).  What DDPG_agent.learn() (DDPG/DDPG_agent.py:72-106) does through ~140 autograd
// kernels at batch 256 is done here in six launches (sample -- csrc/ttnet.hip -- then):
//
//   k_fwd_multi           learn()'s first phase: up to four forwards in one launch (target actor and the target critic's
//                         state branch on s', Q(s,a) and mu(s) with what their backward needs: normalised
//                         pre-activations, 1/sigma, post-ReLU activations); k_fwd_small<CRITIC> is one of them alone
//   k_bwd_rows_pair       per-row backward of both nets on different workgroups: [critic: q' and the TD target for its
//                         rows ->] head -> ReLU -> LayerNorm2 -> dH1 = dX2 * W2 (MFMA) -> ReLU -> LayerNorm1
//   k_bwd_weights         dW2 = dX2^T * H1 and dW1 = dX1^T * S on the MFMA (K = batch), all bias / LayerNorm / head
//                         gradients as deterministic column sums (no atomics), then (one rank) torch.optim.Adam's
//                         update + the soft target update on each element just finished
//   k_adam_soft           Adam + soft update as a launch of its own (data-parallel ranks: after the all-reduce)
//
// The structs, device bodies and host conversions are in ttlearn_bodies.h, which the population's launches (csrc/ttpop.hip) share as
// well, the checked conversions of the launches with option forms in ttlearn_host.h; this file holds the lone kernels and entry points.
#include "ttlearn_host.h"
#include "ttp2p.h"             // the peer-to-peer gradient exchange of data-parallel ranks: k_adam_soft_p2p reads it

namespace {

template <bool CRITIC>
__global__ __launch_bounds__(64 * NW) void k_fwd_small(const int n, const float *__restrict__ obs,
                                                   const float *__restrict__ action, const float *__restrict__ w1e,
                                                   const float *__restrict__ b1e, const float *__restrict__ g1e,
                                                   const float *__restrict__ be1e, const Weights W,
                                                   float *__restrict__ out, const Saved sv, float *__restrict__ dq_da,
                                                   float *__restrict__ z_state) {
    // (n .. be1e: 14 dwords of leading scalar arguments = the preloaded prefix; w1e .. be1e repeat W.w1, b1, g1, be1)
    __shared__ __attribute__((aligned(16))) float h1_s[H1S_FLOATS];
    __shared__ __attribute__((aligned(16))) float z_s[TR * DS];
    __shared__ __attribute__((aligned(16))) float w1_s[H1 * IN];
    KernargWarm<64 + (int)sizeof(Weights) + 8 + (int)sizeof(Saved) + 16> warm;
    warm.issue();
    KBEGIN(3);
    const EarlyW E{w1e, b1e, g1e, be1e};
    auto hook = [&]() __attribute__((always_inline)) { warm.wait(); };
    fwd_small_body<CRITIC, decltype(hook)>(n, obs, action, W, out, sv, dq_da, z_state, h1_s, z_s, w1_s, blockIdx.x * TR, nullptr, false, 0.f,
                                           0.f, nullptr, 0u, &E, hook);
    KEND(3);
}

// learn()'s forwards in one launch (FwdJobs): workgroup b serves job b / blocks_per_job
__global__ __launch_bounds__(64 * NW) void k_fwd_multi(const FwdJobs J) {
    __shared__ __attribute__((aligned(16))) float h1_s[H1S_FLOATS];
    __shared__ __attribute__((aligned(16))) float z_s[TR * DS];
    __shared__ __attribute__((aligned(16))) float w1_s[H1 * IN];
    kernarg_warm<(int)sizeof(FwdJobs)>();
    const int job = blockIdx.x / J.blocks_per_job, row0 = (blockIdx.x - job * J.blocks_per_job) * TR;
    const FwdJob &q = J.j[job];
    KBEGIN(0);
#ifdef TT_STAMPS   // the last end of the PREVIOUS learn()'s last launch, before this learn() overwrites anything: [5][0][0]
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        unsigned long long m = 0;
        for (int i = threadIdx.x; i < 512; i += 64) m = max(m, g_kblk[4][i][1]);
        for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned long long)__shfl_xor((long long)m, o));
        if (threadIdx.x == 0) g_kblk[5][0][0] = m;
    }
#endif
    const float *orow = nullptr;
    bool have_act = false;
    float act_r0 = 0.f, act_r1 = 0.f;
    if (J.sampled) {
        ttnet::await_progress(J.R.progress, J.R.k_dev);
        if (J.k_snapshot && blockIdx.x == 0 && threadIdx.x == 0) *J.k_snapshot = *J.R.k_dev;
        TT_SAMPLED_ROWS(J.R, J.n, row0, q, job, J.write_s, J.write_s2, orow, have_act, act_r0, act_r1);
    }
    if (q.critic)
        fwd_small_body<true>(J.n, q.obs, q.action, q.W, q.out, q.sv, q.dq_da, q.z_state, h1_s, z_s, w1_s, row0, orow, have_act, act_r0, act_r1);
    else
        fwd_small_body<false>(J.n, q.obs, q.action, q.W, q.out, q.sv, nullptr, nullptr, h1_s, z_s, w1_s, row0, orow);
    KEND(0);
}

// The critic's per-row backward (with the TD prologue) and the ACTOR's unit backward in one launch, on different
// workgroups.  The actor's per-row gradients are linear in the row's d(loss)/d(pre-tanh) = -(1/B) dQ/da (1 - mu^2), and dQ/da
// needs the UPDATED critic (DDPG_agent.py:100-103) -- but everything else of the actor's backward (ReLU masks, both
// LayerNorm backwards, dH1 = dX2 * W2) only needs what the forward saved.  So that part runs HERE, beside the critic's
// backward, for a unit gradient, and k_bwd_weights multiplies row b by the real number once the critic has been updated and
// dQ/da is known: the actor's backward is off the chain's critical path.  (So mu_out is not read here: the factor that needs
// mu is k_bwd_weights' RowScale.)
__global__ __launch_bounds__(64 * NW) void k_bwd_rows_pair(const int n, const float scale_c, const float *__restrict__ q_out,
                                                           const Weights Wc, const Saved sv_c, const BwdOut o_c, const TdIn td,
                                                           const float *__restrict__ mu_out, const Weights Wa, const Saved sv_a,
                                                           const BwdOut o_a, const ImageJob img) {
    __shared__ __attribute__((aligned(16))) float dx2_s[DXS_FLOATS];
    __shared__ float red[2 * NW * TR];
    __shared__ float rsc_s[TR];
    TT_BWD_ROWS_PAIR_FRONT(nb, n, td, img);
    KBEGIN(1);
    if ((int)blockIdx.x < nb) {
        bwd_rows_body<true>(n, scale_c, q_out, Wc, sv_c, o_c, td, dx2_s, red, rsc_s, blockIdx.x * TR);
    } else {
        bwd_rows_body<false>(n, 0.f, nullptr, Wa, sv_a, o_a, TdIn{}, dx2_s, red, rsc_s, ((int)blockIdx.x - nb) * TR);
    }
    KEND(1);
}

// (three workgroups per CU: beside the policy's grid ~85 CUs are free for the ~205 of this launch -- 168 registers: bwd_weights_body)
template <bool ROWSCALE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k_bwd_weights(const int n, const int critic, const float *__restrict__ obs,
                                                     const float *__restrict__ action, const Saved sv,
                                                     const BwdOut d, const Grads G, const AdamFused A, const RowScale RS) {
    __shared__ __attribute__((aligned(16))) float part[4][4][256];     // [wave][tile][lane*4 + r]
    __shared__ float f_s[ROWSCALE ? MAXB : 1];                         // the rows' factors, computed once per workgroup
    __shared__ __attribute__((aligned(16))) _Float16 stage_s[4 * 1024];   // forward-image pieces of a dW2 workgroup's patch
    kernarg_warm<24 + (int)sizeof(Saved) + (int)sizeof(BwdOut) + (int)sizeof(Grads) + (int)sizeof(AdamFused) + (int)sizeof(RowScale)>();
    bwd_weights_body<ROWSCALE, false>(blockIdx.x, n, critic, obs, action, sv, d, G, A, RS, part, f_s, TailSync{nullptr, nullptr, 0, nullptr}, 0,
                                      stage_s);
}

// learn()'s last two launches in ONE grid (the single-rank chain where the policy launch is small or learn() repeats per step):
// workgroups [0, nb) are k_fwd_small<critic> on (s, mu(s)) -- Q(s, mu(s)) and dQ/da through the UPDATED critic (DDPG_agent.py:100-103)
// --, the rest are k_bwd_weights<actor>, which request their operands, optimizer state and step count at once as always and then
// wait for the row workgroups' dQ/da in device memory (TailSync) instead of behind a launch boundary: the boundary (1.5-1.9 us),
// the kernel entry and the operand round trip of the weight-gradient launch leave learn()'s chain.  The row workgroups are
// dispatched first, so they never wait for a CU behind the workgroups that wait for them.  512 threads per workgroup (the row
// kernel's geometry); a weight-gradient workgroup uses the first 256.  LDS: the row kernel's tiles and the weight kernel's share it.
__global__ __launch_bounds__(64 * NW) void k_actor_tail(const int n, const float *__restrict__ obs, const float *__restrict__ mu,
                                                        const Weights Wc, float *__restrict__ q_out, float *__restrict__ dq_da,
                                                        const Saved sv, const BwdOut d, const Grads G, const AdamFused A,
                                                        const RowScale RS, const TailSync ts) {
    __shared__ __attribute__((aligned(16))) float lds[H1S_FLOATS + TR * DS + H1 * IN];
    const int nb = (n + TR - 1) / TR;
    if ((int)blockIdx.x < nb) {
        const long long epoch = *A.step_dev;
        KBEGIN(3);
        TT_ACTOR_TAIL_ROWS(n, obs, mu, Wc, q_out, dq_da, lds, ts, blockIdx.x, epoch);
        KEND(3);
        return;
    }
    if (threadIdx.x >= 256) return;
    const long long epoch = *A.step_dev;
    TT_ACTOR_TAIL_WEIGHTS((int)blockIdx.x - nb, n, obs, sv, d, G, A, RS, lds, ts, epoch);
}

// ------------------------------------------------------------------------------------------------------
// torch.optim.Adam (amsgrad off, weight decay added to the gradient: networks.py:49-50,133) for every parameter
// tensor of a net in one launch, followed by the soft target update theta' <- theta' + tau*(theta - theta')
// (DDPG_agent.py:108-131).  step_dev holds the 1-based step count of THIS update.
__global__ __launch_bounds__(256) void k_adam_soft(const AdamTable T, const long long *__restrict__ step_dev,
                                                   const float lr, const float beta1, const float beta2,
                                                   const float eps, const float weight_decay, const float tau,
                                                   const float *__restrict__ bias_corr) {
    TT_ADAM_SOFT_ELEMENT(T.g[ti][i])      // csrc/ttlearn_sites.h: the text k_adam_soft_clip holds too
}

// k_adam_soft for data-parallel ranks WITHOUT a collective launch in front of it (include/ttenv.h: tt_p2p_*): the gradient of
// element i is the mean over the ranks of G_r[i], read from every rank's exchange block (this rank's own included) and summed
// in rank order -- the same bits on every rank.  A workgroup takes EPT x 256 consecutive elements of one tensor (few, fat
// workgroups: each of them waits and acquires once).  Hand-over (per site, epoch = this learn step's number):
//   publish  the launch's FIRST workgroup: system-scope release, then epoch -> word [site][me] of every rank's block.  The launch
//            that wrote G_me is the one in front of this one on its stream, so it is complete and written back by now;
//   wait     every workgroup: until the words [site][0..world) of its OWN block hold the epoch (relaxed system-scope loads of local
//            fine-grained memory, bounded), then a system-scope acquire;
//   read     G_r[i] by system-scope loads (never from a cache that could hold the previous step's value of the same address).
#ifndef TT_P2P_EPT
#define TT_P2P_EPT 4
#endif
constexpr int P2P_EPT = TT_P2P_EPT;
__global__ __launch_bounds__(256) void k_adam_soft_p2p(const AdamTable T, const ttp2p::Args X, const long long *__restrict__ step_dev,
                                                       const float lr, const float beta1, const float beta2, const float eps,
                                                       const float weight_decay, const float tau,
                                                       const float *__restrict__ bias_corr) {
    const long long step = *step_dev;
    int ti = 0;
    while (ti + 1 < T.count && (int)blockIdx.x >= T.block_start[ti + 1]) ++ti;
    const int base = ((int)blockIdx.x - T.block_start[ti]) * (256 * P2P_EPT) + threadIdx.x;
    const int n = T.numel[ti];
    // everything that does not depend on the exchange is requested first -- this rank's parameters, Adam moments, targets, bias
    // corrections -- so that those loads fly while the workgroup waits for the arrival words
    float pv[P2P_EPT], mv[P2P_EPT], vv[P2P_EPT], tv[P2P_EPT];
    const bool has_t = T.tgt[ti] != nullptr;
#pragma unroll
    for (int e = 0; e < P2P_EPT; ++e) {
        const int i = min(base + e * 256, n - 1);
        pv[e] = T.p[ti][i]; mv[e] = T.m[ti][i]; vv[e] = T.v[ti][i];
        tv[e] = has_t ? T.tgt[ti][i] : 0.f;
    }
    float bcc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (bias_corr) {
#pragma unroll
        for (int q = 0; q < 5; ++q) bcc[q] = bias_corr[q];
    }
    if (threadIdx.x == 0) {
        const int epoch = (int)step;
        if (blockIdx.x == 0) {
#ifndef TT_P2P_NOFENCE
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
#endif
            for (int r = 0; r < X.world; ++r)
                __hip_atomic_store(X.arrive[r] + X.site * ttp2p::MAXR + X.me, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        const int *mine = X.arrive[X.me] + X.site * ttp2p::MAXR;
        const unsigned long long t0 = wall_clock64();
        bool gave_up = false;
        for (int r = 0; r < X.world && !gave_up; ++r) {
            while (!ttnet::epoch_reached(__hip_atomic_load(mine + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM), epoch)) {
                __builtin_amdgcn_s_sleep(8);
                if (wall_clock64() - t0 > X.wait_ticks) {      // never hang: mark (host-visible) and go on; the caller treats the ranks as diverged
                    __hip_atomic_store(X.gave_up_host, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    gave_up = true;
                    break;
                }
            }
        }
#ifndef TT_P2P_NOFENCE
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
#endif
    }
    __syncthreads();
    const size_t goff = X.tensor_offset[ti];           // the tensor's place (floats) in the site's flat buffer
    float gsum[P2P_EPT];
#pragma unroll
    for (int e = 0; e < P2P_EPT; ++e) gsum[e] = 0.f;
    for (int r = 0; r < X.world; ++r) {                 // rank order: the same sum on every rank
        const float *src = X.grad[r] + goff;
        float part[P2P_EPT];
#pragma unroll
        for (int e = 0; e < P2P_EPT; ++e) {
            const int i = base + e * 256;
            // (this rank's own buffer: an ordinary load -- its backward launch is over; a peer's: system scope, served by the
            // owner's memory, never by a cache of this GPU that could still hold last step's value of the same address)
            part[e] = i >= n ? 0.f : (r == X.me ? src[i] : __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
        }
#pragma unroll
        for (int e = 0; e < P2P_EPT; ++e) gsum[e] = __fadd_rn(gsum[e], part[e]);
    }
    float bc1, bc2;
    adam_bias_corrections(beta1, beta2, step, bias_corr != nullptr, bcc, bc1, bc2);
    const float sqrt_bc2 = sqrtf(bc2);
    const float world_f = (float)X.world;
#pragma unroll
    for (int e = 0; e < P2P_EPT; ++e) {
        const int i = base + e * 256;
        if (i >= n) continue;
        const float grad = X.world > 1 ? __fdiv_rn(gsum[e], world_f) : gsum[e];
        float p = pv[e];
        const float g = fmaf(weight_decay, p, grad);
        const float m = fmaf(beta1, mv[e], (1.f - beta1) * g);          // exp_avg.lerp_(grad, 1 - beta1)
        const float v = fmaf(beta2, vv[e], (1.f - beta2) * g * g);
        T.m[ti][i] = m;
        T.v[ti][i] = v;
        const float denom = sqrtf(v) / sqrt_bc2 + eps;
        p -= (lr / bc1) * (m / denom);
        T.p[ti][i] = p;
        float tg = 0.f;
        if (has_t) {
            tg = tv[e];
            tg = fmaf(tau, p - tg, tg);
            T.tgt[ti][i] = tg;
        }
        if (ti == 4 && (T.img_p || T.img_t)) {
            const int nn = i / H1, k = i - nn * H1;
            if (T.img_p) img_store(T.img_p, nn, k, p, true);
            if (T.img_t && has_t) img_store(T.img_t, nn, k, tg, false);
        }
    }
}

// the image of fc2 from scratch (tt_mlp_fc2_image_pack): one thread per weight; the padding of the buffer is never written
__global__ __launch_bounds__(256) void k_img_pack(const float *__restrict__ w2, _Float16 *__restrict__ img) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H2 * H1) return;
    const int nn = i / H1, k = i - nn * H1;
    img_store(img, nn, k, w2[i], true);
}

}  // namespace

extern "C" {

int tt_mlp_forward_save(int n, int critic, const float *obs, const float *action, const tt_mlp_weights *w, float *out,
                        const tt_mlp_saved *saved, float *dq_da, tt_stream_t stream) {
    if (n < 0 || !obs || !out || !ok_shape(w, critic != 0) || (critic && !action)) return TT_EINVAL;
    if (n == 0) return TT_OK;
    Saved sv{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (saved && !to_saved(saved, sv)) return TT_EINVAL;
    hipLaunchKernelGGL(critic ? k_fwd_small<true> : k_fwd_small<false>, dim3((n + TR - 1) / TR), dim3(64 * NW), 0, stream, n, obs, action, w->w1,
                       w->b1, w->g1, w->be1, to_weights(w), out, sv, critic ? dq_da : nullptr, static_cast<float *>(nullptr));
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

static int forward_multi_impl(int n, int count, const tt_fwd_job *jobs, const tt_sample_args *sample, int64_t *k_snapshot,
                              tt_stream_t stream) {
    if (n < 0 || count < 1 || count > 4 || !jobs) return TT_EINVAL;
    if (n == 0) return TT_OK;
    FwdJobs J{};
    J.n = n;
    J.blocks_per_job = (n + TR - 1) / TR;
    J.write_s = J.write_s2 = -1;
    if (sample) {
        if (sample->batch != n) return TT_EINVAL;
        const int rc = ttnet::make_ring_sample(sample, J.R);
        if (rc != TT_OK) return rc;
        J.sampled = 1;
        J.R.progress = const_cast<int *>(sample->step_progress);
        J.k_snapshot = reinterpret_cast<long long *>(k_snapshot);
    }
    for (int i = 0; i < count; ++i)
        if (!to_fwd_job(jobs[i], i, sample, J)) return TT_EINVAL;
    if (sample && (J.write_s < 0 || J.write_s2 < 0)) return TT_EINVAL;      // the later launches need all five batch buffers
    hipLaunchKernelGGL(k_fwd_multi, dim3(count * J.blocks_per_job), dim3(64 * NW), 0, stream, J);
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

int tt_mlp_forward_multi(int n, int count, const tt_fwd_job *jobs, tt_stream_t stream) {
    return forward_multi_impl(n, count, jobs, nullptr, nullptr, stream);
}

int tt_mlp_forward_multi_sampled(int n, int count, const tt_fwd_job *jobs, const tt_sample_args *sample, int64_t *k_snapshot,
                                 tt_stream_t stream) {
    if (!sample) return TT_EINVAL;
    return forward_multi_impl(n, count, jobs, sample, k_snapshot, stream);
}

int tt_mlp_backward_rows_pair(int n, float scale_critic, const float *q_out, const tt_mlp_weights *critic,
                              const tt_mlp_saved *saved_critic, const tt_mlp_bwd_ws *ws_critic, const tt_td_input *tdi,
                              const float *mu_out, const tt_mlp_weights *actor, const tt_mlp_saved *saved_actor,
                              const tt_mlp_bwd_ws *ws_actor, const tt_image_job *image, tt_stream_t stream) {
    const char *const who = "tt_mlp_backward_rows_pair";
    RowsPair R;
    if (const int rc = to_rows_pair(who, n, q_out, critic, saved_critic, ws_critic, tdi, mu_out, actor, saved_actor, ws_actor, image, R)) return rc;
    hipLaunchKernelGGL(k_bwd_rows_pair, R.grid, dim3(64 * NW), 0, stream, n, scale_critic, q_out, R.Wc, R.sc, R.oc, R.td, mu_out, R.Wa, R.sa,
                       R.oa, R.img);
    return launched(who);
}

int tt_mlp_backward_weights(int n, int critic, const float *obs, const float *action, const tt_mlp_saved *saved,
                            const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, const float *row_dq_da, const float *row_mu,
                            float row_scale, int count, float *const *params, float *const *exp_avg, float *const *exp_avg_sq,
                            float *const *targets, const int64_t *step_dev, float lr, float beta1, float beta2, float eps,
                            float weight_decay, float tau, const tt_fc2_images *images, const float *bias_corr,
                            tt_stream_t stream) {
    const char *const who = "tt_mlp_backward_weights";
    if (critic && !action) return fail(TT_EINVAL, "%s: action is NULL for the critic", who);
    WeightsLaunch L;      // (count = 0: gradients only; else Adam + soft update applied in the same launch, one rank)
    if (const int rc = to_weights_launch(who, false, n, critic, obs, saved, ws, grads, row_dq_da, row_mu, row_scale, count, params, exp_avg,
                                         exp_avg_sq, targets, step_dev, lr, beta1, beta2, eps, weight_decay, tau, images, bias_corr, L))
        return rc;
    hipLaunchKernelGGL(row_dq_da ? k_bwd_weights<true> : k_bwd_weights<false>, dim3(critic ? WG_CRITIC_WEIGHTS : WG_ACTOR_WEIGHTS), dim3(256), 0,
                       stream, n, critic, obs, action, L.sv, L.o, L.G, L.A, L.rs);
    return launched(who);
}

int tt_mlp_actor_tail(int n, const float *obs, const float *mu, const tt_mlp_weights *critic, float *q_out, float *dq_da,
                      const tt_mlp_saved *saved, const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, float row_scale, int count,
                      float *const *params, float *const *exp_avg, float *const *exp_avg_sq, float *const *targets,
                      const int64_t *step_dev, float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                      const tt_fc2_images *images, const float *bias_corr, int32_t *tail_words, int32_t *gave_up_host,
                      tt_stream_t stream) {
    const char *const who = "tt_mlp_actor_tail";
    Tail T;
    if (const int rc = to_actor_tail(who, n, obs, mu, critic, q_out, dq_da, saved, ws, grads, row_scale, count, params, exp_avg, exp_avg_sq,
                                     targets, step_dev, lr, beta1, beta2, eps, weight_decay, tau, images, bias_corr, tail_words, gave_up_host, T))
        return rc;
    hipLaunchKernelGGL(k_actor_tail, T.grid, dim3(64 * NW), 0, stream, n, obs, mu, T.Wc, q_out, dq_da, T.sv, T.o, T.G, T.A, T.rs, T.ts);
    return launched(who);
}

int tt_adam_soft_update(int count, float *const *params, const float *const *grads, float *const *exp_avg,
                        float *const *exp_avg_sq, float *const *targets, const int32_t *numel, const int64_t *step_dev,
                        float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                        const tt_fc2_images *images, const float *bias_corr, tt_stream_t stream) {
    if (count <= 0 || count > MAXT || !params || !grads || !exp_avg || !exp_avg_sq || !numel || !step_dev) return TT_EINVAL;
    AdamTable T{};
    const int blocks = fill_adam_table(T, 256, count, params, grads, exp_avg, exp_avg_sq, targets, numel, images);
    if (blocks < 0) return TT_EINVAL;
    hipLaunchKernelGGL(k_adam_soft, dim3(blocks), dim3(256), 0, stream, T, reinterpret_cast<const long long *>(step_dev), lr,
                       beta1, beta2, eps, weight_decay, tau, bias_corr);
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

int tt_adam_soft_update_p2p(tt_p2p *x, int site, int count, float *const *params, float *const *exp_avg,
                            float *const *exp_avg_sq, float *const *targets, const int32_t *numel, const int64_t *step_dev,
                            float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                            const tt_fc2_images *images, const float *bias_corr, tt_stream_t stream) {
    if (!x || site < 0 || site >= x->sites || count <= 0 || count > MAXT || !params || !exp_avg || !exp_avg_sq || !numel || !step_dev)
        return TT_EINVAL;
    AdamTable T{};
    ttp2p::Args X{};
    const int blocks = fill_adam_table(T, 256 * P2P_EPT, count, params, nullptr, exp_avg, exp_avg_sq, targets, numel, images);
    if (blocks < 0) return TT_EINVAL;
    size_t off = 0;
    for (int i = 0; i < count; ++i) {
        X.tensor_offset[i] = (unsigned)off;
        off += (size_t)numel[i];
    }
    if (off != (size_t)x->numel[site]) return TT_EINVAL;      // the tensors must tile the site's buffer exactly
    X.world = x->world; X.me = x->rank; X.site = site;
    for (int r = 0; r < x->world; ++r) {
        if (!x->attached[r] || !x->block[r] || !x->flags[r]) return TT_EINVAL;      // every peer's blocks must have been opened (tt_p2p_attach)
        X.arrive[r] = reinterpret_cast<int *>(x->flags[r]);
        X.grad[r] = reinterpret_cast<const float *>(x->block[r] + x->offset[site]);
    }
    X.gave_up_host = x->gave_up_host;
    X.wait_ticks = x->wait_ticks;
    hipLaunchKernelGGL(k_adam_soft_p2p, dim3(blocks), dim3(256), 0, stream, T, X, reinterpret_cast<const long long *>(step_dev), lr,
                       beta1, beta2, eps, weight_decay, tau, bias_corr);
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

uint64_t tt_mlp_fc2_image_bytes(void) { return (uint64_t)IMG_HALVES * 2; }

int tt_mlp_fc2_image_pack(const tt_mlp_weights *w, tt_stream_t stream) {
    if (!w || !w->w2 || !w->fc2_img || w->fc1_dims != H1 || w->fc2_dims != H2) return TT_EINVAL;
    hipLaunchKernelGGL(k_img_pack, dim3((H2 * H1 + 255) / 256), dim3(256), 0, stream, w->w2,
                       reinterpret_cast<_Float16 *>(w->fc2_img));
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

#ifdef TT_STAMPS
int tt_debug_blocks(unsigned long long *out1024) {
    return hipMemcpyFromSymbol(out1024, HIP_SYMBOL(g_blk), sizeof(unsigned long long) * 1024) == hipSuccess ? 0 : -3;
}
int tt_debug_wst(unsigned long long *out32) {
    return hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_wst), sizeof(unsigned long long) * 32) == hipSuccess ? 0 : -3;
}
int tt_debug_kblocks(unsigned long long *out6x1024) {
    return hipMemcpyFromSymbol(out6x1024, HIP_SYMBOL(g_kblk), sizeof(unsigned long long) * 6 * 1024) == hipSuccess ? 0 : -3;
}
int tt_debug_log_learn(int k, unsigned long long *out, int reset) {
    if (k < 0 || k >= 5) return -1;
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_log_learn), sizeof(TTLog), sizeof(TTLog) * (size_t)k) != hipSuccess) return -3;
    if (reset) { const unsigned long long z = 0; if (hipMemcpyToSymbol(HIP_SYMBOL(g_log_learn), &z, sizeof(z), sizeof(TTLog) * (size_t)k) != hipSuccess) return -3; }
    return 0;
}
int tt_debug_learn_poll(unsigned long long *out4) {
    return hipMemcpyFromSymbol(out4, HIP_SYMBOL(ttnet::g_poll), sizeof(unsigned long long) * 4) == hipSuccess ? 0 : -3;
}
int tt_debug_substamps(unsigned long long *out16) {
    return hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_sub), sizeof(unsigned long long) * 16) == hipSuccess ? 0 : -3;
}
int tt_debug_stamps(unsigned long long *out32) {
    return hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 32) == hipSuccess ? 0 : -3;
}
#endif

}  // extern "C"
