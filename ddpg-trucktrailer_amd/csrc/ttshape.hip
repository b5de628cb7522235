// ttshape.hip -- the loss shape of the lone learn(): a Huber critic loss and a pre-activation penalty on the actor, inside the
// launches learn() makes anyway (MI355X, gfx950; include/ttenv.h: tt_loss_shape).
//
//   k_bwd_rows_pair_shaped     k_bwd_rows_pair's grid, workgroup for workgroup (critic rows, actor rows, the tick workgroup, the
//                              policy image's workgroups).  The critic's rows clamp the TD error to [-delta, delta] before the scale
//                              (huber_loss's d/dq; delta = 0: no clamp); the actor's rows, which hold h2 and w3 in registers for the
//                              unit backward, also form the head's pre-activation pre[b] = b3 + sum_j h2[b][j] w3[j] and store it.
//   k_bwd_weights_shaped       k_bwd_weights<row factors> for the actor: row b's factor is fmaf(k, pre[b], f(b)), k = 2c/B.
//   k_actor_tail_shaped        k_actor_tail with the same factor: the same TailSync hand-over, the same dispatch order, no wait added.
//
// The bodies are those of ttlearn_bodies.h (bwd_rows_body<.., .., SHAPED>, bwd_weights_body<.., .., PREPEN>), the entry points' checks,
// conversions and refuse_shape those of ttlearn_host.h; every other translation unit's instantiations are the ones they were.  With delta
// = 0 and k = 0 these launches leave the bits of those they stand in for: fmaf(0, pre, f) is f for every finite pre (-0.0 can come back +0.0).
#include "ttlearn_host.h"

namespace {

__global__ __launch_bounds__(64 * NW) void k_bwd_rows_pair_shaped(const int n, const float scale_c, const float *__restrict__ q_out,
                                                                  const Weights Wc, const Saved sv_c, const BwdOut o_c, const TdIn td,
                                                                  const float *__restrict__ mu_out, const Weights Wa, const Saved sv_a,
                                                                  const BwdOut o_a, const ImageJob img, const float huber_delta,
                                                                  float *__restrict__ pre_out) {
    __shared__ __attribute__((aligned(16))) float dx2_s[DXS_FLOATS];
    __shared__ float red[2 * NW * TR];
    __shared__ float rsc_s[TR];
    TT_BWD_ROWS_PAIR_FRONT(nb, n, td, img);
    KBEGIN(1);
    if ((int)blockIdx.x < nb) {
        bwd_rows_body<true, false, true>(n, scale_c, q_out, Wc, sv_c, o_c, td, dx2_s, red, rsc_s, blockIdx.x * TR, nullptr, huber_delta);
    } else {
        bwd_rows_body<false, false, true>(n, 0.f, nullptr, Wa, sv_a, o_a, TdIn{}, dx2_s, red, rsc_s, ((int)blockIdx.x - nb) * TR, nullptr,
                                          0.f, pre_out);
    }
    KEND(1);
}

// (three workgroups per CU, as k_bwd_weights: <= 168 registers)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k_bwd_weights_shaped(
    const int n, const float *__restrict__ obs, const Saved sv, const BwdOut d, const Grads G, const AdamFused A, const RowScale RS,
    const float pre_scale, const float *__restrict__ pre) {
    __shared__ __attribute__((aligned(16))) float part[4][4][256];     // [wave][tile][lane*4 + r]
    __shared__ float f_s[MAXB];                                        // the rows' factors, computed once per workgroup
    __shared__ __attribute__((aligned(16))) _Float16 stage_s[4 * 1024];   // forward-image pieces of a dW2 workgroup's patch
    kernarg_warm<24 + (int)sizeof(Saved) + (int)sizeof(BwdOut) + (int)sizeof(Grads) + (int)sizeof(AdamFused) + (int)sizeof(RowScale)>();
    bwd_weights_body<true, false, true>(blockIdx.x, n, 0, obs, nullptr, sv, d, G, A, RS, part, f_s, TailSync{nullptr, nullptr, 0, nullptr},
                                        0, stage_s, pre_scale, pre);
}

// k_actor_tail with the penalty's term in the rows' factors: row workgroups first, the weight workgroups wait for their dQ/da words
__global__ __launch_bounds__(64 * NW) void k_actor_tail_shaped(const int n, const float *__restrict__ obs, const float *__restrict__ mu,
                                                               const Weights Wc, float *__restrict__ q_out, float *__restrict__ dq_da,
                                                               const Saved sv, const BwdOut d, const Grads G, const AdamFused A,
                                                               const RowScale RS, const TailSync ts, const float pre_scale,
                                                               const float *__restrict__ pre) {
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
    TT_ACTOR_TAIL_WEIGHTS_SHAPED(true, (int)blockIdx.x - nb, n, obs, sv, d, G, A, RS, lds, ts, epoch, pre_scale, pre);
}

}  // namespace

extern "C" {

int tt_mlp_backward_rows_pair_shaped(int n, float scale_critic, const float *q_out, const tt_mlp_weights *critic,
                                     const tt_mlp_saved *saved_critic, const tt_mlp_bwd_ws *ws_critic, const tt_td_input *tdi,
                                     const float *mu_out, const tt_mlp_weights *actor, const tt_mlp_saved *saved_actor,
                                     const tt_mlp_bwd_ws *ws_actor, const tt_image_job *image, const tt_loss_shape *shape,
                                     tt_stream_t stream) {
    const char *const who = "tt_mlp_backward_rows_pair_shaped";
    if (const int rc = refuse_shape(who, shape)) return rc;
    RowsPair R;
    if (const int rc = to_rows_pair(who, n, q_out, critic, saved_critic, ws_critic, tdi, mu_out, actor, saved_actor, ws_actor, image, R)) return rc;
    hipLaunchKernelGGL(k_bwd_rows_pair_shaped, R.grid, dim3(64 * NW), 0, stream, n, scale_critic, q_out, R.Wc, R.sc, R.oc, R.td, mu_out, R.Wa,
                       R.sa, R.oa, R.img, shape->huber_delta, shape->pre);
    return launched(who);
}

int tt_mlp_backward_weights_shaped(int n, int critic, const float *obs, const float *action, const tt_mlp_saved *saved,
                                   const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, const float *row_dq_da, const float *row_mu,
                                   float row_scale, int count, float *const *params, float *const *exp_avg, float *const *exp_avg_sq,
                                   float *const *targets, const int64_t *step_dev, float lr, float beta1, float beta2, float eps,
                                   float weight_decay, float tau, const tt_fc2_images *images, const float *bias_corr,
                                   const tt_loss_shape *shape, tt_stream_t stream) {
    const char *const who = "tt_mlp_backward_weights_shaped";
    (void)action;
    if (const int rc = refuse_shape(who, shape)) return rc;
    if (critic) return fail(TT_EINVAL, "%s: the critic has no shaped weight launch (its loss shape is in the rows launch)", who);
    WeightsLaunch L;
    if (const int rc = to_weights_launch(who, true, n, 0, obs, saved, ws, grads, row_dq_da, row_mu, row_scale, count, params, exp_avg, exp_avg_sq,
                                         targets, step_dev, lr, beta1, beta2, eps, weight_decay, tau, images, bias_corr, L))
        return rc;
    hipLaunchKernelGGL(k_bwd_weights_shaped, dim3(WG_ACTOR_WEIGHTS), dim3(256), 0, stream, n, obs, L.sv, L.o, L.G, L.A, L.rs, shape->pre_scale,
                       static_cast<const float *>(shape->pre));
    return launched(who);
}

int tt_mlp_actor_tail_shaped(int n, const float *obs, const float *mu, const tt_mlp_weights *critic, float *q_out, float *dq_da,
                             const tt_mlp_saved *saved, const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, float row_scale,
                             int count, float *const *params, float *const *exp_avg, float *const *exp_avg_sq, float *const *targets,
                             const int64_t *step_dev, float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                             const tt_fc2_images *images, const float *bias_corr, int32_t *tail_words, int32_t *gave_up_host,
                             const tt_loss_shape *shape, tt_stream_t stream) {
    const char *const who = "tt_mlp_actor_tail_shaped";
    if (const int rc = refuse_shape(who, shape)) return rc;
    Tail T;
    if (const int rc = to_actor_tail(who, n, obs, mu, critic, q_out, dq_da, saved, ws, grads, row_scale, count, params, exp_avg, exp_avg_sq,
                                     targets, step_dev, lr, beta1, beta2, eps, weight_decay, tau, images, bias_corr, tail_words, gave_up_host, T))
        return rc;
    hipLaunchKernelGGL(k_actor_tail_shaped, T.grid, dim3(64 * NW), 0, stream, n, obs, mu, T.Wc, q_out, dq_da, T.sv, T.o, T.G, T.A, T.rs, T.ts,
                       shape->pre_scale, static_cast<const float *>(shape->pre));
    return launched(who);
}

}  // extern "C"
