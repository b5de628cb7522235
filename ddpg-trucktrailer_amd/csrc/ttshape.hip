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
// The bodies are those of ttlearn_bodies.h (bwd_rows_body<.., .., SHAPED>, bwd_weights_body<.., .., PREPEN>); the instantiations of
// every other translation unit are the ones they were.  With delta = 0 and k = 0 these launches leave the bits of the launches they
// stand in for: fmaf(0, pre, f) is f for every finite pre (a factor -0.0 can come back as +0.0).
#include "tthost.h"
#include "ttlearn_bodies.h"

#include <cmath>

namespace {

using tthost::fail;

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

// what every shaped entry point refuses of a tt_loss_shape: TT_OK, or TT_EINVAL with "<who>: <reason>"
int refuse_shape(const char *who, const tt_loss_shape *s) {
    if (!s) return fail(TT_EINVAL, "%s: shape is NULL", who);
    if (!std::isfinite(s->huber_delta) || s->huber_delta < 0.f)
        return fail(TT_EINVAL, "%s: shape->huber_delta = %g is not a finite number >= 0", who, (double)s->huber_delta);
    if (!std::isfinite(s->pre_scale) || s->pre_scale < 0.f)
        return fail(TT_EINVAL, "%s: shape->pre_scale = %g is not a finite number >= 0", who, (double)s->pre_scale);
    if (s->pre_scale > 0.f && !s->pre) return fail(TT_EINVAL, "%s: shape->pre is NULL with pre_scale = %g > 0", who, (double)s->pre_scale);
    return TT_OK;
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
    ImageJob ij{};
    if (image) {
        const tt_mlp_weights *w = image->actor;
        const tt_ring_cursor *c = image->cursor;
        if (!ok_shape(w, false) || !w->split_ws || !c || !c->cursor || !c->k_dev || c->slots <= 0)
            return fail(TT_EINVAL, "%s: the image job lacks the actor's weights, its image buffers or the ring cursor", who);
        if (tdi && (c->k_dev == tdi->step_dev || c->k_dev == tdi->window_dev))
            return fail(TT_EINVAL, "%s: the image cursor's step number is a counter this launch advances", who);
        ij.W = ttnet::to_weights(w);
        ij.ws = reinterpret_cast<unsigned char *>(w->split_ws);
        ij.ws_alt = reinterpret_cast<unsigned char *>(w->split_ws_alt);
        ij.cur = ttnet::RingCursor{reinterpret_cast<const long long *>(c->k_dev), c->slots, c->cursor};
        ij.on = 1;
    }
    Saved sc, sa;
    BwdOut oc, oa;
    TdIn td;
    if (n <= 0) return fail(TT_EINVAL, "%s: n = %d rows, not >= 1", who, n);
    if (!q_out || !mu_out) return fail(TT_EINVAL, "%s: q_out or mu_out is NULL", who);
    if (!ok_shape(critic, true) || !ok_shape(actor, false)) return fail(TT_EINVAL, "%s: the critic's or the actor's weights are missing or not 23-400-300", who);
    if (!to_saved(saved_critic, sc) || !to_saved(saved_actor, sa)) return fail(TT_EINVAL, "%s: a saved forward lacks an array", who);
    if (!to_bwd_out(ws_critic, oc) || !to_bwd_out(ws_actor, oa)) return fail(TT_EINVAL, "%s: a per-row workspace lacks an array", who);
    if (oc.dx2 == oa.dx2) return fail(TT_EINVAL, "%s: ws_critic and ws_actor are the same workspace", who);
    if (!to_td(tdi, td)) return fail(TT_EINVAL, "%s: the TD input lacks an array or the target critic", who);
    hipLaunchKernelGGL(k_bwd_rows_pair_shaped, dim3(2 * ((n + TR - 1) / TR) + 1 + (ij.on ? IMAGE_WGS : 0)), dim3(64 * NW), 0, stream, n,
                       scale_critic, q_out, to_weights(critic), sc, oc, td, mu_out, to_weights(actor), sa, oa, ij, shape->huber_delta,
                       shape->pre);
    return hipGetLastError() == hipSuccess ? TT_OK : fail(TT_EHIP, "%s: the launch failed", who);
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
    if (!row_dq_da || !row_mu) return fail(TT_EINVAL, "%s: row_dq_da or row_mu is NULL (the actor with row factors only)", who);
    if (n <= 0 || n > MAXB) return fail(TT_EINVAL, "%s: n = %d rows, not in [1, %d]", who, n, MAXB);
    if (!obs) return fail(TT_EINVAL, "%s: obs is NULL", who);
    Saved sv;
    BwdOut o;
    if (!to_saved(saved, sv)) return fail(TT_EINVAL, "%s: the saved forward lacks an array", who);
    if (!to_bwd_out(ws, o)) return fail(TT_EINVAL, "%s: the per-row workspace lacks an array", who);
    if (!ok_shape(grads, false)) return fail(TT_EINVAL, "%s: grads is missing or not 23-400-300", who);
    if (count != 0 && count != 10) return fail(TT_EINVAL, "%s: count = %d tensors, not 0 or 10", who, count);
    AdamFused A{};
    if (count && !to_adam(false, count, params, exp_avg, exp_avg_sq, targets, step_dev, lr, beta1, beta2, eps, weight_decay, tau, images,
                          bias_corr, A))
        return fail(TT_EINVAL, "%s: the optimizer step lacks a tensor or the step count", who);
    const RowScale rs{row_dq_da, row_mu, row_scale};
    hipLaunchKernelGGL(k_bwd_weights_shaped, dim3(WG_ACTOR_WEIGHTS), dim3(256), 0, stream, n, obs, sv, o, to_grads(grads), A, rs,
                       shape->pre_scale, static_cast<const float *>(shape->pre));
    return hipGetLastError() == hipSuccess ? TT_OK : fail(TT_EHIP, "%s: the launch failed", who);
}

int tt_mlp_actor_tail_shaped(int n, const float *obs, const float *mu, const tt_mlp_weights *critic, float *q_out, float *dq_da,
                             const tt_mlp_saved *saved, const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, float row_scale,
                             int count, float *const *params, float *const *exp_avg, float *const *exp_avg_sq, float *const *targets,
                             const int64_t *step_dev, float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                             const tt_fc2_images *images, const float *bias_corr, int32_t *tail_words, int32_t *gave_up_host,
                             const tt_loss_shape *shape, tt_stream_t stream) {
    const char *const who = "tt_mlp_actor_tail_shaped";
    if (const int rc = refuse_shape(who, shape)) return rc;
    Saved sv;
    BwdOut o;
    AdamFused A;
    if (n <= 0 || n > MAXB) return fail(TT_EINVAL, "%s: n = %d rows, not in [1, %d]", who, n, MAXB);
    if (!obs || !mu || !q_out || !dq_da) return fail(TT_EINVAL, "%s: obs, mu, q_out or dq_da is NULL", who);
    if (!ok_shape(critic, true)) return fail(TT_EINVAL, "%s: the critic's weights are missing or not 23-400-300", who);
    if (!to_saved(saved, sv)) return fail(TT_EINVAL, "%s: the saved forward lacks an array", who);
    if (!to_bwd_out(ws, o)) return fail(TT_EINVAL, "%s: the per-row workspace lacks an array", who);
    if (!ok_shape(grads, false)) return fail(TT_EINVAL, "%s: grads is missing or not 23-400-300", who);
    if (!to_adam(false, count, params, exp_avg, exp_avg_sq, targets, step_dev, lr, beta1, beta2, eps, weight_decay, tau, images, bias_corr, A))
        return fail(TT_EINVAL, "%s: the optimizer step lacks a tensor or the step count, or count = %d is not 10", who, count);
    if (!tail_words) return fail(TT_EINVAL, "%s: tail_words is NULL", who);
    const int nb = (n + TR - 1) / TR;
    if (nb > 64) return fail(TT_EINVAL, "%s: %d row workgroups, more than the 64 one wave polls", who, nb);
    const RowScale rs{dq_da, mu, row_scale};
    const TailSync ts{tail_words, reinterpret_cast<unsigned long long *>(tail_words + 64), nb, gave_up_host};
    hipLaunchKernelGGL(k_actor_tail_shaped, dim3(nb + WG_ACTOR_WEIGHTS), dim3(64 * NW), 0, stream, n, obs, mu, to_weights(critic), q_out,
                       dq_da, sv, o, to_grads(grads), A, rs, ts, shape->pre_scale, static_cast<const float *>(shape->pre));
    return hipGetLastError() == hipSuccess ? TT_OK : fail(TT_EHIP, "%s: the launch failed", who);
}

}  // extern "C"
