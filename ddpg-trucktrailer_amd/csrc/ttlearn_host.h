// ttlearn_host.h -- the host side that the lone learn()'s launches share across their options (csrc/ttlearn.hip the plain ones,
// csrc/ttshape.hip with a tt_loss_shape, csrc/ttdemo.hip with a tt_demo_loss, csrc/ttclip.hip the optimizer step with a tt_grad_clip): one
// checked conversion per launch (and the table of the optimizer launches of their own, fill_adam_table), from the C arguments
// (include/ttenv.h) to the structs the kernels take.  Each returns TT_OK, or TT_EINVAL with the message "<who>: <reason>", `who` the
// entry point called; that is then its option's own refusals, the conversion, its own launch.  Host only.
#pragma once
#include <climits>
#include <cmath>

#include "tthost.h"
#include "ttlearn_bodies.h"

namespace {

using tthost::fail;

// what every entry point with a tt_loss_shape refuses of it
int refuse_shape(const char *who, const tt_loss_shape *s) {
    if (!s) return fail(TT_EINVAL, "%s: shape is NULL", who);
    if (!std::isfinite(s->huber_delta) || s->huber_delta < 0.f)
        return fail(TT_EINVAL, "%s: shape->huber_delta = %g is not a finite number >= 0", who, (double)s->huber_delta);
    if (!std::isfinite(s->pre_scale) || s->pre_scale < 0.f)
        return fail(TT_EINVAL, "%s: shape->pre_scale = %g is not a finite number >= 0", who, (double)s->pre_scale);
    if (s->pre_scale > 0.f && !s->pre) return fail(TT_EINVAL, "%s: shape->pre is NULL with pre_scale = %g > 0", who, (double)s->pre_scale);
    return TT_OK;
}

// how every entry point here ends, after its hipLaunchKernelGGL
int launched(const char *who) { return hipGetLastError() == hipSuccess ? TT_OK : fail(TT_EHIP, "%s: the launch failed", who); }

// the policy image's pack inside the rows-pair launch; image NULL: none (ij stays off)
int to_image_job(const char *who, const tt_image_job *image, const tt_td_input *tdi, ImageJob &ij) {
    ij = ImageJob{};
    if (!image) return TT_OK;
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
    return TT_OK;
}

// k_bwd_rows_pair[_shaped]: the kernel's arguments between n, scale_c, q_out and the option's own, and the grid
struct RowsPair { Weights Wc, Wa; Saved sc, sa; BwdOut oc, oa; TdIn td; ImageJob img; dim3 grid; };

int to_rows_pair(const char *who, int n, const float *q_out, const tt_mlp_weights *critic, const tt_mlp_saved *saved_critic,
                 const tt_mlp_bwd_ws *ws_critic, const tt_td_input *tdi, const float *mu_out, const tt_mlp_weights *actor,
                 const tt_mlp_saved *saved_actor, const tt_mlp_bwd_ws *ws_actor, const tt_image_job *image, RowsPair &R) {
    if (const int rc = to_image_job(who, image, tdi, R.img)) return rc;
    if (n <= 0) return fail(TT_EINVAL, "%s: n = %d rows, not >= 1", who, n);
    if (!q_out || !mu_out) return fail(TT_EINVAL, "%s: q_out or mu_out is NULL", who);
    if (!ok_shape(critic, true) || !ok_shape(actor, false))
        return fail(TT_EINVAL, "%s: the critic's or the actor's weights are missing or not 23-400-300", who);
    if (!to_saved(saved_critic, R.sc) || !to_saved(saved_actor, R.sa)) return fail(TT_EINVAL, "%s: a saved forward lacks an array", who);
    if (!to_bwd_out(ws_critic, R.oc) || !to_bwd_out(ws_actor, R.oa)) return fail(TT_EINVAL, "%s: a per-row workspace lacks an array", who);
    if (R.oc.dx2 == R.oa.dx2) return fail(TT_EINVAL, "%s: ws_critic and ws_actor are the same workspace", who);
    if (!to_td(tdi, R.td)) return fail(TT_EINVAL, "%s: the TD input lacks an array or the target critic", who);
    R.Wc = to_weights(critic);
    R.Wa = to_weights(actor);
    R.grid = dim3(2 * ((n + TR - 1) / TR) + 1 + (R.img.on ? IMAGE_WGS : 0));
    return TT_OK;
}

// k_bwd_weights<..>, k_bwd_weights_shaped: A stays off with count = 0 (gradients only).  rows_required: the launch has no form without
// row factors; otherwise row_dq_da and row_mu come together or not at all, and only with them is n bounded by the kernel's table of factors.
struct WeightsLaunch { Saved sv; BwdOut o; Grads G; AdamFused A; RowScale rs; };

int to_weights_launch(const char *who, bool rows_required, int n, int critic, const float *obs, const tt_mlp_saved *saved,
                      const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, const float *row_dq_da, const float *row_mu, float row_scale,
                      int count, float *const *params, float *const *exp_avg, float *const *exp_avg_sq, float *const *targets,
                      const int64_t *step_dev, float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                      const tt_fc2_images *images, const float *bias_corr, WeightsLaunch &L) {
    if (rows_required ? !row_dq_da || !row_mu : (row_dq_da == nullptr) != (row_mu == nullptr))
        return fail(TT_EINVAL, "%s: row_dq_da or row_mu is NULL (the actor with row factors only)", who);
    const int max_n = row_dq_da ? MAXB : INT_MAX;
    if (n <= 0 || n > max_n) return fail(TT_EINVAL, "%s: n = %d rows, not in [1, %d]", who, n, max_n);
    if (!obs) return fail(TT_EINVAL, "%s: obs is NULL", who);
    if (!to_saved(saved, L.sv)) return fail(TT_EINVAL, "%s: the saved forward lacks an array", who);
    if (!to_bwd_out(ws, L.o)) return fail(TT_EINVAL, "%s: the per-row workspace lacks an array", who);
    if (!ok_shape(grads, critic != 0)) return fail(TT_EINVAL, "%s: grads is missing or not 23-400-300", who);
    const int tensors = critic ? 12 : 10;
    if (count != 0 && count != tensors) return fail(TT_EINVAL, "%s: count = %d tensors, not 0 or %d", who, count, tensors);
    L.A = AdamFused{};
    if (count && !to_adam(critic != 0, count, params, exp_avg, exp_avg_sq, targets, step_dev, lr, beta1, beta2, eps, weight_decay, tau,
                          images, bias_corr, L.A))
        return fail(TT_EINVAL, "%s: the optimizer step lacks a tensor or the step count", who);
    L.G = to_grads(grads);
    L.rs = RowScale{row_dq_da, row_mu, row_scale};
    return TT_OK;
}

// k_actor_tail[_shaped, _demo<..>]: the kernel's arguments from Wc on (without q_out and dq_da, which the caller holds) and the grid.
// tail_words: [0, 64) the row workgroups' hints, [64, 64 + 2 n) the rows' 8-byte words, which one wave polls.
struct Tail { Weights Wc; Saved sv; BwdOut o; Grads G; AdamFused A; RowScale rs; TailSync ts; dim3 grid; };

int to_actor_tail(const char *who, int n, const float *obs, const float *mu, const tt_mlp_weights *critic, const float *q_out,
                  const float *dq_da, const tt_mlp_saved *saved, const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, float row_scale,
                  int count, float *const *params, float *const *exp_avg, float *const *exp_avg_sq, float *const *targets,
                  const int64_t *step_dev, float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                  const tt_fc2_images *images, const float *bias_corr, int32_t *tail_words, int32_t *gave_up_host, Tail &T) {
    if (n <= 0 || n > MAXB) return fail(TT_EINVAL, "%s: n = %d rows, not in [1, %d]", who, n, MAXB);
    if (!obs || !mu || !q_out || !dq_da) return fail(TT_EINVAL, "%s: obs, mu, q_out or dq_da is NULL", who);
    if (!ok_shape(critic, true)) return fail(TT_EINVAL, "%s: the critic's weights are missing or not 23-400-300", who);
    if (!to_saved(saved, T.sv)) return fail(TT_EINVAL, "%s: the saved forward lacks an array", who);
    if (!to_bwd_out(ws, T.o)) return fail(TT_EINVAL, "%s: the per-row workspace lacks an array", who);
    if (!ok_shape(grads, false)) return fail(TT_EINVAL, "%s: grads is missing or not 23-400-300", who);
    if (!to_adam(false, count, params, exp_avg, exp_avg_sq, targets, step_dev, lr, beta1, beta2, eps, weight_decay, tau, images, bias_corr, T.A))
        return fail(TT_EINVAL, "%s: the optimizer step lacks a tensor or the step count, or count = %d is not 10", who, count);
    if (!tail_words) return fail(TT_EINVAL, "%s: tail_words is NULL", who);
    const int nb = (n + TR - 1) / TR;
    if (nb > 64) return fail(TT_EINVAL, "%s: %d row workgroups, more than the 64 one wave polls", who, nb);
    T.Wc = to_weights(critic);
    T.G = to_grads(grads);
    T.rs = RowScale{dq_da, mu, row_scale};      // (the tail's factors come from the rows' words; the demo form never reads dq_da here)
    T.ts = TailSync{tail_words, reinterpret_cast<unsigned long long *>(tail_words + 64), nb, gave_up_host};
    T.grid = dim3(nb + WG_ACTOR_WEIGHTS);
    return TT_OK;
}

// The table of the optimizer launches of their own (k_adam_soft, k_adam_soft_p2p, k_adam_soft_clip): the tensors, the fc2 images and
// each tensor's first workgroup at `per_block` elements per workgroup.  grads NULL: the peer-to-peer step, whose gradients come from
// the exchange.  Returns the launch's workgroups, or -1 for a missing or empty tensor or images that do not go with the list.
int fill_adam_table(AdamTable &T, int per_block, int count, float *const *params, const float *const *grads, float *const *exp_avg,
                    float *const *exp_avg_sq, float *const *targets, const int32_t *numel, const tt_fc2_images *images) {
    if (images && (images->net || images->target)) {       // tensors must then be in tt_mlp_weights order: w2 is number 4
        if (count < 5 || numel[4] != H2 * H1) return -1;
        T.img_p = reinterpret_cast<_Float16 *>(images->net);
        T.img_t = reinterpret_cast<_Float16 *>(images->target);
    }
    T.count = count;
    int blocks = 0;
    for (int i = 0; i < count; ++i) {
        if (!params[i] || (grads && !grads[i]) || !exp_avg[i] || !exp_avg_sq[i] || numel[i] <= 0) return -1;
        T.p[i] = params[i]; T.g[i] = grads ? grads[i] : nullptr; T.m[i] = exp_avg[i]; T.v[i] = exp_avg_sq[i];
        T.tgt[i] = targets ? targets[i] : nullptr;
        T.numel[i] = numel[i];
        T.block_start[i] = blocks;
        blocks += (numel[i] + per_block - 1) / per_block;
    }
    T.block_start[count] = blocks;
    return blocks;
}

}  // namespace
