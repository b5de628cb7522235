// ttdemo.hip -- the demonstration loss of the lone learn(): a behaviour-cloning term on the batch rows that came from the replay
// side buffer, gated by a Q-filter, inside the launches learn() makes anyway (MI355X, gfx950; include/ttenv.h: tt_demo_loss;
// DESIGN.md section 25).
//
//   k_fwd_small_demo      k_fwd_small<critic>'s launch of the five-launch chain: Q(s, mu(s)) and dQ/da through the UPDATED critic.
//                         Lane 0 of a row also forms m[b] = demonstration row [and q[b] > q_pi[b]] and the EFFECTIVE derivative
//                         dq_eff[b] = m ? fmaf(-k, mu[b] - a[b], dQ/da[b]) : dQ/da[b], k = 2 lambda; dq_da keeps the true one.
//   k_actor_tail_demo     k_actor_tail's grid: the row half with the same term -- the 8-byte hand-over word carries dq_eff --, the
//                         weight half word for word what it is (PREPEN = a learner with a LossShape).  No wait, flag or atomic added.
//
// The actor's row factor (scale dQ/da)(1 - mu^2), scale = -1/B, is linear in dQ/da, and the cloning term's derivative at the
// pre-activation is (2 lambda / B) m (mu - a)(1 - mu^2): the whole term is the factor of dq_eff.  The separate weight launch needs no
// kernel of its own: tt_mlp_backward_weights[_shaped] with row_dq_da = dq_eff.  The body is fwd_small_body<true, .., DEMO>
// (ttlearn_bodies.h), the tail's checks and conversion those of every tail (ttlearn_host.h); other units' instantiations are unchanged.
// A row with m = 0 keeps the bits of dQ/da, so a batch without demonstration rows leaves the bits of the launches these stand in for.
// The _lanes entry points take expert_lanes by value -- tt_demo_loss keeps its layout -- and make a ring row of
// a lane < expert_lanes a demonstration row as well; the entry points without the count are those with 0, the same launches.
// The _labels entry points take a tt_demo_labels as well: a ring row of a labelled lane clones the ring's label
// (the expert's decision on the state the policy acted in) in place of the stored action, unfiltered, code 3; with NULL they are the
// _lanes entry points, the same launches.  The label's fields travel in DemoIn (no further kernel).
#include "ttlearn_host.h"

namespace {

__global__ __launch_bounds__(64 * NW) void k_fwd_small_demo(const int n, const float *__restrict__ obs, const float *__restrict__ action,
                                                            const float *__restrict__ w1e, const float *__restrict__ b1e,
                                                            const float *__restrict__ g1e, const float *__restrict__ be1e,
                                                            const Weights W, float *__restrict__ out, const Saved sv,
                                                            float *__restrict__ dq_da, const DemoIn demo) {
    // (n .. be1e: the preloaded prefix, as k_fwd_small's)
    __shared__ __attribute__((aligned(16))) float h1_s[H1S_FLOATS];
    __shared__ __attribute__((aligned(16))) float z_s[TR * DS];
    __shared__ __attribute__((aligned(16))) float w1_s[H1 * IN];
    KernargWarm<64 + (int)sizeof(Weights) + 8 + (int)sizeof(Saved) + 8 + (int)sizeof(DemoIn)> warm;
    warm.issue();
    KBEGIN(3);
    const EarlyW E{w1e, b1e, g1e, be1e};
    auto hook = [&]() __attribute__((always_inline)) { warm.wait(); };
    fwd_small_body<true, decltype(hook), true>(n, obs, action, W, out, sv, dq_da, nullptr, h1_s, z_s, w1_s, blockIdx.x * TR, nullptr, false,
                                               0.f, 0.f, nullptr, 0u, &E, hook, demo);
    KEND(3);
}

// k_actor_tail with the demonstration term in the dQ/da the row workgroups hand on; PREPEN: the learner also has a LossShape
template <bool PREPEN>
__global__ __launch_bounds__(64 * NW) void k_actor_tail_demo(const int n, const float *__restrict__ obs, const float *__restrict__ mu,
                                                             const Weights Wc, float *__restrict__ q_out, float *__restrict__ dq_da,
                                                             const Saved sv, const BwdOut d, const Grads G, const AdamFused A,
                                                             const RowScale RS, const TailSync ts, const float pre_scale,
                                                             const float *__restrict__ pre, const DemoIn demo) {
    __shared__ __attribute__((aligned(16))) float lds[H1S_FLOATS + TR * DS + H1 * IN];
    const int nb = (n + TR - 1) / TR;
    if ((int)blockIdx.x < nb) {
        const long long epoch = *A.step_dev;
        KBEGIN(3);
        TT_ACTOR_TAIL_ROWS_DEMO(true, n, obs, mu, Wc, q_out, dq_da, lds, ts, blockIdx.x, epoch, demo);
        KEND(3);
        return;
    }
    if (threadIdx.x >= 256) return;
    const long long epoch = *A.step_dev;
    TT_ACTOR_TAIL_WEIGHTS_SHAPED(PREPEN, (int)blockIdx.x - nb, n, obs, sv, d, G, A, RS, lds, ts, epoch, pre_scale, pre);
}

// what both entry points refuse of a tt_demo_loss: TT_OK, or TT_EINVAL with "<who>: <reason>"
int refuse_demo(const char *who, const tt_demo_loss *dl, const float *dq_da, const int32_t expert_lanes, const tt_demo_labels *lb,
                DemoIn &out) {
    if (!dl) return fail(TT_EINVAL, "%s: demo is NULL", who);
    if (expert_lanes < 0) return fail(TT_EINVAL, "%s: expert_lanes = %d is negative", who, (int)expert_lanes);
    if (!std::isfinite(dl->k) || dl->k < 0.f) return fail(TT_EINVAL, "%s: demo->k = %g is not a finite number >= 0", who, (double)dl->k);
    if (!dl->a || !dl->idx || !dl->dq_eff || !dl->code) return fail(TT_EINVAL, "%s: demo->a, idx, dq_eff or code is NULL", who);
    if (dl->q_filter && !dl->q) return fail(TT_EINVAL, "%s: demo->q is NULL with q_filter set", who);
    if (!dq_da) return fail(TT_EINVAL, "%s: dq_da is NULL (the true derivative has a buffer of its own)", who);
    if (dl->dq_eff == dq_da) return fail(TT_EINVAL, "%s: demo->dq_eff is dq_da", who);
    out = DemoIn{dl->a, dl->idx, dl->q, dl->k, dl->q_filter ? 1 : 0, dl->dq_eff, dl->code, (int)expert_lanes, 0, nullptr, 0, 0, 0};
    if (lb) {
        if (!lb->label) return fail(TT_EINVAL, "%s: labels->label is NULL", who);
        if (lb->n_envs < 1 || lb->slots < 1)
            return fail(TT_EINVAL, "%s: labels of %d envs and %d slots, not >= 1 each", who, (int)lb->n_envs, (int)lb->slots);
        if (lb->first < 0) return fail(TT_EINVAL, "%s: labels->first = %d is negative", who, (int)lb->first);
        if (lb->count < 1) return fail(TT_EINVAL, "%s: labels->count = %d, not >= 1", who, (int)lb->count);
        if ((int64_t)lb->first + (int64_t)lb->count > (int64_t)lb->n_envs)
            return fail(TT_EINVAL, "%s: labelled lanes [%d, %d + %d) leave the %d envs", who, (int)lb->first, (int)lb->first, (int)lb->count,
                        (int)lb->n_envs);
        if (lb->first < expert_lanes)
            return fail(TT_EINVAL, "%s: labels->first = %d overlaps the %d expert lanes", who, (int)lb->first, (int)expert_lanes);
        out.label_first = lb->first; out.label = lb->label; out.label_n = lb->n_envs; out.label_slots = lb->slots; out.label_count = lb->count;
    }
    return TT_OK;
}

}  // namespace

extern "C" {

// both forms of the forward: `who` names the entry point in every refusal
static int forward_save_demo(const char *who, int n, int critic, const float *obs, const float *action, const tt_mlp_weights *w, float *out,
                             const tt_mlp_saved *saved, float *dq_da, const tt_demo_loss *demo, int32_t expert_lanes,
                             const tt_demo_labels *labels, tt_stream_t stream) {
    DemoIn din;
    if (const int rc = refuse_demo(who, demo, dq_da, expert_lanes, labels, din)) return rc;
    if (!critic) return fail(TT_EINVAL, "%s: the actor has no demonstration form (the term is in the critic's pass on (s, mu(s)))", who);
    if (n < 0) return fail(TT_EINVAL, "%s: n = %d rows, not >= 0", who, n);
    if (!obs || !out || !action) return fail(TT_EINVAL, "%s: obs, action or out is NULL", who);
    if (!ok_shape(w, true)) return fail(TT_EINVAL, "%s: the critic's weights are missing or not 23-400-300", who);
    Saved sv{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (saved && !to_saved(saved, sv)) return fail(TT_EINVAL, "%s: the saved forward lacks an array", who);
    if (n == 0) return TT_OK;
    hipLaunchKernelGGL(k_fwd_small_demo, dim3((n + TR - 1) / TR), dim3(64 * NW), 0, stream, n, obs, action, w->w1, w->b1, w->g1, w->be1,
                       to_weights(w), out, sv, dq_da, din);
    return launched(who);
}

int tt_mlp_forward_save_demo(int n, int critic, const float *obs, const float *action, const tt_mlp_weights *w, float *out,
                             const tt_mlp_saved *saved, float *dq_da, const tt_demo_loss *demo, tt_stream_t stream) {
    return forward_save_demo("tt_mlp_forward_save_demo", n, critic, obs, action, w, out, saved, dq_da, demo, 0, nullptr, stream);
}

int tt_mlp_forward_save_demo_lanes(int n, int critic, const float *obs, const float *action, const tt_mlp_weights *w, float *out,
                                   const tt_mlp_saved *saved, float *dq_da, const tt_demo_loss *demo, int32_t expert_lanes,
                                   tt_stream_t stream) {
    return forward_save_demo("tt_mlp_forward_save_demo_lanes", n, critic, obs, action, w, out, saved, dq_da, demo, expert_lanes, nullptr,
                             stream);
}

int tt_mlp_forward_save_demo_labels(int n, int critic, const float *obs, const float *action, const tt_mlp_weights *w, float *out,
                                    const tt_mlp_saved *saved, float *dq_da, const tt_demo_loss *demo, int32_t expert_lanes,
                                    const tt_demo_labels *labels, tt_stream_t stream) {
    return forward_save_demo("tt_mlp_forward_save_demo_labels", n, critic, obs, action, w, out, saved, dq_da, demo, expert_lanes, labels,
                             stream);
}

static int actor_tail_demo(const char *who, int n, const float *obs, const float *mu, const tt_mlp_weights *critic, float *q_out,
                           float *dq_da, const tt_mlp_saved *saved, const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, float row_scale,
                           int count, float *const *params, float *const *exp_avg, float *const *exp_avg_sq, float *const *targets,
                           const int64_t *step_dev, float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                           const tt_fc2_images *images, const float *bias_corr, int32_t *tail_words, int32_t *gave_up_host,
                           const tt_loss_shape *shape, const tt_demo_loss *demo, int32_t expert_lanes, const tt_demo_labels *labels,
                           tt_stream_t stream) {
    DemoIn din;
    if (const int rc = refuse_demo(who, demo, dq_da, expert_lanes, labels, din)) return rc;
    if (shape)
        if (const int rc = refuse_shape(who, shape)) return rc;
    Tail T;
    if (const int rc = to_actor_tail(who, n, obs, mu, critic, q_out, dq_da, saved, ws, grads, row_scale, count, params, exp_avg, exp_avg_sq,
                                     targets, step_dev, lr, beta1, beta2, eps, weight_decay, tau, images, bias_corr, tail_words, gave_up_host, T))
        return rc;
    hipLaunchKernelGGL(shape ? k_actor_tail_demo<true> : k_actor_tail_demo<false>, T.grid, dim3(64 * NW), 0, stream, n, obs, mu, T.Wc, q_out,
                       dq_da, T.sv, T.o, T.G, T.A, T.rs, T.ts, shape ? shape->pre_scale : 0.f,
                       shape ? static_cast<const float *>(shape->pre) : nullptr, din);
    return launched(who);
}

int tt_mlp_actor_tail_demo(int n, const float *obs, const float *mu, const tt_mlp_weights *critic, float *q_out, float *dq_da,
                           const tt_mlp_saved *saved, const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, float row_scale, int count,
                           float *const *params, float *const *exp_avg, float *const *exp_avg_sq, float *const *targets,
                           const int64_t *step_dev, float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                           const tt_fc2_images *images, const float *bias_corr, int32_t *tail_words, int32_t *gave_up_host,
                           const tt_loss_shape *shape, const tt_demo_loss *demo, tt_stream_t stream) {
    return actor_tail_demo("tt_mlp_actor_tail_demo", n, obs, mu, critic, q_out, dq_da, saved, ws, grads, row_scale, count, params, exp_avg,
                           exp_avg_sq, targets, step_dev, lr, beta1, beta2, eps, weight_decay, tau, images, bias_corr, tail_words,
                           gave_up_host, shape, demo, 0, nullptr, stream);
}

int tt_mlp_actor_tail_demo_lanes(int n, const float *obs, const float *mu, const tt_mlp_weights *critic, float *q_out, float *dq_da,
                                 const tt_mlp_saved *saved, const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, float row_scale,
                                 int count, float *const *params, float *const *exp_avg, float *const *exp_avg_sq,
                                 float *const *targets, const int64_t *step_dev, float lr, float beta1, float beta2, float eps,
                                 float weight_decay, float tau, const tt_fc2_images *images, const float *bias_corr,
                                 int32_t *tail_words, int32_t *gave_up_host, const tt_loss_shape *shape, const tt_demo_loss *demo,
                                 int32_t expert_lanes, tt_stream_t stream) {
    return actor_tail_demo("tt_mlp_actor_tail_demo_lanes", n, obs, mu, critic, q_out, dq_da, saved, ws, grads, row_scale, count, params,
                           exp_avg, exp_avg_sq, targets, step_dev, lr, beta1, beta2, eps, weight_decay, tau, images, bias_corr, tail_words,
                           gave_up_host, shape, demo, expert_lanes, nullptr, stream);
}

int tt_mlp_actor_tail_demo_labels(int n, const float *obs, const float *mu, const tt_mlp_weights *critic, float *q_out, float *dq_da,
                                  const tt_mlp_saved *saved, const tt_mlp_bwd_ws *ws, const tt_mlp_weights *grads, float row_scale,
                                  int count, float *const *params, float *const *exp_avg, float *const *exp_avg_sq,
                                  float *const *targets, const int64_t *step_dev, float lr, float beta1, float beta2, float eps,
                                  float weight_decay, float tau, const tt_fc2_images *images, const float *bias_corr,
                                  int32_t *tail_words, int32_t *gave_up_host, const tt_loss_shape *shape, const tt_demo_loss *demo,
                                  int32_t expert_lanes, const tt_demo_labels *labels, tt_stream_t stream) {
    return actor_tail_demo("tt_mlp_actor_tail_demo_labels", n, obs, mu, critic, q_out, dq_da, saved, ws, grads, row_scale, count, params,
                           exp_avg, exp_avg_sq, targets, step_dev, lr, beta1, beta2, eps, weight_decay, tau, images, bias_corr, tail_words,
                           gave_up_host, shape, demo, expert_lanes, labels, stream);
}

}  // extern "C"
