// tttd3.h -- what TD3's translation units (csrc/tttd3.hip: one agent; csrc/ttpop_td3.hip: a population) share: the per-agent
// descriptor, the TD3 prologue of a critic's row workgroup and the host checks that fill a descriptor.  Everything is in an anonymous
// namespace, as everything of ttlearn_bodies.h and ttpop.h is: each translation unit has its own copy, and the kernels keep their names.
#pragma once
#include "tthost.h"
#include "ttlearn_bodies.h"

#include <cmath>
#include <cstdio>

namespace {

using tthost::fail;

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

bool finite_nonneg(const float x) { return std::isfinite(x) && x >= 0.f; }

// tt_td3_agent -> Td3Agent (host checks only: no HIP call).  a: the agent's index in a population, whose messages name it
// ("tt_pop_td3_create: agent <a>: ..."); a < 0: the lone agent of tt_td3_create, whose messages are "tt_td3_create: ...".
int to_td3_agent(const tt_td3_agent &g, const int a, const int n, Td3Agent &P) {
    char at[64];        // what every message starts with (a "%s" argument, never a format)
    if (a < 0) snprintf(at, sizeof at, "tt_td3_create");
    else snprintf(at, sizeof at, "tt_pop_td3_create: agent %d", a);
    P = Td3Agent{};
    P.n = n;
    if (!finite_nonneg(g.target_noise)) return fail(TT_EINVAL, "%s: target_noise = %g is negative or not finite", at, (double)g.target_noise);
    if (!finite_nonneg(g.noise_clip)) return fail(TT_EINVAL, "%s: noise_clip = %g is negative or not finite", at, (double)g.noise_clip);
    const tt_sample_args *smp = g.sample;
    if (!smp) return fail(TT_EINVAL, "%s: sample (tt_sample_args) is NULL", at);
    if (smp->batch != n) return fail(TT_EINVAL, "%s: the sample draws batches of %d rows, not batch = %d", at, smp->batch, n);
    if (smp->step_progress || smp->draws > 1) return fail(TT_EINVAL, "%s: step_progress / draws > 1 in the sample are not supported", at);
    if (smp->side && smp->side->count > 0) return fail(TT_EINVAL, "%s: the sample has a side buffer (not supported)", at);
    if (ttnet::make_ring_sample(smp, P.R) != TT_OK) return fail(TT_EINVAL, "%s: bad tt_sample_args", at);
    P.R.seed_stride = smp->seed_stride;
    const tt_fwd_job *jobs = g.jobs;
    if (!jobs) return fail(TT_EINVAL, "%s: jobs is NULL", at);
    // the six forwards, in their order: target actor on s', both target critics' state branches on s', Q1(s, a), Q2(s, a), mu(s)
    bool shape = !jobs[0].critic && jobs[0].obs == smp->s2_out && !jobs[5].critic && jobs[5].obs == smp->s_out && jobs[5].saved;
    for (int i = 1; i <= 2; ++i) shape = shape && jobs[i].critic && jobs[i].obs == smp->s2_out && jobs[i].z_state;
    for (int i = 3; i <= 4; ++i) shape = shape && jobs[i].critic && jobs[i].obs == smp->s_out && jobs[i].action == smp->a_out && jobs[i].saved;
    if (!shape) return fail(TT_EINVAL, "%s: the jobs are not TD3's six forwards on the draw", at);
    P.write_s = P.write_s2 = -1;
    for (int i = 0; i < 6; ++i) {
        FwdJobs one{};
        one.write_s = one.write_s2 = 0;
        if (!to_fwd_job(jobs[i], 0, smp, one))
            return fail(TT_EINVAL, "%s: forward job %d is incomplete or has an action other than the draw's a on s", at, i);
        P.j[i] = one.j[0];
        if (jobs[i].obs == smp->s_out && P.write_s < 0) P.write_s = i;
        if (jobs[i].obs == smp->s2_out && P.write_s2 < 0) P.write_s2 = i;
    }
    if (!jobs[0].out || !jobs[3].out || !jobs[4].out || !jobs[5].out)
        return fail(TT_EINVAL, "%s: mu'(s'), Q1(s, a), Q2(s, a) and mu(s) need outputs", at);
    P.scale_c = (float)(2.0 / n);
    P.q_out[0] = jobs[3].out; P.q_out[1] = jobs[4].out; P.mu_out = jobs[5].out;
    P.Wc[0] = P.j[3].W; P.Wc[1] = P.j[4].W; P.Wa = P.j[5].W;
    P.sv_c[0] = P.j[3].sv; P.sv_c[1] = P.j[4].sv; P.sv_a = P.j[5].sv;
    const tt_td_input *tdi = g.td;
    TdIn td{};
    if (!to_td(tdi, td) || !tdi->step_dev || !tdi->q_out || !tdi->bias_corr_out)
        return fail(TT_EINVAL, "%s: bad tt_td_input (arrays, q_out, a step counter and bias_corr_out are required)", at);
    if (tdi->window_dev) return fail(TT_EINVAL, "%s: window_dev is set (the pipelined order is not supported)", at);
    if (!g.z_state_2 || !ok_shape(g.target_critic_2, true)) return fail(TT_EINVAL, "%s: z_state_2 or target_critic_2 is missing", at);
    if (!g.eps_out || !g.y2_out || !g.q2t_out) return fail(TT_EINVAL, "%s: eps_out, y2_out and q2t_out are required", at);
    if (!g.step_snapshot || !g.actor_step_dev || !g.actor_bias_corr_out)
        return fail(TT_EINVAL, "%s: step_snapshot, actor_step_dev and actor_bias_corr_out are required", at);
    if (!g.q_pi || !g.dq_da || !g.tail_words) return fail(TT_EINVAL, "%s: q_pi, dq_da and tail_words are required", at);
    // the parts of the description belong together: the prologue reads what the forwards and the draw of the SAME update leave
    if (tdi->z_state != jobs[1].z_state || g.z_state_2 != jobs[2].z_state)
        return fail(TT_EINVAL, "%s: td->z_state / z_state_2 are not the z_state outputs of forward jobs 1 and 2", at);
    if (tdi->mu_target != jobs[0].out) return fail(TT_EINVAL, "%s: td->mu_target is not the output of forward job 0 (the target actor)", at);
    if (tdi->reward != smp->r_out || tdi->done != smp->d_out)
        return fail(TT_EINVAL, "%s: td->reward / td->done are not the draw's r_out / d_out", at);
    if (tdi->target_critic != jobs[1].w || g.target_critic_2 != jobs[2].w)
        return fail(TT_EINVAL, "%s: td->target_critic / target_critic_2 are not the networks of forward jobs 1 and 2", at);
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
        return fail(TT_EINVAL, "%s: a per-row workspace (tt_mlp_bwd_ws) is incomplete", at);
    if (P.o_c[0].dx2 == P.o_c[1].dx2 || P.o_c[0].dx2 == P.o_a.dx2 || P.o_c[1].dx2 == P.o_a.dx2)
        return fail(TT_EINVAL, "%s: two networks share a per-row workspace", at);
    for (int net = 0; net < 3; ++net) {
        const tt_pop_net &t = net == 0 ? g.critic : net == 1 ? g.critic_2 : g.actor;
        const bool critic = net < 2;
        if (!ok_shape(t.grads, critic)) return fail(TT_EINVAL, "%s: network %d has no gradient buffers", at, net);
        if (critic) {
            for (int v = 0; v < 2; ++v)
                if (!to_adam(true, t.count, t.params, t.exp_avg, t.exp_avg_sq, t.targets, tdi->step_dev, t.lr, t.beta1, t.beta2, t.eps,
                             t.weight_decay, v == 0 ? t.tau : 0.f, t.images, tdi->bias_corr_out, P.Ac[net][v]))
                    return fail(TT_EINVAL, "%s: network %d has an incomplete optimizer step", at, net);
            P.Gc[net] = to_grads(t.grads);
        } else {
            if (!to_adam(false, t.count, t.params, t.exp_avg, t.exp_avg_sq, t.targets, g.actor_step_dev, t.lr, t.beta1, t.beta2, t.eps,
                         t.weight_decay, t.tau, t.images, g.actor_bias_corr_out, P.Aa))
                return fail(TT_EINVAL, "%s: network %d has an incomplete optimizer step", at, net);
            P.Ga = to_grads(t.grads);
        }
    }
    if (g.critic.grads->w1 == g.critic_2.grads->w1) return fail(TT_EINVAL, "%s: the two critics share a gradient buffer", at);
    P.q_pi = g.q_pi;
    P.dq_da = g.dq_da;
    P.RSa = RowScale{g.dq_da, P.mu_out, (float)(-1.0 / n)};
    P.ts = TailSync{g.tail_words, reinterpret_cast<unsigned long long *>(g.tail_words + 64), (n + TR - 1) / TR, g.gave_up_host};
    return TT_OK;
}

}  // namespace
