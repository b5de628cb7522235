// ttpop.hip -- learn() of a POPULATION of K independent DDPG agents in the four launches of one agent's learn() (MI355X, gfx950).
//
// Agent a of a population is a lone serial-order loop of its own (its env, replay ring, OU noise, policy launch and env step); only
// its learn() launches are shared: each launch below runs the workgroups of all K agents, and a workgroup finds its agent and its
// block within the agent's grid from blockIdx.x.  The bodies are those of ttlearn_bodies.h, called with the arguments the lone
// launches of ttlearn.hip pass:
//
//   k_pop_fwd_multi            k_fwd_multi, sampled: agent a's draw from agent a's ring (seed + u * seed_stride), its four forwards
//   k_pop_bwd_rows_pair        k_bwd_rows_pair: TD prologue, critic rows, actor unit rows, the counter workgroup
//   k_pop_bwd_weights<false>   k_bwd_weights<false> on the critic: gradients + Adam + soft update + fc2 image patch
//   k_pop_actor_tail           k_actor_tail: Q(s, mu(s)) and dQ/da rows, then the actor's weight gradients + Adam
//
// and, off the learn() path, k_pop_exploit (tt_pop_exploit): population-based training's exploit/explore step between vector steps.
// With per-agent n-step returns (tt_pop_learn_set_nstep) the first launch is k_pop_fwd_multi_nstep of csrc/ttpop_nstep.hip instead;
// the other three are the same, an agent's td.gamma then holding its discount gamma ** n.
// With per-agent gradient-norm clipping (tt_pop_learn_set_clip) the descriptors' optimizers are off: the critic's weight launch and
// the actor tail leave gradients only, and each is followed by k_pop_grad_sqnorm and k_pop_adam_soft_clip of csrc/ttclip.hip --
// eight launches.  No kernel of this file changes for it.
//
// So each agent's results are the bits of its lone learn() (tests/test_gpu_population.py).  Per-agent arguments live in device
// memory (PopAgent), filled once at tt_pop_learn_create: a launch takes (K, B, descriptors, u) and is graph-capturable.
// The descriptors are read through the CONSTANT address space, as kernel arguments are: the bodies index the Adam tables with a
// run-time tensor number (an array copied into registers would go to scratch), and constant loads are scalar loads that the
// compiler may issue as early as it likes (nothing in a launch writes them).
#include "tthost.h"
#include "ttpop.h"
#include "ttpop_exploit.h"

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <vector>

using tthost::fail;

namespace {

// grid: K x 4 x nb, agent-major; within an agent, job-major as k_fwd_multi
__global__ __launch_bounds__(64 * NW) void k_pop_fwd_multi(const int K, const int n, const PopAgent *__restrict__ D, const int u) {
    __shared__ __attribute__((aligned(16))) float h1_s[H1S_FLOATS];
    __shared__ __attribute__((aligned(16))) float z_s[TR * DS];
    __shared__ __attribute__((aligned(16))) float w1_s[H1 * IN];
    const int nb = (n + TR - 1) / TR, ag = (int)blockIdx.x / (4 * nb);
    if (ag >= K) return;
    const int lb = (int)blockIdx.x - ag * 4 * nb, job = lb / nb, row0 = (lb - job * nb) * TR;
    const PopAgent &P = agent_of(D, ag);
    const FwdJob &q = P.F.j[job];
    ttnet::RingSample R = P.F.R;
    R.seed += (unsigned long long)u * R.seed_stride;        // DDPGRollout._sample_key(u)
    const float *orow;
    bool have_act = false;
    float act_r0 = 0.f, act_r1 = 0.f;
    TT_SAMPLED_ROWS(R, n, row0, q, job, P.F.write_s, P.F.write_s2, orow, have_act, act_r0, act_r1);
    if (q.critic)
        fwd_small_body<true>(n, q.obs, q.action, q.W, q.out, q.sv, q.dq_da, q.z_state, h1_s, z_s, w1_s, row0, orow, have_act, act_r0, act_r1);
    else
        fwd_small_body<false>(n, q.obs, q.action, q.W, q.out, q.sv, nullptr, nullptr, h1_s, z_s, w1_s, row0, orow);
}

// grid: K x (2 nb + 1), agent-major: critic rows, actor unit rows, the counter workgroup (k_bwd_rows_pair without the image rider)
__global__ __launch_bounds__(64 * NW) void k_pop_bwd_rows_pair(const int K, const int n, const PopAgent *__restrict__ D) {
    __shared__ __attribute__((aligned(16))) float dx2_s[DXS_FLOATS];
    __shared__ float red[2 * NW * TR];
    __shared__ float rsc_s[TR];
    const int nb = (n + TR - 1) / TR, ag = (int)blockIdx.x / (2 * nb + 1);
    if (ag >= K) return;
    const int lb = (int)blockIdx.x - ag * (2 * nb + 1);
    const PopAgent &P = agent_of(D, ag);
    if (lb == 2 * nb) {
        if (threadIdx.x == 0) clock_tick(P.td);
        return;
    }
    if (lb < nb)
        bwd_rows_body<true>(n, P.scale_c, P.q_out, P.Wc, P.sv_c, P.o_c, P.td, dx2_s, red, rsc_s, lb * TR);
    else
        bwd_rows_body<false>(n, 0.f, nullptr, P.Wa, P.sv_a, P.o_a, TdIn{}, dx2_s, red, rsc_s, (lb - nb) * TR);
}

// grid: K x 210, agent-major: the critic's weight gradients with its optimizer step
template <bool ROWSCALE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k_pop_bwd_weights(const int K, const int n,
                                                                                             const PopAgent *__restrict__ D) {
    __shared__ __attribute__((aligned(16))) float part[4][4][256];
    __shared__ float f_s[ROWSCALE ? MAXB : 1];
    __shared__ __attribute__((aligned(16))) _Float16 stage_s[4 * 1024];
    const int ag = (int)blockIdx.x / WG_CRITIC_WEIGHTS;
    if (ag >= K) return;
    const PopAgent &P = agent_of(D, ag);
    bwd_weights_body<ROWSCALE, false>((int)blockIdx.x - ag * WG_CRITIC_WEIGHTS, n, 1, P.s, P.a, P.sv_c, P.o_c, P.Gc, P.Ac,
                                      RowScale{nullptr, nullptr, 1.f}, part, f_s, TailSync{nullptr, nullptr, 0, nullptr}, 0, stage_s);
}

// grid: K x nb row workgroups FIRST (every agent's), then K x 200 weight workgroups.  A weight workgroup waits in device memory for
// its agent's rows (TailSync), so every producer it may wait for is dispatched before any waiting workgroup: the row workgroups
// never queue for a CU behind workgroups that wait for them.  Each agent keeps its own tail words, and its epoch is its own step.
__global__ __launch_bounds__(64 * NW) void k_pop_actor_tail(const int K, const int n, const PopAgent *__restrict__ D) {
    __shared__ __attribute__((aligned(16))) float lds[H1S_FLOATS + TR * DS + H1 * IN];
    const int nb = (n + TR - 1) / TR, rows = K * nb;
    if ((int)blockIdx.x < rows) {
        const int ag = (int)blockIdx.x / nb, lb = (int)blockIdx.x - ag * nb;
        const PopAgent &P = agent_of(D, ag);
        const long long epoch = *P.Aa.step_dev;
        TT_ACTOR_TAIL_ROWS(n, P.s, P.mu_out, P.Wc, P.q_pi, P.dq_da, lds, P.ts, lb, epoch);
        return;
    }
    const int ag = ((int)blockIdx.x - rows) / WG_ACTOR_WEIGHTS;
    if (threadIdx.x >= 256 || ag >= K) return;
    const PopAgent &P = agent_of(D, ag);
    const long long epoch = *P.Aa.step_dev;
    TT_ACTOR_TAIL_WEIGHTS((int)blockIdx.x - rows - ag * WG_ACTOR_WEIGHTS, n, P.s, P.sv_a, P.o_a, P.Ga, P.Aa, P.RSa, lds, P.ts, epoch);
}

// ---- PBT exploit/explore (tt_pop_exploit): dst's learning state <- src's, then dst's hyperparameters, in one launch ----
// A pair's copy is 92 regions: per network (critic 12 tensors, then actor 10) and tensor t, its parameters, Adam m, Adam v and
// target parameters (4 t + {0, 1, 2, 3}), then the four fc2 images (critic net / target, actor net / target).  Each region is cut
// into EX_CHUNK-byte pieces, one workgroup each (csrc/ttpop_exploit.h: the piece copy, shared with k_pop_td3_exploit).
// Nothing else is copied: dst's env, ring, noise, step_dev, bias corrections, tail words and scratch buffers stay its own.
struct ExploitList {
    int n;
    tt_pop_exploit_pair p[TT_POP_MAX_AGENTS];
};

constexpr int EX_TENSOR_REGIONS = 4 * (12 + 10), EX_REGIONS = EX_TENSOR_REGIONS + 4;

__host__ __device__ constexpr size_t ex_region_bytes(const int r) {
    return r < EX_TENSOR_REGIONS ? (size_t)ex_numel((r < 48 ? r : r - 48) >> 2) * 4 : IMG_HALVES * 2;
}
__host__ __device__ constexpr int ex_region_chunks(const int r) { return ex_chunks(ex_region_bytes(r)); }
constexpr int ex_chunks_per_pair() {
    int s = 0;
    for (int r = 0; r < EX_REGIONS; ++r) s += ex_region_chunks(r);
    return s;
}
constexpr int EX_CHUNKS = ex_chunks_per_pair();

// grid: pairs x EX_CHUNKS, pair-major.  No pair's dst is another pair's src (tt_pop_exploit checks), so every byte a workgroup reads
// is written by no workgroup of the launch.  The descriptors' pointers are read, never written; the hyperparameter words are written
// with plain global stores and read by the later launches on the stream (the same contract as the copy at tt_pop_learn_create).
__global__ __launch_bounds__(EX_THREADS) void k_pop_exploit(const ExploitList L, PopAgent *__restrict__ D) {
    const int pair = (int)blockIdx.x / EX_CHUNKS, piece = (int)blockIdx.x - pair * EX_CHUNKS;
    if (pair >= L.n) return;
    const tt_pop_exploit_pair q = L.p[pair];
    if (piece == 0 && threadIdx.x == 0) {
        PopAgent &W = D[q.dst];
        W.Aa.lr = q.alpha;
        W.Ac.lr = q.beta;
        W.Aa.tau = q.tau;
        W.Ac.tau = q.tau;
        W.td.gamma = q.gamma;
    }
    if (q.dst == q.src) return;
    int r = 0, c = piece;
    while (r < EX_REGIONS - 1 && c >= ex_region_chunks(r)) c -= ex_region_chunks(r++);
    const PopAgent &S = agent_of(D, q.src), &T = agent_of(D, q.dst);
    const char *from;
    char *to;
    if (r < EX_TENSOR_REGIONS) {
        const bool actor = r >= 48;
        const int local = actor ? r - 48 : r, t = local >> 2, kind = local & 3;
        from = reinterpret_cast<const char *>(ex_tensor(actor ? S.Aa : S.Ac, kind, t));
        to = reinterpret_cast<char *>(ex_tensor(actor ? T.Aa : T.Ac, kind, t));
    } else {
        const int i = r - EX_TENSOR_REGIONS;
        const AdamFused &As = i < 2 ? S.Ac : S.Aa, &At = i < 2 ? T.Ac : T.Aa;
        from = reinterpret_cast<const char *>((i & 1) ? As.img_t : As.img_p);
        to = reinterpret_cast<char *>((i & 1) ? At.img_t : At.img_p);
    }
    if (!from || !to) return;                      // (images off)
    ex_copy_piece(from, to, ex_region_bytes(r), c);
}

// one agent's tt_pop_agent -> PopAgent (host checks only: no HIP call)
int to_pop_agent(const tt_pop_agent &g, const int a, const int n, PopAgent &P) {
    P = PopAgent{};
    const tt_sample_args *smp = g.sample;
    if (!smp) return fail(TT_EINVAL, "tt_pop_learn_create: agent %d has no sample (tt_sample_args)", a);
    if (smp->batch != n) return fail(TT_EINVAL, "tt_pop_learn_create: agent %d draws batches of %d rows, not the population's B", a, smp->batch);
    if (smp->step_progress || (smp->draws > 1)) return fail(TT_EINVAL, "tt_pop_learn_create: agent %d: step_progress / draws are not for populations", a);
    if (smp->side && smp->side->count > 0) return fail(TT_EINVAL, "tt_pop_learn_create: agent %d has a side buffer (not in populations)", a);
    if (ttnet::make_ring_sample(smp, P.F.R) != TT_OK) return fail(TT_EINVAL, "tt_pop_learn_create: agent %d: bad tt_sample_args", a);
    P.F.R.seed_stride = smp->seed_stride;
    P.F.n = n;
    P.F.blocks_per_job = (n + TR - 1) / TR;
    P.F.sampled = 1;
    P.F.write_s = P.F.write_s2 = -1;
    const tt_fwd_job *jobs = g.jobs;
    if (!jobs) return fail(TT_EINVAL, "tt_pop_learn_create: agent %d has no forward jobs", a);
    // the lone learn()'s four forwards, in their order: target actor on s', the target critic's state branch on s', Q(s, a), mu(s)
    if (jobs[0].critic || jobs[0].obs != smp->s2_out || !jobs[1].critic || jobs[1].obs != smp->s2_out || !jobs[1].z_state ||
        !jobs[2].critic || jobs[2].obs != smp->s_out || jobs[2].action != smp->a_out || !jobs[2].saved || jobs[3].critic ||
        jobs[3].obs != smp->s_out || !jobs[3].saved)
        return fail(TT_EINVAL, "tt_pop_learn_create: agent %d: the jobs are not learn()'s four forwards on its draw", a);
    for (int i = 0; i < 4; ++i)
        if (!to_fwd_job(jobs[i], i, smp, P.F))
            return fail(TT_EINVAL, "tt_pop_learn_create: agent %d: forward job %d is incomplete or has an action other than the draw's a on s", a, i);
    P.scale_c = (float)(2.0 / n);
    P.q_out = jobs[2].out;
    P.mu_out = jobs[3].out;
    P.Wc = P.F.j[2].W;
    P.Wa = P.F.j[3].W;
    P.sv_c = P.F.j[2].sv;
    P.sv_a = P.F.j[3].sv;
    if (!P.q_out || !P.mu_out) return fail(TT_EINVAL, "tt_pop_learn_create: agent %d: Q(s, a) and mu(s) need outputs", a);
    if (!to_bwd_out(g.critic.ws, P.o_c) || !to_bwd_out(g.actor.ws, P.o_a) || P.o_c.dx2 == P.o_a.dx2)
        return fail(TT_EINVAL, "tt_pop_learn_create: agent %d: the per-row workspaces (tt_mlp_bwd_ws) are incomplete or shared", a);
    const tt_td_input *tdi = g.td;
    if (!to_td(tdi, P.td) || !tdi->step_dev || tdi->window_dev)
        return fail(TT_EINVAL, "tt_pop_learn_create: agent %d: bad tt_td_input (a step counter is required, a window counter is not for populations)", a);
    P.s = smp->s_out;
    P.a = smp->a_out;
    for (int net = 0; net < 2; ++net) {
        const tt_pop_net &t = net ? g.actor : g.critic;
        const bool critic = net == 0;
        if (!ok_shape(t.grads, critic)) return fail(TT_EINVAL, "tt_pop_learn_create: agent %d: network %d has no gradient buffers", a, net);
        AdamFused &A = critic ? P.Ac : P.Aa;
        if (!to_adam(critic, t.count, t.params, t.exp_avg, t.exp_avg_sq, t.targets, tdi->step_dev, t.lr, t.beta1, t.beta2, t.eps,
                     t.weight_decay, t.tau, t.images, tdi->bias_corr_out, A))
            return fail(TT_EINVAL, "tt_pop_learn_create: agent %d: network %d has an incomplete optimizer step", a, net);
        (critic ? P.Gc : P.Ga) = to_grads(t.grads);
    }
    if (!g.q_pi || !g.dq_da || !g.tail_words) return fail(TT_EINVAL, "tt_pop_learn_create: agent %d: q_pi, dq_da and tail_words are required", a);
    P.q_pi = g.q_pi;
    P.dq_da = g.dq_da;
    P.RSa = RowScale{g.dq_da, P.mu_out, (float)(-1.0 / n)};
    P.ts = TailSync{g.tail_words, reinterpret_cast<unsigned long long *>(g.tail_words + 64), (n + TR - 1) / TR, g.gave_up_host};
    return TT_OK;
}


// the device address of agent P's td.gamma (its TD discount)
float *td_gamma_of(PopAgent *P) { return reinterpret_cast<float *>(reinterpret_cast<char *>(P) + offsetof(PopAgent, td) + offsetof(TdIn, gamma)); }

// what tt_pop_learn_set_nstep ("agent" i) and tt_pop_exploit_nstep ("pair" i) refuse in one tt_pop_nstep, for a ring of `slots`
// slots (host only: no HIP call)
int check_pop_nstep(const char *who, const char *what, const int i, const struct tt_pop_nstep &q, const int slots, const int reserve) {
    char at[200];       // "<who>: agent <i>", the name every message starts with (a "%s" argument, never a format)
    snprintf(at, sizeof at, "%s: %s %d", who, what, i);
    if (const int rc = tthost::refuse_nstep(at, q.n_step, q.gamma)) return rc;
    if (q.n_step == 1 && q.discount != q.gamma) return fail(TT_EINVAL, "%s: discount is not gamma although n_step is 1", at);
    if (q.n_step > 1 && !(q.discount > 0.f && q.discount < q.gamma))
        return fail(TT_EINVAL, "%s: discount is outside (0, gamma) although n_step > 1", at);
    return tthost::refuse_nstep_window(at, q.n_step, slots, reserve);
}

}  // namespace

struct tt_population {
    int K = 0, n = 0;
    PopAgent *dev = nullptr;
    PopNstep *table = nullptr;           // per-agent {n_step, gamma}: made by tt_pop_learn_set_nstep, then there for good
    std::vector<int> slots, reserve;     // each agent's ring, for the window check of a later n_step
    bool clipped = false;                // tt_pop_learn_set_clip was called: learn() is eight launches for good
    ttpop::ClipBufs clip{};              // the clip's tables and buffers (library-owned device memory)
};

// what tt_pop_learn_set_clip ("agent" a) and tt_pop_clip_write ("entry" i) refuse in one tt_pop_clip (host only: no HIP call)
static int check_pop_clip(const char *who, const char *what, const int i, const struct tt_pop_clip &q) {
    const float v[2] = {q.max_norm_critic, q.max_norm_actor};
    for (int net = 0; net < 2; ++net)
        if (!std::isfinite(v[net]) || v[net] < 0.f)
            return fail(TT_EINVAL, "%s: %s %d: max_norm_%s = %g is neither a finite number > 0 nor 0 (this network is not clipped)", who,
                        what, i, net ? "actor" : "critic", (double)v[net]);
    return TT_OK;
}

static void free_clip(ttpop::ClipBufs &c) {
    for (void *p : {c.tables, c.clip, c.partials, c.out, c.counts})
        if (p) (void)hipFree(p);
    c = ttpop::ClipBufs{};
}

// what tt_pop_exploit and tt_pop_exploit_nstep (`who`) refuse in a list of pairs, which goes into L (host only: no HIP call)
static int check_pairs(const char *who, const tt_population *h, const int pairs, const tt_pop_exploit_pair *list, ExploitList &L) {
    return check_pairs(who, h, pairs, list, L, [](const tt_pop_exploit_pair &) { return true; },
                       [](const tt_pop_exploit_pair &, int) { return TT_OK; });
}

extern "C" {

int tt_pop_learn_create(int count, int batch, const tt_pop_agent *agents, tt_population **out) {
    static const char who[] = "tt_pop_learn_create";
    if (const int rc = check_create(who, count, batch, agents, out)) return rc;
    std::vector<PopAgent> host(count);
    for (int a = 0; a < count; ++a) {
        const int rc = to_pop_agent(agents[a], a, batch, host[a]);
        if (rc != TT_OK) return rc;
    }
    PopAgent *dev = nullptr;
    if (const int rc = upload_descriptors(who, host, dev)) return rc;
    tt_population *h = new tt_population{count, batch, dev};
    for (int a = 0; a < count; ++a) {
        h->slots.push_back(agents[a].sample->slots);
        h->reserve.push_back(agents[a].sample->reserve);
    }
    *out = h;
    return TT_OK;
}

int tt_pop_learn(tt_population *h, int update, tt_stream_t stream) {
    if (!h) return fail(TT_EINVAL, "tt_pop_learn: handle is NULL");
    if (update < 0) return fail(TT_EINVAL, "tt_pop_learn: update = %d < 0", update);
    const int K = h->K, n = h->n, nb = (n + TR - 1) / TR;
    if (h->table) ttpop::launch_fwd_multi_nstep(K, n, h->dev, h->table, update, stream);
    else hipLaunchKernelGGL(k_pop_fwd_multi, dim3(K * 4 * nb), dim3(64 * NW), 0, stream, K, n, h->dev, update);
    hipLaunchKernelGGL(k_pop_bwd_rows_pair, dim3(K * (2 * nb + 1)), dim3(64 * NW), 0, stream, K, n, h->dev);
    hipLaunchKernelGGL(k_pop_bwd_weights<false>, dim3(K * WG_CRITIC_WEIGHTS), dim3(256), 0, stream, K, n, h->dev);
    if (h->clipped) {           // (the descriptors' optimizers are off: the two launches above and below leave gradients only)
        ttpop::launch_pop_grad_sqnorm(K, 0, h->clip, stream);
        ttpop::launch_pop_adam_soft_clip(K, 0, h->dev, h->clip, stream);
    }
    hipLaunchKernelGGL(k_pop_actor_tail, dim3(K * (nb + WG_ACTOR_WEIGHTS)), dim3(64 * NW), 0, stream, K, n, h->dev);
    if (h->clipped) {
        ttpop::launch_pop_grad_sqnorm(K, 1, h->clip, stream);
        ttpop::launch_pop_adam_soft_clip(K, 1, h->dev, h->clip, stream);
    }
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

int tt_pop_exploit(tt_population *h, int pairs, const tt_pop_exploit_pair *list, tt_stream_t stream) {
    ExploitList L{};
    const int rc = check_pairs("tt_pop_exploit", h, pairs, list, L);
    if (rc != TT_OK) return rc;
    if (h->table)
        return fail(TT_EINVAL, "tt_pop_exploit: this population has an n-step table, where an agent's discount is gamma ** n_step and not the "
                      "pair's gamma: use tt_pop_exploit_nstep");
    hipLaunchKernelGGL(k_pop_exploit, dim3(pairs * EX_CHUNKS), dim3(EX_THREADS), 0, stream, L, h->dev);
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

int tt_pop_learn_set_nstep(tt_population *h, const struct tt_pop_nstep *per_agent) {
    static const char who[] = "tt_pop_learn_set_nstep";
    if (!h) return fail(TT_EINVAL, "tt_pop_learn_set_nstep: handle is NULL");
    if (!per_agent) return fail(TT_EINVAL, "tt_pop_learn_set_nstep: per_agent is NULL");
    const int K = h->K;
    std::vector<PopNstep> host(K);
    for (int a = 0; a < K; ++a) {
        const int rc = check_pop_nstep(who, "agent", a, per_agent[a], h->slots[a], h->reserve[a]);
        if (rc != TT_OK) return rc;
        host[a] = PopNstep{per_agent[a].n_step, per_agent[a].gamma};
    }
    if (hipDeviceSynchronize() != hipSuccess) return fail(TT_EHIP, "tt_pop_learn_set_nstep: hipDeviceSynchronize");
    if (!h->table && hipMalloc(&h->table, sizeof(PopNstep) * K) != hipSuccess) {
        h->table = nullptr;
        return fail(TT_ENOMEM, "tt_pop_learn_set_nstep: hipMalloc");
    }
    bool ok = hipMemcpy(h->table, host.data(), sizeof(PopNstep) * K, hipMemcpyHostToDevice) == hipSuccess;
    for (int a = 0; a < K && ok; ++a)
        ok = hipMemcpy(td_gamma_of(h->dev + a), &per_agent[a].discount, sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    return ok ? TT_OK : fail(TT_EHIP, "tt_pop_learn_set_nstep: hipMemcpy");
}

int tt_pop_exploit_nstep(tt_population *h, int pairs, const tt_pop_exploit_pair *list, const struct tt_pop_nstep *ns, tt_stream_t stream) {
    static const char who[] = "tt_pop_exploit_nstep";
    ExploitList L{};
    const int rc = check_pairs(who, h, pairs, list, L);
    if (rc != TT_OK) return rc;
    if (!ns) return fail(TT_EINVAL, "tt_pop_exploit_nstep: ns is NULL");
    if (!h->table) return fail(TT_EINVAL, "tt_pop_exploit_nstep: this population has no n-step table (tt_pop_learn_set_nstep makes it)");
    ttpop::NstepWrites W{};
    W.n = pairs;
    for (int i = 0; i < pairs; ++i) {
        const int dst = list[i].dst, rc2 = check_pop_nstep(who, "pair", i, ns[i], h->slots[dst], h->reserve[dst]);
        if (rc2 != TT_OK) return rc2;
        if (ns[i].gamma != list[i].gamma) return fail(TT_EINVAL, "tt_pop_exploit_nstep: pair %d: ns.gamma is not the pair's gamma", i);
        L.p[i].gamma = ns[i].discount;      // k_pop_exploit stores the pair's gamma into dst's td.gamma: the discount's place
        W.dst[i] = dst;
        W.n_step[i] = ns[i].n_step;
        W.gamma[i] = ns[i].gamma;
    }
    hipLaunchKernelGGL(k_pop_exploit, dim3(pairs * EX_CHUNKS), dim3(EX_THREADS), 0, stream, L, h->dev);
    ttpop::launch_set_nstep(W, h->table, stream);
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

int tt_pop_nstep(tt_population *h, int agent, struct tt_pop_nstep *out) {
    if (!h) return fail(TT_EINVAL, "tt_pop_nstep: handle is NULL");
    if (!out) return fail(TT_EINVAL, "tt_pop_nstep: out is NULL");
    if (agent < 0 || agent >= h->K) return fail(TT_EINVAL, "tt_pop_nstep: agent %d is not in [0, K = %d)", agent, h->K);
    float discount;
    if (hipMemcpy(&discount, td_gamma_of(h->dev + agent), sizeof discount, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(TT_EHIP, "tt_pop_nstep: hipMemcpy");
    PopNstep e{1, discount};                // (no table: the one-step draw)
    if (h->table && hipMemcpy(&e, h->table + agent, sizeof e, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(TT_EHIP, "tt_pop_nstep: hipMemcpy");
    out->n_step = e.n_step;
    out->gamma = e.gamma;
    out->discount = discount;
    return TT_OK;
}

int tt_pop_learn_set_clip(tt_population *h, const struct tt_pop_clip *per_agent) {
    static const char who[] = "tt_pop_learn_set_clip";
    if (!h) return fail(TT_EINVAL, "tt_pop_learn_set_clip: handle is NULL");
    if (!per_agent) return fail(TT_EINVAL, "tt_pop_learn_set_clip: per_agent is NULL");
    const int K = h->K;
    std::vector<PopClip> values(K);
    for (int a = 0; a < K; ++a) {
        if (const int rc = check_pop_clip(who, "agent", a, per_agent[a])) return rc;
        values[a] = PopClip{{per_agent[a].max_norm_critic, per_agent[a].max_norm_actor}};
    }
    if (hipDeviceSynchronize() != hipSuccess) return fail(TT_EHIP, "tt_pop_learn_set_clip: hipDeviceSynchronize");
    if (h->clipped)             // (the tables stand: only the values are new)
        return hipMemcpy(h->clip.clip, values.data(), sizeof(PopClip) * K, hipMemcpyHostToDevice) == hipSuccess
                   ? TT_OK : fail(TT_EHIP, "tt_pop_learn_set_clip: hipMemcpy");
    std::vector<PopAgent> host(K);
    if (hipMemcpy(host.data(), h->dev, sizeof(PopAgent) * K, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(TT_EHIP, "tt_pop_learn_set_clip: hipMemcpy");
    // the tensor tables with the gradient pointers, filled once; every agent's grid of a network is the same
    const size_t tb = ttpop::clip_table_bytes();
    std::vector<char> tables(tb * K * 2);
    ttpop::ClipBufs c{};
    for (int a = 0; a < K; ++a)
        for (int net = 0; net < 2; ++net) {
            long long total = 0;
            // (agent 0's call gives the network's workgroups, the same for every agent; agent a's first is a times that)
            const int blocks = ttpop::fill_pop_clip_table(&host[a], net, a * c.blocks[net], tables.data() + tb * (a * 2 + net), &total);
            if (blocks <= 0) return fail(TT_EINVAL, "tt_pop_learn_set_clip: agent %d: network %d lacks a tensor", a, net);
            c.blocks[net] = blocks;
            c.chunk[net] = (total + TT_GRAD_CLIP_PARTIALS - 1) / TT_GRAD_CLIP_PARTIALS;
        }
    const size_t np = sizeof(double) * K * 2 * TT_GRAD_CLIP_PARTIALS, no = sizeof(float) * K * 4, nc = sizeof(long long) * K * 4;
    bool ok = hipMalloc(&c.tables, tables.size()) == hipSuccess && hipMalloc(&c.clip, sizeof(PopClip) * K) == hipSuccess &&
              hipMalloc(&c.partials, np) == hipSuccess && hipMalloc(&c.out, no) == hipSuccess && hipMalloc(&c.counts, nc) == hipSuccess;
    if (!ok) {
        free_clip(c);
        return fail(TT_ENOMEM, "tt_pop_learn_set_clip: hipMalloc");
    }
    for (PopAgent &P : host) P.Ac.on = P.Aa.on = 0;        // the weight-gradient launches leave the gradient and skip the optimizer
    ok = hipMemcpy(c.tables, tables.data(), tables.size(), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(c.clip, values.data(), sizeof(PopClip) * K, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemset(c.partials, 0, np) == hipSuccess && hipMemset(c.out, 0, no) == hipSuccess && hipMemset(c.counts, 0, nc) == hipSuccess &&
         hipMemcpy(h->dev, host.data(), sizeof(PopAgent) * K, hipMemcpyHostToDevice) == hipSuccess &&
         hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        free_clip(c);
        return fail(TT_EHIP, "tt_pop_learn_set_clip: hipMemcpy");
    }
    h->clip = c;
    h->clipped = true;
    return TT_OK;
}

int tt_pop_clip_write(tt_population *h, int count, const int32_t *agents, const struct tt_pop_clip *values, tt_stream_t stream) {
    static const char who[] = "tt_pop_clip_write";
    if (!h) return fail(TT_EINVAL, "tt_pop_clip_write: handle is NULL");
    if (!agents) return fail(TT_EINVAL, "tt_pop_clip_write: agents is NULL");
    if (!values) return fail(TT_EINVAL, "tt_pop_clip_write: values is NULL");
    if (!h->clipped) return fail(TT_EINVAL, "tt_pop_clip_write: this population has no clip table (tt_pop_learn_set_clip makes it)");
    if (count < 1 || count > h->K) return fail(TT_EINVAL, "tt_pop_clip_write: count = %d, not in [1, K = %d]", count, h->K);
    ttpop::ClipWrites W{};
    W.n = count;
    for (int i = 0; i < count; ++i) {
        if (agents[i] < 0 || agents[i] >= h->K)
            return fail(TT_EINVAL, "tt_pop_clip_write: entry %d: agent %d is not in [0, K = %d)", i, (int)agents[i], h->K);
        for (int j = 0; j < i; ++j)
            if (agents[j] == agents[i]) return fail(TT_EINVAL, "tt_pop_clip_write: entries %d and %d both name agent %d", j, i, (int)agents[i]);
        if (const int rc = check_pop_clip(who, "entry", i, values[i])) return rc;
        W.agent[i] = agents[i];
        W.max_norm[i][0] = values[i].max_norm_critic;
        W.max_norm[i][1] = values[i].max_norm_actor;
    }
    ttpop::launch_clip_write(W, h->clip.clip, stream);
    return hipGetLastError() == hipSuccess ? TT_OK : fail(TT_EHIP, "tt_pop_clip_write: the launch failed");
}

int tt_pop_clip(tt_population *h, int agent, struct tt_pop_clip *value, float out[4], int64_t counts[4]) {
    if (!h) return fail(TT_EINVAL, "tt_pop_clip: handle is NULL");
    if (!value || !out || !counts) return fail(TT_EINVAL, "tt_pop_clip: value, out or counts is NULL");
    if (agent < 0 || agent >= h->K) return fail(TT_EINVAL, "tt_pop_clip: agent %d is not in [0, K = %d)", agent, h->K);
    if (!h->clipped) return fail(TT_EINVAL, "tt_pop_clip: this population has no clip table (tt_pop_learn_set_clip makes it)");
    PopClip e;
    if (hipMemcpy(&e, static_cast<const PopClip *>(h->clip.clip) + agent, sizeof e, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(out, static_cast<const float *>(h->clip.out) + 4 * agent, sizeof(float) * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(counts, static_cast<const long long *>(h->clip.counts) + 4 * agent, sizeof(int64_t) * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(TT_EHIP, "tt_pop_clip: hipMemcpy");
    value->max_norm_critic = e.max_norm[0];
    value->max_norm_actor = e.max_norm[1];
    return TT_OK;
}

int tt_pop_hyper(tt_population *h, int agent, float out[4]) {
    if (!h) return fail(TT_EINVAL, "tt_pop_hyper: handle is NULL");
    if (!out) return fail(TT_EINVAL, "tt_pop_hyper: out is NULL");
    if (agent < 0 || agent >= h->K) return fail(TT_EINVAL, "tt_pop_hyper: agent %d is not in [0, K = %d)", agent, h->K);
    PopAgent P;
    if (hipMemcpy(&P, h->dev + agent, sizeof P, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(TT_EHIP, "tt_pop_hyper: hipMemcpy");
    out[0] = P.Aa.lr;
    out[1] = P.Ac.lr;
    out[2] = P.Aa.tau;
    out[3] = P.td.gamma;
    if (h->table) {                         // (td.gamma is the discount gamma ** n_step there)
        PopNstep e;
        if (hipMemcpy(&e, h->table + agent, sizeof e, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(TT_EHIP, "tt_pop_hyper: hipMemcpy");
        out[3] = e.gamma;
    }
    return TT_OK;
}

int tt_pop_learn_destroy(tt_population *h) {
    if (!h) return TT_OK;
    const hipError_t e = hipFree(h->dev), e2 = h->table ? hipFree(h->table) : hipSuccess;
    free_clip(h->clip);
    delete h;
    return e == hipSuccess && e2 == hipSuccess ? TT_OK : TT_EHIP;
}

}  // extern "C"
