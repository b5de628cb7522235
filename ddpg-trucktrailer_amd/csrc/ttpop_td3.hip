// ttpop_td3.hip -- TD3's learn() for a POPULATION of K independent agents in the launches of one agent's TD3 update (MI355X, gfx950).
//
// What csrc/ttpop.hip is to csrc/ttlearn.hip, this file is to csrc/tttd3.hip: agent a is a lone TD3 loop of its own, only its
// learn() launches are shared.  Each launch below runs the workgroups of all K agents; a workgroup finds its agent and its block
// within the agent's grid from blockIdx.x and then does exactly what the lone launch's workgroup does, with the arguments the lone
// launch passes (the bodies of ttlearn_bodies.h, the prologue and the descriptor of tttd3.h):
//
//   k_pop_td3_fwd_multi        K x (full ? 6 : 5) x nb, agent-major; inside an agent job-major: k_td3_fwd_multi.  The agent's first
//                              workgroup leaves its step_snap.
//   k_pop_td3_bwd_rows         K x ((full ? 3 : 2) x nb + 1), agent-major: critic 1's rows, critic 2's rows, [the actor's unit rows,]
//                              then that agent's counter workgroup: k_td3_bwd_rows.
//   k_pop_td3_bwd_weights      K x 2 x 210, agent-major, critic-major inside: k_td3_bwd_weights (the tau = 0 variant on critic-only
//                              updates).
//   k_pop_td3_actor_tail       full updates only: the K x nb row workgroups of ALL agents first, then the K x 200 weight workgroups:
//                              no workgroup that waits in device memory has a lower flat index than any producer (the dispatch-order
//                              rule of k_pop_actor_tail).  Each agent has its own TailSync words and gave_up_host, and its epoch is
//                              its own ACTOR step count.  The tail's bounded wait is the only wait in device memory here.
//
// and, off the learn() path, k_pop_td3_exploit (tt_pop_td3_exploit): PBT's exploit/explore step for six networks.
//
// So each agent's results are the bits of its lone TD3 update (tests/test_gpu_population_td3.py).  The descriptors are Td3Agent[K]
// in device memory, filled once at tt_pop_td3_create and read through the constant address space: a launch takes
// (K, descriptors, u, full) and is graph-capturable.  `full` is a launch argument, so policy_delay is one value for the whole
// population; sigma, clip, alpha, beta, tau and gamma are each agent's own.  The sampled-row prologue of the first launch and the
// actor tail are the text of csrc/ttlearn_sites.h, as in every other family.
#include "ttpop_exploit.h"
#include "tttd3.h"

#include <cstddef>
#include <vector>

namespace {

// grid: K x (full ? 6 : 5) x nb, agent-major; within an agent job-major as k_td3_fwd_multi
__global__ __launch_bounds__(64 * NW) void k_pop_td3_fwd_multi(const int K, const Td3Agent *__restrict__ D, const int u, const int full) {
    __shared__ __attribute__((aligned(16))) float h1_s[H1S_FLOATS];
    __shared__ __attribute__((aligned(16))) float z_s[TR * DS];
    __shared__ __attribute__((aligned(16))) float w1_s[H1 * IN];
    const int n = td3_of(D).n, nb = (n + TR - 1) / TR, per = (full ? 6 : 5) * nb, ag = (int)blockIdx.x / per;      // (one B for all)
    if (ag >= K) return;
    const Td3Agent &P = td3_of(D + ag);
    const int lb = (int)blockIdx.x - ag * per, job = lb / nb, row0 = (lb - job * nb) * TR;
    if (lb == 0 && threadIdx.x == 0) *P.step_snap = *P.step_dev;      // (the next launch ticks step_dev)
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

// grid: K x ((full ? 3 : 2) x nb + 1), agent-major: critic 1's rows, critic 2's rows, [the actor's unit rows,] the agent's counter
// workgroup
__global__ __launch_bounds__(64 * NW) void k_pop_td3_bwd_rows(const int K, const Td3Agent *__restrict__ D, const int u, const int full) {
    __shared__ __attribute__((aligned(16))) float dx2_s[DXS_FLOATS];
    __shared__ float red[2 * NW * TR];
    __shared__ float rsc_s[TR];
    const int n = td3_of(D).n, nb = (n + TR - 1) / TR, groups = full ? 3 : 2, per = groups * nb + 1, ag = (int)blockIdx.x / per;
    if (ag >= K) return;
    const Td3Agent &P = td3_of(D + ag);
    const int lb = (int)blockIdx.x - ag * per;
    if (lb == groups * nb) {
        if (threadIdx.x == 0) {
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

// grid: K x 2 x 210, agent-major, critic-major inside: a critic's weight gradients with its optimizer step
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k_pop_td3_bwd_weights(const int K,
                                                                                                 const Td3Agent *__restrict__ D,
                                                                                                 const int u, const int full) {
    __shared__ __attribute__((aligned(16))) float part[4][4][256];
    __shared__ float f_s[1];
    __shared__ __attribute__((aligned(16))) _Float16 stage_s[4 * 1024];
    const int ag = (int)blockIdx.x / (2 * WG_CRITIC_WEIGHTS);
    if (ag >= K) return;
    const int lb = (int)blockIdx.x - ag * 2 * WG_CRITIC_WEIGHTS, c = lb / WG_CRITIC_WEIGHTS;
    const Td3Agent &P = td3_of(D + ag);
    bwd_weights_body<false, false>(lb - c * WG_CRITIC_WEIGHTS, P.n, 1, P.s, P.a, P.sv_c[c], P.o_c[c], P.Gc[c], P.Ac[c][full ? 0 : 1],
                                   RowScale{nullptr, nullptr, 1.f}, part, f_s, TailSync{nullptr, nullptr, 0, nullptr}, 0, stage_s);
}

// grid: K x nb row workgroups FIRST (every agent's), then K x 200 weight workgroups: Q1(s, mu(s)) and dQ/da through each agent's
// updated critic 1, then its actor's weight gradients + Adam + soft update.  A weight workgroup waits in device memory for its agent's
// rows (TailSync, bounded), so every producer is dispatched before any workgroup that may wait for it.
__global__ __launch_bounds__(64 * NW) void k_pop_td3_actor_tail(const int K, const Td3Agent *__restrict__ D, const int u, const int full) {
    __shared__ __attribute__((aligned(16))) float lds[H1S_FLOATS + TR * DS + H1 * IN];
    const int n = td3_of(D).n, nb = (n + TR - 1) / TR, rows = K * nb;
    if ((int)blockIdx.x < rows) {
        const int ag = (int)blockIdx.x / nb, lb = (int)blockIdx.x - ag * nb;
        const Td3Agent &P = td3_of(D + ag);
        const long long epoch = *P.Aa.step_dev;
        TT_ACTOR_TAIL_ROWS(n, P.s, P.mu_out, P.Wc[0], P.q_pi, P.dq_da, lds, P.ts, lb, epoch);
        return;
    }
    const int ag = ((int)blockIdx.x - rows) / WG_ACTOR_WEIGHTS;
    if (threadIdx.x >= 256 || ag >= K) return;
    const Td3Agent &P = td3_of(D + ag);
    const long long epoch = *P.Aa.step_dev;
    TT_ACTOR_TAIL_WEIGHTS((int)blockIdx.x - rows - ag * WG_ACTOR_WEIGHTS, n, P.s, P.sv_a, P.o_a, P.Ga, P.Aa, P.RSa, lds, P.ts, epoch);
}

// ---- PBT exploit/explore (tt_pop_td3_exploit): dst's learning state <- src's, then dst's hyperparameters, in one launch ----
// k_pop_exploit's shape for six networks.  A pair's copy is 142 regions: per trained network (critic 1 and critic 2 with 12 tensors
// each, then the actor with 10) and tensor t, its parameters, Adam m, Adam v and target parameters (4 t + {0, 1, 2, 3}), then the six
// fc2 images (network / target of critic 1, critic 2, the actor), each whole: its forward and its backward halves.  Each region is
// cut into EX_CHUNK-byte pieces, one workgroup each (csrc/ttpop_exploit.h: the piece copy, shared with k_pop_exploit).  Nothing else
// is copied: dst's env, ring, noise seed, both step counts, both bias-correction buffers, step_snap, tail words and scratch buffers
// stay its own.
struct Exploit3List {
    int n;
    tt_pop_td3_pair p[TT_POP_MAX_AGENTS];
};

constexpr int X3_CRITIC = 4 * 12, X3_TENSOR_REGIONS = 2 * X3_CRITIC + 4 * 10, X3_REGIONS = X3_TENSOR_REGIONS + 6;

__host__ __device__ constexpr size_t x3_region_bytes(const int r) {
    return r < X3_TENSOR_REGIONS ? (size_t)ex_numel((r % X3_CRITIC) >> 2) * 4 : IMG_HALVES * 2;
}
__host__ __device__ constexpr int x3_region_chunks(const int r) { return ex_chunks(x3_region_bytes(r)); }
constexpr int x3_chunks_per_pair() {
    int s = 0;
    for (int r = 0; r < X3_REGIONS; ++r) s += x3_region_chunks(r);
    return s;
}
constexpr int X3_CHUNKS = x3_chunks_per_pair();

// trained network i of a descriptor (0, 1: the critics; 2: the actor).  Both variants of a critic hold the same tensors and images.
__device__ __forceinline__ const AdamFused &x3_net(const Td3Agent &P, const int i) { return i < 2 ? P.Ac[i][0] : P.Aa; }

// grid: pairs x X3_CHUNKS, pair-major.  No pair's dst is another pair's src (tt_pop_td3_exploit checks), so every byte a workgroup
// reads is written by no workgroup of the launch.  The descriptors' pointers are read, never written; the hyperparameter words are
// written with plain global stores and read by the later launches on the stream.
__global__ __launch_bounds__(EX_THREADS) void k_pop_td3_exploit(const Exploit3List L, Td3Agent *__restrict__ D) {
    const int pair = (int)blockIdx.x / X3_CHUNKS, piece = (int)blockIdx.x - pair * X3_CHUNKS;
    if (pair >= L.n) return;
    const tt_pop_td3_pair q = L.p[pair];
    if (piece == 0 && threadIdx.x == 0) {
        Td3Agent &W = D[q.dst];
        W.Aa.lr = q.alpha;
        W.Aa.tau = q.tau;
        for (int c = 0; c < 2; ++c) {
            W.Ac[c][0].lr = q.beta;
            W.Ac[c][1].lr = q.beta;
            W.Ac[c][0].tau = q.tau;        // (the tau = 0 variant of critic-only updates stays 0)
        }
        W.gamma = q.gamma;
        W.sigma = q.target_noise;
        W.clip = q.noise_clip;
    }
    if (q.dst == q.src) return;
    int r = 0, c = piece;
    while (r < X3_REGIONS - 1 && c >= x3_region_chunks(r)) c -= x3_region_chunks(r++);
    const Td3Agent &S = td3_of(D + q.src), &T = td3_of(D + q.dst);
    const char *from;
    char *to;
    if (r < X3_TENSOR_REGIONS) {
        const int net = r / X3_CRITIC, local = r - net * X3_CRITIC, t = local >> 2, kind = local & 3;
        from = reinterpret_cast<const char *>(ex_tensor(x3_net(S, net), kind, t));
        to = reinterpret_cast<char *>(ex_tensor(x3_net(T, net), kind, t));
    } else {
        const int i = r - X3_TENSOR_REGIONS;
        const AdamFused &As = x3_net(S, i >> 1), &At = x3_net(T, i >> 1);
        from = reinterpret_cast<const char *>((i & 1) ? As.img_t : As.img_p);
        to = reinterpret_cast<char *>((i & 1) ? At.img_t : At.img_p);
    }
    if (!from || !to) return;                      // (images off)
    ex_copy_piece(from, to, x3_region_bytes(r), c);
}

// what two agents of one population may not share (host only: no HIP call): each list holds one agent's addresses of a kind
struct Owned {
    const void *steps[2], *tail, *rows[3], *grads[3];
};
Owned owned_of(const Td3Agent &P) {
    return Owned{{P.step_dev, P.tick_a.step_dev}, P.ts.hints, {P.o_c[0].dx2, P.o_c[1].dx2, P.o_a.dx2}, {P.Gc[0].w1, P.Gc[1].w1, P.Ga.w1}};
}
template <int NA, int NB>
bool overlap(const void *const (&x)[NA], const void *const (&y)[NB]) {
    for (const void *p : x)
        for (const void *q : y)
            if (p == q) return true;
    return false;
}

}  // namespace

struct tt_pop_td3 {
    int K = 0, n = 0;
    Td3Agent *dev = nullptr;
};

extern "C" {

int tt_pop_td3_create(int count, int batch, const tt_td3_agent *agents, tt_pop_td3 **out) {
    static const char who[] = "tt_pop_td3_create";
    if (const int rc = check_create(who, count, batch, agents, out)) return rc;
    std::vector<Td3Agent> host(count);
    for (int a = 0; a < count; ++a) {
        const int rc = to_td3_agent(agents[a], a, batch, host[a]);
        if (rc != TT_OK) return rc;
    }
    for (int a = 0; a < count; ++a)
        for (int b = a + 1; b < count; ++b) {
            const Owned x = owned_of(host[a]), y = owned_of(host[b]);
            if (overlap(x.steps, y.steps)) return fail(TT_EINVAL, "tt_pop_td3_create: agents %d and %d share a step counter", a, b);
            if (x.tail == y.tail) return fail(TT_EINVAL, "tt_pop_td3_create: agents %d and %d share their tail words", a, b);
            if (overlap(x.rows, y.rows)) return fail(TT_EINVAL, "tt_pop_td3_create: agents %d and %d share a per-row workspace", a, b);
            if (overlap(x.grads, y.grads)) return fail(TT_EINVAL, "tt_pop_td3_create: agents %d and %d share a gradient buffer", a, b);
        }
    Td3Agent *dev = nullptr;
    if (const int rc = upload_descriptors(who, host, dev)) return rc;
    *out = new tt_pop_td3{count, batch, dev};
    return TT_OK;
}

int tt_pop_td3_learn(tt_pop_td3 *h, int update, int full, tt_stream_t stream) {
    if (update < 0) return fail(TT_EINVAL, "tt_pop_td3_learn: update = %d < 0", update);
    if (!h) return fail(TT_EINVAL, "tt_pop_td3_learn: handle is NULL");
    const int K = h->K, nb = (h->n + TR - 1) / TR, f = full ? 1 : 0;
    hipLaunchKernelGGL(k_pop_td3_fwd_multi, dim3(K * (f ? 6 : 5) * nb), dim3(64 * NW), 0, stream, K, h->dev, update, f);
    hipLaunchKernelGGL(k_pop_td3_bwd_rows, dim3(K * ((f ? 3 : 2) * nb + 1)), dim3(64 * NW), 0, stream, K, h->dev, update, f);
    hipLaunchKernelGGL(k_pop_td3_bwd_weights, dim3(K * 2 * WG_CRITIC_WEIGHTS), dim3(256), 0, stream, K, h->dev, update, f);
    if (f) hipLaunchKernelGGL(k_pop_td3_actor_tail, dim3(K * nb + K * WG_ACTOR_WEIGHTS), dim3(64 * NW), 0, stream, K, h->dev, update, f);
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

int tt_pop_td3_exploit(tt_pop_td3 *h, int pairs, const tt_pop_td3_pair *list, tt_stream_t stream) {
    static const char who[] = "tt_pop_td3_exploit";
    Exploit3List L{};
    const int rc = check_pairs(
        who, h, pairs, list, L, [](const tt_pop_td3_pair &q) { return std::isfinite(q.target_noise) && std::isfinite(q.noise_clip); },
        [](const tt_pop_td3_pair &q, const int i) {
            if (q.target_noise < 0.f || q.noise_clip < 0.f) return fail(TT_EINVAL, "%s: pair %d: target_noise and noise_clip must not be negative", who, i);
            return (int)TT_OK;
        });
    if (rc != TT_OK) return rc;
    hipLaunchKernelGGL(k_pop_td3_exploit, dim3(pairs * X3_CHUNKS), dim3(EX_THREADS), 0, stream, L, h->dev);
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

int tt_pop_td3_hyper(tt_pop_td3 *h, int agent, float out[6]) {
    if (!h) return fail(TT_EINVAL, "tt_pop_td3_hyper: handle is NULL");
    if (!out) return fail(TT_EINVAL, "tt_pop_td3_hyper: out is NULL");
    if (agent < 0 || agent >= h->K) return fail(TT_EINVAL, "tt_pop_td3_hyper: agent %d is not in [0, K = %d)", agent, h->K);
    Td3Agent P;
    if (hipMemcpy(&P, h->dev + agent, sizeof P, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(TT_EHIP, "tt_pop_td3_hyper: hipMemcpy");
    out[0] = P.Aa.lr;
    out[1] = P.Ac[0][0].lr;
    out[2] = P.Aa.tau;
    out[3] = P.gamma;
    out[4] = P.sigma;
    out[5] = P.clip;
    return TT_OK;
}

int tt_pop_td3_destroy(tt_pop_td3 *h) {
    if (!h) return TT_OK;
    const hipError_t e = hipFree(h->dev);
    delete h;
    return e == hipSuccess ? TT_OK : TT_EHIP;
}

}  // extern "C"
