// ttclip.hip -- gradient-norm clipping of learn(): torch.nn.utils.clip_grad_norm_ in front of optimizer.step(), as the optimizer
// launch of one network (MI355X, gfx950; include/ttenv.h: tt_grad_clip, tt_pop_clip; DESIGN.md sections 34 and 36).
//
//   k_grad_sqnorm        the sum of squares of a network's gradient tensors, in f64 (the square of an f32 is exact there): the
//                        concatenated index space in CLIP_WGS equal runs, one per workgroup; a thread adds its elements in a fixed
//                        order, the workgroup its 256 threads by a fixed tree through LDS, and stores ONE partial, partials[w].
//                        No atomics, no wait between workgroups: the same inputs give the same bits, eager or replayed.
//   k_adam_soft_clip     k_adam_soft (csrc/ttlearn.hip): its grid, its table, its arithmetic -- on coef * grad.  Every workgroup adds
//                        the partials in index order (the same bits in each), norm = sqrt(sum), coef = max_norm / (norm + 1e-6)
//                        where that is below 1, else 1.  With coef = 1 the product is exact and the launch leaves k_adam_soft's bits.
//
// and for a population (csrc/ttpop.hip: tt_pop_learn_set_clip), each launch running every agent's workgroups, agent-major:
//
//   k_pop_grad_sqnorm      K x CLIP_WGS: workgroup (a, w) is workgroup w of k_grad_sqnorm on agent a's tensors (the same text)
//   k_pop_adam_soft_clip   K x blocks: k_adam_soft_clip with lr .. tau, the step count, the bias corrections and the fc2 images read
//                          from agent a's descriptor (what k_pop_exploit writes in place), max_norm from the clip table and the
//                          tensors from a table in device memory; max_norm = 0: coef is 1 by definition, whatever the norm
//   k_pop_clip_write       tt_pop_clip_write's table writes
//
// The gradient buffers are read only: they keep the unclipped gradient (the learn log's norms are theirs).  A non-finite norm gets
// no special case (clip_grad_norm_'s error_if_nonfinite=False): coef is then 0 (norm = inf) or NaN, and so is what it multiplies.
#include "ttlearn_host.h"
#include "ttpop.h"

namespace {

constexpr int CLIP_WGS = TT_GRAD_CLIP_PARTIALS;

// the elements [lo, hi) of one tensor, by the whole workgroup: scalar loads up to the first 16-byte boundary, 16 B per lane from
// there, scalar loads for the rest -- nothing outside [lo, hi) is read.  Thread t's order: head element t, vectors t, t + 256, ..
// (x, y, z, w each), tail element t.
__device__ __forceinline__ double sq_run(const float *__restrict__ g, const int lo, const int hi, double acc) {
    const int t = threadIdx.x;
    const int to_boundary = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(g + lo) & 15u)) & 15u) >> 2);
    const int head = min(to_boundary, hi - lo);
    const int nvec = (hi - lo - head) >> 2;
    const int tail0 = lo + head + 4 * nvec;
    if (t < head) {
        const double x = (double)g[lo + t];
        acc += x * x;
    }
    const float4 *__restrict__ v = reinterpret_cast<const float4 *>(g + lo + head);
    for (int j = t; j < nvec; j += 256) {
        const float4 q = v[j];
        const double x = (double)q.x, y = (double)q.y, z = (double)q.z, w = (double)q.w;
        acc += x * x;
        acc += y * y;
        acc += z * z;
        acc += w * w;
    }
    if (t < hi - tail0) {
        const double x = (double)g[tail0 + t];
        acc += x * x;
    }
    return acc;
}

// workgroup w: the elements [w * chunk, (w + 1) * chunk) of the tensors laid end to end (chunk: the host's ceil(total / CLIP_WGS)),
// its sum into dst.  Text, by the rule of csrc/ttlearn_sites.h: k_grad_sqnorm sees what it saw when the lines were its own.
// T: an AdamTable (a kernel argument, or a reference into device memory); w, chunk, dst: expressions of the site.
#define TT_GRAD_SQNORM_WORKGROUP(T, w, chunk, dst)                                                                                      \
    __shared__ double red[256];                                                                                                         \
    const long long begin = (long long)(w) * (chunk), end = begin + (chunk);                                                            \
    double acc = 0.0;                                                                                                                   \
    long long off = 0;                                                                                                                  \
    for (int ti = 0; ti < (T).count; ++ti) {                                                                                            \
        const long long n = (T).numel[ti];                                                                                              \
        const long long lo = max(begin - off, 0LL), hi = min(end - off, n);                                                             \
        if (lo < hi) acc = sq_run((T).g[ti], (int)lo, (int)hi, acc);                                                                    \
        off += n;                                                                                                                       \
    }                                                                                                                                   \
    red[threadIdx.x] = acc;                                                                                                             \
    __syncthreads();                                                                                                                    \
    for (int s = 128; s > 0; s >>= 1) {                                                                                                 \
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];                                                             \
        __syncthreads();                                                                                                                \
    }                                                                                                                                   \
    if (threadIdx.x == 0) (dst) = red[0];

__global__ __launch_bounds__(256) void k_grad_sqnorm(const AdamTable T, const long long chunk, double *__restrict__ partials) {
    TT_GRAD_SQNORM_WORKGROUP(T, blockIdx.x, chunk, partials[blockIdx.x])
}

// entry i of an array in device memory that no launch reading it writes, as a reference into the constant address space (agent_of)
template <class E>
__device__ __forceinline__ const E &const_entry(const E *base, const int i) {
    return *(const E *)((const __attribute__((address_space(4))) E *)base + i);
}

// grid: K x CLIP_WGS, agent-major.  tables: AdamTable[K][2], partials: [K][2][CLIP_WGS].
__global__ __launch_bounds__(256) void k_pop_grad_sqnorm(const int K, const int net, const AdamTable *__restrict__ tables,
                                                         const long long chunk, double *__restrict__ partials) {
    const int ag = (int)blockIdx.x / CLIP_WGS, w = (int)blockIdx.x - ag * CLIP_WGS;
    if (ag >= K) return;
    const AdamTable &T = const_entry(tables, ag * 2 + net);
    TT_GRAD_SQNORM_WORKGROUP(T, w, chunk, partials[(ag * 2 + net) * CLIP_WGS + w])
}

// k_adam_soft with the clip coefficient on the gradient (the element update is k_adam_soft's text: TT_ADAM_SOFT_ELEMENT)
__global__ __launch_bounds__(256) void k_adam_soft_clip(const AdamTable T, const long long *__restrict__ step_dev, const float lr,
                                                        const float beta1, const float beta2, const float eps,
                                                        const float weight_decay, const float tau,
                                                        const float *__restrict__ bias_corr, const float max_norm,
                                                        const double *__restrict__ partials, float *__restrict__ out,
                                                        long long *__restrict__ counts) {
    double sum = 0.0;
    for (int w = 0; w < CLIP_WGS; ++w) sum += partials[w];      // index order, in every workgroup: the same bits
    const double norm = sqrt(sum);
    float coef = (float)((double)max_norm / (norm + 1e-6));
    coef = coef > 1.f ? 1.f : coef;                             // (not fminf: a NaN stays a NaN)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out[0] = (float)norm;
        out[1] = coef;
        if (counts) {
            counts[0] += 1;
            counts[1] += coef < 1.f ? 1 : 0;
        }
    }
    TT_ADAM_SOFT_ELEMENT(__fmul_rn(coef, T.g[ti][i]))      // the product rounded on its own
}

// what TT_ADAM_SOFT_ELEMENT reads of its table T, for a population: the tensors of the agent's table in device memory, the fc2 images
// of its descriptor
struct PopAdamView {
    float *const *p, *const *m, *const *v, *const *tgt;
    const int *numel, *block_start;
    int count;
    _Float16 *img_p, *img_t;
};

// grid: K x blocks, agent-major; agent a's table counts its block_start from a * blocks, so the element text finds the tensor from
// blockIdx.x as k_adam_soft_clip does.  clip: PopClip[K]; partials, out, counts: [K][2][..].
__global__ __launch_bounds__(256) void k_pop_adam_soft_clip(const int K, const int net, const int blocks, const PopAgent *__restrict__ D,
                                                            const AdamTable *__restrict__ tables, const PopClip *__restrict__ clip,
                                                            const double *__restrict__ partials, float *__restrict__ out,
                                                            long long *__restrict__ counts) {
    const int ag = (int)blockIdx.x / blocks;
    if (ag >= K) return;
    const PopAgent &P = agent_of(D, ag);
    const AdamFused &A = net ? P.Aa : P.Ac;
    const AdamTable &tab = const_entry(tables, ag * 2 + net);
    const PopAdamView T{tab.p, tab.m, tab.v, tab.tgt, tab.numel, tab.block_start, tab.count, A.img_p, A.img_t};
    const long long *step_dev = A.step_dev;
    const float lr = A.lr, beta1 = A.beta1, beta2 = A.beta2, eps = A.eps, weight_decay = A.weight_decay, tau = A.tau;
    const float *bias_corr = A.bias_corr;
    const float max_norm = const_entry(clip, ag).max_norm[net];
    const double *part = partials + (ag * 2 + net) * CLIP_WGS;
    double sum = 0.0;
    for (int w = 0; w < CLIP_WGS; ++w) sum += part[w];          // index order, in every workgroup: the same bits
    const double norm = sqrt(sum);
    float coef = (float)((double)max_norm / (norm + 1e-6));
    coef = coef > 1.f ? 1.f : coef;                             // (not fminf: a NaN stays a NaN)
    if (max_norm == 0.f) coef = 1.f;                            // this agent does not clip this network: no norm reaches coef
    if ((int)blockIdx.x == ag * blocks && threadIdx.x == 0) {
        out[(ag * 2 + net) * 2] = (float)norm;
        out[(ag * 2 + net) * 2 + 1] = coef;
        long long *c = counts + (ag * 2 + net) * 2;
        c[0] += 1;
        c[1] += coef < 1.f ? 1 : 0;
    }
    TT_ADAM_SOFT_ELEMENT(__fmul_rn(coef, tab.g[ti][i]))     // the product rounded on its own
}

// one workgroup: thread i writes agent[i]'s entry, with plain global stores (read by the later launches on the stream, the contract
// of k_pop_exploit's hyperparameter words)
__global__ __launch_bounds__(64) void k_pop_clip_write(const ttpop::ClipWrites W, PopClip *__restrict__ T) {
    const int i = threadIdx.x;
    if (i >= W.n) return;
    T[W.agent[i]].max_norm[0] = W.max_norm[i][0];
    T[W.agent[i]].max_norm[1] = W.max_norm[i][1];
}

}  // namespace

namespace ttpop {

size_t clip_table_bytes() { return sizeof(AdamTable); }

int fill_pop_clip_table(const void *agent, const int net, const int first_block, void *table, long long *total) {
    const PopAgent &P = *static_cast<const PopAgent *>(agent);
    const AdamFused &A = net ? P.Aa : P.Ac;
    const Grads &G = net ? P.Ga : P.Gc;
    const float *const g[MAXT] = {G.w1, G.b1, G.g1, G.be1, G.w2, G.b2, G.g2, G.be2, G.w3, G.b3, G.wa, G.ba};
    const int count = net ? 10 : 12;
    int32_t numel[MAXT];
    *total = 0;
    for (int t = 0; t < count; ++t) *total += numel[t] = t == 0 ? H1 * IN : t < 4 ? H1 : t == 4 ? H2 * H1 : t < 9 ? H2 : t == 9 ? 1 : H2;
    AdamTable T{};
    const tt_fc2_images images{A.img_p, A.img_t};
    const int blocks = fill_adam_table(T, 256, count, A.p, g, A.m, A.v, A.tgt, numel, &images);
    if (blocks <= 0) return -1;
    for (int t = 0; t <= count; ++t) T.block_start[t] += first_block;
    *static_cast<AdamTable *>(table) = T;
    return blocks;
}

void launch_pop_grad_sqnorm(const int K, const int net, const ClipBufs &c, hipStream_t stream) {
    hipLaunchKernelGGL(k_pop_grad_sqnorm, dim3(K * CLIP_WGS), dim3(256), 0, stream, K, net, static_cast<const AdamTable *>(c.tables),
                       c.chunk[net], static_cast<double *>(c.partials));
}

void launch_pop_adam_soft_clip(const int K, const int net, const void *agents, const ClipBufs &c, hipStream_t stream) {
    hipLaunchKernelGGL(k_pop_adam_soft_clip, dim3(K * c.blocks[net]), dim3(256), 0, stream, K, net, c.blocks[net],
                       static_cast<const PopAgent *>(agents), static_cast<const AdamTable *>(c.tables),
                       static_cast<const PopClip *>(c.clip), static_cast<const double *>(c.partials), static_cast<float *>(c.out),
                       static_cast<long long *>(c.counts));
}

void launch_clip_write(const ClipWrites &w, void *clip, hipStream_t stream) {
    hipLaunchKernelGGL(k_pop_clip_write, dim3(1), dim3(64), 0, stream, w, static_cast<PopClip *>(clip));
}

}  // namespace ttpop

extern "C" {

int tt_adam_soft_update_clipped(int count, float *const *params, const float *const *grads, float *const *exp_avg,
                                float *const *exp_avg_sq, float *const *targets, const int32_t *numel, const int64_t *step_dev,
                                float lr, float beta1, float beta2, float eps, float weight_decay, float tau,
                                const tt_fc2_images *images, const float *bias_corr, const tt_grad_clip *clip, tt_stream_t stream) {
    const char *const who = "tt_adam_soft_update_clipped";
    if (!clip) return fail(TT_EINVAL, "%s: clip is NULL", who);
    if (!clip->partials || !clip->out) return fail(TT_EINVAL, "%s: clip->partials or clip->out is NULL", who);
    if (!std::isfinite(clip->max_norm) || !(clip->max_norm > 0.f))
        return fail(TT_EINVAL, "%s: clip->max_norm = %g is not a finite number > 0", who, (double)clip->max_norm);
    if (count < 1 || count > MAXT) return fail(TT_EINVAL, "%s: count = %d tensors, not in [1, %d]", who, count, MAXT);
    if (!params || !grads || !exp_avg || !exp_avg_sq || !numel || !step_dev)
        return fail(TT_EINVAL, "%s: params, grads, exp_avg, exp_avg_sq, numel or step_dev is NULL", who);
    long long total = 0;
    for (int i = 0; i < count; ++i) {
        if (numel[i] < 0) return fail(TT_EINVAL, "%s: numel[%d] = %d is negative", who, i, (int)numel[i]);
        total += numel[i];
    }
    AdamTable T{};
    const int blocks = fill_adam_table(T, 256, count, params, grads, exp_avg, exp_avg_sq, targets, numel, images);
    if (blocks <= 0)
        return fail(TT_EINVAL, "%s: a tensor is missing or empty, or the fc2 images do not go with the tensor list", who);
    const long long chunk = (total + CLIP_WGS - 1) / CLIP_WGS;
    hipLaunchKernelGGL(k_grad_sqnorm, dim3(CLIP_WGS), dim3(256), 0, stream, T, chunk, clip->partials);
    hipLaunchKernelGGL(k_adam_soft_clip, dim3(blocks), dim3(256), 0, stream, T, reinterpret_cast<const long long *>(step_dev), lr, beta1,
                       beta2, eps, weight_decay, tau, bias_corr, clip->max_norm, static_cast<const double *>(clip->partials), clip->out,
                       reinterpret_cast<long long *>(clip->counts));
    return launched(who);
}

}  // extern "C"
