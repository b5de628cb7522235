// ttlearnlog.hip -- the learn log: per-update losses, Q / TD / dQ/da / mu statistics and gradient norms of learn(), reduced on the
// device from the buffers the update leaves behind (MI355X, gfx950; include/ttenv.h: tt_learn_log_*).
//
// k_learn_log is ONE launch per update for every agent of the handle, behind the update's last launch on its stream.  Grid:
// agents x (1 + 2 G) workgroups of 256 threads, G = TT_LEARN_LOG_CHUNKS.  Of an agent's workgroups
//
//   0                  the row statistics: thread t takes rows t, t + 256, ... of y, q, q_pi, dq_da and mu in f64, a tree (stride
//                      128 and 64 through LDS, 32 .. 1 by lane shuffles in wave 0) folds the 256 partial results, thread 0 writes
//                      the record's head
//   1 + g G + c        chunk c of gradient g (0 critic, 1 actor): ceil(ceil(numel / 4) / G) float4 per chunk -- 16-byte aligned,
//                      the ragged last float4 read element by element -- thread t takes float4 t, t + 256, ... of the chunk into
//                      four f64 sums of squares (one per component, added 0 + 1 + 2 + 3), the same tree folds them, thread 0 leaves
//                      {sum of squares, step, non-finite count} in the record's part [g G + c]
//
// No workgroup waits for another or reads what another wrote, there is no fence, no atomic and no write index: every workgroup
// derives the record's slot from the step count alone, slot = (step / every) % capacity, so eager launches and graph replays land in
// the same place, and every order of additions is fixed by B and numel.  The host adds the 2 G parts in index order and takes the
// roots when it drains (a last workgroup doing that on the device would need the ticket that cost the episode log 10 -> 78 us,
// DESIGN.md section 3.4).  A part carries the step it belongs to: a record is complete when all its parts carry the head's step.
#include "tthost.h"
#include "ttenv.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

using tthost::fail;

namespace {

#ifdef TT_LEARN_LOG_CHUNKS_TRY               // (a measurement build with another G: build.py's `defines`)
constexpr int G = TT_LEARN_LOG_CHUNKS_TRY;
#else
constexpr int G = TT_LEARN_LOG_CHUNKS;       // workgroups per gradient
#endif
constexpr int NT = 256;                      // threads per workgroup
constexpr int MAXB = 1024;
constexpr int NROW = 14;                     // values of the row workgroup: [0, 8) sums, [8, 10) minima, [10, 14) maxima
constexpr int NSUM = 8, NMIN = 2;
static_assert(NROW + 2 == TT_LEARN_LOG_NVALUES, "a record's values: 14 of the rows and the two norms");

struct LogJob {
    const float *y, *q, *q_pi, *dq_da, *mu;
    const float *grad[2];
    int numel[2];
    const long long *step_dev;
};

struct Part {
    double sumsq;
    long long step;
    int nonfinite, pad_;
};

struct Record {
    long long step;                          // -1: empty
    int nonfinite, pad_;                     // among the 5 B row values
    double v[NROW];                          // TT_LEARN_LOG_NVALUES' first 14, in the header's order
    Part part[2 * G];
};

__device__ __forceinline__ int nonfinite(const float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 1 : 0; }

// a / b and a % b of a wave-uniform step count: 32-bit while the count fits (one reciprocal), the 64-bit routine beyond
__device__ __forceinline__ void divmod(const unsigned long long a, const unsigned b, unsigned long long &quot, unsigned &rem) {
    if ((a >> 32) == 0) {
        const unsigned a32 = (unsigned)a;
        quot = a32 / b;
        rem = a32 % b;
    } else {
        quot = a / b;
        rem = (unsigned)(a % b);
    }
}

// Fold r[] and cnt over the workgroup's 256 threads in one fixed order, into thread 0's registers: 256 -> 128 -> 64 through LDS (the
// upper half of the threads left hands its values to the lower half: each level has its own LDS rows, so one barrier a level), then
// 64 -> 1 inside wave 0 by lane shuffles (x[l] with x[l + 32], + 16, ... + 1).  r[0 .. NS) are sums, the next NMN minima, then maxima.
template <int NS, int NMN, int NMX>
__device__ __forceinline__ void fold(double (&r)[NS + NMN + NMX], int &cnt, double (*sh)[NT / 2 + NT / 4], int *shn, const int t) {
    constexpr int NV = NS + NMN + NMX;
    const auto take = [&](const int v, const double o) __attribute__((always_inline)) {
        if (v < NS) r[v] += o;
        else if (v < NS + NMN) r[v] = fmin(r[v], o);
        else r[v] = fmax(r[v], o);
    };
#pragma unroll
    for (int stride = NT / 2, base = 0; stride >= 64; base += stride, stride >>= 1) {
        if (t >= stride && t < 2 * stride) {
#pragma unroll
            for (int v = 0; v < NV; ++v) sh[v][base + t - stride] = r[v];
            shn[base + t - stride] = cnt;
        }
        __syncthreads();
        if (t < stride) {
#pragma unroll
            for (int v = 0; v < NV; ++v) take(v, sh[v][base + t]);
            cnt += shn[base + t];
        }
    }
    if (t < 64) {
#pragma unroll
        for (int stride = 32; stride >= 1; stride >>= 1) {
#pragma unroll
            for (int v = 0; v < NV; ++v) take(v, __shfl_down(r[v], stride));
            cnt += __shfl_down(cnt, stride);
        }
    }
}

// the record an update with this step count goes to, or nullptr when its step count leaves none
__device__ __forceinline__ Record *slot_of(Record *ring, const int a, const long long step, const int capacity, const int every) {
    if (step < 0) return nullptr;
    unsigned long long index = (unsigned long long)step, lap;
    unsigned rem = 0, slot;
    if (every != 1) divmod((unsigned long long)step, (unsigned)every, index, rem);
    if (rem != 0) return nullptr;
    divmod(index, (unsigned)capacity, lap, slot);
    return ring + ((size_t)a * capacity + slot);
}

__global__ __launch_bounds__(NT) void k_learn_log(const LogJob *__restrict__ jobs, Record *__restrict__ ring, const int B,
                                                  const int capacity, const int every) {
    __shared__ double sh[NROW][NT / 2 + NT / 4];
    __shared__ int shn[NT / 2 + NT / 4];
    constexpr int PER = 1 + 2 * G;
    const int t = threadIdx.x;
    const int a = blockIdx.x / PER, w = blockIdx.x - a * PER;
    // the descriptor through the constant address space (nothing in a launch writes it), the step count through a vector load: as
    // a scalar load it is a second dependent round trip of the scalar cache in front of everything
    const LogJob &J = *(const LogJob *)((const __attribute__((address_space(4))) LogJob *)jobs + a);
    const long long *sp = J.step_dev;
    asm volatile("" : "+v"(sp));
    long long step_v = *sp;
    // every > 1: most launches leave no record, and they return here.  every == 1: only the record's ADDRESS needs the step count,
    // so the loads of the data go out with the load of the count, not behind it (one memory round trip less in front of the sums)
    if (every != 1) {
        const long long step = ((long long)__builtin_amdgcn_readfirstlane((int)(step_v >> 32)) << 32) |
                               (unsigned)__builtin_amdgcn_readfirstlane((int)step_v);
        if (!slot_of(ring, a, step, capacity, every)) return;
    }

    if (w == 0) {
        // [0, 8) sums: (q - y)^2, q_pi, q, y, |y - q|, |dq_da|, |mu|, 1 - mu^2; [8, 10) minima of q, y; [10, 14) maxima of q, y, |y - q|, |dq_da|
        double r[NROW] = {0., 0., 0., 0., 0., 0., 0., 0., INFINITY, INFINITY, -INFINITY, -INFINITY, 0., 0.};
        int bad = 0;
#pragma unroll 4
        for (int b = t; b < B; b += NT) {
            const float yf = J.y[b], qf = J.q[b], pf = J.q_pi[b], df = J.dq_da[b], mf = J.mu[b];
            bad += nonfinite(yf) + nonfinite(qf) + nonfinite(pf) + nonfinite(df) + nonfinite(mf);
            const double y = yf, q = qf, p = pf, d = fabs((double)df), m = mf;
            const double e = q - y, td = fabs(y - q);
            r[0] += e * e;
            r[1] += p;
            r[2] += q;
            r[3] += y;
            r[4] += td;
            r[5] += d;
            r[6] += fabs(m);
            r[7] += 1. - m * m;
            r[8] = fmin(r[8], q); r[9] = fmin(r[9], y);
            r[10] = fmax(r[10], q); r[11] = fmax(r[11], y);
            r[12] = fmax(r[12], td);
            r[13] = fmax(r[13], d);
        }
        fold<NSUM, NMIN, NROW - NSUM - NMIN>(r, bad, sh, shn, t);
        if (t == 0) {
            asm volatile("" : "+v"(step_v));       // (the count is first needed here)
            Record *R = slot_of(ring, a, step_v, capacity, every);
            if (!R) return;
            const double n = (double)B;
            R->v[0] = r[0] / n;                    // critic_loss
            R->v[1] = -(r[1] / n);                 // actor_loss
            R->v[2] = r[2] / n;  R->v[3] = r[8];  R->v[4] = r[10];      // q
            R->v[5] = r[3] / n;  R->v[6] = r[9];  R->v[7] = r[11];      // y
            R->v[8] = r[4] / n;  R->v[9] = r[12];                      // |y - q|
            R->v[10] = r[5] / n; R->v[11] = r[13];                     // |dq_da|
            R->v[12] = r[6] / n;                   // mean |mu|
            R->v[13] = r[7] / n;                   // mean 1 - mu^2
            R->nonfinite = bad;
            R->pad_ = 0;
            R->step = step_v;
        }
        return;
    }

    const int g = (w - 1) / G, c = (w - 1) - g * G;
    const float *__restrict__ x = J.grad[g];
    const int n = J.numel[g];
    const int nvec = (n + 3) >> 2, nfull = n >> 2, per = (nvec + G - 1) / G;
    const int v0 = c * per, v1 = min(nvec, v0 + per), v1full = min(nfull, v1);
    double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
    int bad = 0;
#pragma unroll 4
    for (int i = v0 + t; i < v1full; i += NT) {
        const float4 f = *reinterpret_cast<const float4 *>(x + 4 * i);
        bad += nonfinite(f.x) + nonfinite(f.y) + nonfinite(f.z) + nonfinite(f.w);
        s0 = fma((double)f.x, (double)f.x, s0);
        s1 = fma((double)f.y, (double)f.y, s1);
        s2 = fma((double)f.z, (double)f.z, s2);
        s3 = fma((double)f.w, (double)f.w, s3);
    }
    // the ragged last float4 (numel % 4 elements), by the thread whose turn it would be in the chunk that holds it
    if (nfull < nvec && nfull >= v0 && nfull < v1 && ((nfull - v0) & (NT - 1)) == t) {
        const int e = 4 * nfull;
        const float f0 = x[e], f1 = e + 1 < n ? x[e + 1] : 0.f, f2 = e + 2 < n ? x[e + 2] : 0.f;
        bad += nonfinite(f0) + nonfinite(f1) + nonfinite(f2);
        s0 = fma((double)f0, (double)f0, s0);
        s1 = fma((double)f1, (double)f1, s1);
        s2 = fma((double)f2, (double)f2, s2);
    }
    double r[1] = {((s0 + s1) + s2) + s3};
    fold<1, 0, 0>(r, bad, sh, shn, t);
    if (t == 0) {
        asm volatile("" : "+v"(step_v));
        Record *R = slot_of(ring, a, step_v, capacity, every);
        if (!R) return;
        Part &P = R->part[g * G + c];
        P.sumsq = r[0];
        P.nonfinite = bad;
        P.pad_ = 0;
        P.step = step_v;
    }
}

}  // namespace

struct tt_learn_log {
    int K = 0, B = 0, capacity = 0, every = 1;
    LogJob *jobs = nullptr;
    Record *ring = nullptr;
};

extern "C" {

int tt_learn_log_create(int agents, int batch, const tt_learn_log_job *jobs, int64_t capacity, int32_t every, tt_learn_log **out) {
    if (!out) return fail(TT_EINVAL, "tt_learn_log_create: out is NULL");
    *out = nullptr;
    if (agents < 1 || agents > TT_POP_MAX_AGENTS) return fail(TT_EINVAL, "tt_learn_log_create: agents = %d, not in [1, %d]", agents, TT_POP_MAX_AGENTS);
    if (batch < 1 || batch > MAXB) return fail(TT_EINVAL, "tt_learn_log_create: batch = %d rows, not in [1, %d]", batch, MAXB);
    if (!jobs) return fail(TT_EINVAL, "tt_learn_log_create: jobs is NULL");
    if (capacity < 1 || capacity > TT_LEARN_LOG_MAX_CAPACITY)
        return fail(TT_EINVAL, "tt_learn_log_create: capacity = %d records, not in [1, %d]", (int)std::clamp<int64_t>(capacity, INT32_MIN, INT32_MAX),
                      TT_LEARN_LOG_MAX_CAPACITY);
    if (every < 1) return fail(TT_EINVAL, "tt_learn_log_create: every = %d < 1", every);
    std::vector<LogJob> host(agents);
    for (int a = 0; a < agents; ++a) {
        const tt_learn_log_job &j = jobs[a];
        if (!j.y || !j.q || !j.q_pi || !j.dq_da || !j.mu || !j.grad_critic || !j.grad_actor || !j.step_dev)
            return fail(TT_EINVAL, "tt_learn_log_create: agent %d has a NULL pointer", a);
        if (j.numel_critic <= 0 || j.numel_actor <= 0)
            return fail(TT_EINVAL, "tt_learn_log_create: agent %d: numel <= 0 (numel_critic = %d)", a, j.numel_critic);
        if ((reinterpret_cast<uintptr_t>(j.grad_critic) | reinterpret_cast<uintptr_t>(j.grad_actor)) & 15)
            return fail(TT_EINVAL, "tt_learn_log_create: agent %d: a gradient is not 16-byte aligned", a);
        host[a] = LogJob{j.y, j.q, j.q_pi, j.dq_da, j.mu, {j.grad_critic, j.grad_actor}, {j.numel_critic, j.numel_actor},
                         reinterpret_cast<const long long *>(j.step_dev)};
    }
    LogJob *dj = nullptr;
    Record *ring = nullptr;
    const size_t ring_bytes = sizeof(Record) * (size_t)agents * (size_t)capacity;
    if (hipMalloc(&dj, sizeof(LogJob) * agents) != hipSuccess) return fail(TT_ENOMEM, "tt_learn_log_create: hipMalloc");
    if (hipMalloc(&ring, ring_bytes) != hipSuccess) {
        (void)hipFree(dj);
        return fail(TT_ENOMEM, "tt_learn_log_create: hipMalloc");
    }
    // every byte 0xff: step = -1 in every head and part
    if (hipMemcpy(dj, host.data(), sizeof(LogJob) * agents, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(ring, 0xff, ring_bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        (void)hipFree(dj);
        (void)hipFree(ring);
        return fail(TT_EHIP, "tt_learn_log_create: filling the device block");
    }
    tt_learn_log *h = new tt_learn_log;
    h->K = agents; h->B = batch; h->capacity = (int)capacity; h->every = every;
    h->jobs = dj; h->ring = ring;
    *out = h;
    return TT_OK;
}

int tt_learn_log_append(tt_learn_log *h, tt_stream_t stream) {
    if (!h) return fail(TT_EINVAL, "tt_learn_log_append: handle is NULL");
    hipLaunchKernelGGL(k_learn_log, dim3(h->K * (1 + 2 * G)), dim3(NT), 0, stream, h->jobs, h->ring, h->B, h->capacity, h->every);
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

int tt_learn_log_drain(tt_learn_log *h, int agent, int64_t after_step, int64_t max, int64_t *step_out, double *values_out,
                       int32_t *nonfinite_out, int64_t *count) {
    if (!h) return fail(TT_EINVAL, "tt_learn_log_drain: handle is NULL");
    if (!count) return fail(TT_EINVAL, "tt_learn_log_drain: count is NULL");
    *count = 0;
    if (agent < 0 || agent >= h->K) return fail(TT_EINVAL, "tt_learn_log_drain: agent %d is not in [0, agents = %d)", agent, h->K);
    if (max < 0) return fail(TT_EINVAL, "tt_learn_log_drain: max < 0");
    if (max > 0 && (!step_out || !values_out || !nonfinite_out)) return fail(TT_EINVAL, "tt_learn_log_drain: an output array is NULL");
    std::vector<Record> host(h->capacity);
    if (hipDeviceSynchronize() != hipSuccess) return fail(TT_EHIP, "tt_learn_log_drain: hipDeviceSynchronize");
    if (hipMemcpy(host.data(), h->ring + (size_t)agent * h->capacity, sizeof(Record) * host.size(), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(TT_EHIP, "tt_learn_log_drain: hipMemcpy");
    std::vector<const Record *> found;
    for (int s = 0; s < h->capacity; ++s) {
        const Record &r = host[s];
        if (r.step < 0 || r.step <= after_step || r.step % h->every != 0 || (r.step / h->every) % h->capacity != s) continue;
        bool complete = true;
        for (int p = 0; p < 2 * G; ++p) complete = complete && r.part[p].step == r.step;
        if (complete) found.push_back(&r);
    }
    std::sort(found.begin(), found.end(), [](const Record *x, const Record *y) { return x->step < y->step; });
    const int64_t n = std::min<int64_t>(max, (int64_t)found.size());
    for (int64_t i = 0; i < n; ++i) {
        const Record &r = *found[i];
        step_out[i] = r.step;
        for (int v = 0; v < NROW; ++v) values_out[v * max + i] = r.v[v];
        int bad = r.nonfinite;
        for (int g = 0; g < 2; ++g) {
            double ss = 0.;
            for (int c = 0; c < G; ++c) {              // index order: the one order every drain of these parts adds in
                ss += r.part[g * G + c].sumsq;
                bad += r.part[g * G + c].nonfinite;
            }
            values_out[(NROW + g) * max + i] = std::sqrt(ss);
        }
        nonfinite_out[i] = bad;
    }
    *count = n;
    return TT_OK;
}

int tt_learn_log_clear(tt_learn_log *h, tt_stream_t stream) {
    if (!h) return fail(TT_EINVAL, "tt_learn_log_clear: handle is NULL");
    return hipMemsetAsync(h->ring, 0xff, sizeof(Record) * (size_t)h->K * (size_t)h->capacity, stream) == hipSuccess
               ? TT_OK
               : fail(TT_EHIP, "tt_learn_log_clear: hipMemsetAsync");
}

int tt_learn_log_destroy(tt_learn_log *h) {
    if (!h) return fail(TT_EINVAL, "tt_learn_log_destroy: handle is NULL");
    const hipError_t e = hipFree(h->jobs), e2 = hipFree(h->ring);
    delete h;
    return e == hipSuccess && e2 == hipSuccess ? TT_OK : TT_EHIP;
}

}  // extern "C"
