// ttnstep.hip -- n-step returns in the replay draw of the trajectory ring (MI355X, gfx950).  Two kernels beside the one-step
// ones, which stay as they are (csrc/ttnet.hip: k_ring_sample, csrc/ttlearn.hip: k_fwd_multi):
//
//   k_ring_sample_nstep   the lone draw into the batch buffers, one wave per row (tt_ring_sample_nstep)
//   k_fwd_multi_nstep     learn()'s first launch making that draw itself (tt_mlp_forward_multi_sampled_nstep): the sampled
//                         prologue with the n-step pick (TT_SAMPLED_ROWS_NSTEP, csrc/ttlearn_sites.h), then fwd_small_body as there
//
// A batch row is (s, a) of the base step t0, R = the discounted sum of up to n rewards, s' = the observation m steps later and
// D = 1 when a done ended the walk (csrc/ttnstep.h: nstep_pick).  Rows without a done all have the discount gamma^n, so the TD
// prologue of k_bwd_rows_pair takes it by value in tt_td_input.gamma and nothing behind this launch changes.
#include "tthost.h"
#include "ttlearn_bodies.h"
#include "ttnstep.h"

using tthost::fail;

namespace {

// one wave per batch row, the lanes as in ring_sample_row: 0..22 copy s, 32..54 copy s', 63 the scalars
__global__ __launch_bounds__(64) void k_ring_sample_nstep(const ttnet::RingSample R, const int n_step, const float gamma) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= R.batch) return;
    const ttnet::NstepPick p = ttnet::nstep_pick(R, b, n_step, gamma);
    const float *src = ttnet::nstep_s(R, p), *src2 = ttnet::nstep_s2(R, p);
    if (lane < ttnet::IN) R.s_out[(size_t)b * ttnet::IN + lane] = src[lane];
    else if (lane >= 32 && lane < 32 + ttnet::IN) R.s2_out[(size_t)b * ttnet::IN + lane - 32] = src2[lane - 32];
    if (lane == 63) {
        R.a_out[b] = ttnet::nstep_a(R, p);
        R.r_out[b] = p.R;
        R.d_out[b] = (uint8_t)p.D;
        if (R.idx_out) { R.idx_out[2 * b] = p.t0; R.idx_out[2 * b + 1] = p.e; }
    }
}

// learn()'s forwards in one launch with the n-step draw made here (FwdJobs with sampled = 1): workgroup b serves job
// b / blocks_per_job.  The jobs on s read their rows at t0, the jobs on s' at t0 + m; the workgroups of job write_s leave s, a
// (and the index), those of job write_s2 leave s', R, D in the batch buffers for the launches that follow.
__global__ __launch_bounds__(64 * NW) void k_fwd_multi_nstep(const FwdJobs J, const int n_step, const float gamma) {
    __shared__ __attribute__((aligned(16))) float h1_s[H1S_FLOATS];
    __shared__ __attribute__((aligned(16))) float z_s[TR * DS];
    __shared__ __attribute__((aligned(16))) float w1_s[H1 * IN];
    kernarg_warm<(int)sizeof(FwdJobs) + 8>();
    const int job = blockIdx.x / J.blocks_per_job, row0 = (blockIdx.x - job * J.blocks_per_job) * TR;
    const FwdJob &q = J.j[job];
    ttnet::await_progress(J.R.progress, J.R.k_dev);
    if (J.k_snapshot && blockIdx.x == 0 && threadIdx.x == 0) *J.k_snapshot = *J.R.k_dev;
    TT_SAMPLED_ROWS_NSTEP(J.R, J.n, row0, q, job, J.write_s, J.write_s2, n_step, gamma, orow, have_act, act_r0, act_r1);
    if (q.critic)
        fwd_small_body<true>(J.n, q.obs, q.action, q.W, q.out, q.sv, q.dq_da, q.z_state, h1_s, z_s, w1_s, row0, orow, have_act, act_r0, act_r1);
    else
        fwd_small_body<false>(J.n, q.obs, q.action, q.W, q.out, q.sv, nullptr, nullptr, h1_s, z_s, w1_s, row0, orow);
}

// what both entry points refuse beyond make_ring_sample's own checks (host only: no HIP call); `who` names the entry point
int check_nstep(const char *who, const tt_sample_args *a, const int n_step, const float gamma, ttnet::RingSample &R) {
    if (!a) return fail(TT_EINVAL, "%s: no sample (tt_sample_args)", who);
    if (const int rc = tthost::refuse_nstep(who, n_step, gamma)) return rc;
    if (ttnet::make_ring_sample(a, R) != TT_OK) return fail(TT_EINVAL, "%s: bad tt_sample_args", who);
    if (const int rc = tthost::refuse_nstep_window(who, n_step, a->slots, a->reserve)) return rc;
    if (n_step > 1 && R.side.count > 0) return fail(TT_EINVAL, "%s: a side buffer (%d tuples) with n_step %d: side tuples are single steps", who, R.side.count, n_step);
    if (a->draws > 1) return fail(TT_EINVAL, "%s: draws = %d: one draw per launch", who, a->draws);
    return TT_OK;
}

}  // namespace

extern "C" {

int tt_ring_sample_nstep(const tt_sample_args *sample, int n_step, float gamma, tt_stream_t stream) {
    ttnet::RingSample R;
    const int rc = check_nstep("tt_ring_sample_nstep", sample, n_step, gamma, R);
    if (rc != TT_OK || sample->batch == 0) return rc;
    hipLaunchKernelGGL(k_ring_sample_nstep, dim3(sample->batch), dim3(64), 0, stream, R, n_step, gamma);
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

int tt_mlp_forward_multi_sampled_nstep(int n, int count, const tt_fwd_job *jobs, const tt_sample_args *sample, int n_step,
                                       float gamma, int64_t *k_snapshot, tt_stream_t stream) {
    static const char who[] = "tt_mlp_forward_multi_sampled_nstep";
    if (n < 0 || count < 1 || count > 4 || !jobs)
        return fail(TT_EINVAL, "tt_mlp_forward_multi_sampled_nstep: n = %d, count = %d or no jobs", n, count);
    FwdJobs J{};
    const int rc = check_nstep(who, sample, n_step, gamma, J.R);
    if (rc != TT_OK) return rc;
    if (sample->batch != n) return fail(TT_EINVAL, "tt_mlp_forward_multi_sampled_nstep: the draw has %d rows, the forwards %d", sample->batch, n);
    J.n = n;
    J.blocks_per_job = (n + TR - 1) / TR;
    J.write_s = J.write_s2 = -1;
    J.sampled = 1;
    J.R.progress = const_cast<int *>(sample->step_progress);
    J.k_snapshot = reinterpret_cast<long long *>(k_snapshot);
    for (int i = 0; i < count; ++i)
        if (!to_fwd_job(jobs[i], i, sample, J))
            return fail(TT_EINVAL, "tt_mlp_forward_multi_sampled_nstep: forward job %d is incomplete or does not read the draw's buffers", i);
    if (J.write_s < 0 || J.write_s2 < 0)      // the later launches need all five batch buffers
        return fail(TT_EINVAL, "tt_mlp_forward_multi_sampled_nstep: the jobs need at least one on s and one on s'");
    if (n == 0) return TT_OK;
    hipLaunchKernelGGL(k_fwd_multi_nstep, dim3(count * J.blocks_per_job), dim3(64 * NW), 0, stream, J, n_step, gamma);
    return hipGetLastError() == hipSuccess ? TT_OK : TT_EHIP;
}

}  // extern "C"
