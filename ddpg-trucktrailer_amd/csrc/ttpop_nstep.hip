// ttpop_nstep.hip -- n-step returns in a population's learn() (MI355X, gfx950): each agent draws n-step tuples with its own n and
// gamma inside the shared first launch.  Two kernels beside those of csrc/ttpop.hip, which stay as they are:
//
//   k_pop_fwd_multi_nstep   k_pop_fwd_multi with the sampled prologue of k_fwd_multi_nstep (TT_SAMPLED_ROWS_NSTEP,
//                           csrc/ttlearn_sites.h; the pick is csrc/ttnstep.h's); fwd_small_body as there
//   k_pop_set_nstep         the table writes of tt_pop_exploit_nstep, after k_pop_exploit on the same stream
//
// A workgroup takes n_step and gamma from its agent's entry of a table in device memory (PopNstep), read through the constant
// address space as the descriptors are: they are scalars of the workgroup, so nstep_pick's grouped loads stay uniform.  The agent's
// discount gamma ** n_step is its td.gamma, and the three launches behind this one are the one-step population's (csrc/ttnstep.h has
// the argument).  In a translation unit of its own, so that no kernel of ttpop.hip or ttnstep.hip gains a neighbour that shares its
// inlined helpers (the head of ttlearn_sites.h tells why).
#include "ttnstep.h"
#include "ttpop.h"

namespace {

// grid: K x 4 x nb, agent-major; within an agent, job-major as k_fwd_multi.  The jobs on s read their rows at t0, the jobs on s' at
// t0 + m; the workgroups of job write_s leave s, a (and the index), those of job write_s2 leave s', R, D in the batch buffers.
__global__ __launch_bounds__(64 * NW) void k_pop_fwd_multi_nstep(const int K, const int n, const PopAgent *__restrict__ D,
                                                                 const PopNstep *__restrict__ T, const int u) {
    __shared__ __attribute__((aligned(16))) float h1_s[H1S_FLOATS];
    __shared__ __attribute__((aligned(16))) float z_s[TR * DS];
    __shared__ __attribute__((aligned(16))) float w1_s[H1 * IN];
    const int nb = (n + TR - 1) / TR, ag = (int)blockIdx.x / (4 * nb);
    if (ag >= K) return;
    const int lb = (int)blockIdx.x - ag * 4 * nb, job = lb / nb, row0 = (lb - job * nb) * TR;
    const PopAgent &P = agent_of(D, ag);
    const PopNstep &N = *(const PopNstep *)((const __attribute__((address_space(4))) PopNstep *)T + ag);
    const int n_step = N.n_step;
    const float gamma = N.gamma;
    const FwdJob &q = P.F.j[job];
    ttnet::RingSample R = P.F.R;
    R.seed += (unsigned long long)u * R.seed_stride;        // DDPGRollout._sample_key(u)
    TT_SAMPLED_ROWS_NSTEP(R, n, row0, q, job, P.F.write_s, P.F.write_s2, n_step, gamma, orow, have_act, act_r0, act_r1);
    if (q.critic)
        fwd_small_body<true>(n, q.obs, q.action, q.W, q.out, q.sv, q.dq_da, q.z_state, h1_s, z_s, w1_s, row0, orow, have_act, act_r0, act_r1);
    else
        fwd_small_body<false>(n, q.obs, q.action, q.W, q.out, q.sv, nullptr, nullptr, h1_s, z_s, w1_s, row0, orow);
}

// one workgroup: thread i writes dst[i]'s table entry, with plain global stores (read by the later launches on the stream, the
// contract of k_pop_exploit's hyperparameter words)
__global__ __launch_bounds__(64) void k_pop_set_nstep(const ttpop::NstepWrites W, PopNstep *__restrict__ T) {
    const int i = threadIdx.x;
    if (i >= W.n) return;
    T[W.dst[i]].n_step = W.n_step[i];
    T[W.dst[i]].gamma = W.gamma[i];
}

}  // namespace

namespace ttpop {

void launch_fwd_multi_nstep(int K, int n, const void *agents, const void *table, int u, hipStream_t stream) {
    const int nb = (n + TR - 1) / TR;
    hipLaunchKernelGGL(k_pop_fwd_multi_nstep, dim3(K * 4 * nb), dim3(64 * NW), 0, stream, K, n, static_cast<const PopAgent *>(agents),
                       static_cast<const PopNstep *>(table), u);
}

void launch_set_nstep(const NstepWrites &w, void *table, hipStream_t stream) {
    hipLaunchKernelGGL(k_pop_set_nstep, dim3(1), dim3(64), 0, stream, w, static_cast<PopNstep *>(table));
}

}  // namespace ttpop
