// ttpop.h -- what the population's translation units (csrc/ttpop.hip, csrc/ttpop_nstep.hip) share: the per-agent descriptor, the
// per-agent n-step table entry and the host launchers of ttpop_nstep.hip's kernels.  The device types are in an anonymous namespace,
// as everything of ttlearn_bodies.h is: each translation unit has its own copy, and the kernels keep their names.
#pragma once
#include "ttlearn_bodies.h"

namespace {

struct PopAgent {
    // k_pop_fwd_multi: the lone sampled launch's argument (R.seed: the key of update 0; update u adds u * R.seed_stride)
    FwdJobs F;
    // k_pop_bwd_rows_pair
    float scale_c;                       // 2 / B
    const float *q_out, *mu_out;         // Q(s, a), mu(s) of the forwards
    Weights Wc, Wa;                      // critic, actor
    Saved sv_c, sv_a;
    BwdOut o_c, o_a;
    TdIn td;
    // k_pop_bwd_weights (critic) and the weight workgroups of k_pop_actor_tail (actor)
    const float *s, *a;                  // the draw's batch buffers
    Grads Gc, Ga;
    AdamFused Ac, Aa;
    RowScale RSa;                        // {dq_da, mu, -1 / B}
    float *q_pi, *dq_da;
    TailSync ts;                         // this agent's own tail words; its epoch is its own step count
};

// agent a's descriptor, as a reference into the constant address space (see the head of the file)
__device__ __forceinline__ const PopAgent &agent_of(const PopAgent *D, const int a) {
    return *(const PopAgent *)((const __attribute__((address_space(4))) PopAgent *)D + a);
}

// agent a's entry of the n-step table (tt_pop_learn_set_nstep): what its draw walks with.  The discount gamma ** n_step is not
// here: it is the agent's td.gamma, where the TD prologue has always read it.
struct PopNstep {
    int n_step;
    float gamma;
};

// agent a's entry of the clip table (tt_pop_learn_set_clip): max_norm of its critic [0] and its actor [1]; 0 = that network is not
// clipped (its coefficient is 1 whatever the norm)
struct PopClip {
    float max_norm[2];
};

}  // namespace

namespace ttpop {

// one table write of tt_pop_exploit_nstep (a launch argument)
struct NstepWrites {
    int n;
    int dst[TT_POP_MAX_AGENTS];
    int n_step[TT_POP_MAX_AGENTS];
    float gamma[TT_POP_MAX_AGENTS];
};

// csrc/ttpop_nstep.hip.  agents: PopAgent[K], table: PopNstep[K], both in device memory.
void launch_fwd_multi_nstep(int K, int n, const void *agents, const void *table, int u, hipStream_t stream);
void launch_set_nstep(const NstepWrites &w, void *table, hipStream_t stream);

// one table write of tt_pop_clip_write (a launch argument)
struct ClipWrites {
    int n;
    int agent[TT_POP_MAX_AGENTS];
    float max_norm[TT_POP_MAX_AGENTS][2];
};

// what tt_pop_learn_set_clip makes, all in device memory: tables AdamTable[K][2] (agent a's tensors of network `net`, with its
// gradients; block_start counts from a * blocks[net], the agent's first workgroup of the clipped optimizer launch), clip PopClip[K],
// partials f64 [K][2][TT_GRAD_CLIP_PARTIALS], out f32 [K][2][2] = {norm, coef}, counts int64 [K][2][2] = {updates, clipped updates}
struct ClipBufs {
    void *tables, *clip, *partials, *out, *counts;
    int blocks[2];              // fill_adam_table's count per network (the same for every agent)
    long long chunk[2];         // ceil(a network's elements / TT_GRAD_CLIP_PARTIALS)
};

// csrc/ttclip.hip.  agents: PopAgent[K] in device memory; net: 0 the critic, 1 the actor.
void launch_pop_grad_sqnorm(int K, int net, const ClipBufs &c, hipStream_t stream);
void launch_pop_adam_soft_clip(int K, int net, const void *agents, const ClipBufs &c, hipStream_t stream);
void launch_clip_write(const ClipWrites &w, void *clip, hipStream_t stream);
// agent a's table of network `net` from its descriptor P (a host copy), its first workgroup at `first_block`; returns the network's
// workgroups, or -1 as fill_adam_table does.  total: the network's elements.
int fill_pop_clip_table(const void *P, int net, int first_block, void *table, long long *total);
size_t clip_table_bytes();

}  // namespace ttpop
