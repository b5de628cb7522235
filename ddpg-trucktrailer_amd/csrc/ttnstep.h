// ttnstep.h -- the n-step replay draw from the trajectory ring (include/ttenv.h: tt_ring_sample_nstep has the semantics).
//
// The ring is time-major, so the n steps of env e after a stored transition (t0, e) sit next to it: rew[t0 + j][e], done[t0 + j][e].
// The base step is drawn only from positions whose n steps lie inside the intact window; then a row either has no `done` among
// its n steps -- discount gamma^n, the same for every such row, which the TD launch takes by value -- or ends at the first done
// (D = 1: the TD prologue ignores q' and the discount).  So only the draw differs from the one-step learn().
//
// nstep_pick() is what both kernels of csrc/ttnstep.hip call, so the lone draw and learn()'s own draw agree bit for bit.  A caller
// that does not use R (or m, D) pays nothing for it: the loads behind an unused member are dropped by the compiler.
#pragma once
#include "ttnet_common.h"

namespace ttnet {

struct NstepPick {
    int t0, m, e;      // slot of the base step, steps taken (1 .. n_step), env
    int t2;            // slot of s' = (t0 + m) mod slots
    float R;           // r_t0 + gamma r_(t0+1) + ... + gamma^(m-1) r_(t0+m-1), f32, fused multiply-adds in this order
    int D;             // 1: a done at step t0 + m - 1 ended the walk
};

// Batch row b of the draw R (n_step in 1 .. TT_NSTEP_MAX; the host checks it).  Philox call, key and counter are those of
// ring_sample_index, r[0] picks the step and r[1] the env; n_step = 1 is that function's ring draw bit for bit.
__device__ __forceinline__ NstepPick nstep_pick(const RingSample &R, const int b, const int n_step, const float gamma) {
    const int n_envs = R.n_envs, slots = R.slots;
    const long long k0 = *R.k_dev - R.lag, k = k0 > 0 ? k0 : 0;
    const long long cap = slots - 1 - R.reserve;
    const long long avail = k < cap ? k : cap;
    const long long avail_n0 = avail - (n_step - 1), avail_n = avail_n0 > 1 ? avail_n0 : 1;      // (< 1: an early launch; rows are in-bounds, meaningless)
    uint32_t r[4];
    philox4x32((uint32_t)b, (uint32_t)k, (uint32_t)(k >> 32), 0x5A3Du, (uint32_t)R.seed, (uint32_t)(R.seed >> 32), r);
    const long long back = (n_step - 1) + (long long)(((unsigned long long)r[0] * (unsigned long long)avail_n) >> 32);
    NstepPick p;
    p.t0 = (int)(((k - 1 - back) % slots + slots) % slots);
    p.e = (int)(((unsigned long long)r[1] * (unsigned long long)n_envs) >> 32);
    // The n rewards and n done flags: every load of a group of four leaves before anything is looked at, from addresses inside the
    // ring whatever the flags will say (steps beyond n_step - 1 re-read step n_step - 1).  A walk that loads step j + 1 only once
    // done[j] is known is n dependent round trips to L2 (the reason bwd_rows_body's phase A gives for its own loads).
    float rw[TT_NSTEP_MAX];
    uint8_t dn[TT_NSTEP_MAX];
    int sl = p.t0;
#pragma unroll
    for (int c = 0; c < TT_NSTEP_MAX; c += 4) {
        if (c < n_step) {                                 // (uniform: n_step is a launch constant)
#pragma unroll
            for (int j = c; j < c + 4; ++j) {
                const size_t at = (size_t)sl * n_envs + p.e;
                rw[j] = R.rew[at];
                dn[j] = R.done[at];
                if (j + 1 < n_step) sl = sl + 1 == slots ? 0 : sl + 1;
            }
        } else {
#pragma unroll
            for (int j = c; j < c + 4; ++j) { rw[j] = 0.f; dn[j] = 0; }
        }
    }
    // step 0 enters as it is stored (1 * r + 0 is r, and a reward of -0 keeps its sign: n_step = 1 leaves tt_ring_sample's bits)
    float g = gamma, sum = rw[0];
    int m = n_step, D = dn[0] ? 1 : 0;
    if (D) m = 1;
#pragma unroll
    for (int j = 1; j < TT_NSTEP_MAX; ++j) {
        const bool use = j < n_step && !D;
        sum = use ? fmaf(g, rw[j], sum) : sum;
        if (use && dn[j]) { D = 1; m = j + 1; }
        g *= gamma;
    }
    p.m = m;
    p.R = sum;
    p.D = D;
    const int t2 = p.t0 + m;                              // m <= 16, slots >= 3: at most a few turns
    p.t2 = t2 % slots;
    return p;
}

// the picked row's pieces: s and a at the base step, s' m steps later
__device__ __forceinline__ const float *nstep_s(const RingSample &R, const NstepPick &p) {
    return R.obs + ((size_t)p.t0 * R.n_envs + p.e) * IN;
}
__device__ __forceinline__ const float *nstep_s2(const RingSample &R, const NstepPick &p) {
    return R.obs + ((size_t)p.t2 * R.n_envs + p.e) * IN;
}
__device__ __forceinline__ float nstep_a(const RingSample &R, const NstepPick &p) {
    return R.act[(size_t)p.t0 * R.n_envs + p.e];
}

}  // namespace ttnet
