// ttlearn_sites.h -- device text that several of learn()'s kernels hold word for word, written ONCE: the sampled-row prologue of the
// first launch (one-step and n-step), the two halves of the actor tail, the front of the rows-pair launch and the element update of
// the optimizer launches.  The kernels that use it are in csrc/ttlearn.hip, ttpop.hip, ttnstep.hip, ttpop_nstep.hip, tttd3.hip,
// ttpop_td3.hip, ttshape.hip, ttdemo.hip and ttclip.hip.
//
// These are function-like MACROS, not functions, on purpose.  As __forceinline__ functions (the job indices by value or by
// reference alike) the prologue and the tail changed the instructions of the kernels they served: csrc/ttpop.hip came out different
// in 1320 hunks of k_pop_fwd_multi's assembly and 17 of k_pop_actor_tail's -- register numbering, load order and a few other
// instructions -- although every call was inlined.  As text the compiler sees what it saw when each kernel had its own copy, and
// the .text section of every code object of the library stays byte for byte what it was.  That is the gate of every change to this
// file that is not meant to change a kernel:
//
//     python -m ddpg_trucktrailer_amd.kernel_resources --text before.so after.so
//
// Do not bridge two of the macros with an inline adaptor function, and do not turn one into a function, without that comparison.
//
// Rules of the text: an argument is an expression of the SITE and is pasted as written (`blockIdx.x` stays unsigned, `J.R` stays a
// kernel argument, `R` a local copy); outputs are variables the site has declared and names declared here live in the macro's own
// block -- except in TT_SAMPLED_ROWS_NSTEP, which tells why, and in TT_BWD_ROWS_PAIR_FRONT and TT_ADAM_SOFT_ELEMENT, which are the
// opening text of their kernels.  What differs between sites stays at the site: finding the agent and the job, the seed of the launch's draw,
// await_progress and the snapshots of the step numbers, KBEGIN / KEND, the load of the epoch.
#pragma once

// ---- the sampled-row prologue of learn()'s first launch: one-step draw ----
// SMP: the launch's ttnet::RingSample (an lvalue: `J.R`, or a local copy `R`), n: batch rows, row0: the workgroup's first row, q: its FwdJob, job: the job's number,
// write_s / write_s2: the jobs whose workgroups leave the batch rows for the later launches.
// Out: orow = the lane's row of the draw (s or s' in the ring; lanes l15 = 0..15 hold the workgroup's 16 rows), and -- a critic job
// with an action -- have_act and the wave's two actions.
// The workgroups of job write_s copy s, a and the draw's index, those of job write_s2 copy s', r, d into the batch buffers: thread
// i < 16 x 23 copies one feature.  (Loads here and the stores after the forward -- so that its own loads do not queue behind this
// copy -- changed nothing: 18.2 us for the slowest workgroup either way.)
#define TT_SAMPLED_ROWS(SMP, n, row0, q, job, write_s, write_s2, orow, have_act, act_r0, act_r1)                                        \
    do {                                                                                                                                \
        static_assert(TR / NW == 2, "two rows per wave");                                                                               \
        const int tid = threadIdx.x, wave = tid >> 6, l15 = tid & 15;                                                                   \
        const bool from_s = (q).obs == (SMP).s_out; /* this job reads s (else s') */                                                    \
        {                                                                                                                               \
            const ttnet::RingPick p = ttnet::ring_sample_index(SMP, min((row0) + l15, (n) - 1));                                        \
            orow = from_s ? ttnet::ring_pick_s(SMP, p) : ttnet::ring_pick_s2(SMP, p);                                                   \
        }                                                                                                                               \
        if ((q).critic && (q).action) {                                                                                                 \
            act_r0 = ttnet::ring_pick_a(SMP, ttnet::ring_sample_index(SMP, min((row0) + wave * 2, (n) - 1)));                           \
            act_r1 = ttnet::ring_pick_a(SMP, ttnet::ring_sample_index(SMP, min((row0) + wave * 2 + 1, (n) - 1)));                       \
            have_act = true;                                                                                                            \
        }                                                                                                                               \
        if ((job) == (write_s) || (job) == (write_s2)) {                                                                                \
            const int lr = tid / ttnet::IN, c = tid - lr * ttnet::IN, b = (row0) + lr;                                                  \
            if (lr < TR && b < (n)) {                                                                                                   \
                const ttnet::RingPick p = ttnet::ring_sample_index(SMP, b);                                                             \
                if ((job) == (write_s)) {                                                                                               \
                    (SMP).s_out[(size_t)b * ttnet::IN + c] = ttnet::ring_pick_s(SMP, p)[c];                                             \
                    if (c == 0) {                                                                                                       \
                        (SMP).a_out[b] = ttnet::ring_pick_a(SMP, p);                                                                    \
                        if ((SMP).idx_out) { (SMP).idx_out[2 * b] = p.side ? -1 : p.t; (SMP).idx_out[2 * b + 1] = p.side ? p.j : p.e; } \
                    }                                                                                                                   \
                }                                                                                                                       \
                if ((job) == (write_s2)) {                                                                                              \
                    (SMP).s2_out[(size_t)b * ttnet::IN + c] = ttnet::ring_pick_s2(SMP, p)[c];                                           \
                    if (c == 0) { (SMP).r_out[b] = ttnet::ring_pick_r(SMP, p); (SMP).d_out[b] = ttnet::ring_pick_d(SMP, p); }           \
                }                                                                                                                       \
            }                                                                                                                           \
        }                                                                                                                               \
    } while (0)

// ---- the same with the n-step pick (csrc/ttnstep.h: nstep_pick; the site includes that header) ----
// A second body, not an adaptor over the first: the pick's type, R and D taken from the pick, and orow through a BRANCH, not a
// select -- only the rows at t0 + m need the walk's done flags.  The jobs on s read their rows at t0, the jobs on s' at t0 + m.
// Unlike TT_SAMPLED_ROWS this one DECLARES its four outputs, and tid, wave, l15 and from_s with them, in the kernel's scope: with
// have_act and the two actions declared in front of tid, k_pop_fwd_multi_nstep came out with three of its instructions in another
// order.  Both sites draw unconditionally, so nothing needs the outputs before this text.
#define TT_SAMPLED_ROWS_NSTEP(SMP, n, row0, q, job, write_s, write_s2, n_step, gamma, orow, have_act, act_r0, act_r1)                   \
    static_assert(TR / NW == 2, "two rows per wave");                                                                                   \
    const int tid = threadIdx.x, wave = tid >> 6, l15 = tid & 15;                                                                       \
    const bool from_s = (q).obs == (SMP).s_out; /* this job reads s (else s') */                                                        \
    const float *orow;                                                                                                                  \
    if (from_s) orow = ttnet::nstep_s(SMP, ttnet::nstep_pick(SMP, min((row0) + l15, (n) - 1), n_step, gamma));                          \
    else orow = ttnet::nstep_s2(SMP, ttnet::nstep_pick(SMP, min((row0) + l15, (n) - 1), n_step, gamma));                                \
    bool have_act = false;                                                                                                              \
    float act_r0 = 0.f, act_r1 = 0.f;                                                                                                   \
    if ((q).critic && (q).action) {                                                                                                     \
        act_r0 = ttnet::nstep_a(SMP, ttnet::nstep_pick(SMP, min((row0) + wave * 2, (n) - 1), n_step, gamma));                           \
        act_r1 = ttnet::nstep_a(SMP, ttnet::nstep_pick(SMP, min((row0) + wave * 2 + 1, (n) - 1), n_step, gamma));                       \
        have_act = true;                                                                                                                \
    }                                                                                                                                   \
    if ((job) == (write_s) || (job) == (write_s2)) {                                                                                    \
        const int lr = tid / ttnet::IN, c = tid - lr * ttnet::IN, b = (row0) + lr;                                                      \
        if (lr < TR && b < (n)) {                                                                                                       \
            const ttnet::NstepPick p = ttnet::nstep_pick(SMP, b, n_step, gamma);                                                        \
            if ((job) == (write_s)) {                                                                                                   \
                (SMP).s_out[(size_t)b * ttnet::IN + c] = ttnet::nstep_s(SMP, p)[c];                                                     \
                if (c == 0) {                                                                                                           \
                    (SMP).a_out[b] = ttnet::nstep_a(SMP, p);                                                                            \
                    if ((SMP).idx_out) { (SMP).idx_out[2 * b] = p.t0; (SMP).idx_out[2 * b + 1] = p.e; }                                 \
                }                                                                                                                       \
            }                                                                                                                           \
            if ((job) == (write_s2)) {                                                                                                  \
                (SMP).s2_out[(size_t)b * ttnet::IN + c] = ttnet::nstep_s2(SMP, p)[c];                                                   \
                if (c == 0) { (SMP).r_out[b] = p.R; (SMP).d_out[b] = (uint8_t)p.D; }                                                    \
            }                                                                                                                           \
        }                                                                                                                               \
    }

// ---- the actor tail, row half: a row workgroup of Q(s, mu(s)) and dQ/da through the UPDATED critic ----
// lds: the kernel's one LDS array of H1S_FLOATS + TR * DS + H1 * IN floats; lb: the workgroup's number among its agent's row
// workgroups; epoch: the learn step (the site loads it).  Hand-over order: every wave's row words have left (vmcnt(0)), the
// workgroup's barrier, then ONE relaxed agent-scope store of the epoch into the workgroup's hint (TailSync, ttlearn_bodies.h).
// DEMO, demo: the demonstration loss's term in the dQ/da a row hands on (csrc/ttdemo.hip; fwd_small_body's DemoIn); the plain form
// passes fwd_small_body's defaults.
#define TT_ACTOR_TAIL_ROWS_DEMO(DEMO, n, obs, mu, Wc, q_out, dq_da, lds, ts, lb, epoch, demo)                                           \
    do {                                                                                                                                \
        const Saved none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};                                                         \
        fwd_small_body<true, NoHook, DEMO>(n, obs, mu, Wc, q_out, none, dq_da, nullptr, lds, (lds) + H1S_FLOATS,                        \
                                           (lds) + H1S_FLOATS + TR * DS, (lb) * TR, nullptr, false, 0.f, 0.f, ts.rows,                  \
                                           (unsigned)(epoch), nullptr, NoHook(), demo);                                                 \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* every wave: its rows' words have been sent */                               \
        __syncthreads();                                                                                                                \
        if (threadIdx.x == 0) __hip_atomic_store(ts.hints + (lb), (int)(epoch), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);            \
    } while (0)
#define TT_ACTOR_TAIL_ROWS(n, obs, mu, Wc, q_out, dq_da, lds, ts, lb, epoch)                                                            \
    TT_ACTOR_TAIL_ROWS_DEMO(false, n, obs, mu, Wc, q_out, dq_da, lds, ts, lb, epoch, DemoIn{})

// ---- the actor tail, weight half: a weight-gradient workgroup (its first 256 threads) carves the row kernel's LDS ----
// blk: the workgroup's number among its agent's WG_ACTOR_WEIGHTS.  PREPEN, pre_scale, pre: the loss shape's penalty term
// (csrc/ttshape.hip); the plain form passes bwd_weights_body's defaults.
#define TT_ACTOR_TAIL_WEIGHTS_SHAPED(PREPEN, blk, n, obs, sv, d, G, A, RS, lds, ts, epoch, pre_scale, pre)                              \
    do {                                                                                                                                \
        static_assert(sizeof(lds) >= sizeof(float) * (4 * 4 * 256 + MAXB + 2048), "the weight kernel's LDS fits");                      \
        float (&part)[4][4][256] = *reinterpret_cast<float (*)[4][4][256]>(lds);                                                        \
        bwd_weights_body<true, true, PREPEN>(blk, n, 0, obs, nullptr, sv, d, G, A, RS, part, (lds) + 4 * 4 * 256, ts, epoch,            \
                                             reinterpret_cast<_Float16 *>((lds) + 4 * 4 * 256 + MAXB), pre_scale, pre);                 \
    } while (0)
#define TT_ACTOR_TAIL_WEIGHTS(blk, n, obs, sv, d, G, A, RS, lds, ts, epoch)                                                             \
    TT_ACTOR_TAIL_WEIGHTS_SHAPED(false, blk, n, obs, sv, d, G, A, RS, lds, ts, epoch, 0.f, nullptr)

// ---- the front of k_bwd_rows_pair and k_bwd_rows_pair_shaped: everything before the row workgroups ----
// Declares nb (the row workgroups per net) in the kernel's scope; the tick workgroup and the image's workgroups RETURN from the
// kernel here.
#define TT_BWD_ROWS_PAIR_FRONT(nb, n, td, img)                                                                                          \
    kernarg_warm<16 + 2 * ((int)sizeof(Weights) + (int)sizeof(Saved) + (int)sizeof(BwdOut)) + (int)sizeof(TdIn) + 8>();                 \
    const int nb = ((n) + TR - 1) / TR;                                                                                                 \
    if ((int)blockIdx.x == 2 * nb) { /* the extra workgroup: counters + bias corrections (nothing in this launch reads them) */         \
        if (threadIdx.x == 0) clock_tick(td);                                                                                           \
        return;                                                                                                                         \
    }                                                                                                                                   \
    if ((int)blockIdx.x > 2 * nb) { /* the image's workgroups (they read a SNAPSHOT of the step number: see ImageJob) */                \
        ttnet::split_pack_body((img).W, false, (img).ws, (img).ws_alt, nullptr, (img).cur,                                              \
                               ((int)blockIdx.x - 2 * nb - 1) * (64 * NW) + (int)threadIdx.x);                                          \
        ttnet::publish_image((img).cur, IMAGE_WGS);                                                                                     \
        return;                                                                                                                         \
    }

// ---- one element of the optimizer launches of their own: k_adam_soft (csrc/ttlearn.hip) and k_adam_soft_clip (csrc/ttclip.hip) ----
// torch.optim.Adam (amsgrad off, weight decay added to the gradient) on element i of the tensor the workgroup belongs to, the soft
// target update and the fc2 image stores; the threads past the tensor's end RETURN from the kernel here.  GRAD: the element's
// gradient, an expression in ti and i (declared here) -- what the two kernels differ in.  The rest are the kernels' argument names.
#define TT_ADAM_SOFT_ELEMENT(GRAD)                                                                                                      \
    int ti = 0;                                                                                                                         \
    while (ti + 1 < T.count && (int)blockIdx.x >= T.block_start[ti + 1]) ++ti;                                                          \
    const int i = ((int)blockIdx.x - T.block_start[ti]) * 256 + threadIdx.x;                                                            \
    if (i >= T.numel[ti]) return;                                                                                                       \
    float bcc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};                                                                                           \
    if (bias_corr) {                                                                                                                    \
        _Pragma("unroll")                                                                                                               \
        for (int q = 0; q < 5; ++q) bcc[q] = bias_corr[q];                                                                              \
    }                                                                                                                                   \
    float bc1, bc2;                                                                                                                     \
    adam_bias_corrections(beta1, beta2, *step_dev, bias_corr != nullptr, bcc, bc1, bc2);                                                \
    float p = T.p[ti][i];                                                                                                               \
    const float g = fmaf(weight_decay, p, GRAD);                                                                                        \
    const float m = fmaf(beta1, T.m[ti][i], (1.f - beta1) * g); /* exp_avg.lerp_(grad, 1 - beta1) */                                    \
    const float v = fmaf(beta2, T.v[ti][i], (1.f - beta2) * g * g);                                                                     \
    T.m[ti][i] = m;                                                                                                                     \
    T.v[ti][i] = v;                                                                                                                     \
    const float denom = sqrtf(v) / sqrtf(bc2) + eps;                                                                                    \
    p -= (lr / bc1) * (m / denom);                                                                                                      \
    T.p[ti][i] = p;                                                                                                                     \
    float tg = 0.f;                                                                                                                     \
    if (T.tgt[ti]) {                                                                                                                    \
        tg = T.tgt[ti][i];                                                                                                              \
        tg = fmaf(tau, p - tg, tg);                                                                                                     \
        T.tgt[ti][i] = tg;                                                                                                              \
    }                                                                                                                                   \
    if (ti == 4 && (T.img_p || T.img_t)) {                                                                                              \
        const int nn = i / H1, k = i - nn * H1;                                                                                         \
        if (T.img_p) img_store(T.img_p, nn, k, p, true);                                                                                \
        if (T.img_t && T.tgt[ti]) img_store(T.img_t, nn, k, tg, false);                                                                 \
    }
