// ttenv_step.h -- env.step for one env held in registers: StepOut, step_env, and the info rows a step may write (Info, write_info).
// Every kernel that steps an env (k_step and its log / curriculum forms, k_rollout, k_step_hold, the MPC planner) calls step_env.
// Part of csrc/ttenv.hip's translation unit, inside its anonymous namespace.  Needs ttenv.h (TT_V_*, TT_F_*, TT_I_*), ttenv_math.h
// and ttenv_state.h before it.
#pragma once

struct Info {
    double *comp;
    uint8_t *violation;
    uint8_t *flags;
};

struct StepOut {
    double total, c_prog, c_head, c_orient, staged, safety, explore, final_bonus, back, c_smooth, budget;
    uint32_t viol, flags;
    bool done;
};

// env.step for one env held in registers (simv2.py:499-545 + reward_functionv1.py:442-506)
__device__ __forceinline__ void step_env(const KParams &P, Env &e, float action, float *of, StepOut &o) {
    const KTable &T = kTable;
    // ---- simv2.py:504-505: clip in f64 against np.radians(45)
    const double delta = fmin(fmax((double)action, -P.max_steer), P.max_steer);
    double sd, cd;
    tt_sincos(T, delta, sd, cd);
    const double w1 = P.v_over_L1 * (sd / cd);  // truck yaw rate, constant over the step

    // ---- one Dormand-Prince step (scipy RK45 tableau).  Positions do not feed back, so they are accumulated
    // straight into their B-weighted sums; every stage's sin/cos is a small rotation of the initial ones.
    const double h = P.h, v = P.v, vL2 = P.v / e.L2, hoL2 = P.ho / e.L2, how1 = P.ho * w1;
    double sp1, cp1, sp2, cp2;
    tt_sincos(T, e.psi1, sp1, cp1);
    tt_sincos(T, e.psi2, sp2, cp2);
    const double beta = h * w1;
    double k2[6];
    double ax1 = 0.0, ay1 = 0.0, ax2 = 0.0, ay2 = 0.0, apsi2 = 0.0;
    double s1 = sp1, c1 = cp1;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        double s2 = sp2, c2 = cp2;
        if (s > 0) {
            double acc = T.A[s][0] * k2[0];
#pragma unroll
            for (int j = 1; j < s; ++j) acc = fma(T.A[s][j], k2[j], acc);
            double sb, cb, sg2, cg2;
            tt_sincos_small(T, T.C[s] * beta, sb, cb);
            tt_sincos_small(T, h * acc, sg2, cg2);
            s1 = sp1 * cb + cp1 * sb; c1 = cp1 * cb - sp1 * sb;
            s2 = sp2 * cg2 + cp2 * sg2; c2 = cp2 * cg2 - sp2 * sg2;
        }
        const double sth = s1 * c2 - c1 * s2, cth = c1 * c2 + s1 * s2;
        const double v2 = v * cth + how1 * sth;
        k2[s] = vL2 * sth - hoL2 * w1 * cth;
        if (s != 1) {  // B[1] = 0
            const double bs = T.B[s];
            apsi2 = fma(bs, k2[s], apsi2);
            ax1 = fma(bs, v * c1, ax1);
            ay1 = fma(bs, v * s1, ay1);
            ax2 = fma(bs, v2 * c2, ax2);
            ay2 = fma(bs, v2 * s2, ay2);
        }
    }
    // stage 6 sits at c = 1: its truck heading IS the new truck heading, so (s1, c1) carry over
    e.psi1 += beta;
    const double dpsi2 = h * apsi2;
    e.psi2 += dpsi2;
    e.x1 = fma(h, ax1, e.x1); e.y1 = fma(h, ay1, e.y1); e.x2 = fma(h, ax2, e.x2); e.y2 = fma(h, ay2, e.y2);
    double s2, c2;
    {
        double sg2, cg2;
        tt_sincos_small(T, dpsi2, sg2, cg2);
        s2 = sp2 * cg2 + cp2 * sg2; c2 = cp2 * cg2 - sp2 * sg2;
    }

    // ---- observation (simv2.py:519), cast to f32 like np.array(..., dtype=float32)
    const double dx = e.g.gx - e.x2, dy = e.g.gy - e.y2;
    const double cur = sqrt(dx * dx + dy * dy);
    const uint32_t pk = e.pk;
    const uint32_t steps = pk_steps(pk) + 1u;  // episode_steps is incremented before the reward (simv2.py:523)
    uint32_t stages = pk_stages(pk);
    const double init = e.dinit + 1e-6;

    // The reward's three tanh -- dynamic weights (:189-238): tanh(7(jp - 0.3)); progress (:144-187):
    // tanh(prev - cur), tanh((hist[0] - cur)/2) -- are (1 - t)/(1 + t), t = exp(-2|x|).  Two of them, 1/cur
    // and 1/init share ONE division through the product of the denominators.
    const bool first = pk_age(pk) == 0u || P.stateless != 0;  // reward_state is None (:40-76)
    const uint32_t age = first ? 1u : pk_age(pk) + 1u;         // step_count_for_backward_tracking after this step (:258)
    const double prev = first ? cur : e.prev, d3 = first ? cur : e.d3, d1 = first ? cur : e.d1;
    const double inst = prev - cur;
    const double net = (d3 - cur) * 0.5;
    const double t_i = tt_exp_neg(T, -2.0 * fabs(inst)), t_n = tt_exp_neg(T, -2.0 * fabs(net));
    const double q_i = 1.0 + t_i, q_n = 1.0 + t_n;
    const double cur_s = cur > 0.0 ? cur : 1.0;
    const double qq = q_i * q_n, ci = cur_s * init;
    const double r_all = 1.0 / (qq * ci);
    const double inv_cur = cur > 0.0 ? r_all * (qq * init) : 0.0;
    const double inv_init = r_all * (qq * cur_s);
    const double th = copysign((1.0 - t_i) * (r_all * (ci * q_n)), inst);
    const double tn = copysign((1.0 - t_n) * (r_all * (ci * q_i)), net);

    observe(P, e.g, e.x1, e.y1, e.x2, e.y2, s1, c1, s2, c2, sd, cd, dx, dy, cur, inv_cur, of);

    // ---- reward (reward_functionv1.py:442-506)
    // int(initial_distance / 0.40096) + 75 (:38): the quotient by one multiplication, and by the real division (what
    // numpy does) only where the two could truncate differently -- next to an integer (wave-uniform, almost never)
    const double rq = init * P.inv_step_length;
    int rmax = (int)rq;
    if (__any(fabs(rq - rint(rq)) <= 1e-11 * rq)) rmax = (int)(init / P.step_length);
    rmax += P.extra_steps;
    const float steer_now = tt_atan2_readback(delta, sd, cd, of[10], of[11]);  // np.arctan2(obs[10], obs[11]) (:37)
    if (first) {
        e.cum = 0.0;
        e.closest = cur;
        e.psteer = steer_now;
        stages = 0u;
    } else if (cur < e.closest) {
        e.closest = cur;
    }
    const double jp = fmin(fmax((init - cur) * inv_init, 0.0), 1.0);
    const double wa = 7.0 * (jp - 0.3);
    const double t_w = tt_exp_neg(T, -2.0 * fabs(wa));
    const double tw = copysign((1.0 - t_w) / (1.0 + t_w), wa);
    const double w_orient = (tw + 1.0) * 0.5;
    const double w_head = 1.0 - w_orient;
    const bool mono = (d1 >= prev) && (prev >= cur);
    const double progress = (inst > 0.0 ? th : th * 0.5) + tn * 0.5 + (mono ? 0.2 : 0.0);
    // heading (:285-309): cos(atan2(dy,dx) - (co + pi)) with co = np.arctan2(obs[6], obs[7]) in f32.
    // co = wrap(psi2) + eps with |eps| ~ 1e-7, so its sin/cos are a rotation of (s2, c2) by eps.
    double heading;
    {
        const double w2 = tt_wrap_pi(T, e.psi2);
        const double eps = (double)tt_atan2_readback(w2, s2, c2, of[6], of[7]) - w2;
        const double half = 1.0 - 0.5 * eps * eps;
        const double sco = s2 * half + c2 * eps, cco = c2 * half - s2 * eps;
        heading = cur > 0.0 ? -(dx * cco + dy * sco) * inv_cur : -cco;
    }
    // orientation (:311-324): f32 * 15.0 stays f32 in numpy
    const float orient15 = of[20] * 15.0f;
    // staged bonuses (:338-367) and success: only within 5 m of the goal (wave-uniform skip otherwise)
    double staged = 0.0;
    bool at_goal = false;
    if (__any(cur <= 5.0)) {
        // |np.arctan2(obs[19], obs[20])| with obs[19], obs[20] = sin, cos(goalyaw - psi2)
        const double oa = tt_wrap_pi(T, e.gyaw - e.psi2);
        const double ori_err = (double)fabsf(tt_atan2_readback(oa, e.g.sg * c2 - e.g.cg * s2, e.g.cg * c2 + e.g.sg * s2,
                                                               of[19], of[20]));
        if (cur <= 5.0) staged += 10.0;   // every step, no latch (Q2)
        if (cur <= 2.0 && ori_err <= 45.0 * kDeg && !(stages & 1u)) { staged += 25.0; stages |= 1u; }
        at_goal = cur <= P.pos_thr && ori_err <= P.ori_thr;
        if (at_goal && !(stages & 2u)) { staged += 100.0; stages |= 2u; }
    }
    // safety (:369-421)
    double safety = 0.0;
    uint32_t viol = TT_V_NONE;
    const double hitch = fabs(e.psi1 - e.psi2);
    if (hitch > 85.0 * kDeg) { safety += -500.0; viol = TT_V_JACKKNIFE; }
    else if (hitch > 70.0 * kDeg) { safety += -50.0; viol = TT_V_JACKKNIFE_WARNING; }
    const double lox = fmin(e.x1, e.x2), hix = fmax(e.x1, e.x2), loy = fmin(e.y1, e.y2), hiy = fmax(e.y1, e.y2);
    const bool outside = lox < P.minx || hix > P.maxx || loy < P.miny || hiy > P.maxy;
    if (lox < P.minx - 2.0 || hix > P.maxx + 2.0 || loy < P.miny - 2.0 || hiy > P.maxy + 2.0) {
        safety += -500.0; viol = TT_V_MAJOR_BOUNDARY;
    } else if (outside) {
        safety += -50.0; viol = TT_V_MINOR_BOUNDARY;
    }
    const bool passed = e.g.gy > e.y2;
    if (passed) { safety += -500.0; viol = TT_V_PAST_THE_GOAL; }
    if ((int)steps >= rmax) { safety += -500.0; viol = TT_V_MAX_STEP; }
    const bool excessive = cur > e.closest + 6.0;  // :120-124
    if (excessive) { safety += -500.0; viol = TT_V_EXCESSIVE_BACKWARD; }
    // exploration (:423-439)
    const double explore = (double)steps < rmax * 0.5 ? 4.0 : ((double)steps < rmax * 0.8 ? 2.0 : 0.0);
    // backward-movement budget (:240-283)
    e.cum += fmax(0.0, cur - prev);
    const double budget = 5.0 * fmin(1.0, (double)age * 0.02);  // step_count_for_backward_tracking (stateless: always 1)
    const double excess = fmax(0.0, e.cum - budget);
    double back = 0.0;
    if (__any(excess > 0.0)) back = excess > 0.0 ? -(excess * sqrt(excess)) * 0.5 : 0.0;
    // smoothness against the episode's FIRST steering (:326-335; previous_steering is never refreshed)
    const double smooth = (double)fabsf(steer_now - e.psteer) * (1.0 / (90.0 * kDeg));
    o.final_bonus = at_goal ? 200.0 : 0.0;

    o.c_prog = progress * 15.0; o.c_head = heading * 15.0 * w_head;
    o.c_orient = (double)orient15 * w_orient; o.c_smooth = smooth * -25.0;
    o.staged = staged; o.safety = safety; o.explore = explore; o.back = back; o.budget = budget;
    o.total = 0.0 + o.c_prog + o.c_head + o.c_orient + staged + safety + explore + back + o.c_smooth + o.final_bonus;

    // ---- flags (simv2.py:528-541)
    uint32_t fl = 0u;
    if (hitch > 90.0 * kDeg) fl |= TT_F_JACKKNIFE;
    if (outside) fl |= TT_F_OUT_OF_MAP;
    if (steps >= pk_max(pk)) fl |= TT_F_MAX_STEPS;
    if (at_goal) fl |= TT_F_GOAL_REACHED | TT_F_SUCCESS;
    if (passed) fl |= TT_F_GOAL_PASSED;
    if (excessive) fl |= TT_F_EXCESSIVE_BACK;
    o.flags = fl; o.viol = viol;
    o.done = (fl & P.term_mask) != 0u;

    // carry for the next step: window [hist1..hist4] <- [hist2, hist3, hist4, cur]
    e.d3 = first ? cur : e.d2; e.d2 = d1; e.d1 = prev; e.prev = cur;
    e.pk = pk_make(steps, pk_max(pk), stages, age);
}

__device__ __forceinline__ void write_info(const Info &info, size_t N, int i, const Env &e, const StepOut &o) {
    if (info.comp) {
        double *c = info.comp + i;
        c[TT_I_TOTAL * N] = o.total; c[TT_I_PROGRESS * N] = o.c_prog; c[TT_I_HEADING * N] = o.c_head;
        c[TT_I_ORIENT * N] = o.c_orient; c[TT_I_STAGED * N] = o.staged; c[TT_I_SAFETY * N] = o.safety;
        c[TT_I_EXPLORE * N] = o.explore; c[TT_I_FINAL * N] = o.final_bonus; c[TT_I_BACKWARD * N] = o.back;
        c[TT_I_SMOOTH * N] = o.c_smooth; c[TT_I_CUMBACK * N] = e.cum; c[TT_I_BUDGET * N] = o.budget;
    }
    if (info.violation) info.violation[i] = (uint8_t)o.viol;
    if (info.flags) info.flags[i] = (uint8_t)o.flags;
}
