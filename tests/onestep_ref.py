"""One env step in plain numpy at a chosen precision: the yardstick of tests/test_onestep_cpu.py and tests/test_gpu_onestep.py.

Vectorised over lanes and parametrised by dtype (np.float64, np.longdouble).  It mirrors oracle/simv2_twin.py operation for
operation -- FixedStepTwin.integrate, observation, reward_step -- with these differences, each there because the twin's form
is not a usable yardstick at the accuracy the HIP kernel has ("One-step tests"):

  * the starting headings are reduced EXACTLY (fractions.Fraction against a 60-digit pi) to r = psi - 2 pi k, k such that
    |r2| <= pi, psi1 with psi2's k, before anything is integrated; what comes back are the heading INCREMENTS and the sin/cos
    of the new reduced headings, never `psi + increment` rounded at ulp(psi);
  * the 23 observations come back in `dtype`, before the cast; round_f32() gives their correctly rounded f32 and the distance
    of each from the nearest f32 rounding tie;
  * the reward reads the rounded f32 observation, as the reference does, but each np.arctan2(f32, f32) is
    f32(arctan2 in `dtype`): the correctly rounded value, where a library's atan2f may be an f32 ulp off; products the
    reference forms in f32 (`obs[20] * 15.0`) stay f32;
  * the reward returns every row of the kernel's info block and the margin of every comparison it took.
"""
from fractions import Fraction

import numpy as np

LD = np.longdouble
PI = Fraction("3.14159265358979323846264338327950288419716939937510582097494")      # 60 digits
F64, F32 = np.float64, np.float32
INFO_ROWS = ("total_reward", "progress_reward", "heading_reward", "orientation_reward", "staged_success", "safety_penalty",
             "exploration_bonus", "final_success_bonus", "backward_penalty", "smoothness_penalty", "cumulative_backward",
             "movement_budget")             # the kernel's info block, in its order (include/ttenv.h TT_I_*)
F_JACKKNIFE, F_OUT_OF_MAP, F_MAX_STEPS, F_GOAL_REACHED, F_GOAL_PASSED, F_EXCESSIVE_BACK, F_SUCCESS = (1 << i for i in range(7))

# scipy RK45 tableau as exact fractions (oracle/simv2_twin.py FixedStepTwin holds their f64 roundings)
A = ((), ("1/5",), ("3/40", "9/40"), ("44/45", "-56/15", "32/9"), ("19372/6561", "-25360/2187", "64448/6561", "-212/729"),
     ("9017/3168", "-355/33", "46732/5247", "49/176", "-5103/18656"))
B = ("35/384", "0", "500/1113", "125/192", "-2187/6784", "11/84")


def check_dtype(dtype):
    if dtype is LD:
        assert np.finfo(LD).eps < 2e-19, "np.longdouble is not the 80-bit extended format here"
    else:
        assert dtype is F64


def const(fr, dtype):
    """A rational constant rounded once to dtype."""
    return from_fraction(Fraction(fr), dtype)


class P:
    """Constants of the env (simv2.py:23-101), f64 values as the reference holds them."""
    v1x, L1, dt, ho = -5.012, 5.0, 0.08, 0.0
    map_min, map_max = -40.0, 40.0
    max_steer = float(np.radians(45))
    M = float(np.sqrt(80 ** 2 + 80 ** 2))
    pos_thr, ori_thr = 0.5, float(np.deg2rad(15))
    step_length, extra_steps = 0.40096, 75


def from_fraction(fr, dtype):
    hi = float(fr)
    return dtype(hi) + dtype(float(fr - Fraction(hi))) if dtype is LD else dtype(hi)


def reduce_headings(psi1, psi2, dtype, exact=True):
    """(r1, r2, k): psi - 2 pi k with |r2| <= pi.  exact=False is the trap: psi - k * fl(2 pi) in dtype."""
    psi1, psi2 = np.asarray(psi1, F64), np.asarray(psi2, F64)
    r1, r2, ks = np.empty(psi1.shape, dtype), np.empty(psi1.shape, dtype), np.empty(psi1.shape, np.int64)
    for i in range(psi1.size):
        f2 = Fraction(float(psi2.flat[i]))
        k = round(f2 / (2 * PI))
        ks.flat[i] = k
        if exact:
            r2.flat[i] = from_fraction(f2 - 2 * k * PI, dtype)
            r1.flat[i] = from_fraction(Fraction(float(psi1.flat[i])) - 2 * k * PI, dtype)
        else:
            r2.flat[i] = dtype(psi2.flat[i]) - dtype(k) * dtype(2 * np.pi)
            r1.flat[i] = dtype(psi1.flat[i]) - dtype(k) * dtype(2 * np.pi)
    return r1, r2, ks


def _rhs(y, tan_d, L2, dtype, sin, cos):
    """simv2.py:269-303 / Simv2Twin._rhs on rows y [6][n]."""
    v, L1, ho = dtype(P.v1x), dtype(P.L1), dtype(P.ho)
    hitch = y[0] - y[1]
    w1 = (v / L1) * tan_d
    v2 = v * cos(hitch) + ho * w1 * sin(hitch)
    w2 = (v / L2) * sin(hitch) - (ho / L2) * w1 * cos(hitch)
    return [w1, w2, v * cos(y[0]), v * sin(y[0]), v2 * cos(y[1]), v2 * sin(y[1])]


def increments(y0, delta, L2, dtype, sin=np.sin, cos=np.cos):
    """One fixed Dormand-Prince step of h = dt (FixedStepTwin.integrate) from rows y0 [6][n] with the clipped steering delta:
    -> h * sum(b k), the increment BEFORE it is added to y0."""
    h = dtype(P.dt)
    tan_d = sin(delta) / cos(delta) if sin is not np.sin else np.tan(delta)
    L2 = np.asarray(L2, dtype)
    zero = np.zeros(np.shape(y0[0]), dtype)
    k = []
    for i in range(6):
        y = [y0[q] + h * sum((const(a, dtype) * kj[q] for a, kj in zip(A[i], k)), zero) for q in range(6)]
        k.append(_rhs(y, tan_d, L2, dtype, sin, cos))
    return [h * sum(const(b, dtype) * kj[q] for b, kj in zip(B, k)) for q in range(6)]


def observation(h1, h2, r1, r2, x1, y1, x2, y2, steering, goal, ori_err, dtype, sin=np.sin, cos=np.cos):
    """simv2.py:103-181.  h1, h2: the headings whose sin and cos are taken -- f64 inputs as they stand (the library reduces an
    exact argument exactly, and keeps a sine next to a zero to its relative accuracy) or, after a step, the reduced heading plus
    its increment; r1, r2: the reduced headings for the angle differences; ori_err = gyaw - psi2 from reduced_difference, so
    that nothing is rounded at the size of a wound angle.  The goal yaw is an f64 input.  -> [n, 23] in dtype."""
    gx, gy = np.asarray(goal[:, 0], dtype), np.asarray(goal[:, 1], dtype)
    centre, half, M = dtype(0.0), dtype(40.0), dtype(P.M)
    dxg, dyg = gx - x2, gy - y2
    dist = np.sqrt((x2 - gx) ** 2 + (y2 - gy) ** 2)
    to_goal = np.arctan2(dyg, dxg)
    c2, s2 = cos(h2), sin(h2)
    d_long = dxg * c2 + dyg * s2
    d_lat = -dxg * s2 + dyg * c2
    hitch = r1 - r2
    head_err = to_goal - (r2 + const(PI, dtype))
    gyaw = np.asarray(goal[:, 2], dtype)
    gy_s, gy_c = sin(gyaw), cos(gyaw)
    st = np.asarray(steering, dtype)
    return np.stack([
        (x1 - centre) / half, (y1 - centre) / half, sin(h1), cos(h1),
        (x2 - centre) / half, (y2 - centre) / half, s2, c2,
        sin(hitch), cos(hitch), sin(st), cos(st),
        (gx - centre) / half, (gy - centre) / half, gy_s, gy_c,
        np.clip(dist / M, 0, 1), np.clip(d_long / M, -1, 1), np.clip(d_lat / M, -1, 1),
        sin(ori_err), cos(ori_err), sin(head_err), cos(head_err)], axis=-1)


def reduced_difference(a, b, dtype):
    """(a - b) - 2 pi k for f64 a, b, formed exactly, k such that the result lies in [-pi, pi]."""
    out = np.empty(len(a), dtype)
    for i in range(len(a)):
        d = Fraction(float(a[i])) - Fraction(float(b[i]))
        out[i] = from_fraction(d - 2 * round(d / (2 * PI)) * PI, dtype)
    return out


def round_f32(x):
    """-> (f32(x) correctly rounded, distance of x from the nearest f32 rounding tie in units of the f32 spacing there,
    the same distance in absolute terms).  A representable x is 0.5 spacings from a tie."""
    x = np.asarray(x)
    r = x.astype(F32)
    rl = r.astype(x.dtype)
    other = np.where(x > rl, np.nextafter(r, F32(np.inf)), np.nextafter(r, F32(-np.inf))).astype(x.dtype)
    gap = np.abs(other - rl)
    absd = np.abs(x - (rl + other) / 2)
    return r, (absd / gap).astype(F64), absd.astype(F64)


def atan2_f32(y, x, dtype):
    """np.arctan2(f32, f32) as the correctly rounded f32 of the real value."""
    return np.arctan2(np.asarray(y, F32).astype(dtype), np.asarray(x, F32).astype(dtype)).astype(F32)


class Carry:
    """reward_functionv1.get_persistent_state() for n lanes (oracle/simv2_twin.py RewardCarry)."""

    def __init__(self, n, dtype):
        z = lambda: np.zeros(n, dtype)
        self.prev, self.cum, self.closest, self.hist = z(), z(), z(), [z() for _ in range(5)]
        self.bt = np.zeros(n, np.int64)
        self.stages = np.zeros((n, 3), bool)
        self.psteer = np.zeros(n, F32)
        self.t = 0             # reward evaluations so far; 0 <=> `reward_state is None`


def reward(obs32, state, steps, start_xy, goal, carry, dtype):
    """reward_step of the twin, vectorised: obs32 [n,23] f32 (rounded), state rows [6][n] in dtype (of the headings it reads
    psi1 - psi2 alone: pass the reduced ones), steps the step count after this step.
    -> (info [n,12] dtype in INFO_ROWS order, flags u8, violation u8, margins [n] f64 (the smallest distance of any comparison it
    took from its threshold), frac [n] f64 (distance of init / 0.40096 from an integer))."""
    n = len(obs32)
    gx, gy = np.asarray(goal[:, 0], dtype), np.asarray(goal[:, 1], dtype)
    sx, sy = np.asarray(start_xy[:, 0], dtype), np.asarray(start_xy[:, 1], dtype)
    r1, r2, x1, y1, x2, y2 = state
    cur = np.sqrt((x2 - gx) ** 2 + (y2 - gy) ** 2)
    init = np.sqrt((gx - sx) ** 2 + (gy - sy) ** 2) + dtype(1e-6)
    q = init / dtype(P.step_length)
    rmax = np.floor(q).astype(np.int64) + P.extra_steps
    frac = np.abs(q - np.rint(q)).astype(F64)
    steer_now = atan2_f32(obs32[:, 10], obs32[:, 11], dtype)
    margins = [np.full(n, np.inf)]
    near = lambda a, b: margins.append(np.abs(np.asarray(a, dtype) - b).astype(F64))
    c = carry
    c.t += 1               # at t = 1 the whole window is `cur`, at t = 2 all but its last entry are one value: comparisons
    t = c.t                # between copies of one number have no margin to speak of and are exact on every side
    if t == 1:
        c.prev, c.psteer, c.cum, c.bt = cur.copy(), steer_now.copy(), np.zeros(n, dtype), np.zeros(n, np.int64)
        c.hist, c.stages, c.closest = [cur.copy() for _ in range(5)], np.zeros((n, 3), bool), cur.copy()
    else:
        near(cur, c.closest)
        c.closest = np.where(cur < c.closest, cur, c.closest)

    jp = np.clip((init - cur) / init, 0.0, 1.0)
    w_orient = (np.tanh(dtype(7.0) * (jp - dtype(0.3))) + 1) / dtype(2.0)
    w_head = 1 - w_orient

    inst = c.prev - cur
    if t >= 2:
        near(inst, 0)
    prog = np.where(inst > 0, np.tanh(inst), np.tanh(inst) * dtype(0.5))
    c.hist = c.hist[1:] + [cur.copy()]
    prog_net = np.tanh((c.hist[0] - cur) / dtype(2.0)) * dtype(0.5)
    mono = (c.hist[-3] >= c.hist[-2]) & (c.hist[-2] >= c.hist[-1])
    if t >= 3:
        near(c.hist[-3], c.hist[-2])
    progress = prog + prog_net + np.where(mono, dtype(0.2), dtype(0))

    want = np.arctan2(gy - y2, gx - x2)
    have = atan2_f32(obs32[:, 6], obs32[:, 7], dtype)
    diff = want - (have.astype(dtype) + dtype(np.deg2rad(180)))
    diff = np.arctan2(np.sin(diff), np.cos(diff))
    heading = np.cos(diff)

    orient15 = obs32[:, 20] * F32(15.0)                                      # f32 * python float stays f32

    ori_err = np.abs(atan2_f32(obs32[:, 19], obs32[:, 20], dtype)).astype(dtype)
    staged = np.zeros(n, dtype)
    near(cur, 5.0); near(cur, 2.0); near(cur, P.pos_thr)
    inside2 = cur <= 2.0
    margins.append(np.where(inside2, np.abs(ori_err - dtype(np.deg2rad(45))), np.inf).astype(F64))
    margins.append(np.where(cur <= P.pos_thr, np.abs(ori_err - dtype(P.ori_thr)), np.inf).astype(F64))
    staged += np.where(cur <= 5.0, 10, 0)
    s2_ = inside2 & (ori_err <= dtype(np.deg2rad(45))) & ~c.stages[:, 1]
    staged += np.where(s2_, 25, 0)
    c.stages[:, 1] |= s2_
    success = (cur <= P.pos_thr) & (ori_err <= dtype(P.ori_thr))
    s3_ = success & ~c.stages[:, 2]
    staged += np.where(s3_, 100, 0)
    c.stages[:, 2] |= s3_

    safety, viol = np.zeros(n, dtype), np.zeros(n, np.uint8)

    def hit(m, pen, v):
        nonlocal safety, viol
        safety = safety + np.where(m, dtype(pen), dtype(0))
        viol = np.where(m, np.uint8(v), viol)

    hitch = np.abs(r1 - r2)
    for deg in (85, 70, 90):
        near(hitch, dtype(np.deg2rad(deg)))
    hit(hitch > dtype(np.deg2rad(85)), -500, 1)
    hit((hitch > dtype(np.deg2rad(70))) & ~(hitch > dtype(np.deg2rad(85))), -50, 2)
    pos = np.stack([x1, x2, y1, y2])
    for edge in (P.map_min - 2, P.map_min, P.map_max, P.map_max + 2):
        margins.append(np.abs(pos - dtype(edge)).min(0).astype(F64))
    major = ((pos < P.map_min - 2) | (pos > P.map_max + 2)).any(0)
    minor = ((pos < P.map_min) | (pos > P.map_max)).any(0)
    hit(major, -500, 3)
    hit(minor & ~major, -50, 4)
    near(gy, y2)
    passed = gy > y2
    hit(passed, -500, 5)
    hit(steps >= rmax, -500, 6)
    near(cur, c.closest + dtype(6.0))
    excessive = cur > c.closest + dtype(6.0)
    hit(excessive, -500, 7)

    explore = np.where(steps < rmax * 0.5, 4.0, np.where(steps < rmax * 0.8, 2.0, 0.0)).astype(dtype)

    c.cum = c.cum + np.maximum(0, cur - c.prev)
    c.bt = c.bt + 1
    budget = dtype(5.0) * np.minimum(1.0, c.bt / 50).astype(dtype)
    near(c.cum, budget)
    excess = np.maximum(0, c.cum - budget)
    back = np.where(excess > 0, -(excess ** dtype(1.5)) * dtype(0.5), dtype(0))

    smooth = np.abs(steer_now - c.psteer).astype(dtype) / dtype(np.deg2rad(90))       # f32 difference, f64 division

    final = np.where(success, dtype(200.0), dtype(0))
    c.prev = cur.copy()

    progress_r = progress * dtype(15.0)
    heading_r = heading * dtype(15.0) * w_head
    orient_r = orient15.astype(dtype) * w_orient
    smooth_r = smooth * dtype(-25.0)
    total = dtype(0) + progress_r + heading_r + orient_r + staged + safety + explore + back + smooth_r + final
    info = np.stack([total, progress_r, heading_r, orient_r, staged, safety, explore, final, back, smooth_r, c.cum, budget], -1)
    flags = ((hitch > dtype(np.deg2rad(90))) * F_JACKKNIFE + minor * F_OUT_OF_MAP + success * (F_GOAL_REACHED | F_SUCCESS)
             + passed * F_GOAL_PASSED + excessive * F_EXCESSIVE_BACK).astype(np.uint8)
    return info, flags, viol, np.min(margins, axis=0), frac


def max_episode_steps(start_xy, goal):
    """simv2.py compute_max_steps in f64, as set_pose sets it."""
    d0 = np.sqrt((goal[:, 0] - start_xy[:, 0]) ** 2 + (goal[:, 1] - start_xy[:, 1]) ** 2)
    return (d0 / P.step_length).astype(np.int64) + P.extra_steps


def step(state0, action, goal, L2, dtype, sin=np.sin, cos=np.cos, exact=True):
    """One env step of n lanes from the f64 states state0 [n,6] with f32 actions: the kinematics and the observation.
    -> dict: inc [n,6] (h sum(b k), before the add), red [n,6] (the new state with REDUCED headings: what sin/cos, the
    observation and the reward read), new [n,6] (the new state with the headings as state0 + inc, rounded once in dtype),
    obs [n,23] in dtype, k [n] the winding taken out."""
    check_dtype(dtype)
    state0 = np.asarray(state0, F64)
    delta = np.clip(np.asarray(action, F32).astype(F64), -P.max_steer, P.max_steer).astype(dtype)     # simv2.py:504 clips in f64
    r1, r2, k = reduce_headings(state0[:, 0], state0[:, 1], dtype, exact)
    y0 = [r1, r2] + [state0[:, q].astype(dtype) for q in range(2, 6)]
    inc = increments(y0, delta, L2, dtype, sin, cos)
    red = [a + b for a, b in zip(y0, inc)]
    ori_err = reduced_difference(goal[:, 2], state0[:, 1], dtype) - inc[1]          # gyaw - (psi2 + increment)
    obs = observation(red[0], red[1], *red, delta, goal, ori_err, dtype, sin, cos)
    new = [state0[:, 0].astype(dtype) + inc[0], state0[:, 1].astype(dtype) + inc[1]] + red[2:]
    return dict(inc=np.stack(inc, -1), red=np.stack(red, -1), new=np.stack(new, -1), obs=obs, k=k)


def observe(state, steering, goal, dtype):
    """The observation of f64 states as they stand (env.observe(steering); steering is not clipped)."""
    check_dtype(dtype)
    state = np.asarray(state, F64)
    r1, r2, _ = reduce_headings(state[:, 0], state[:, 1], dtype)
    y = [r1, r2] + [state[:, q].astype(dtype) for q in range(2, 6)]
    return observation(state[:, 0].astype(dtype), state[:, 1].astype(dtype), *y, np.asarray(steering, F32).astype(dtype), goal,
                       reduced_difference(goal[:, 2], state[:, 1], dtype), dtype)


def placed_state(start, L2, dtype):
    """simv2.py:481-496: trailer at the start pose, truck L2 ahead, the state rounded to f32.
    -> (state [n,6] f64 holding f32 values, distance of x1, y1 from an f32 rounding tie [n,2] in f32 spacings)."""
    check_dtype(dtype)
    start = np.asarray(start, F64)
    yaw = start[:, 2].astype(dtype)
    x1 = start[:, 0].astype(dtype) + np.asarray(L2, dtype) * np.cos(yaw)
    y1 = start[:, 1].astype(dtype) + np.asarray(L2, dtype) * np.sin(yaw)
    x1r, tx, _ = round_f32(x1)
    y1r, ty, _ = round_f32(y1)
    yaw = start[:, 2].astype(F32)
    st = np.stack([yaw, yaw, x1r, y1r, start[:, 0].astype(F32), start[:, 1].astype(F32)], -1).astype(F64)
    return st, np.stack([tx, ty], -1)


def split(x):
    """dtype array -> (hi f64, lo f32): 53 + 24 bits, so hi + lo holds a longdouble's 64 wherever lo is a normal f32."""
    hi = np.asarray(x).astype(F64)
    return hi, (np.asarray(x) - hi.astype(np.asarray(x).dtype)).astype(F32)


def join(hi, lo):
    return hi.astype(LD) + lo.astype(LD)


def ulp64(x):
    return np.spacing(np.abs(np.asarray(x).astype(F64)))
