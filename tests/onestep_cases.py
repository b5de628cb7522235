"""Lanes of the one-step tests (tests/test_onestep_cpu.py, tests/test_gpu_onestep.py) and the builder of their fixture
tests/golden/f9_onestep.npz (tests/golden/make_golden_onestep.py writes what build_fixture() returns).

960 lanes in ONE env handle, six strata interleaved (lane i belongs to stratum i % 6), so that every 64-lane wave mixes them:

  S1 generic    psi2 in [-pi, pi], hitch within +-80 deg, both axles inside +-38 m, L2 in {7.0, 10.192}, random goal pose;
  S2 seams      psi1 and/or psi2, and the goal yaw, at fl(k pi/4), fl(k pi/2), k in [-8, 8], displaced by
                {0, +-1, +-2, +-8 ulp, +-1e-9}: the quadrant seams of tt_sincos;
  S3 cut        psi2 and / or gyaw - psi2 at an odd multiple of pi within {0, +-1, +-4 ulp, +-1e-12}: tt_wrap_pi's cut; the
                step of some lanes crosses it;
  S4 wound      S1 and S2 lanes with both headings moved by +-{1, 1e3, 1e5} turns;
  S5 steering   S1 lanes whose f32 action is beyond the clip, on it, next to it, a zero of either sign, a subnormal;
  S6 reward     lanes whose reward is followed for four steps: trailer 8 to 60 m from the goal, start pose elsewhere (jp spans
                [0, 1]), approaching, receding and tangential lanes (|inst|, |net| < 1e-3).

Everything expected comes from tests/onestep_ref.py at np.longdouble.  A lane is REDRAWN (its seam values kept) when
  (a) one of its observation entries lies within 2**-16 f32 spacings of an f32 rounding tie, or within the absolute f64 error
      A_j that the entry's formula has in the kernel (FLOOR_*; derivation in DESIGN.md "One-step tests");
  (b) in S6, a comparison of the reward has a margin under 1e-9 at any of the four steps, or init / 0.40096 lies within 1e-9 of
      an integer.
Where a seam itself forces an entry to be tiny (sin(hitch) of two equal seams, sin(gyaw - psi2) on the cut, a heading that
stays on its seam through the step; sin(hitch) = 0 of every freshly placed pose, whose two headings are one number) no redraw
can help: the entry is kept and marked in the fixture's `exact_*` masks as
not held to its bits but to |error| <= A_j."""
import numpy as np

import onestep_ref as R

LD, F64, F32 = R.LD, R.F64, R.F32
STRATA = ("S1_generic", "S2_seams", "S3_cut", "S4_wound", "S5_steering", "S6_reward")
NS, PER, T = len(STRATA), 160, 4
N = NS * PER
SEED = 20260
S1, S2, S3, S4, S5, S6 = range(6)
TIE = 2.0 ** -16                  # (a): f32 spacings
MARGIN = 1e-9                     # (b)
REDRAW_CAP = 0.02
# absolute f64 error of each entry's formula in the kernel: after a step the sin/cos of the headings are rotations
# of the step's first ones; observe() and set_pose() call tt_sincos on the heading itself (relative error: no floor)
_e = lambda k: 2.0 ** -k
FLOOR_STEP = np.array([_e(52), _e(52), _e(51), _e(51), _e(52), _e(52), _e(51), _e(51), _e(49), _e(49), 0, 0, _e(52), _e(52), 0, 0,
                       _e(51), _e(49), _e(49), _e(49), _e(49), _e(47), _e(47)])
FLOOR_DIRECT = np.array([_e(52), _e(52), 0, 0, _e(52), _e(52), 0, 0, _e(50), _e(50), 0, 0, _e(52), _e(52), 0, 0,
                         _e(51), _e(49), _e(49), _e(50), _e(50), _e(47), _e(47)])
SEAM_ENTRIES = (2, 3, 6, 7, 8, 9, 14, 15, 19, 20)      # the entries a seam can force; any other entry is always redrawn
SEAM_STRATA = (S2, S3, S4)

ULPS2 = (0, 1, -1, 2, -2, 8, -8, "+1e-9", "-1e-9")
ULPS3 = (0, 1, -1, 4, -4, "+1e-12", "-1e-12")
WINDS = (1, -1, 1000, -1000, 100000, -100000)
SPECIAL_ACTIONS = [0.8, -0.8, 2.0, -2.0, 1e3, -1e3, 0.0, -0.0, float(np.finfo(F32).smallest_subnormal),
                   -float(np.finfo(F32).smallest_subnormal)]
for _s in (1.0, -1.0):
    _m = F32(_s * R.P.max_steer)
    SPECIAL_ACTIONS += [float(_m), float(np.nextafter(_m, F32(np.inf))), float(np.nextafter(_m, F32(-np.inf)))]


def displaced(x, d):
    """x moved by d ulps (int) or by the amount a string names."""
    x = F64(x)
    if isinstance(d, str):
        return F64(x + float(d))
    for _ in range(abs(d)):
        x = np.nextafter(x, F64(np.inf) if d > 0 else F64(-np.inf))
    return x


def seam(j, salt, wind=0):
    """The j-th seam value: fl(n * fl(pi/4)) for n = k or 2k (+ 8 * wind), k in [-8, 8], displaced.  -> (value, n)."""
    q = (j * 7 + salt) % (17 * 2 * len(ULPS2))
    k, unit, d = q % 17 - 8, 1 + (q // 17) % 2, ULPS2[q // 34]
    n = k * unit + 8 * wind
    return displaced(F64(n) * F64(np.pi / 4), d), n


class Lanes:
    """The inputs of all N lanes."""

    def __init__(self):
        self.state0 = np.zeros((N, 6))
        self.goal = np.zeros((N, 3))
        self.start = np.zeros((N, 3))
        self.L2 = np.zeros(N)
        self.actions = np.zeros((T, N), F32)
        self.stratum = np.arange(N) % NS
        self.seam_lane = np.zeros(N, bool)          # lanes that carry a seam value (all of S2 and S3, the S2 half of S4)


def _body(rng, psi2, L2, lim):
    """Trailer axle uniform in the square, truck axle L2 ahead, both within +-lim."""
    while True:
        x2, y2 = rng.uniform(-lim, lim, 2)
        x1, y1 = x2 + L2 * np.cos(psi2), y2 + L2 * np.sin(psi2)
        if abs(x1) <= lim and abs(y1) <= lim:
            return x1, y1, x2, y2


def _goal_far(rng, x2, y2):
    """A goal pose inside +-38 m, at least 1 m from the trailer axle (the heading-error entries' error floor grows as 1/distance)."""
    while True:
        gx, gy = rng.uniform(-38, 38, 2)
        if np.hypot(gx - x2, gy - y2) >= 1.0:
            return gx, gy


def _generic(L, i, rng, j):
    L2 = (7.0, 10.192)[j % 2]
    psi2 = rng.uniform(-np.pi, np.pi)
    psi1 = psi2 + rng.uniform(-1, 1) * np.radians(80)
    L.L2[i] = L2
    L.state0[i] = (psi1, psi2) + _body(rng, psi2, L2, 38.0)
    L.goal[i] = _goal_far(rng, *L.state0[i, 4:6]) + (rng.uniform(-np.pi, np.pi),)
    L.actions[:, i] = rng.uniform(-1, 1, T) * R.P.max_steer


def _seams(L, i, rng, j, wind=0):
    _generic(L, i, rng, j)
    L.seam_lane[i] = True
    hitch = rng.uniform(-1, 1) * np.radians(80)
    a2, n2 = seam(j, 3, wind)
    which = j % 3
    if which == 0:                       # both on seams, at most one eighth of a turn apart
        d = (j // 3) % 3 - 1
        ulp = ULPS2[(j // 9) % len(ULPS2)]
        psi2, psi1 = a2, displaced(F64(n2 + d) * F64(np.pi / 4), ulp)
    elif which == 1:
        psi1, _ = seam(j, 5, wind)
        psi2 = F64(psi1 - hitch)
    else:
        psi2, psi1 = a2, F64(a2 + hitch)
    L.state0[i, :2] = psi1, psi2
    L.state0[i, 2:] = _body(rng, float(psi2), L.L2[i], 38.0)
    L.goal[i] = _goal_far(rng, *L.state0[i, 4:6]) + (seam(j, 1)[0],)


def _cut(L, i, rng, j):
    _generic(L, i, rng, j)
    L.seam_lane[i] = True
    odd = (1, -1, 3, -3, 5, -7)[(j // 3) % 6]
    on_cut = lambda m, s: displaced(F64(m) * F64(np.pi), ULPS3[(j // 18 + s) % len(ULPS3)])
    which = j % 3
    hitch = rng.uniform(-1, 1) * np.radians(80)
    if which == 0:                       # psi2 on the cut, any goal yaw
        psi2 = on_cut(odd, 0)
        gyaw = rng.uniform(-np.pi, np.pi)
    elif which == 1:                     # gyaw - psi2 on the cut: psi2 a multiple of 2**-20, so that the f64 sum keeps the seam's bits
        psi2 = F64(np.round(rng.uniform(-0.5, 0.5) * 2 ** 20) / 2 ** 20)
        gyaw = F64(psi2 + on_cut((1, -1)[(j // 3) % 2], 0))
    else:                                # both
        psi2 = on_cut(odd, 0)
        gyaw = F64(psi2 + on_cut((1, -1)[(j // 3) % 2], 2))
    L.state0[i, :2] = F64(psi2 + hitch), psi2
    L.state0[i, 2:] = _body(rng, float(psi2), L.L2[i], 38.0)
    L.goal[i] = _goal_far(rng, *L.state0[i, 4:6]) + (gyaw,)


def _wound(L, i, rng, j):
    w = WINDS[(j // 2) % len(WINDS)]
    if j % 2:
        _seams(L, i, rng, j // 2, wind=w)
    else:
        _generic(L, i, rng, j)
        L.state0[i, :2] += F64(2 * np.pi) * w            # both moved by the same f64 amount: the hitch keeps all but ulp(psi)


def _steering(L, i, rng, j):
    _generic(L, i, rng, j)
    if j < 6 * len(SPECIAL_ACTIONS):
        L.actions[0, i] = F32(SPECIAL_ACTIONS[j % len(SPECIAL_ACTIONS)])


def _reward(L, i, rng, j):
    """Goal and start are set by _reward_goals once the trailer's path is known (it does not depend on them)."""
    L2 = (7.0, 10.192)[j % 2]
    psi2 = rng.uniform(-np.pi, np.pi)
    L.L2[i] = L2
    L.state0[i] = (psi2 + rng.uniform(-1, 1) * np.radians(30), psi2) + _body(rng, psi2, L2, 33.0)
    a = rng.uniform(-1, 1, T) * R.P.max_steer
    L.actions[:, i] = a[0] if j % 8 == 5 else a


def _reward_goals(L, idx, rng):
    """S6 goals: kind j % 4 = 0 ahead of the motion (approach), 1 behind it (recede), 2 on the perpendicular bisector of the
    trailer's second step, moved off it so that |inst| at step 2 is a random figure under 1e-3, 3 anywhere."""
    idx = np.asarray(idx)
    if not len(idx):
        return
    st, pts = L.state0[idx], []
    dummy = np.zeros((len(idx), 3))
    for t in range(2):
        st = R.step(st, L.actions[t, idx], dummy, L.L2[idx], F64)["new"]
        pts.append(st[:, 4:6])
    for n, i in enumerate(idx):
        j = i // NS
        x2, y2, psi2 = L.state0[i, 4], L.state0[i, 5], L.state0[i, 1]
        while True:
            cur = rng.uniform(10, 57)
            kind = j % 4
            if kind == 2:
                p1, p2 = pts[0][n], pts[1][n]
                d = np.hypot(*(p2 - p1))
                tdir = (p2 - p1) / d
                side = rng.choice((-1.0, 1.0))
                inst = rng.uniform(-1, 1) * 1e-3
                g = (p1 + p2) / 2 + side * cur * np.array([-tdir[1], tdir[0]]) + tdir * (inst * cur / d)
            else:
                phi = (psi2 + np.pi + rng.uniform(-1, 1), psi2 + rng.uniform(-1, 1), 0, rng.uniform(-np.pi, np.pi))[kind]
                g = np.array([x2, y2]) + cur * np.array([np.cos(phi), np.sin(phi)])
            if np.abs(g).max() <= 40.0:
                break
        L.goal[i] = g[0], g[1], rng.uniform(-np.pi, np.pi)
        init = np.hypot(g[0] - x2, g[1] - y2) / (1 - rng.uniform(-0.2, 0.8))       # jp = (init - cur) / init, clipped at 0
        a = rng.uniform(-np.pi, np.pi)
        L.start[i] = g[0] + init * np.cos(a), g[1] + init * np.sin(a), rng.uniform(-np.pi, np.pi)


def seam_values(L, i):
    """The coordinates of seam lane i that no redraw may move."""
    s, j = i % NS, i // NS
    if s == S3:
        return {0: (L.state0[i, 1],), 1: (L.goal[i, 2] - L.state0[i, 1],), 2: (L.state0[i, 1], L.goal[i, 2])}[j % 3]
    which = (j // 2 if s == S4 else j) % 3
    return tuple(L.state0[i, q] for q in {0: (0, 1), 1: (0,), 2: (1,)}[which]) + (L.goal[i, 2],)


DRAW = (_generic, _seams, _cut, _wound, _steering, _reward)


def draw(L, idx, rng):
    """(Re)draw lanes idx: seam values are functions of the lane number, everything else comes from rng."""
    for i in idx:
        s, j = i % NS, i // NS
        DRAW[s](L, i, rng, j)
        if s != S6:
            L.start[i] = L.state0[i, 4], L.state0[i, 5], L.state0[i, 1]      # placed where the trailer is, at its heading
    _reward_goals(L, [i for i in idx if i % NS == S6], rng)


def exact_mask(obs_ld, floor):
    """-> (f32 rounding, mask of the entries far enough from a tie to be held to their bits)."""
    r, rel, absd = R.round_f32(obs_ld)
    return r, (rel >= TIE) & (absd >= floor)


def evaluate(L, idx, dtype=LD):
    """The reference's results for lanes idx: dict of arrays (first axis = len(idx) unless noted)."""
    idx = np.asarray(idx)
    goal, L2, start = L.goal[idx], L.L2[idx], L.start[idx]
    out = {}
    placed, tie_xy = R.placed_state(start, L2, dtype)
    out["placed_tie"] = tie_xy.min(-1)
    out["obs_pose"], out["exact_pose"] = exact_mask(R.observe(placed, np.zeros(len(idx), F32), goal, dtype), FLOOR_DIRECT)
    out["obs_observe"], out["exact_observe"] = exact_mask(R.observe(L.state0[idx], L.actions[0, idx], goal, dtype), FLOOR_DIRECT)
    carry = R.Carry(len(idx), dtype)
    st = L.state0[idx]
    for k in "inc new obs exact info flags viol margin hitch cur inside".split():
        out[k] = []
    for t in range(T):
        res = R.step(st, L.actions[t, idx], goal, L2, dtype)
        o32, ex = exact_mask(res["obs"], FLOOR_STEP)
        info, flags, viol, margin, frac = R.reward(o32, list(res["red"].T), t + 1, start[:, :2], goal, carry, dtype)
        red = res["red"].astype(F64)
        for k, v in (("inc", res["inc"]), ("new", res["new"]), ("obs", o32), ("exact", ex), ("info", info), ("flags", flags),
                     ("viol", viol), ("margin", margin), ("hitch", np.abs(red[:, 0] - red[:, 1])),
                     ("cur", np.hypot(goal[:, 0] - red[:, 4], goal[:, 1] - red[:, 5])), ("inside", 40 - np.abs(red[:, 2:]).max(-1))):
            out[k].append(v)
        st = res["new"].astype(F64)               # the state is an f64 array between steps
    out = {k: np.stack(v) if isinstance(v, list) else v for k, v in out.items()}
    out["frac"] = frac
    out["k"] = res["k"]
    return out


def rejected(L, idx, ev):
    """-> (lanes of idx to redraw [bool], the three exact masks with the entries a seam forces left False)."""
    idx = np.asarray(idx)
    s = idx % NS
    seamy = np.isin(s, SEAM_STRATA) & L.seam_lane[idx]
    forced_ok = np.zeros(23, bool)
    forced_ok[list(SEAM_ENTRIES)] = True
    bad = ev["placed_tie"] < TIE
    for ex in (ev["exact_pose"], ev["exact_observe"], ev["exact"][0]):
        bad |= (~ex & ~(seamy[:, None] & forced_ok[None, :]))[:, np.arange(23) != 8 if ex is ev["exact_pose"] else slice(None)].any(-1)
    s6 = s == S6
    bad |= s6 & (~ev["exact"]).any((0, 2))                       # the reward reads the f32 observation of every step
    bad |= s6 & ((ev["margin"].min(0) < MARGIN) | (ev["frac"] < MARGIN))
    return bad


def make_lanes():
    """Draw all lanes, redraw the rejected ones until none is left.  -> (Lanes, reference results of all lanes at longdouble,
    redraws per stratum)."""
    rng = np.random.default_rng(SEED)
    L = Lanes()
    idx = np.arange(N)
    draw(L, idx, rng)
    redraws = np.zeros(NS, int)
    for _ in range(50):
        ev = evaluate(L, idx)
        bad = idx[rejected(L, idx, ev)]
        if not len(bad):
            break
        np.add.at(redraws, bad % NS, 1)
        draw(L, bad, rng)
        idx = bad
    else:
        raise AssertionError("lanes are still rejected after 50 rounds")
    return L, evaluate(L, np.arange(N)), redraws


def yardsticks(L, ev, dtype=F64, lanes=None, **how):
    """E_q, q = psi1, psi2, x1, y1, x2, y2: the worst |increment of the reference at `dtype` - increment at longdouble| over the S1
    lanes (before the increment is added to anything), first step.  how: sin / cos / exact passed on to R.step (the negative
    controls)."""
    lanes = np.flatnonzero(L.stratum == S1) if lanes is None else lanes
    got = R.step(L.state0[lanes], L.actions[0, lanes], L.goal[lanes], L.L2[lanes], dtype, **how)["inc"]
    return np.abs(got.astype(LD) - ev["inc"][0][lanes]).max(0).astype(F64)


def state_bound(new_ref, E, factor):
    """The bound of test 3a per lane and component: half an f64 ulp of the new state (the kernel stores it rounded) + factor * E_q."""
    return 0.5 * R.ulp64(new_ref) + factor * np.asarray(E)[None, :]


def census(L, ev):
    """What the generator asserts the strata contain."""
    s6 = L.stratum == S6
    cur = ev["cur"]
    d = cur[:-1] - cur[1:]                            # inst of steps 2..4
    wrap = lambda a: a - 2 * np.pi * np.round(a / (2 * np.pi))
    s3 = L.stratum == S3
    before, after = wrap(L.state0[:, 1]), wrap(ev["new"][0][:, 1].astype(F64))
    init = np.hypot(L.goal[:, 0] - L.start[:, 0], L.goal[:, 1] - L.start[:, 1])
    jp = np.clip((init - cur[0]) / init, 0, 1)
    return dict(approach=int((d[:, s6] > 0).any(0).sum()), recede=int((d[:, s6] < 0).any(0).sum()),
                small_inst=int((np.abs(d[:, s6]) < 1e-3).any(0).sum()),
                crosses_cut=int((s3 & (np.abs(before) > 3) & (np.abs(after) > 3) & (before * after < 0)).sum()),
                jp_low=int((s6 & (jp < 0.3)).sum()), jp_high=int((s6 & (jp > 0.3)).sum()), jp_zero=int((s6 & (jp == 0)).sum()),
                s6_hitch_deg=float(np.degrees(ev["hitch"][:, s6].max())), s6_inside=float(ev["inside"][:, s6].min()),
                s6_cur=(float(cur[:, s6].min()), float(cur[:, s6].max())),
                passed=int((ev["flags"][:, s6] & R.F_GOAL_PASSED).any(0).sum()),
                held_loosely=int((~ev["exact"][0]).sum() + (~ev["exact_pose"]).sum() + (~ev["exact_observe"]).sum()))


MINIMA = dict(approach=40, recede=40, small_inst=20, crosses_cut=10, jp_low=30, jp_high=30, jp_zero=5, passed=5)


def build_fixture():
    """-> {name: array}: inputs, expected values as (hi f64, lo f32) pairs, masks, yardsticks, census."""
    L, ev, redraws = make_lanes()
    assert (redraws < REDRAW_CAP * PER).all(), f"redrawn per stratum {redraws.tolist()}: a stratum is badly chosen"
    c = census(L, ev)
    for k, v in MINIMA.items():
        assert c[k] >= v, (k, c)
    assert c["s6_hitch_deg"] <= 60 and c["s6_inside"] > 3 and 8 <= c["s6_cur"][0] and c["s6_cur"][1] <= 60, c
    assert L.seam_lane[L.stratum == S2].all() and L.seam_lane[L.stratum == S3].all()
    assert L.seam_lane[L.stratum == S4].sum() == PER // 2
    fresh = Lanes()                      # the seam values are functions of the lane number: any other draw gives the same ones
    seamy = np.flatnonzero(L.seam_lane)
    draw(fresh, seamy, np.random.default_rng(0))
    for i in seamy:
        assert seam_values(L, i) == seam_values(fresh, i), i
    s6 = np.flatnonzero(L.stratum == S6)
    fx = dict(strata=np.array(STRATA), stratum=L.stratum.astype(np.uint8), seam_lane=L.seam_lane, state0=L.state0, goal=L.goal,
              start=L.start, L2=L.L2, actions=L.actions, redraws=redraws, E=yardsticks(L, ev),
              max_episode_steps=R.max_episode_steps(L.start[:, :2], L.goal).astype(np.int32),
              obs_pose=ev["obs_pose"], exact_pose=ev["exact_pose"], obs_observe=ev["obs_observe"], exact_observe=ev["exact_observe"],
              obs_step=ev["obs"][0], exact_step=ev["exact"][0], obs_s6=ev["obs"][1:, s6],
              flags=ev["flags"][:, s6], viol=ev["viol"][:, s6], info_s6=ev["info"][:, s6].astype(F64),
              info_step1=ev["info"][0][:, :4].astype(F64),
              census_keys=np.array(sorted(MINIMA)), census=np.array([c[k] for k in sorted(MINIMA)]))
    fx["inc_hi"], fx["inc_lo"] = R.split(ev["inc"][0])
    fx["new_hi"], fx["new_lo"] = R.split(ev["new"][0])
    return fx
