"""What tests/test_goal_zone_cpu.py (CPU) and tests/test_gpu_goal_zone.py (GPU) share: deterministic scenarios that take the env
step where a random policy almost never goes -- inside 5 m of the goal, through both stage latches, the final bonus, the
backward budget, several flags at once, headings wound many turns -- and the census that proves they do.

numpy only, `default_rng` with fixed seeds, every action precomputed in f32 so that the C oracle and the HIP kernel are fed the
same bits.  A scenario is a namespace of start [N,3], goal [N,3], L2 [N], kind [N], state0 [N,6] or None (raw state put on top
of the pose), term_mask or None (the default 0x3F), actions [T,N] f32.

Scenario A (default term_mask, N = 1000 = 15 waves of 64 and a 40-lane tail).  Per lane a goal of its own (x in [-20, 20],
y in [-35, -10], yaw pi/2 +- 0.3, L2 in [5, 10]) and a start above it (x = gx + N(0, 0.4), y = gy + U(0.3, 12),
yaw = gyaw + U(-0.35, 0.35)); kind = lane % 8 so every wave mixes the kinds:
  0..2  as drawn, action = per-lane constant U(-0.08, 0.08) + per-step N(0, 0.03)
  3     the same, times 30 every 7th step (far past the steering clip)
  4     steered uniformly in +-pi/4
  5     yaw + pi, 0.5..4 m above the goal: drives away (budget, backward penalty, excessive backward)
  6     20..40 m above the goal (far: the wave-uniform skip of the staged block when a whole wave is far)
  7     |x| in [39, 42.5]: minor and major boundary
Wave 13 (lanes 832..895) is all kind 6 (the skip path) and wave 14 (896..959) is kind 6 except lane 917, which is near (one lane
takes the staged block for the wave).

Scenario B (term_mask = F_MAX_STEPS only, N = 549): A's near-goal placement without kinds; the lanes run on past the goal, out
of the map, into the backward penalty, until their step limit, so the latches are read after they were set.

Scenario C (wound headings, N = 832): 64 base lanes placed as in A with a hitch offset in +-0.5 rad, repeated 12 times with
2*pi*k added to psi1 and psi2 through a raw state, k = WINDS; then 64 seam lanes 3 m from their goal whose psi2 lies within
1e-9 of +-pi, +-pi/2 and odd multiples of pi/4 (the sin/cos reduction's quadrant seams and the cut of the wrap to [-pi, pi]),
half of them with the goal yaw half a turn away so the orientation error sits on the cut too.  30 steps, steering +-0.3 + noise.
tt_env_set_state refuses no heading, so the copies are wound to k = 100000 (|psi| = 6.3e5; the reduction states |x| < 1e6).

Census of the C oracle alone on these inputs (census(), asserted with far lower minima in test_goal_zone_cpu.py):
                                   A (121 steps)   B (104 steps)
  ends: jackknife                  224             469 (B: flags set on the step that ends the lane, its step limit)
        out of map                 102             365
        max steps                  0               549
        goal reached / success     133             0 (116 lanes reach it; none ENDS there)
        past goal                  444             549
        excessive backward         111             549
  live lane-steps                  26908           49485
  lane-steps within 5 m            7216            11667
  25-stage / 100-stage payments    411 / 133       415 / 116
  final bonuses                    133             236
  at the goal, 100 already latched 0               120
  backward-penalty lane-steps      1747            35763
  wave-steps, near and far mixed   803             547
  violations minor / major         56 / 44         0 / 0 (labels 5 and 7 written over them)
  labels 5 / 7 over an earlier one 10              31359
  exploration tier 2 / tier 0      597 / 0         14931 / 10226
  distinct flag bytes              8               15: 00 10 11 12 13 30 31 32 33 34 35 36 37 48 58 (hex)
  everything finite                yes             yes
C (30 steps, 12696 live lane-steps): 172 successes, 484 / 172 stage payments, 206 jackknife and 406 past-goal ends; the oracle's
own drift between the k = 0 copy and a wound copy: obs 6.0e-8, state 4.3e-9, reward terms 9.0e-7 at k = 100000; 3.0e-8 / 2.1e-10
/ 1.2e-9 at |k| = 10000; flags identical.
"""
from types import SimpleNamespace

import numpy as np

from oracle import c_oracle

WAVE = 64
WINDS = (0, 1, -1, 7, -7, 100, -100, 1000, -1000, 10000, -10000, 100000)
I = {k: i for i, k in enumerate(c_oracle.INFO_KEYS)}


def _near_goal(rng, n):
    goal = np.stack([rng.uniform(-20, 20, n), rng.uniform(-35, -10, n), np.pi / 2 + rng.uniform(-0.3, 0.3, n)], 1)
    L2 = rng.uniform(5, 10, n)
    start = np.stack([goal[:, 0] + rng.normal(0, 0.4, n), goal[:, 1] + rng.uniform(0.3, 12, n),
                      goal[:, 2] + rng.uniform(-0.35, 0.35, n)], 1)
    return start, goal, L2


def _steering(rng, n, T):
    return (rng.uniform(-0.08, 0.08, n)[None, :] + rng.normal(0, 0.03, (T, n)))


def scenario_a():
    rng = np.random.default_rng(20240)
    n, T = 1000, 140
    start, goal, L2 = _near_goal(rng, n)
    kind = np.arange(n) % 8
    kind[13 * WAVE:15 * WAVE] = 6
    kind[14 * WAVE + 21] = 0
    act = _steering(rng, n, T)
    k3, k4, k5, k6, k7 = (kind == k for k in (3, 4, 5, 6, 7))
    act[::7, k3] *= 30.0
    act[:, k4] = rng.uniform(-np.pi / 4, np.pi / 4, (T, int(k4.sum())))
    start[k5, 1] = goal[k5, 1] + rng.uniform(0.5, 4, int(k5.sum()))
    start[k5, 2] += np.pi
    start[k6, 1] = goal[k6, 1] + rng.uniform(20, 40, int(k6.sum()))
    start[k7, 0] = rng.choice([-1.0, 1.0], int(k7.sum())) * rng.uniform(39, 42.5, int(k7.sum()))
    return SimpleNamespace(name="A", start=start, goal=goal, L2=L2, kind=kind, state0=None, term_mask=None,
                           actions=act.astype(np.float32))


def scenario_b():
    rng = np.random.default_rng(20241)
    n, T = 549, 120
    start, goal, L2 = _near_goal(rng, n)
    return SimpleNamespace(name="B", start=start, goal=goal, L2=L2, kind=np.zeros(n, int), state0=None,
                           term_mask=c_oracle.F_MAX_STEPS, actions=_steering(rng, n, T).astype(np.float32))


def _raw_state(x2, y2, psi1, psi2, L2):
    return np.stack([psi1, psi2, x2 + L2 * np.cos(psi2), y2 + L2 * np.sin(psi2), x2, y2], 1)


def scenario_c():
    rng = np.random.default_rng(20242)
    nb, T = 64, 30
    start, goal, L2 = _near_goal(rng, nb)
    psi2 = start[:, 2]
    psi1 = psi2 + rng.uniform(-0.5, 0.5, nb)
    base = _raw_state(start[:, 0], start[:, 1], psi1, psi2, L2)
    states, winds = [], []
    for k in WINDS:
        s = base.copy()
        s[:, 0] += 2 * np.pi * k
        s[:, 1] += 2 * np.pi * k
        states.append(s)
        winds.append(np.full(nb, k))
    act = np.tile(rng.choice([-0.3, 0.3], nb)[None, :] + rng.normal(0, 0.03, (T, nb)), (1, len(WINDS)))
    # seam lanes: psi2 = m*pi/4 + eps, hitch 0 (psi2 then stays at the seam while the truck turns), 3 m ahead of a goal at
    # (0, -10) (every heading keeps truck and trailer inside the map)
    m = np.repeat([1, -1, 2, -2, 3, -3, 4, -4], 8)
    eps = np.tile([-1e-9, -1e-12, -1e-15, 0.0, 1e-15, 1e-12, 1e-9, 3e-10], 8)
    spsi = m * (np.pi / 4) + eps
    ns = len(m)
    sgoal = np.stack([np.zeros(ns), np.full(ns, -10.0), m * (np.pi / 4) + np.pi * (np.arange(ns) % 2)], 1)
    sL2 = np.full(ns, 7.0)
    sx, sy = 3.0 * np.cos(spsi), -10.0 + 3.0 * np.sin(spsi)
    states.append(_raw_state(sx, sy, spsi, spsi, sL2))
    winds.append(np.zeros(ns, int))
    sact = rng.choice([-0.3, 0.3], ns)[None, :] + rng.normal(0, 0.03, (T, ns))
    reps = len(WINDS)
    return SimpleNamespace(name="C",
                           start=np.concatenate([np.tile(start, (reps, 1)), np.stack([sx, sy, spsi], 1)]),
                           goal=np.concatenate([np.tile(goal, (reps, 1)), sgoal]),
                           L2=np.concatenate([np.tile(L2, reps), sL2]),
                           kind=np.concatenate([np.zeros(nb * reps, int), np.ones(ns, int)]),     # 1: seam lane
                           wind=np.concatenate(winds), n_base=nb,
                           state0=np.concatenate(states), term_mask=None,
                           actions=np.concatenate([act, sact], 1).astype(np.float32))


def replace_odd(sc, seed=20243):
    """Scenario A's second act: the odd lanes placed again near their goals (start [k,3], idx [k]) and 40 steps of steering."""
    rng = np.random.default_rng(seed)
    n = len(sc.start)
    idx = np.arange(1, n, 2)
    g = sc.goal[idx]
    start = np.stack([g[:, 0] + rng.normal(0, 0.4, len(idx)), g[:, 1] + rng.uniform(0.3, 12, len(idx)),
                      g[:, 2] + rng.uniform(-0.35, 0.35, len(idx))], 1)
    return start, idx, _steering(rng, n, 40).astype(np.float32)


def make_oracle(sc, lanes=None):
    """A COracle holding the scenario (or its `lanes`) as placed; -> (oracle, obs0 [n,23])."""
    sel = slice(None) if lanes is None else lanes
    start = sc.start[sel]
    ora = c_oracle.COracle(len(start))
    if sc.term_mask is not None:
        ora.params.term_mask = int(sc.term_mask)
    obs0 = ora.place(start, goal=sc.goal[sel], L2=sc.L2[sel])
    if sc.state0 is not None:
        for i, y in enumerate(sc.state0[sel]):
            ora.set_state(i, y)
            obs0[i] = ora.observe(i)
    return ora, obs0


def place_lanes(ora, idx, start):
    """set_pose(start, idx=idx) on the oracle: lanes idx placed afresh at start [k,3], each keeping its goal and L2."""
    import ctypes as C
    place = c_oracle.lib().tto_place
    for i, s in zip(idx, np.ascontiguousarray(start, np.float64)):
        e = ora.envs[int(i)]
        goal, L2 = (C.c_double * 3)(*e.goal), C.c_double(e.L2)      # copies: tto_place clears the env first
        place(C.byref(ora.params), C.byref(e), (C.c_double * 3)(*s), goal, L2, None)


def oracle_trace(sc, ora=None, actions=None, alive=None):
    """Step the scenario's oracle (or `ora` with `actions`) until no lane of `alive` (default all) is left or the actions run
    out, keeping everything: obs0 [N,23] (None with `ora`), and per step obs, rew, done, info, state, flags, viol, alive (the
    lanes that had not finished BEFORE the step: the ones a test compares); T steps.  `ora` is left where the run ended."""
    obs0 = None
    if ora is None:
        ora, obs0 = make_oracle(sc)
    actions = sc.actions if actions is None else actions
    alive = np.ones(ora.n, bool) if alive is None else alive.copy()
    rec = {k: [] for k in ("obs", "rew", "done", "info", "state", "flags", "viol", "alive")}
    for a in actions:
        obs, rew, done, info = ora.step(a, nthreads=4)
        for k, v in zip(rec, (obs, rew, done, info, ora.state(), ora.flags(), ora.violation(), alive.copy())):
            rec[k].append(v)
        alive &= ~done
        if not alive.any():
            break
    return SimpleNamespace(ora=ora, obs0=obs0, T=len(rec["obs"]), **{k: np.stack(v) for k, v in rec.items()})


class Tally:
    """Counts of causes and branches over the lanes still alive, from one side's step outputs (the oracle's or the kernel's):
    flags [N] u8, violation [N] u8, done [N] bool, info [N,12] f64."""

    def __init__(self, n):
        self.n = n
        self.c = dict(jackknife=0, out_of_map=0, max_steps=0, goal_reached=0, past_goal=0, excessive=0, success=0,
                      within_5m=0, pay25=0, pay100=0, final_bonus=0, reentry_latched=0, backward_penalty=0, mixed_waves=0,
                      minor_boundary=0, major_boundary=0, explore_tier2=0, explore_tier0=0, max_steps_with_other=0,
                      overrides_5_7=0, live_lane_steps=0, steps=0)
        self.flag_bytes = set()
        self.pad = (-n) % WAVE

    def add(self, alive, done, flags, viol, info):
        c, m = self.c, alive
        ended = m & done
        for b, k in enumerate(("jackknife", "out_of_map", "max_steps", "goal_reached", "past_goal", "excessive", "success")):
            c[k] += int(((flags[ended] >> b) & 1).sum())
        staged, final = info[:, I["staged_success"]], info[:, I["final_success_bonus"]]
        near = staged >= 10.0
        pay100 = staged >= 110.0
        pay25 = (staged == 35.0) | (staged == 135.0)
        c["within_5m"] += int((m & near).sum())
        c["pay25"] += int((m & pay25).sum())
        c["pay100"] += int((m & pay100).sum())
        c["final_bonus"] += int((m & (final == 200.0)).sum())
        c["reentry_latched"] += int((m & (final == 200.0) & ~pay100).sum())
        c["backward_penalty"] += int((m & (info[:, I["backward_penalty"]] < 0.0)).sum())
        w_near = np.pad(m & near, (0, self.pad)).reshape(-1, WAVE).any(1)
        w_far = np.pad(m & ~near, (0, self.pad)).reshape(-1, WAVE).any(1)
        c["mixed_waves"] += int((w_near & w_far).sum())
        c["minor_boundary"] += int((m & (viol == 4)).sum())
        c["major_boundary"] += int((m & (viol == 3)).sum())
        c["explore_tier2"] += int((m & (info[:, I["exploration_bonus"]] == 2.0)).sum())
        c["explore_tier0"] += int((m & (info[:, I["exploration_bonus"]] == 0.0)).sum())
        c["max_steps_with_other"] += int((m & ((flags & c_oracle.F_MAX_STEPS) != 0) & ((flags & ~np.uint8(c_oracle.F_MAX_STEPS)) != 0)).sum())
        # a later violation label written over an earlier one: past-the-goal (5) or excessive-backward (7) on a step whose
        # safety sum holds more than that one -500
        c["overrides_5_7"] += int((m & ((viol == 5) | (viol == 7)) & (info[:, I["safety_penalty"]] < -500.0)).sum())
        c["live_lane_steps"] += int(m.sum())
        c["steps"] += 1
        self.flag_bytes.update(int(f) for f in np.unique(flags[m]))

    def result(self):
        return dict(self.c, distinct_flag_bytes=len(self.flag_bytes), flag_bytes=sorted(self.flag_bytes))


def census(sc, nthreads=4):
    """Step a COracle alone through the scenario, every lane to its own end (or the scenario's last action); -> Tally.result()
    plus `finite` (every observation, reward and state of a live lane was finite) and `all_done`."""
    ora, _ = make_oracle(sc)
    n = ora.n
    tally, alive, finite = Tally(n), np.ones(n, bool), True
    for a in sc.actions:
        obs, rew, done, info = ora.step(a, nthreads=nthreads)
        tally.add(alive, done, ora.flags(), ora.violation(), info)
        finite &= bool(np.isfinite(obs[alive]).all() and np.isfinite(info[alive]).all() and np.isfinite(ora.state()[alive]).all())
        alive = alive & ~done
        if not alive.any():
            break
    return dict(tally.result(), finite=finite, all_done=not alive.any())


# census minima (conditions on the inputs; the recipe gives several times as much)
MINIMA_A = dict(success=50, jackknife=50, out_of_map=50, past_goal=50, excessive=50, pay25=100, pay100=50,
                backward_penalty=500, mixed_waves=200, minor_boundary=20, major_boundary=20)
MINIMA_B = dict(reentry_latched=50, explore_tier2=1000, explore_tier0=1000, distinct_flag_bytes=10, max_steps_with_other=1)


def check_minima(counts, minima):
    low = {k: (counts[k], v) for k, v in minima.items() if counts[k] < v}
    assert not low, f"census below its minimum (got, wanted): {low}"


if __name__ == "__main__":
    for make in (scenario_a, scenario_b, scenario_c):
        sc = make()
        print(sc.name, len(sc.start), census(sc))
