#!/usr/bin/env python3
"""Fixture F8: the goal zone, captured from the REAL reference.

24 lanes of tests/goal_zone_cases.py's scenario A -- three of each kind (as drawn / saturating every 7th step / steered
uniformly / driving away / far / at the map's edge), each with a goal, goal yaw and trailer length of its own -- stepped by the
reference with the scenario's own f32 actions to their own end.  Among them at least 4 that succeed (both stage bonuses, the
final bonus, goal_reached) and at least 2 that take the 25-point stage but never the 100-point one.  The lanes are chosen by
what the C oracle does with them (deterministic); what the reference then did is asserted below before anything is written.

Scenario B's lanes are not terminated by the flags the reference ends an episode on.  The reference's step() itself resets
nothing when it returns done (simv2.py:499-545: the state, the step counter and the reward carry go on), so it steps on cleanly
and two of B's lanes are recorded too, `b<lane>`, to their step limit: `done` is what the reference returned on every step (any
flag), which is what the default term_mask gives when a caller keeps stepping a finished lane.  They pin the re-entry of the goal
with the 100-point latch already set (final bonus paid again, stage not) against the reference itself.

Runs only in the build container (needs /root/reference); writes tests/golden/f8_goal_zone.npz with make_golden.py's trajectory
fields less `state0` and `carry` (no lane has a raw state; the carry shows in the rewards); a trajectory's name holds its lane
and kind."""
import os
import sys

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402
import goal_zone_cases as Z  # noqa: E402


FIELDS = ("start", "goal", "L2", "max_episode_steps", "actions", "states", "obs0", "obs", "reward", "done", "violation", "flags",
          "info", "success")


def outcomes(sc):
    """Per lane of the scenario, from the C oracle alone: (succeeded, paid the 25-point stage, paid the 100-point stage,
    at the goal with the 100-point latch already set)."""
    ora, _ = Z.make_oracle(sc)
    n = ora.n
    alive = np.ones(n, bool)
    succ, p25, p100, again = (np.zeros(n, bool) for _ in range(4))
    for a in sc.actions:
        _, _, done, info = ora.step(a, nthreads=4)
        staged, final = info[:, Z.I["staged_success"]], info[:, Z.I["final_success_bonus"]]
        p25 |= alive & ((staged == 35.0) | (staged == 135.0))
        p100 |= alive & (staged >= 110.0)
        again |= alive & (final == 200.0) & (staged < 110.0)
        succ |= alive & done & ((ora.flags() & Z.c_oracle.F_SUCCESS) != 0)
        alive &= ~done
    return succ, p25, p100, again


def pick_a(sc):
    succ, p25, p100, _ = outcomes(sc)
    only25 = p25 & ~p100
    lanes = []
    for kind in range(8):
        of_kind = [i for i in range(13 * Z.WAVE) if sc.kind[i] == kind]
        wanted = [succ, only25] if kind < 4 else []
        chosen = []
        for w in wanted:
            hit = [i for i in of_kind if w[i] and i not in chosen]
            if hit:
                chosen.append(hit[0])
        chosen += [i for i in of_kind if i not in chosen and not succ[i] and not only25[i]][:3 - len(chosen)]
        lanes += sorted(chosen)
    return lanes


def record(Env, sc, lane, stop_on_done=True):
    env = Env()
    obs0 = mg.override_pose(env, sc.start[lane], goal=sc.goal[lane], L2=sc.L2[lane])
    actions = sc.actions[:, lane]
    if not stop_on_done:
        actions = actions[:int(env.max_episode_steps)]
    t = mg.run_trajectory(env, obs0, actions, stop_on_done=stop_on_done)
    return {k: t[k] for k in FIELDS}


def main():
    Env = mg.import_simv2()
    trajs, names = [], []
    a = Z.scenario_a()
    for lane in pick_a(a):
        t = record(Env, a, lane)
        trajs.append(t); names.append(f"a{lane:03d}_kind{int(a.kind[lane])}")
        print(f"F8 {names[-1]}: len {len(t['actions'])}, flags {t['flags'][-1].astype(int)}, success {bool(t['success'][-1])}, "
              f"staged {sorted(set(t['info'][:, 5].tolist()))}, return {t['reward'].sum():.3f}")
    assert len(trajs) == 24 and all(t["done"][-1] and not t["done"][:-1].any() for t in trajs)
    assert all(sum(n.endswith(f"kind{k}") for n in names) == 3 for k in range(8))
    paid = lambda t, v: bool(np.isin(t["info"][:, 5], v).any())
    assert sum(bool(t["success"][-1]) and t["info"][-1, 8] == 200.0 for t in trajs) >= 4
    assert sum(paid(t, [35.0]) and not paid(t, [110.0, 135.0]) for t in trajs) >= 2

    b = Z.scenario_b()
    _, _, _, again = outcomes(b)
    for lane in np.nonzero(again)[0][:2]:
        t = record(Env, b, int(lane), stop_on_done=False)
        assert len(t["actions"]) == int(t["max_episode_steps"]) and t["flags"][-1][2] and not t["flags"][:-1, 2].any()
        latched = np.cumsum(t["info"][:, 5] >= 110.0) > 0
        assert ((t["info"][:, 8] == 200.0) & (t["info"][:, 5] < 110.0) & latched).any(), "no re-entry with the latch set"
        trajs.append(t); names.append(f"b{int(lane):03d}")
        print(f"F8 {names[-1]}: len {len(t['actions'])}, first done at {int(np.argmax(t['done']))}, final bonuses "
              f"{int((t['info'][:, 8] == 200.0).sum())}, 100-stages {int((t['info'][:, 5] >= 110.0).sum())}, "
              f"violations {sorted(set(t['violation'].tolist()))}, finite {bool(np.isfinite(t['reward']).all())}")

    mg.save_group(os.path.join(HERE, "f8_goal_zone.npz"), trajs, names,
                  "reference simv2 on lanes of tests/goal_zone_cases.py scenario A (to their end) and B (on past done, to the "
                  f"step limit), per-lane goal / L2 through the callers' pose-override pattern ({mg.versions()})")


if __name__ == "__main__":
    main()
