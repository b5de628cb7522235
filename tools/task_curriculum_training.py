#!/usr/bin/env python3
"""GPU: one training run on randomised tasks, with or without the task curriculum, and a greedy evaluation at its end on tasks drawn
from a scratch randomised env (DESIGN.md sections 39 and 40; the record is profiles/task_curriculum_training.md).

DDPGRollout at N lanes with episode randomisation (--goal, --L2) and, with --task-curriculum NGX,NGY,NGYAW,NL2[,EVERY[,MODE]], the task
curriculum.  After every report block a line with the block's episodes and successes (and task_summary's numbers); at the end the
evaluation of the actor without noise on --eval-lanes tasks -- start, goal and L2 of a scratch env with the same ranges, reset with
--eval-seed: the same tasks for every run with the same arguments -- with the success rate per L2 bin of the EVALUATION (both kinds of
run have it), and, with the task curriculum, the training-time table from task_summary.
Usage: task_curriculum_training.py [--task-curriculum 4,4,4,4] [--L2 5,10] [--goal=-10,10,-32,-28,1.3,1.8] [--eval-lanes 1024]
                                   [--eval-seed 1234] [--l2-bins 4] n_envs ring_slots updates_per_step batch vector_steps report_every [seed]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ddpg_trucktrailer_amd.evaluation import Evaluator, summary
from ddpg_trucktrailer_amd.randomize import EpisodeRandomization
from ddpg_trucktrailer_amd.rollout import DDPGRollout
from ddpg_trucktrailer_amd.task_curriculum import TaskCurriculum, task_summary
from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task-curriculum", default=None)
    ap.add_argument("--L2", default="5,10")
    ap.add_argument("--goal", default="-10,10,-32,-28,1.3,1.8")
    ap.add_argument("--eval-lanes", type=int, default=1024)
    ap.add_argument("--eval-seed", type=int, default=1234)
    ap.add_argument("--l2-bins", type=int, default=4)
    ap.add_argument("numbers", nargs="+", type=int)
    a = ap.parse_args()
    n, slots, upd, batch, total, every = a.numbers[:6]
    seed = a.numbers[6] if len(a.numbers) > 6 else 27
    l2 = tuple(float(x) for x in a.L2.split(","))
    x0, x1, y0, y1, yaw0, yaw1 = (float(x) for x in a.goal.split(","))
    rand = EpisodeRandomization(goal=((x0, y0, yaw0), (x1, y1, yaw1)), L2=l2)
    task = None
    if a.task_curriculum:
        parts = a.task_curriculum.split(",")
        task = TaskCurriculum(tuple(int(x) for x in parts[:4]), **({"every": int(parts[4])} if len(parts) > 4 else {}),
                              **({"mode": parts[5]} if len(parts) > 5 else {}))
    env = TruckTrailerVecEnv(n)
    env.reset(seed=seed)
    loop = DDPGRollout(env, batch_size=batch, replay_slots=slots, seed=seed, updates_per_step=upd, graph_steps=20,
                       episode_log=min(n * every, 1 << 24), randomize=rand, task_curriculum=task)
    print(f"N = {n}, ring {slots}, {upd} updates per vector step, batch {batch}, seed {seed}, {rand}" + (f", {task}" if task else ""), flush=True)

    def table(rows):
        return " ".join(f"[{lo:g}, {hi:g}) {'-' if rate is None else f'{rate:.3f}'} ({seen})" for lo, hi, seen, rate in rows)

    s, t0 = 0, time.time()
    while s < total:
        k = min(every, total - s)
        loop.run(k)
        s += k
        r = loop.drain_episodes()
        m = max(1, len(r["ret"]))
        line = (f"vector steps {s:6d}: episodes {len(r['ret']):6d}  mean return {r['ret'].sum().item() / m:9.1f}  successes "
                f"{int(r['success'].sum().item()):6d} ({100 * r['success'].double().sum().item() / m:4.1f} %)")
        if task is not None:
            st = task_summary(env.task_curriculum_state(), env.randomization_ranges())
            line += (f"  cells seen {100 * st['cells_seen']:5.1f} %, mean p {st['mean_p']:.3f}, top-decile weight "
                     f"{100 * st['top_decile_weight']:4.1f} %")
        print(line + f"  {time.time() - t0:.0f}s", flush=True)
    if task is not None:
        st = task_summary(env.task_curriculum_state(), env.randomization_ranges())
        for name in ("L2", "goal_x", "goal_y", "goal_yaw"):
            print(f"training, success by {name} (seen-weighted running rate per bin, episodes seen): {table(st['by_' + name])}")
    # the evaluation set: a scratch randomised env's episode 0 (a pure function of the ranges and the seed)
    scratch = TruckTrailerVecEnv(a.eval_lanes)
    scratch.enable_randomization(rand)
    scratch.reset(seed=a.eval_seed)
    e = scratch.episode()
    ev = Evaluator(a.eval_lanes, poses=e["start"], goal=e["goal"], L2=e["L2"], device=scratch.device)
    rec = loop.evaluate(ev)
    out = summary(rec)
    print(f"evaluation on {a.eval_lanes} tasks (eval seed {a.eval_seed}): mean return {out['mean_return']:9.1f}  success rate "
          f"{out['success_rate']:5.3f}  mean length {out['mean_len']:6.1f}")
    ok = np.asarray(rec["success"].cpu()).astype(bool)
    length = np.asarray(e["L2"].cpu())
    edges = np.linspace(l2[0], l2[1], a.l2_bins + 1)
    which = np.minimum(a.l2_bins - 1, np.searchsorted(edges, length, side="right") - 1)
    rows = [(edges[b], edges[b + 1], int((which == b).sum()), float(ok[which == b].mean()) if (which == b).any() else None)
            for b in range(a.l2_bins)]
    print(f"evaluation, success by L2 (rate, tasks): {table(rows)}")


if __name__ == "__main__":
    main()
