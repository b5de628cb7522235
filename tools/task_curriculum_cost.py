#!/usr/bin/env python3
"""GPU: what the task curriculum costs in the loop, and that a loop without it costs what the parent commit's does (DESIGN.md
section 40).

ms per vector step of DDPGRollout at --envs lanes (65536: the default loop; 4096) with --updates updates per step, B = 256,
graph-replayed: `legs` legs each of
    off         the plain loop;
    randomised  the randomised loop, EpisodeRandomization(goal=--goal, L2=--L2) (section 39's `on`);
    task        the same ranges with TaskCurriculum(--bins, every=--every): the task curriculum's step kernel, which adds the counting
                and the weighted pick for finished lanes only, and one small launch every `every` steps between graph replays;
and, with --parent-tree DIR (a checkout of the parent commit with its library built), the parent's loop ("parent").  Every leg is a
fresh process; the variants alternate within a round and their order from round to round.  Every leg is printed, and written to --out.

The gate is the rule of DESIGN.md section 13 on the off leg: its median at most the parent's median plus the parent legs' own
max - min (it launches the parent's kernels).  task - randomised and task - off are records, not gates.
Usage: task_curriculum_cost.py [--envs 65536] [--updates 1] [--legs 3] [--steps 400] [--warmup 60] [--L2 5,10]
                               [--goal=-10,10,-32,-28,1.3,1.8] [--bins 4,4,4,4] [--every 64] [--parent-tree DIR] [--out FILE]
       task_curriculum_cost.py --leg off|randomised|task [--tree DIR] ...      (one leg in this process; prints "LEG <ms per vector step>")"""
import option_cost


def main():
    a = option_cost.parse([("--envs", dict(type=int, default=65536)), ("--updates", dict(type=int, default=1)),
                           ("--L2", dict(default="5,10")), ("--goal", dict(default="-10,10,-32,-28,1.3,1.8")),
                           ("--bins", dict(default="4,4,4,4")), ("--every", dict(type=int, default=64))],
                          choices=("off", "randomised", "task"))
    option_cost.N, option_cost.UPD = a.envs, a.updates
    l2 = tuple(float(x) for x in a.L2.split(","))
    x0, x1, y0, y1, yaw0, yaw1 = (float(x) for x in a.goal.split(","))
    goal = ((x0, y0, yaw0), (x1, y1, yaw1))
    bins = tuple(int(x) for x in a.bins.split(","))

    def options():
        if a.leg == "off":
            return {}
        from ddpg_trucktrailer_amd.randomize import EpisodeRandomization
        kw = {"randomize": EpisodeRandomization(goal=goal, L2=l2)}
        if a.leg == "task":
            from ddpg_trucktrailer_amd.task_curriculum import TaskCurriculum
            kw["task_curriculum"] = TaskCurriculum(bins, every=a.every)
        return kw

    def stats(loop):
        if a.leg != "task":
            return ""
        from ddpg_trucktrailer_amd.task_curriculum import task_summary
        s = task_summary(loop.env.task_curriculum_state(), loop.env.randomization_ranges())
        return (f"\nTASK cells seen {s['cells_seen']:.3f}, mean p {s['mean_p']:.4f}, top-decile weight {s['top_decile_weight']:.3f}, success by L2 " +
                " ".join(f"[{lo:g}, {hi:g}) {'-' if rate is None else f'{rate:.3f}'}" for lo, hi, _, rate in s["by_L2"]))

    if a.leg:
        return option_cost.one_leg(a, options, stats=stats)
    option_cost.compare(a, __file__, ["off", "randomised", "task"],
                        ["--envs", str(a.envs), "--updates", str(a.updates), "--L2", a.L2, "--goal=" + a.goal, "--bins", a.bins,
                         "--every", str(a.every)],
                        {"off": "the plain loop", "randomised": "the randomised loop (--goal, --L2)",
                         "task": f"TaskCurriculum({bins}, every={a.every})"}, 42, records=True, echo="TASK ",
                        between=[("task", "randomised")])


if __name__ == "__main__":
    main()
