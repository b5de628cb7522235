#!/usr/bin/env python3
"""GPU: what episode randomisation costs in the loop, and that a loop without it costs what the parent commit's does (DESIGN.md
section 39).

ms per vector step of DDPGRollout at --envs lanes (65536: the default loop; 4096) with --updates updates per step, B = 256,
graph-replayed: `legs` legs each of
    off      the plain loop;
    per-env  the plain loop after a set_pose with the parameters' goal and L2, which turns the per-env path on: the cold-row loads
             (48 more bytes per env-step) are paid, the plain reset piece runs;
    on       the randomised loop, EpisodeRandomization(goal=--goal, L2=--L2): the per-env loads and the randomised step kernel,
             which adds work for finished lanes only;
and, with --parent-tree DIR (a checkout of the parent commit with its library built), the parent's loop ("parent").  Every leg is a
fresh process; the variants alternate within a round and their order from round to round.  Every leg is printed, and written to --out.

The gate is the rule of DESIGN.md section 13 on the off leg: its median at most the parent's median plus the parent legs' own
max - min (it launches the parent's kernels).  per-env - off and on - off are records, not gates; on - per-env is the reset piece's price.
Usage: randomize_cost.py [--envs 65536] [--updates 1] [--legs 3] [--steps 400] [--warmup 60] [--L2 5,10] [--goal=-10,10,-32,-28,1.3,1.8]
                         [--parent-tree DIR] [--out FILE]
       randomize_cost.py --leg off|per-env|on [--tree DIR] ...      (one leg in this process; prints "LEG <ms per vector step>")"""
import option_cost


def main():
    a = option_cost.parse([("--envs", dict(type=int, default=65536)), ("--updates", dict(type=int, default=1)),
                           ("--L2", dict(default="5,10")), ("--goal", dict(default="-10,10,-32,-28,1.3,1.8"))],
                          choices=("off", "per-env", "on"))
    option_cost.N, option_cost.UPD = a.envs, a.updates
    l2 = tuple(float(x) for x in a.L2.split(","))
    x0, x1, y0, y1, yaw0, yaw1 = (float(x) for x in a.goal.split(","))
    goal = ((x0, y0, yaw0), (x1, y1, yaw1))

    def options():
        if a.leg != "on":
            return {}
        from ddpg_trucktrailer_amd.randomize import EpisodeRandomization
        return {"randomize": EpisodeRandomization(goal=goal, L2=l2)}

    def prepare(loop):
        if a.leg != "per-env":
            return
        # the lanes where they are, with the parameters' goal and length written per env: the per-env path, nothing else changed
        import torch
        env = loop.env
        p = env.params
        n = env.n_envs
        env.set_pose(env.episode()["start"], goal=torch.tensor(list(p.goal), dtype=torch.float64).repeat(n, 1),
                     L2=torch.full((n,), float(p.L2), dtype=torch.float64), out=loop.ring.obs[0])

    def stats(loop):
        if a.leg != "on":
            return ""
        from ddpg_trucktrailer_amd.randomize import summary
        s = summary(loop.env.randomization_ranges(), loop.env.episode())
        return "\nRANDOMIZE lanes now (min / mean / max): " + ", ".join(
            f"{k} {s[k][0]:.3f} / {s[k][1]:.3f} / {s[k][2]:.3f}" for k in ("L2", "goal_x", "goal_y", "goal_yaw"))

    if a.leg:
        return option_cost.one_leg(a, options, prepare=prepare, stats=stats)
    option_cost.compare(a, __file__, ["off", "per-env", "on"], ["--envs", str(a.envs), "--updates", str(a.updates), "--L2", a.L2,
                                                                "--goal=" + a.goal],
                        {"off": "the plain loop", "per-env": "the plain loop on the per-env path",
                         "on": "the randomised loop (--goal, --L2)"}, 40, records=True, echo="RANDOMIZE ",
                        between=[("on", "per-env")])


if __name__ == "__main__":
    main()
