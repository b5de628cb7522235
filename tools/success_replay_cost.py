#!/usr/bin/env python3
"""GPU: what success replay costs in the loop, and that a loop without it costs what the parent commit's does.

ms per vector step of DDPGRollout at --envs lanes (65536: the default loop) with --updates updates per step, B = 256, graph-replayed,
with the episode log on and demo_loss (what the option runs with): `legs` legs each of
    off   the loop without the option;
    on    SuccessReplay(--capacity, every=--every): graph replays cut at multiples of `every`, two small launches there, and the
          captures made again each time the region's exposed count moves (the leg exposes it once, before the warm-up's end);
and, with --parent-tree DIR (a checkout of the parent commit with its library built), the parent's loop with off's arguments
("parent").  Every leg is a fresh process; the variants alternate within a round and their order from round to round.  The on leg
also prints the harvest's own time: HIP events around tt_env_harvest's two launches (plan + copy) on the loop's state at the end of
the leg, the median of --harvests calls with the mark rewound to 0 before each, so that every call plans the whole log and copies
the same episodes.

The gate is the rule of DESIGN.md section 13 on the off leg: its median at most the parent's median plus the parent legs' own
max - min.  on - off and the harvest's time are records, not gates.
Usage: success_replay_cost.py [--envs 65536] [--updates 1] [--legs 3] [--steps 400] [--warmup 60] [--capacity 65536] [--every 32]
                              [--harvests 20] [--parent-tree DIR] [--out FILE]
       success_replay_cost.py --leg off|on [--tree DIR] ...      (one leg in this process; prints "LEG <ms per vector step>")"""
import statistics

import option_cost


def main():
    a = option_cost.parse([("--envs", dict(type=int, default=65536)), ("--updates", dict(type=int, default=1)),
                           ("--capacity", dict(type=int, default=65536)), ("--every", dict(type=int, default=32)),
                           ("--harvests", dict(type=int, default=20))], choices=("off", "on"))
    option_cost.N, option_cost.UPD = a.envs, a.updates

    def options():
        from ddpg_trucktrailer_amd.demo_loss import DemoLoss
        kw = {"episode_log": 65536, "demo_loss": DemoLoss(0.5)}
        if a.leg == "on":
            from ddpg_trucktrailer_amd.success_replay import SuccessReplay
            kw["success_replay"] = SuccessReplay(a.capacity, every=a.every)
        return kw

    def stats(loop):
        if a.leg != "on":
            return ""
        import torch
        st = loop.success_replay_stats()
        times = []
        for _ in range(a.harvests):
            loop.ring.harvest["state"][0] = 0
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            loop.harvest()
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1) * 1e3)
        window = int(loop.ring.harvest["state"][0])
        again = loop.success_replay_stats()
        return (f"\nHARVEST in the leg: {st['episodes']} episodes, {st['rows']} rows, {st['rows_cut']} rows cut, {st['expired']} expired, "
                f"{st['exposed']} exposed; tt_env_harvest (plan + copy, HIP events) over the log's {window} records, "
                f"{(again['episodes'] - st['episodes']) // a.harvests} of them eligible with {(again['rows'] - st['rows']) // a.harvests} rows: "
                f"median {statistics.median(times):.1f} us, min {min(times):.1f}, max {max(times):.1f} over {a.harvests} calls")

    if a.leg:
        return option_cost.one_leg(a, options, stats=stats)
    option_cost.compare(a, __file__, ["off", "on"],
                        ["--envs", str(a.envs), "--updates", str(a.updates), "--capacity", str(a.capacity), "--every", str(a.every),
                         "--harvests", str(a.harvests)],
                        {"off": "episode_log + demo_loss", "on": f"+ SuccessReplay({a.capacity}, every={a.every})"}, 40, records=True,
                        echo="HARVEST ")


if __name__ == "__main__":
    main()
