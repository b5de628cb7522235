"""GPU: what the learn log costs the vector loop (DDPGRollout(learn_log=..., learn_log_every=1)), measured as interleaved series
in ONE process -- log off and log on, two series of each, so that off against off is the run's own spread:

  headline      N = 65536, one update per step, pipelined, 20-step graphs: us per vector step
  small         N = 4096, one update per step, pipelined, 20-step graphs: us per vector step
  learn-bound   N = 4096, --updates-per-step U (default 64), pipelined, 4-step graphs: us per update

and the on - off difference per update of each.

usage: learn_log_cost.py [--updates-per-step U] [rounds]          the three tables
       learn_log_cost.py --launch [STEPS]                         only a loop with the log on (N = 4096, U updates per step): run it
                                                                  under `rocprofv3 --kernel-trace --output-format csv -d DIR --`
       learn_log_cost.py --median KERNEL_TRACE_CSV                the median duration of k_learn_log (and of learn()'s other launches)
                                                                  in such a trace"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make(n, updates, graph_steps, log):
    import torch
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    env = TruckTrailerVecEnv(n)
    env.reset(seed=27)
    loop = DDPGRollout(env, batch_size=256, replay_slots=64, seed=27, graph_steps=graph_steps, updates_per_step=updates,
                       learn_log=4096 if log else None, learn_log_every=1)
    loop.run(loop._warm_steps + 2 * graph_steps + 5)      # eager warm-up, captures, first replays
    torch.cuda.synchronize()
    return loop


def series(title, loops, k, rounds, per):
    import torch
    times = {name: [] for name, _ in loops}
    for _ in range(rounds):
        for name, loop in loops:                               # alternate: one timing of each per round
            t0 = time.perf_counter()
            loop.run(k)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / k * 1e6 / per)
    print(title)
    for name, _ in loops:
        t = times[name]
        print(f"  {name:18s} median {statistics.median(t):8.2f}  min {min(t):8.2f}  max {max(t):8.2f}   " + " ".join(f"{x:.2f}" for x in t),
              flush=True)
    m = {name: statistics.median(t) for name, t in times.items()}
    on, off = (m["log on, series A"] + m["log on, series B"]) / 2, (m["log off, series A"] + m["log off, series B"]) / 2
    print(f"  on - off = {on - off:+.2f} us; spread of off against off {abs(m['log off, series A'] - m['log off, series B']):.2f}, "
          f"of on against on {abs(m['log on, series A'] - m['log on, series B']):.2f}", flush=True)
    for name, loop in loops:
        if loop.learner.learn_log is not None:
            rec = loop.drain_learn_log()
            assert len(rec["step"]) and int(rec["nonfinite"].sum()) == 0, name
    return on - off


def table(n, updates, graph_steps, k, rounds, what):
    loops = [(f"log {s}, series {ab}", make(n, updates, graph_steps, s == "on")) for ab in "AB" for s in ("off", "on")]
    for name, lp in loops:
        assert lp.pipeline and lp.graph_steps == graph_steps, name
    d = series(f"N = {n}, {updates} update(s) per vector step, pipelined, {graph_steps}-step graphs: us per {what}", loops, k, rounds,
               updates if what == "update" else 1)
    if what != "update":
        print(f"  = {d / updates:+.2f} us per update", flush=True)


def median_of_trace(path):
    import collections
    import csv
    import re
    durs = collections.defaultdict(list)
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows[len(rows) // 3:]:                            # (the first third: warm-up and eager steps)
        m = re.search(r"k_\w+", r["Kernel_Name"])
        durs[m.group(0) if m else r["Kernel_Name"][:40]].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, v in sorted(durs.items(), key=lambda kv: -len(kv[1])):
        if len(v) >= 20:
            v.sort()
            print(f"  {name:36s} x{len(v):6d}  median {statistics.median(v):7.2f}  p10 {v[len(v) // 10]:7.2f}  p90 {v[len(v) * 9 // 10]:7.2f} us")


def main():
    args = sys.argv[1:]
    updates = 64
    if "--updates-per-step" in args:
        at = args.index("--updates-per-step")
        updates = int(args[at + 1])
        del args[at:at + 2]
    if args and args[0] == "--median":
        return median_of_trace(args[1])
    if args and args[0] == "--launch":
        import torch
        loop = make(4096, updates, 4, True)
        loop.run(int(args[1]) if len(args) > 1 else 40)
        torch.cuda.synchronize()
        rec = loop.drain_learn_log()
        print(f"{len(rec['step'])} records, last update {int(rec['step'][-1])}, critic loss {rec['critic_loss'][-1]:.4g}")
        return
    from ddpg_trucktrailer_amd import _lib as L
    rounds = int(args[0]) if args else 9
    print(f"learn log: {L.LEARN_LOG_CHUNKS} workgroups per gradient")
    table(65536, 1, 20, 200, rounds, "vector step")
    table(4096, 1, 20, 200, rounds, "vector step")
    table(4096, updates, 4, 8, rounds, "update")


if __name__ == "__main__":
    main()
