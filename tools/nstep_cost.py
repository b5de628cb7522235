"""GPU: what n-step returns cost the vector loop (DDPGRollout(n_step=...)), measured as interleaved series in ONE process:

  learn-bound   N = 4096, 64 updates per vector step (the regime of tools/updates_scaling.py): us per update of
                n_step = 1 (twice: the two series against each other are the run's own spread), n_step = 5 (twice), and
                n_step = 1 with every update making its own draw (TT_MULTI_DRAW=0): the launch structure n_step = 5 has,
                so that pair compares the two first launches like for like;
  headline      N = 65536, one update per step, pipelined: us per step of n_step = 1 and n_step = 5, two series each.

usage: nstep_cost.py [rounds]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from ddpg_trucktrailer_amd.rollout import DDPGRollout
from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv


def make(n, updates, graph_steps, n_step, own_draw=False):
    env = TruckTrailerVecEnv(n)
    env.reset(seed=27)
    if own_draw:
        os.environ["TT_MULTI_DRAW"] = "0"
    try:
        loop = DDPGRollout(env, batch_size=256, replay_slots=64, seed=27, graph_steps=graph_steps, updates_per_step=updates, n_step=n_step)
        loop.run(loop._warm_steps + 2 * graph_steps + 5)      # eager warm-up, captures, first replays
        torch.cuda.synchronize()
    finally:
        os.environ.pop("TT_MULTI_DRAW", None)
    return loop


def series(title, loops, k, rounds, per):
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
        print(f"  {name:34s} median {statistics.median(t):8.2f}  min {min(t):8.2f}  max {max(t):8.2f}   "
              + " ".join(f"{x:.2f}" for x in t), flush=True)
    return {name: statistics.median(t) for name, t in times.items()}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    U = 64
    loops = [("n_step 1, series A", make(4096, U, 4, 1)), ("n_step 5, series A", make(4096, U, 4, 5)),
             ("n_step 1, series B", make(4096, U, 4, 1)), ("n_step 5, series B", make(4096, U, 4, 5)),
             ("n_step 1, own draw per update", make(4096, U, 4, 1, own_draw=True))]
    for name, lp in loops:
        assert lp.pipeline and lp.graph_steps == 4, name
    m = series(f"N = 4096, {U} updates per vector step, pipelined, 4-step graphs: us per update", loops, 8, rounds, U)
    spread = abs(m["n_step 1, series A"] - m["n_step 1, series B"])
    d = (m["n_step 5, series A"] + m["n_step 5, series B"]) / 2 - (m["n_step 1, series A"] + m["n_step 1, series B"]) / 2
    print(f"  n_step 5 - n_step 1 = {d:+.2f} us per update; spread of n_step 1 against itself {spread:.2f}; "
          f"n_step 5 - n_step 1 with its own draw = {(m['n_step 5, series A'] + m['n_step 5, series B']) / 2 - m['n_step 1, own draw per update']:+.2f}")
    del loops
    loops = [("n_step 1, series A", make(65536, 1, 20, 1)), ("n_step 5, series A", make(65536, 1, 20, 5)),
             ("n_step 1, series B", make(65536, 1, 20, 1)), ("n_step 5, series B", make(65536, 1, 20, 5))]
    series("N = 65536, one update per vector step, pipelined, 20-step graphs: us per vector step", loops, 200, rounds, 1)


if __name__ == "__main__":
    main()
