#!/usr/bin/env python3
"""GPU: which plain step kernel a randomised env agrees with bit for bit (the record is
profiles/randomize_twin_probe.txt).

Env A has episode randomisation on and is reset with a seed.  Three twins without the option are placed with set_pose(start, goal,
L2) from what A reports and driven with A's actions for --steps steps (episodes of 50 steps: no lane finishes):
    auto0   stepped with auto_reset = 0     (k_step<true, INFO, false, false>)
    auto1   stepped with auto_reset = 1     (k_step<true, INFO, true, false>)
    log1    auto_reset = 1, episode log on  (k_step_log<true, INFO, true, false>)
After every step the six state columns (psi1, psi2, x1, y1, x2, y2) of A and of each twin are compared as 64-bit words: per column
the number of lanes that differ and the largest difference in units of the last place.  Both with and without the info rows.  The
last line of each round compares auto0 with auto1 -- two kernels of the parent commit.
Usage: randomize_twin_probe.py [--envs 130] [--steps 6] [--seed 11]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ddpg_trucktrailer_amd import _lib as L
from ddpg_trucktrailer_amd.randomize import EpisodeRandomization
from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv

COLUMNS = ("psi1", "psi2", "x1", "y1", "x2", "y2")


def make_env(n):
    p = L.default_params(0)
    p.fixed_max_steps = 50
    return TruckTrailerVecEnv(n, params=p)


def words(env):
    return env.state.cpu().numpy().view(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=130)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--seed", type=int, default=11)
    a = ap.parse_args()
    print(f"# columns: {', '.join(COLUMNS)}; N = {a.envs}, reset seed {a.seed}, goal x [-10, 10] y [-32, -28] yaw [1.3, 1.8], L2 [5, 10]")
    for info in (True, False):
        rnd = make_env(a.envs)
        rnd.enable_randomization(EpisodeRandomization(goal=((-10.0, -32.0, 1.3), (10.0, -28.0, 1.8)), L2=(5.0, 10.0)))
        rnd.reset(seed=a.seed)
        e = rnd.episode()
        twins = {}
        for name in ("auto0", "auto1", "log1"):
            twins[name] = make_env(a.envs)
            if name == "log1":
                twins[name].enable_episode_log(1024)
            twins[name].set_pose(e["start"], goal=e["goal"], L2=e["L2"])
        for k in range(a.steps):
            act = rnd.random_actions(seed=5, step=k)
            _, _, done, _ = rnd.step(act, auto_reset=True, info=info)
            assert not bool(done.any()), "a lane finished: the probe compares running episodes only"
            mine = words(rnd)
            for name, twin in twins.items():
                twin.step(act, auto_reset=(name != "auto0"), info=info)
                d = mine - words(twin)
                print(f"info={int(info)} step {k} randomised vs {name}: lanes differing {[int((d[:, c] != 0).sum()) for c in range(6)]} "
                      f"max |ulp| {[int(np.abs(d[:, c]).max()) for c in range(6)]}", flush=True)
        print(f"info={int(info)} after {a.steps} steps, auto0 vs auto1 (both the parent commit's kernels): "
              f"{int((words(twins['auto0']) != words(twins['auto1'])).sum())} of {6 * a.envs} state words differ", flush=True)
        for env in (rnd, *twins.values()):
            env.close()


if __name__ == "__main__":
    main()
