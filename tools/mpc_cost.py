#!/usr/bin/env python3
"""GPU: what one planning launch of the sampling MPC costs (tt_env_mpc_plan), as a record, not a gate.

For each lane count: envs from reset(seed), `warmup` launches, then `reps` launches timed one by one with device events; reported
are the median and the spread of the launch time and the env steps per second inside it, counted as lanes * samples * horizon (an
upper bound on the steps executed: a sample that terminates inside the horizon stops early).
Usage: mpc_cost.py [--lanes 64,1024,16384] [--horizon 40] [--samples 256] [--reps 10] [--warmup 2]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from ddpg_trucktrailer_amd.mpc import MPCConfig, MPCExpert
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", default="64,1024,16384")
    ap.add_argument("--horizon", type=int, default=40)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    cfg = MPCConfig(horizon=a.horizon, samples=a.samples)
    for n in (int(x) for x in a.lanes.split(",")):
        env = TruckTrailerVecEnv(n, device="cuda:0")
        env.reset(seed=1)
        ex = MPCExpert(env, cfg, seed=1)
        for _ in range(a.warmup):
            ex.act()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            ex.act()
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        med = statistics.median(ms)
        print(json.dumps(dict(lanes=n, horizon=cfg.horizon, samples=cfg.samples, reps=a.reps, ms_median=round(med, 4), ms_min=round(min(ms), 4),
                              ms_max=round(max(ms), 4), env_steps_per_launch=n * cfg.samples * cfg.horizon,
                              env_steps_per_s=round(n * cfg.samples * cfg.horizon / (med * 1e-3), 1))), flush=True)
        env.close()


if __name__ == "__main__":
    main()
