#!/usr/bin/env python3
"""GPU: collect demonstrations with the sampling MPC expert (ddpg_trucktrailer_amd/mpc.py) and write the file
tools/train_vector.py --demos reads (expert.save_transitions_npz: obs, act, rew, obs2, done; act is the normalised steering).

--poses exp_gen: the reference generator's starts (0, 10, U(45, 120) degrees) (DDPG/exp_gen.py:31-32); --poses reset: the env's own
start distribution, reset(seed).  One episode per lane; --keep success (default) writes only the episodes that end in
TT_F_SUCCESS, --keep all every episode.  The statistics are printed as one JSON line.
Usage: collect_demos.py OUT.npz [--lanes 1024] [--poses exp_gen|reset] [--seed 0] [--keep success|all] [--max-steps T]
       [--horizon H] [--samples S] [--sigma X] [--rho X] [--temperature X] [--gamma X] [--k-lat X] [--k-yaw X]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from ddpg_trucktrailer_amd.expert import save_transitions_npz
    from ddpg_trucktrailer_amd.mpc import MPCConfig, collect_demonstrations, exp_gen_poses
    d = MPCConfig()
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--lanes", type=int, default=1024)
    ap.add_argument("--poses", choices=("exp_gen", "reset"), default="exp_gen")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--keep", choices=("success", "all"), default="success")
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--horizon", type=int, default=d.horizon)
    ap.add_argument("--samples", type=int, default=d.samples)
    for name in MPCConfig.FIELDS[2:]:
        ap.add_argument("--" + name.replace("_", "-"), type=float, default=getattr(d, name))
    a = ap.parse_args()
    cfg = MPCConfig(**{name: getattr(a, name) for name in MPCConfig.FIELDS})
    poses = exp_gen_poses(a.lanes, a.seed) if a.poses == "exp_gen" else None
    arrays, stats = collect_demonstrations(a.lanes, cfg, poses=poses, seed=a.seed, keep=a.keep, max_steps=a.max_steps)
    if stats["transitions"] == 0:
        print(json.dumps(dict(stats, lanes=None, lengths=None, end_flags=None, config=cfg.as_tuple())))
        sys.exit(f"no episode kept (keep = {a.keep}): {a.out} not written")
    save_transitions_npz(a.out, *arrays)
    brief = {k: v for k, v in stats.items() if k not in ("lanes", "lengths", "end_flags")}
    print(json.dumps(dict(brief, success_rate=stats["successes"] / stats["episodes"], poses=a.poses, config=repr(cfg), out=a.out)))


if __name__ == "__main__":
    main()
