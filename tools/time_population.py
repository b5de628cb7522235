#!/usr/bin/env python3
"""GPU: what a population of K agents buys (ddpg_trucktrailer_amd/population.py).

learn() alone, K in {1, 2, 4, 8, 16} at B = 256: per K a PopulationLearner on K filled rings, a captured graph of `per_graph`
population updates replayed after warm-up, timed with device events over >= `updates` updates; `legs` legs with the K values in
alternating order -> median and spread of us per population update and of aggregate agent-updates/s.  Beside them the lone
FusedLearner's chain (the tail in one launch) timed the same way.
Then the loop: K = 8 x n = 8192 envs at 8 updates per step (1024 env-steps per update per agent) against one agent at N = 65536
with 64 updates per step, in the same process.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/time_population.py --no-loop` separately.
--n-step N: instead of all that, what per-agent n-step returns cost: at K in {1, 4, 8}, us per population
update of the one-step population (no table; two populations, two series), of n = 1 through the n-step table and of n = N, the
variants interleaved within each leg; with --baseline-lib PATH (a libttenv.so built from another commit, loaded beside this one)
that library's one-step population as well, also twice: the distance between two series of one library is the run-to-run spread
the no-table path is held to.
--td3 [DELAY]: instead of all that, TD3 populations: K in {1, 2, 4, 8, 16} PopulationTD3Learners at B = 256
and policy_delay DELAY (default 2: critic-only and full updates in alternation, the average update), beside the lone TD3Learner
(tools/td3_cost.py's leg), all timed the same way in alternating legs; every leg is printed and, with --out, written to a file.
Section 13's rule at K = 1: is the population's median within the lone median plus the lone legs' own max - min?
--grad-clip C[,A]: instead of all that, what per-agent gradient-norm clipping costs: at K in {1, 4, 8}, us per
population update and agent-updates/s of the population without a clip table (two populations, two series), with a table of
zeros, and with max_norm C for every critic and A for every actor (0 or missing: not clipped), the variants interleaved within each
leg; with --baseline-lib PATH that library's population without a table as well, twice.  With --loop-steps N > 0 and not --no-loop,
then the K = 8 x 8192-env loop at 8 updates per step, without the option (this library and the baseline, alternating) and with it.
Usage: time_population.py [--legs 5] [--updates 1000] [--no-loop] [--loop-steps 60] [--n-step N [--ks 1,4,8] [--baseline-lib PATH]]
       time_population.py --grad-clip C[,A] [--ks 1,4,8] [--baseline-lib PATH] [--legs 3] [--no-loop] [--out FILE]
       time_population.py --td3 [DELAY] [--legs 3] [--updates 1000] [--per-graph 100] [--out profiles/population_td3_scaling.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ddpg_trucktrailer_amd import _lib as L  # noqa: E402
from ddpg_trucktrailer_amd.agent import Agent  # noqa: E402
from ddpg_trucktrailer_amd.fused_learn import FusedLearner  # noqa: E402
from ddpg_trucktrailer_amd.population import PopulationLearner, PopulationRollout  # noqa: E402
from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing  # noqa: E402
from ddpg_trucktrailer_amd.rollout import DDPGRollout  # noqa: E402
from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv  # noqa: E402

DEV = torch.device("cuda:0")
B = 256


def ring(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = TrajectoryRing(2048, 16, 23, DEV)
    r.obs.copy_(torch.rand(r.obs.shape, device=DEV, generator=g) * 2 - 1)
    r.act.copy_(torch.rand(r.act.shape, device=DEV, generator=g) * 2 - 1)
    r.rew.copy_(torch.rand(r.rew.shape, device=DEV, generator=g) * 10 - 5)
    r.done.copy_((torch.rand(r.done.shape, device=DEV, generator=g) < 0.05).to(torch.uint8))
    r.k = 15
    r.k_dev.fill_(15)
    return r


def agent(seed):
    torch.manual_seed(seed)
    return Agent(alpha=1e-4, beta=1e-3, input_dims=(23,), tau=1e-3, n_actions=1, batch_size=B, device=DEV, replay=False)


def captured(fn, per_graph):
    for _ in range(3):
        fn(0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for i in range(per_graph):
            fn(i % 8)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    return g


def timed(g, replays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3          # us


def nstep_cost(a):
    """--n-step: the variants of one K are timed back to back within a leg, their order alternating from leg to leg."""
    Ks, N = tuple(a.ks), a.n_step
    replays = max(1, -(-a.updates // a.per_graph))
    base = None
    if a.baseline_lib:
        base = C.CDLL(a.baseline_lib)
        for name in ("tt_pop_learn_create", "tt_pop_learn", "tt_pop_learn_destroy", "tt_last_error"):
            getattr(base, name).restype, getattr(base, name).argtypes = L._SIGNATURES[name]
    variants = [("one-step, no table", None, None), ("one-step, no table again", None, None), ("n = 1 through the table", [1], None),
                (f"n = {N}", [N], None)]
    if base is not None:       # (made alternately with this library's one-step populations: placement in memory is part of the spread)
        variants = [("baseline library", None, base), variants[0], ("baseline library again", None, base)] + variants[1:]
    pops = {}
    for K in Ks:
        for name, n_steps, lib in variants:
            pop = PopulationLearner([agent(100 + i) for i in range(K)], B, rings=[ring(200 + i) for i in range(K)],
                                    seeds=[300 + i for i in range(K)], n_steps=n_steps * K if n_steps else None)
            if lib is not None:
                pop.lib = lib              # (the descriptors are made at the first learn(): by this library)
            pops[K, name] = (pop, captured(pop.learn, a.per_graph))
    res = {key: [] for key in pops}
    for leg in range(a.legs):
        for K in (Ks if leg % 2 == 0 else Ks[::-1]):
            for name, _, _ in (variants if leg % 2 == 0 else variants[::-1]):
                res[K, name].append(timed(pops[K, name][1], replays) / (replays * a.per_graph))
    print(f"# learn() alone, B = {B}, {replays * a.per_graph} graph-replayed updates per leg, {a.legs} legs (variants interleaved, order "
          f"alternating), rings of 16 slots x 2048 envs, 5 % done flags")
    print(f"# device {torch.cuda.get_device_name(0)}")
    print(f"{'K':>3} {'variant':>26} {'us/pop update':>14} {'spread':>16} {'vs no table':>12}")
    for K in Ks:
        ref = statistics.median(res[K, "one-step, no table"])
        for name, _, lib in variants:
            pop, x = pops[K, name][0], res[K, name]
            assert pop.tail_gave_up() == [0] * K
            print(f"{K:3d} {name:>26} {statistics.median(x):14.2f} {min(x):7.2f}-{max(x):7.2f} {statistics.median(x) - ref:+12.2f}")
            if lib is not None:            # its handle has that library's layout: it goes the way it came
                torch.cuda.synchronize()
                lib.tt_pop_learn_destroy(pop._h)
                pop._h = None


def _clip_pair(text):
    from ddpg_trucktrailer_amd.grad_clip import clip_of_values
    parts = [float(x) for x in text.split(",")]
    if not 1 <= len(parts) <= 2:
        raise argparse.ArgumentTypeError(f"--grad-clip {text!r}: C or C,A")
    c, a = parts[0], parts[1] if len(parts) > 1 else 0.0
    if clip_of_values(c, a) is None:
        raise argparse.ArgumentTypeError(f"--grad-clip {text!r}: at least one value above 0")
    return c, a


def _other_library(path):
    base = C.CDLL(path)
    for name in ("tt_pop_learn_create", "tt_pop_learn", "tt_pop_learn_destroy", "tt_last_error"):
        getattr(base, name).restype, getattr(base, name).argtypes = L._SIGNATURES[name]
    return base


def clip_cost(a):
    """--grad-clip: the variants of one K are timed back to back within a leg, their order alternating from leg to leg."""
    from ddpg_trucktrailer_amd.grad_clip import clip_of_values
    Ks, clip = tuple(a.ks), clip_of_values(*a.grad_clip)
    replays = max(1, -(-a.updates // a.per_graph))
    base = _other_library(a.baseline_lib) if a.baseline_lib else None
    label = f"clip {a.grad_clip[0]:g}, {a.grad_clip[1]:g}"
    variants = [("no table", None, None), ("no table again", None, None), ("a table of zeros", "zeros", None), (label, clip, None)]
    if base is not None:       # (made alternately with this library's populations: placement in memory is part of the spread)
        variants = [("baseline library", None, base), variants[0], ("baseline library again", None, base)] + variants[1:]
    lines, pops = [], {}
    for K in Ks:
        for name, what, lib in variants:
            pop = PopulationLearner([agent(100 + i) for i in range(K)], B, rings=[ring(200 + i) for i in range(K)],
                                    seeds=[300 + i for i in range(K)], grad_clips=None if what in (None, "zeros") else what)
            if lib is not None:
                pop.lib = lib              # (the descriptors are made at the first learn(): by this library)
            if what == "zeros":            # (Python makes no table without a value: through the entry point)
                pop._create()
                pop._key = pop._storage_key()
                L.check(pop.lib.tt_pop_learn_set_clip(pop._h, (L.TTPopClip * K)()))
                pop.clip_table = True
            pops[K, name] = (pop, captured(pop.learn, a.per_graph))
    res = {key: [] for key in pops}
    for leg in range(a.legs):
        for K in (Ks if leg % 2 == 0 else Ks[::-1]):
            for name, _, _ in (variants if leg % 2 == 0 else variants[::-1]):
                res[K, name].append(timed(pops[K, name][1], replays) / (replays * a.per_graph))
    lines.append(f"# learn() alone, B = {B}, {replays * a.per_graph} graph-replayed updates per leg, {a.legs} legs (variants interleaved, "
                 f"order alternating), rings of 16 slots x 2048 envs, 5 % done flags")
    lines.append(f"# device {torch.cuda.get_device_name(0)}")
    lines.append(f"{'K':>3} {'variant':>24} {'us/pop update':>14} {'spread':>16} {'agent-updates/s':>16} {'vs no table':>12}  legs")
    for K in Ks:
        ref = statistics.median(res[K, "no table"])
        for name, what, lib in variants:
            pop, x = pops[K, name][0], res[K, name]
            assert pop.tail_gave_up() == [0] * K
            m = statistics.median(x)
            lines.append(f"{K:3d} {name:>24} {m:14.2f} {min(x):7.2f}-{max(x):7.2f} {K * 1e6 / m:16.3e} {m - ref:+12.2f}  " +
                         " ".join(f"{v:.2f}" for v in x))
            if what not in (None, "zeros"):
                st = pop.clip_stats(0)
                lines.append(f"#   agent 0: {st}")
            if lib is not None:            # its handle has that library's layout: it goes the way it came
                torch.cuda.synchronize()
                lib.tt_pop_learn_destroy(pop._h)
                pop._h = None
    if not a.no_loop and a.loop_steps > 0:
        lines.append("")
        lines.append(f"# the loop, K = 8 x n = 8192 envs, 8 updates per step, {a.loop_steps} graph-replayed vector steps after setup, per variant")
        loops = [("no table", None, None), (label, clip, None)]
        if base is not None:
            loops = [("baseline library", None, base), loops[0], ("baseline library again", None, base), ("no table again", None, None), loops[1]]
        for name, what, lib in loops:
            lp = PopulationRollout(8192, [11 + i for i in range(8)], batch_size=B, replay_slots=64, updates_per_step=8, graph_steps=20,
                                   grad_clip=what)
            if lib is not None:
                lp.learner.lib = lib
            lp.run(24)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lp.run(a.loop_steps)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / a.loop_steps
            lines.append(f"{name:>24} {dt * 1e3:8.3f} ms/step  {8 * 8192 / dt:10.3e} env-steps/s  {64 / dt:10.3e} agent-updates/s")
            if what is not None:
                lines.append(f"#   agent 0: {lp.clip_stats(0)}")
            if lib is not None:
                lp.invalidate_graphs()
                lib.tt_pop_learn_destroy(lp.learner._h)
                lp.learner._h = None
            del lp
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


def td3_scaling(a):
    """--td3: us per population update and agent-updates/s of TD3 populations, and the lone TD3Learner beside them."""
    from ddpg_trucktrailer_amd.td3 import PopulationTD3Learner, TD3Config, TD3Learner
    delay, Ks = a.td3, (1, 2, 4, 8, 16)
    assert a.per_graph % delay == 0, "whole delay periods per graph: the same share of full updates in every graph"
    cfg = TD3Config(policy_delay=delay)
    replays = max(1, -(-a.updates // a.per_graph))

    def td3_agent(seed):
        torch.manual_seed(seed)
        return Agent(alpha=1e-4, beta=1e-3, input_dims=(23,), tau=1e-3, n_actions=1, batch_size=B, device=DEV, replay=False, td3=cfg)
    made = {}
    for K in Ks:
        pop = PopulationTD3Learner([td3_agent(100 + i) for i in range(K)], B, [ring(200 + i) for i in range(K)],
                                   [300 + i for i in range(K)])
        made[K] = (pop, captured(lambda u, pop=pop: pop.learn(u, full=(u + 1) % delay == 0), a.per_graph))
    fl = TD3Learner(td3_agent(100), B, ring(200), 300)
    made["lone"] = (fl, captured(lambda u: fl.learn_batch(u=u, full=(u + 1) % delay == 0), a.per_graph))
    names = ("lone",) + Ks
    res = {k: [] for k in names}
    for leg in range(a.legs):
        for k in (names if leg % 2 == 0 else names[::-1]):
            res[k].append(timed(made[k][1], replays) / (replays * a.per_graph))
    for K in Ks:
        assert made[K][0].tail_gave_up() == [0] * K
    assert fl.tail_gave_up() == 0
    lines = [f"# TD3 learn() alone, B = {B}, policy_delay {delay}, {replays * a.per_graph} graph-replayed updates per leg ({a.per_graph} per "
             f"graph), {a.legs} legs (order alternating), rings of 16 slots x 2048 envs, 5 % done flags",
             f"# device {torch.cuda.get_device_name(0)}",
             f"{'K':>6} {'us/pop update':>14} {'max - min':>10} {'agent-updates/s':>16} {'vs K=1':>7}  legs"]
    base = statistics.median(res[1])
    for k in names:
        x, n = res[k], 1 if k == "lone" else k
        m = statistics.median(x)
        lines.append(f"{k!s:>6} {m:14.2f} {max(x) - min(x):10.2f} {n * 1e6 / m:16.3e} {(n / m) / (1 / base):7.2f}  "
                     + "  ".join(f"{v:.2f}" for v in x))
    lone = res["lone"]
    limit = statistics.median(lone) + (max(lone) - min(lone))
    lines.append(f"# K = 1 median {base:.2f} us against the lone TD3Learner's median + its legs' max - min = {limit:.2f} us: "
                 + ("within" if base <= limit else "NOT within"))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--updates", type=int, default=1000)
    ap.add_argument("--per-graph", type=int, default=100)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--loop-steps", type=int, default=60)
    ap.add_argument("--n-step", type=int, default=None)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--ks", type=lambda t: [int(x) for x in t.split(",")], default=[1, 4, 8], help="with --n-step: the K values")
    ap.add_argument("--td3", type=int, nargs="?", const=2, default=None, help="TD3 populations at this policy_delay (default 2)")
    ap.add_argument("--out", default=None, help="with --td3: also write the table to this file; with --grad-clip: append it")
    ap.add_argument("--grad-clip", type=_clip_pair, default=None, help="C[,A]: what per-agent gradient clipping costs")
    a = ap.parse_args()
    if a.td3 is not None:
        return td3_scaling(a)
    if a.grad_clip is not None:
        return clip_cost(a)
    if a.n_step is not None:
        return nstep_cost(a)
    Ks = (1, 2, 4, 8, 16)
    replays = max(1, -(-a.updates // a.per_graph))
    graphs = {}
    for K in Ks:
        pop = PopulationLearner([agent(100 + i) for i in range(K)], B, rings=[ring(200 + i) for i in range(K)],
                                seeds=[300 + i for i in range(K)])
        graphs[K] = (pop, captured(pop.learn, a.per_graph))
    fl = FusedLearner(agent(1), B)
    fl.fuse_tail = True
    lone_ring = ring(2)
    s, act, r, s2, d = lone_ring._batch_bufs(B)[:5]
    args = [lone_ring.sample_args(B, seed=7 + u) for u in range(8)]
    lone = captured(lambda u: fl.learn_batch(s, act, r, s2, d, sample=args[u]), a.per_graph)
    res = {K: [] for K in Ks}
    res["lone"] = []
    for leg in range(a.legs):
        order = list(Ks) if leg % 2 == 0 else list(reversed(Ks))
        for K in order:
            res[K].append(timed(graphs[K][1], replays) / (replays * a.per_graph))
        res["lone"].append(timed(lone, replays) / (replays * a.per_graph))
    for K, (pop, _) in graphs.items():
        assert pop.tail_gave_up() == [0] * K
    print(f"# learn() alone, B = {B}, {replays * a.per_graph} graph-replayed updates per leg, {a.legs} legs (K order alternating)")
    print(f"# device {torch.cuda.get_device_name(0)}")
    print(f"{'K':>6} {'us/pop update':>14} {'spread':>16} {'agent-updates/s':>16} {'vs K=1':>7}")
    base = statistics.median(res[1])
    for K in ("lone",) + Ks:
        m = statistics.median(res[K])
        k = 1 if K == "lone" else K
        print(f"{K!s:>6} {m:14.2f} {min(res[K]):7.2f}-{max(res[K]):7.2f} {k * 1e6 / m:16.3e} {(k / m) / (1 / base):7.2f}")
    if a.no_loop:
        return
    print()
    print(f"# the loop, {a.loop_steps} graph-replayed vector steps after setup")
    out = []
    for name in ("population K=8 x n=8192, 8 upd/step", "one agent N=65536, 64 upd/step"):
        if name.startswith("population"):
            lp = PopulationRollout(8192, [11 + i for i in range(8)], batch_size=B, replay_slots=64, updates_per_step=8, graph_steps=20)
            lp.run(24)
            envs, upd = 8 * 8192, 8 * 8
        else:
            env = TruckTrailerVecEnv(65536, device=DEV)
            env.reset(seed=27)
            lp = DDPGRollout(env, batch_size=B, replay_slots=64, seed=27, updates_per_step=64, graph_steps=20)
            lp.prepare()
            lp.first_launches()
            envs, upd = 65536, 64
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lp.run(a.loop_steps)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.loop_steps
        out.append((name, dt))
        print(f"{name:40s} {dt * 1e3:8.3f} ms/step  {envs / dt:10.3e} env-steps/s  {upd / dt:10.3e} agent-updates/s")


if __name__ == "__main__":
    main()
