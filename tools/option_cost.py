"""What the option-cost tools share (grad_clip_cost.py, loss_shape_cost.py, demo_cost.py, expert_lanes_cost.py, expert_labels_cost.py,
curriculum_cost.py, randomize_cost.py, task_curriculum_cost.py and success_replay_cost.py, which set N and UPD from their own arguments): the configuration, a leg, the fresh child process per leg, the alternation of the variants and the report with
the gate of DESIGN.md section 13 -- the loop without the option costs at most the parent's median plus the parent legs' own
max - min.  A tool keeps its arguments and how it forwards them to a leg, the keyword arguments of its loops and its variants' names."""
import argparse
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, UPD, B, SLOTS, GRAPH_STEPS = 4096, 64, 256, 64, 4
PARENT = "the parent commit's loop"


def parse(own, **leg):
    """The tools' command line: `own`, the tool's [(flag, add_argument's keywords)], among the shared ones; `leg`: what --leg accepts."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=60)
    for flag, kw in own:
        ap.add_argument(flag, **kw)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, **leg)
    ap.add_argument("--tree", default=None)
    return ap.parse_args()


def one_leg(a, options, prepare=None, stats=None):
    """One leg in this process: the loop of --tree (else this tree) with the keyword arguments options() returns (called once the tree
    is importable), prepare(loop) before the warm-up, stats(loop) appended to the line in front of "LEG <ms per vector step>"."""
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else HERE)
    import torch
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    kw = options()
    env = TruckTrailerVecEnv(N)
    env.reset(seed=27)
    loop = DDPGRollout(env, batch_size=B, replay_slots=SLOTS, seed=27, updates_per_step=UPD, graph_steps=GRAPH_STEPS, **kw)
    if prepare:
        prepare(loop)
    loop.run(a.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.run(a.steps)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    assert loop.graph_steps == GRAPH_STEPS and loop.handover_gave_up == [] and loop.learner.tail_gave_up() == 0
    assert all(torch.isfinite(p).all() for p in loop.agent.actor.parameters())
    print(f"pipeline={loop.pipeline} fuse_tail={loop.learner.fuse_tail} updates={int(loop.learner.step_dev.item())}" +
          (stats(loop) if stats else ""))
    print(f"LEG {ms:.5f}")


def run_leg(a, script, variant, forward, echo=None, said=None):
    """One leg of `variant` in a fresh process ("parent": the off leg of --parent-tree); a failed or hung leg ends the tool.  The
    leg's lines that start with `echo` are printed (and the last of them kept in said[variant], where `said` is given)."""
    cmd = [sys.executable, os.path.abspath(script), "--leg", "off" if variant == "parent" else variant, "--steps", str(a.steps),
           "--warmup", str(a.warmup)] + forward
    if variant == "parent":
        cmd += ["--tree", a.parent_tree]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout
    for ln in out.splitlines():
        if echo and ln.startswith(echo):
            print("      " + ln, flush=True)
            if said is not None:
                said[variant] = ln
    return float([ln for ln in out.splitlines() if ln.startswith("LEG ")][-1].split()[1])


def report(res, names, width, steps, warmup, legs, records=False, between=()):
    """The report's lines from res = {variant: [ms per vector step of each leg]} (its order is the report's): the header, a line per
    variant, `on - off` (records: a line per variant with the option, in per cent of off) and the gate, evaluated where res has
    "parent".  between: pairs (a, b) of variants whose medians' difference a - b is a record line of its own, behind `on - off`."""
    names = {"parent": PARENT, **names}
    lines = [f"# DDPGRollout, N = {N}, {UPD} updates per vector step, B = {B}, ring of {SLOTS} slots, whole-step graphs of {GRAPH_STEPS}; "
             f"{steps} timed vector steps per leg after {warmup}, every leg a fresh process, {legs} legs, variants alternating"]
    for v, x in res.items():
        lines.append(f"{names[v]:>{width}}: " + "  ".join(f"leg {i} {t:8.5f}" for i, t in enumerate(x)) +
                     f"  | median {statistics.median(x):8.5f} ms per vector step, max - min {max(x) - min(x):7.5f}")
    off = statistics.median(res["off"])
    spread = max(res["off"]) - min(res["off"])
    for v in (v for v in res if v not in ("off", "parent")):
        on = statistics.median(res[v])
        if records:
            lines.append(f"# {v} - off = {1e3 * (on - off):+.2f} us per vector step ({100 * (on - off) / off:+.2f} %); the off legs' own max - min is "
                         f"{1e3 * spread:.2f} us per vector step (a record, not a gate)")
        else:
            lines.append(f"# {v} - off = {1e3 * (on - off):+.2f} us per vector step = {1e3 * (on - off) / UPD:+.3f} us per update; the off legs' own max - min "
                         f"is {1e3 * spread:.2f} us per vector step: " + ("within it" if on - off <= spread else "beyond it"))
    for a, b in between:
        lines.append(f"# {a} - {b} = {1e3 * (statistics.median(res[a]) - statistics.median(res[b])):+.2f} us per vector step (a record, not a gate)")
    if "parent" in res:
        p = res["parent"]
        limit = statistics.median(p) + (max(p) - min(p))
        lines.append(f"# gate: off median {off:.5f} ms against the parent's median + its legs' max - min = {limit:.5f} ms: "
                     + ("within" if off <= limit else "NOT within"))
    else:
        lines.append("# no --parent-tree: the gate against the parent commit was not evaluated")
    return lines


def compare(a, script, variants, forward, names, width, records=False, echo=None, between=()):
    """The tool without --leg: `a.legs` rounds of every variant (with --parent-tree "parent" too: last, or first for a tool whose
    report is `records`), alternating within a round and in their order from round to round; the report (`between`: report()'s) is
    printed and written to --out, and so is the last of each variant's echoed lines."""
    if a.parent_tree:
        variants = ["parent"] + variants if records else variants + ["parent"]
    res = {v: [] for v in variants}
    said = {}
    for leg in range(a.legs):
        for v in (variants if leg % 2 == 0 else variants[::-1]):
            res[v].append(run_leg(a, script, v, forward, echo, said))
            print(f"round {leg} {v:>{9 if records else 6}}: {res[v][-1]:.5f} ms per vector step", flush=True)
    lines = report(res, names, width, a.steps, a.warmup, a.legs, records, between)
    lines += [f"# the last {v} leg: {ln}" for v, ln in said.items()]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
