#!/usr/bin/env python3
"""GPU: tools/train_vector.py for a population of K agents (ddpg_trucktrailer_amd/population.py): one loop, K seeds, per agent a
progress line per block of vector steps from its own episode log and checkpoint.BestModelTracker (trainv2.py's 100-episode
average, success rate and "best" decisions; the best agent's networks are saved through agents[a].save_models()).  At the end one
training-state file per agent, with the keys of trainv2.py's save_training_state (training_states/<name>_training_state.pkl), so
the reference's multi_training_state_plotter.py overlays the K runs.  --objectives: the detailed episode log, and each agent's line
adds the 100-episode averages of viz_how_agent_learn.py's four objectives (episode_metrics.py).  --pbt READY: population-based
training (pbt.py) -- after each block, the records just drained go to the controller, which every READY vector steps lets the
bottom agents copy a top agent's networks and optimizer state and perturb its hyperparameters; one line per decision
(--pbt-quantile, default 0.25; --pbt-metric return | success, default return).  --n-step N[,N...]: n-step returns, one n for all
agents or one per agent; with --pbt, --pbt-n-steps a,b,c lets the controller move an agent's n among those choices.
--grad-clip C[,A][:C[,A]...]: per-agent gradient-norm clipping (PopulationRollout(grad_clip=)): max_norm C of
the critic and A of the actor (0 or missing: that network is not clipped), one entry for all agents or K entries separated by
colons; each agent's line then adds "clipped x of y" per network, the block's updates with a coefficient below 1.  With --pbt,
--pbt-clip LO,HI lets the controller multiply a copied clip by one of the two factors (PBT(clip_factors=)).  Not with --td3.
--learn-log EVERY: the learn log (PopulationRollout(learn_log=...)), one record per agent and EVERY updates; each agent's line adds
the latest record's critic loss, actor loss, Q mean, |TD| mean and both gradient norms, and the block's non-finite total.
--td3 [DELAY[,SIGMA[,CLIP]]]: a population of TD3 agents (PopulationRollout(td3=TD3Config(...)); defaults 2, 0.2, 0.5), with the
syntax of tools/train_vector.py: the token after --td3 is its value when it holds a comma; a lone DELAY is written --td3=DELAY.
updates_per_step must be a multiple of DELAY; not with --n-step > 1, --pbt-n-steps or --learn-log.  --pbt works unchanged.
--eval-every R --eval-lanes M: after every R-th report block a greedy evaluation (evaluation.Evaluator: no noise, the same M start
poses for every agent, drawn once from first_seed), one summary line per agent; --pbt-on-eval: the block's PBT round ranks on those
records instead of on the training episodes (PBT.step(..., evaluation=); with --pbt, whose window becomes M).
--checkpoint PATH [--save-every BLOCKS]: the whole run in one file (checkpoint.save_population_checkpoint: the population, the PBT
controller, each agent's BestModelTracker and episode count, the block counter and the vector step), written after every BLOCKS-th
report block and at the end of the run, each time over the previous file by a rename.  --resume PATH: continue such a run, bit for
bit, to the vector_steps given: the other positional arguments and the options must be the run's own (a population of another
shape is refused), --eval-every keeps its phase, and one line says from which vector step the run continues.  With --objectives
the 100-episode objective averages start empty after a resume (RunningObjectives is not in the file).
Usage: train_population.py [--objectives] [--n-step N[,N...]] [--learn-log EVERY] [--td3 [DELAY[,SIGMA[,CLIP]]]]
       [--grad-clip C[,A][:C[,A]...]] [--pbt READY [--pbt-quantile Q] [--pbt-metric M] [--pbt-n-steps a,b,c] [--pbt-clip LO,HI]] [--eval-every R --eval-lanes M [--pbt-on-eval]]
       [--checkpoint PATH [--save-every BLOCKS]] [--resume PATH]
       K n_envs_per_agent ring_slots updates_per_step batch vector_steps report_every [first_seed [graph_steps]]"""
import os
import pickle
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddpg_trucktrailer_amd.checkpoint import BestModelTracker, load_population_checkpoint, save_population_checkpoint  # noqa: E402
from ddpg_trucktrailer_amd.population import PopulationRollout  # noqa: E402

detail = "--objectives" in sys.argv[1:]
if detail:
    sys.argv.remove("--objectives")
    from ddpg_trucktrailer_amd.episode_metrics import RunningObjectives  # noqa: E402


def _option(name, cast, default=None):
    if name not in sys.argv[1:]:
        return default
    i = sys.argv.index(name)
    value = cast(sys.argv[i + 1])
    del sys.argv[i:i + 2]
    return value


pbt_ready = _option("--pbt", int)
pbt_quantile = _option("--pbt-quantile", float, 0.25)
pbt_metric = _option("--pbt-metric", str, "return")
_ints = lambda text: [int(x) for x in text.split(",")]
n_step = _option("--n-step", _ints, [1])
pbt_n_steps = _option("--pbt-n-steps", _ints)
learn_every = _option("--learn-log", int)


def _clips(text):
    from ddpg_trucktrailer_amd.grad_clip import clip_of_values
    out = []
    for entry in text.split(":"):
        parts = [float(x) for x in entry.split(",")]
        if not 1 <= len(parts) <= 2:
            sys.exit(f"--grad-clip {text!r}: an entry is C or C,A")
        out.append(clip_of_values(parts[0], parts[1] if len(parts) > 1 else 0.0))
    return out


grad_clip = _option("--grad-clip", _clips)
pbt_clip = _option("--pbt-clip", lambda text: tuple(float(x) for x in text.split(",")))
eval_every = _option("--eval-every", int)
eval_lanes = _option("--eval-lanes", int, 256)
checkpoint_path = _option("--checkpoint", str)
save_every = _option("--save-every", int)
resume_path = _option("--resume", str)
pbt_on_eval = "--pbt-on-eval" in sys.argv[1:]
if pbt_on_eval:
    sys.argv.remove("--pbt-on-eval")
td3 = None
for at, arg in enumerate(sys.argv):
    if at and (arg == "--td3" or arg.startswith("--td3=")):
        from ddpg_trucktrailer_amd.td3 import TD3Config  # noqa: E402
        spec = arg[6:] if arg.startswith("--td3=") else ""
        if arg == "--td3" and at + 1 < len(sys.argv) and "," in sys.argv[at + 1]:
            spec = sys.argv.pop(at + 1)
        del sys.argv[at]
        parts = [x for x in spec.split(",") if x]
        td3 = TD3Config(*([int(parts[0])] + [float(x) for x in parts[1:3]])) if parts else TD3Config()
        break
if pbt_n_steps is not None and pbt_ready is None:
    sys.exit("--pbt-n-steps needs --pbt")
if pbt_clip is not None and (pbt_ready is None or grad_clip is None):
    sys.exit("--pbt-clip needs --pbt and --grad-clip")
if pbt_on_eval and (pbt_ready is None or eval_every is None):
    sys.exit("--pbt-on-eval needs --pbt and --eval-every")
if save_every is not None and (checkpoint_path is None or save_every < 1):
    sys.exit("--save-every BLOCKS (>= 1) needs --checkpoint")
K, n, slots, upd, batch, total, every = (int(x) for x in sys.argv[1:8])
seed0 = int(sys.argv[8]) if len(sys.argv) > 8 else 27
graph_steps = int(sys.argv[9]) if len(sys.argv) > 9 else 20
seeds = [seed0 + a for a in range(K)]
nstep_kw = {}
if n_step != [1] or pbt_n_steps is not None:
    nstep_kw["n_step"] = n_step * K if len(n_step) == 1 else n_step      # (a list: the population keeps an n-step table)
    if pbt_n_steps is not None:
        nstep_kw["n_step_max"] = max(pbt_n_steps + n_step)
if grad_clip is not None:
    if len(grad_clip) not in (1, K):
        sys.exit(f"--grad-clip: one entry for all agents or {K}, not {len(grad_clip)}")
    nstep_kw["grad_clip"] = grad_clip * K if len(grad_clip) == 1 else grad_clip
pop = PopulationRollout(n, seeds, batch_size=batch, replay_slots=slots, updates_per_step=upd, graph_steps=graph_steps,
                        episode_log=min(n * every, 1 << 24), episode_log_detail=detail,
                        # the log holds a report block's records: one per learn_every updates
                        learn_log=None if learn_every is None else min(max(1, upd * every // learn_every + 1), 1 << 22),
                        learn_log_every=learn_every or 1, td3=td3, **nstep_kw)
print(f"K = {K} agents x N = {n} envs, ring {slots} steps, {upd} learn() per vector step = {n / upd:.1f} env-steps per update "
      f"per agent, batch {batch}, seeds {seeds}, n_step {pop.n_steps}" + (f", {td3}" if td3 is not None else "")
      + (f", max_norm [critic, actor] {pop.grad_clips}" if pop.clip_table else ""), flush=True)
for a, ag in enumerate(pop.agents):       # each agent saves its best networks into a directory of its own
    d = os.path.join("tmp", "ddpg", f"seed{seeds[a]}")
    os.makedirs(d, exist_ok=True)
    for net in ag._nets():
        net.checkpoint_dir, net.checkpoint_file = d, os.path.join(d, os.path.basename(net.checkpoint_file))


def learn_line(rec):
    """The latest record of a drained learn log and the block's non-finite total, for a report line."""
    if not len(rec["step"]):
        return "  learn log: no record"
    bad = int(rec["nonfinite"].sum())
    return (f"  update {int(rec['step'][-1])}: critic loss {rec['critic_loss'][-1]:.4g}  actor loss {rec['actor_loss'][-1]:.4g}  "
            f"Q mean {rec['q_mean'][-1]:.4g}  |TD| mean {rec['td_abs_mean'][-1]:.4g}  |grad| critic {rec['grad_norm_critic'][-1]:.4g} "
            f"actor {rec['grad_norm_actor'][-1]:.4g}  non-finite {bad}" + (f"  ({rec['dropped']} records overwritten)" if rec["dropped"] else ""))


clip_seen = [{"critic": (0, 0), "actor": (0, 0)} for _ in range(K)]


def clip_line(a):
    """Agent a's clipped updates of the block per network, from the device's counts (they start again with a resumed handle)."""
    st, parts = pop.clip_stats(a), []
    for key in ("critic", "actor"):
        now = (st[key]["clipped"], st[key]["updates"])
        was = clip_seen[a][key] if clip_seen[a][key][1] <= now[1] else (0, 0)
        clip_seen[a][key] = now
        parts.append(f"{key} clipped {now[0] - was[0]} of {now[1] - was[1]} (max_norm {pop.grad_clips[a][key == 'actor']:.4g}, "
                     f"last |grad| {st[key]['norm']:.4g})")
    return "  " + "  ".join(parts)


trackers = [BestModelTracker() for _ in range(K)]
pbt = None
if pbt_ready is not None:
    from ddpg_trucktrailer_amd.pbt import PBT  # noqa: E402
    # (ranked on evaluations: all of an evaluation's M records count, whatever an agent's training window holds)
    pbt = PBT(K, pbt_ready, seed=seed0, quantile=pbt_quantile, metric=pbt_metric, n_step_choices=pbt_n_steps, clip_factors=pbt_clip,
              **(dict(window=eval_lanes) if pbt_on_eval else {}))
    print(f"PBT: a round every {pbt_ready} vector steps, bottom/top quantile {pbt_quantile}, ranked by {pbt_metric} over the "
          f"last {pbt.window} episodes since an agent's last exploit"
          + (f", n_step explored among {list(pbt.n_step_choices)}" if pbt_n_steps is not None else "")
          + (f", a copied clip times one of {list(pbt.clip_factors)}" if pbt_clip is not None else ""), flush=True)
running = [RunningObjectives() for _ in range(K)] if detail else None
evaluator = None
if eval_every is not None:
    from ddpg_trucktrailer_amd.evaluation import Evaluator, summary  # noqa: E402
    evaluator = Evaluator(eval_lanes, agents=K, seed=seed0, device=pop.device)
    print(f"evaluation: every {eval_every} blocks, {eval_lanes} start poses shared by the {K} agents"
          + (", PBT ranks on it" if pbt_on_eval else ""), flush=True)
blocks = 0
episodes = [0] * K
s = 0


def save_checkpoint():
    state = {"blocks": blocks, "vector_steps": s, "episodes": list(episodes), "trackers": [tr.state_dict() for tr in trackers]}
    save_population_checkpoint(checkpoint_path, pop, pbt, state)


if resume_path is not None:
    state = load_population_checkpoint(resume_path, pop, pbt)
    blocks, s, episodes = int(state["blocks"]), int(state["vector_steps"]), [int(x) for x in state["episodes"]]
    for tr, sd in zip(trackers, state["trackers"]):
        tr.load_state_dict(sd)
    print(f"resumed from {resume_path}: continuing from vector step {s} (block {blocks}), n_step {pop.n_steps}", flush=True)
t0, s0 = time.time(), s
while s < total:
    k = min(every, total - s)
    pop.run(k)
    s += k
    drained = pop.drain_episodes()
    learned = pop.drain_learn_log() if learn_every is not None else None
    for a, r in enumerate(drained):
        m = len(r["ret"])
        best, avg, rate = trackers[a].update_many(r, episodes[a])
        episodes[a] += m
        e = max(1, m)
        lost = f"  ({r['dropped']} records past the log's capacity)" if r["dropped"] else ""
        objs = ""
        if detail:                 # viz_how_agent_learn.py's objectives, 100-episode averages
            running[a].update(r)
            objs = "  " + "  ".join(f"{k[:4]}100 {v if v is not None else float('nan'):8.1f}" for k, v in running[a].last().items())
        print(f"agent {a} seed {seeds[a]}  vector steps {s:7d} ({s * n:.2e} env-steps): episodes {m:7d}  "
              f"mean return {r['ret'].sum().item() / e:9.1f}  successes {int(r['success'].sum().item()):6d}  "
              f"avg100 {avg if avg is not None else float('nan'):9.1f}  success100 {rate if rate is not None else float('nan'):5.2f}  "
              f"{'BEST ' if best else ''}{objs}{lost}{learn_line(learned[a]) if learned is not None else ''}"
              f"{clip_line(a) if pop.clip_table and pop.learner.has_handle else ''}", flush=True)
        if best:
            pop.agents[a].save_models()
    blocks += 1
    evaluation = None
    if evaluator is not None and blocks % eval_every == 0:
        evaluation = pop.evaluate(evaluator)
        for a, r in enumerate(evaluation):
            e = summary(r)
            ends = "  ".join(f"{k} {v}" for k, v in e["flags"].items() if v)
            print(f"evaluation  agent {a} seed {seeds[a]}  vector steps {s:7d}: mean return {e['mean_return']:9.1f}  success rate "
                  f"{e['success_rate']:5.2f}  mean length {e['mean_len']:6.1f}  {ends}  ({evaluator.steps_run} steps)", flush=True)
    if pbt is not None and pbt_on_eval and evaluation is None:
        pbt.observe(drained)           # (no round without an evaluation to rank on)
    elif pbt is not None:
        for d in pbt.step(pop, drained, evaluation if pbt_on_eval else None):
            hyp = "  ".join(f"{k} {d['old'][k]:.4g} -> {d['new'][k]:.4g}" for k in d["new"])
            print(f"PBT step {d['step']}: agent {d['dst']} (score {d['dst_score'][0]:.1f}) <- agent {d['src']} "
                  f"(score {d['src_score'][0]:.1f}): {hyp}", flush=True)
    print(f"  {time.time() - t0:8.1f} s, {(s - s0) * n * K / max(1e-9, time.time() - t0):.3e} env-steps/s over the population", flush=True)
    if save_every is not None and blocks % save_every == 0 and s < total:
        save_checkpoint()
if checkpoint_path is not None:
    save_checkpoint()
    print(f"checkpoint -> {checkpoint_path} (vector step {s})", flush=True)

os.makedirs("training_states", exist_ok=True)
for a, tr in enumerate(trackers):
    name = f"population_seed{seeds[a]}"
    state = {"episode_num": episodes[a], "score_history": tr.score_history, "best_score": tr.best_score,
             "best_success_rate": tr.best_success_rate, "success_history": tr.success_history, "total_steps": tr.total_steps,
             "step_history": tr.step_history, "filename": name}
    with open(os.path.join("training_states", f"{name}_training_state.pkl"), "wb") as f:
        pickle.dump(state, f)
    print(f"training state of agent {a} -> training_states/{name}_training_state.pkl")
