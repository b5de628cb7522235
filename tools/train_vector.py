#!/usr/bin/env python3
"""GPU: training behaviour of the N-env loop at a chosen data/update ratio: per block of vector steps, the mean return
and length of the episodes that ended in it and how many succeeded, read from the env step kernel's episode log (f64
returns, the reference's success test final_success_bonus > 0: trainv2.py:541), with trainv2.py's 100-episode average,
success rate and "best" decisions (checkpoint.BestModelTracker).  The loop runs whole-step graphs of `graph_steps`.
--objectives: the detailed episode log, and each line adds the 100-episode averages of viz_how_agent_learn.py's four objectives
(efficiency, smoothness, precision, safety; episode_metrics.py).
--n-step N: n-step returns in the replay draw (DDPGRollout(n_step=N); default 1, the one-step target).
--learn-log EVERY: the fused learner's learn log (DDPGRollout(learn_log=...)), one record per EVERY updates, and each line adds
the latest record's critic loss, actor loss, Q mean, |TD| mean and both gradient norms, and the block's non-finite total.
--td3 [DELAY[,SIGMA[,CLIP]]]: TD3 instead of DDPG (DDPGRollout(td3=TD3Config(...)); defaults 2, 0.2, 0.5): twin critics, target-policy
smoothing, the actor and the targets updated every DELAY-th update.  The token after --td3 is its value when it holds a comma; a
lone DELAY is written --td3=DELAY.  updates_per_step must be a multiple of DELAY; not with --n-step > 1 or --learn-log.
--huber D / --pre-penalty C: the loss shape (DDPGRollout(loss_shape=LossShape(D, C))): a Huber critic loss
with delta D (torch's definition: half the MSE gradient inside the zone) and / or the penalty C mean(pre^2) on the actor head's
pre-activation.  Not with --td3.
--demos FILE.npz --bc-weight L [--no-q-filter]: the demonstration loss (DDPGRollout(demo_loss=DemoLoss(L, q_filter)); DESIGN.md section
25): FILE holds obs, act, rew, obs2, done (expert.save_transitions_npz) and goes into the ring's side buffer; the batch rows drawn
from it get the behaviour-cloning term L (mu - a)^2, by default only where Q(s, a) > Q(s, mu(s)).  Each line adds the demonstration
rows of the block's last update, how many the filter let through and the term's value.  Not with --td3 or --n-step > 1.
--expert-lanes M [--expert-horizon H] [--expert-samples S] [--expert-seed K]: expert lanes (DDPGRollout(expert=ExpertLanes(M,
MPCConfig(horizon=H, samples=S), seed=K)); defaults H = 64, S = 256, K = the loop's seed): lanes [0, M) of the env
are driven by the sampling MPC expert inside the captured step.  With --bc-weight L (no --demos needed) the ring rows of those lanes
are demonstration rows.  Each line then splits the block's finished episodes and successes into lanes < M (the expert's) and lanes >= M
(the policy's), from the episode log's lane field, so that the expert's successes are not read as the policy's.
--label-lanes L: expert labels (DDPGRollout(labels=ExpertLabels(L, ...)); needs --bc-weight): the L lanes behind the
expert's are driven by the POLICY, and the expert's decision on each of their states goes to the ring's label array -- the cloning term
follows the label on their ring rows, unfiltered.  Takes the expert's --expert-horizon, --expert-samples and --expert-seed (with
--expert-lanes both use the same: one launch plans for both).  Each line then shows demonstration / labelled / applied rows of the block's
last update, and the successes split into the policy's lanes and the others.
--grad-clip C[,A]: gradient-norm clipping (DDPGRollout(grad_clip=GradClip(C, A))): clip_grad_norm_ with max_norm C
in front of the critic's optimizer step and, when given, A in front of the actor's ("-" for C: the actor alone).  Each line adds
"clipped x of y critic / actor updates", the block's share from FusedLearner.clip_stats().  Not with --td3, --bc-weight or the expert options.
--curriculum NX,NY,NYAW[,EVERY[,MODE]]: the start-pose curriculum (DDPGRollout(curriculum=Curriculum((NX, NY, NYAW), every=EVERY,
mode=MODE)); defaults EVERY = 64, MODE = frontier): resets drawn by the success rate of the cell they start in,
counted and drawn inside the env step.  Each line adds the share of cells seen, the mean p and the weight share of the top decile of
cells.  Composes with every learner option; not with the expert options or --objectives.
--randomize-L2 LO,HI and / or --randomize-goal X0,X1,Y0,Y1,YAW0,YAW1: episode randomisation (DDPGRollout(randomize=
EpisodeRandomization(goal=((X0, Y0, YAW0), (X1, Y1, YAW1)), L2=(LO, HI)))): every episode's trailer length and / or
goal is drawn from the range at the lane's reset, inside the env step.  Each line adds the min / mean / max of the lanes' current L2 and
goal.  Composes with every learner option; not with --curriculum, the expert options or --objectives.
--task-curriculum NGX,NGY,NGYAW,NL2[,EVERY[,MODE]]: the task curriculum (DDPGRollout(task_curriculum=TaskCurriculum((NGX, NGY, NGYAW, NL2),
every=EVERY, mode=MODE)); needs a --randomize-*; defaults EVERY = 64, MODE = frontier): the episode's goal and
trailer length drawn by the success rate of the cell of the randomised ranges they lie in, counted and drawn inside the env step.  Each
line adds the share of cells seen, the mean p, the weight share of the top decile of cells and the success rate per L2 bin; the other
dimensions' tables follow on lines of their own.
--success-replay CAP[,EVERY[,TAIL]]: success replay (DDPGRollout(success_replay=SuccessReplay(CAP, every=EVERY, tail=TAIL)); DESIGN.md
section 41; defaults EVERY = 32, TAIL = 0 = whole episodes): every EVERY vector steps the transitions of the episodes that ended in
success are copied from the ring into a region of CAP rows of its side buffer; they are drawn with the ring's transitions and, with
--bc-weight L (no --demos needed), cloned behind the Q-filter.  Each line adds the episodes and rows harvested,
the rows in the draw, the rows cut off episodes longer than the ring's window and the episodes that expired before a harvest.  Not with
--td3, --n-step > 1, the expert options or --demos (the loop makes the region when it makes the ring, and a file's rows go in front).
--bc-weight L --no-demos runs the demonstration launches on an empty side buffer: the other run of a pair.
--eval-every R --eval-lanes M: after every R-th report block a greedy evaluation of the actor (evaluation.Evaluator: no noise, M start
poses drawn once from the seed), one summary line; the networks are saved (Agent.save_models) whenever an evaluation is the best so
far by (success rate, mean return).
Usage: train_vector.py [--objectives] [--n-step N] [--learn-log EVERY] [--td3 [DELAY[,SIGMA[,CLIP]]]] [--huber D] [--pre-penalty C]
       [--demos FILE.npz --bc-weight L [--no-q-filter]] [--expert-lanes M] [--label-lanes L] [--expert-horizon H] [--expert-samples S]
       [--expert-seed K] [--grad-clip C[,A]] [--curriculum NX,NY,NYAW[,EVERY[,MODE]]]
       [--randomize-L2 LO,HI] [--randomize-goal X0,X1,Y0,Y1,YAW0,YAW1] [--task-curriculum NGX,NGY,NGYAW,NL2[,EVERY[,MODE]]]
       [--success-replay CAP[,EVERY[,TAIL]]] [--no-demos] [--eval-every R --eval-lanes M] n_envs ring_slots updates_per_step batch vector_steps report_every [seed [graph_steps]]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddpg_trucktrailer_amd.checkpoint import BestModelTracker
from ddpg_trucktrailer_amd.rollout import DDPGRollout
from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv

detail = "--objectives" in sys.argv[1:]
if detail:
    sys.argv.remove("--objectives")
    from ddpg_trucktrailer_amd.episode_metrics import RunningObjectives
    running = RunningObjectives()
n_step = 1
if "--n-step" in sys.argv[1:]:
    at = sys.argv.index("--n-step")
    n_step = int(sys.argv[at + 1])
    del sys.argv[at:at + 2]
learn_every = None
if "--learn-log" in sys.argv[1:]:
    at = sys.argv.index("--learn-log")
    learn_every = int(sys.argv[at + 1])
    del sys.argv[at:at + 2]
huber, pre_penalty = None, 0.0
if "--huber" in sys.argv[1:]:
    at = sys.argv.index("--huber")
    huber = float(sys.argv[at + 1])
    del sys.argv[at:at + 2]
if "--pre-penalty" in sys.argv[1:]:
    at = sys.argv.index("--pre-penalty")
    pre_penalty = float(sys.argv[at + 1])
    del sys.argv[at:at + 2]
demos, bc_weight, q_filter = None, None, True
if "--demos" in sys.argv[1:]:
    at = sys.argv.index("--demos")
    demos = sys.argv[at + 1]
    del sys.argv[at:at + 2]
if "--bc-weight" in sys.argv[1:]:
    at = sys.argv.index("--bc-weight")
    bc_weight = float(sys.argv[at + 1])
    del sys.argv[at:at + 2]
if "--no-q-filter" in sys.argv[1:]:
    sys.argv.remove("--no-q-filter")
    q_filter = False
success_replay = None
if "--success-replay" in sys.argv[1:]:
    from ddpg_trucktrailer_amd.success_replay import SuccessReplay, summary as success_replay_summary
    at = sys.argv.index("--success-replay")
    success_replay = SuccessReplay(*(int(x) for x in sys.argv[at + 1].split(",")))
    del sys.argv[at:at + 2]
    if demos is not None:
        sys.exit("--success-replay with --demos is not supported by this tool: the loop makes the region with its ring")
expert_opt = {}
label_lanes = None
if "--label-lanes" in sys.argv[1:]:
    at = sys.argv.index("--label-lanes")
    label_lanes = int(sys.argv[at + 1])
    del sys.argv[at:at + 2]
for flag in ("--expert-lanes", "--expert-horizon", "--expert-samples", "--expert-seed"):
    if flag in sys.argv[1:]:
        at = sys.argv.index(flag)
        expert_opt[flag[9:]] = int(sys.argv[at + 1])
        del sys.argv[at:at + 2]
if expert_opt and "lanes" not in expert_opt and label_lanes is None:
    sys.exit("--expert-horizon / --expert-samples / --expert-seed need --expert-lanes M or --label-lanes L")
if label_lanes is not None and bc_weight is None:
    sys.exit("--label-lanes L needs --bc-weight L: labels without a learner that reads them do nothing")
if demos is not None and bc_weight is None:
    sys.exit("--demos FILE.npz needs --bc-weight L")
no_demos = "--no-demos" in sys.argv[1:]      # the demonstration launches on an empty side buffer: the baseline of a --success-replay pair
if no_demos:
    sys.argv.remove("--no-demos")
if bc_weight is not None and demos is None and not expert_opt and label_lanes is None and success_replay is None and not no_demos:
    sys.exit("--bc-weight L needs demonstrations: --demos FILE.npz, --expert-lanes M, --label-lanes L or --success-replay CAP "
             "(--no-demos: run its launches without any)")
demo_loss = None
if bc_weight is not None:
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    demo_loss = DemoLoss(bc_weight, q_filter)
eval_every, eval_lanes = None, 256
if "--eval-every" in sys.argv[1:]:
    at = sys.argv.index("--eval-every")
    eval_every = int(sys.argv[at + 1])
    del sys.argv[at:at + 2]
if "--eval-lanes" in sys.argv[1:]:
    at = sys.argv.index("--eval-lanes")
    eval_lanes = int(sys.argv[at + 1])
    del sys.argv[at:at + 2]
grad_clip = None
if "--grad-clip" in sys.argv[1:]:
    from ddpg_trucktrailer_amd.grad_clip import GradClip
    at = sys.argv.index("--grad-clip")
    grad_clip = GradClip(*[None if x in ("", "-") else float(x) for x in sys.argv[at + 1].split(",")])
    del sys.argv[at:at + 2]
curriculum = None
if "--curriculum" in sys.argv[1:]:
    from ddpg_trucktrailer_amd.curriculum import Curriculum, summary as curriculum_summary
    at = sys.argv.index("--curriculum")
    parts = sys.argv[at + 1].split(",")
    curriculum = Curriculum(tuple(int(x) for x in parts[:3]), **({"every": int(parts[3])} if len(parts) > 3 else {}),
                            **({"mode": parts[4]} if len(parts) > 4 else {}))
    del sys.argv[at:at + 2]
randomize, rnd_goal, rnd_L2 = None, None, None
if "--randomize-L2" in sys.argv[1:]:
    at = sys.argv.index("--randomize-L2")
    rnd_L2 = tuple(float(x) for x in sys.argv[at + 1].split(","))
    del sys.argv[at:at + 2]
if "--randomize-goal" in sys.argv[1:]:
    at = sys.argv.index("--randomize-goal")
    x0, x1, y0, y1, yaw0, yaw1 = (float(x) for x in sys.argv[at + 1].split(","))
    rnd_goal = ((x0, y0, yaw0), (x1, y1, yaw1))
    del sys.argv[at:at + 2]
if rnd_goal is not None or rnd_L2 is not None:
    from ddpg_trucktrailer_amd.randomize import EpisodeRandomization, summary as randomize_summary
    randomize = EpisodeRandomization(goal=rnd_goal, L2=rnd_L2)
task_curriculum = None
if "--task-curriculum" in sys.argv[1:]:
    from ddpg_trucktrailer_amd.task_curriculum import TaskCurriculum, task_summary
    at = sys.argv.index("--task-curriculum")
    parts = sys.argv[at + 1].split(",")
    if randomize is None:
        sys.exit("--task-curriculum needs --randomize-L2 LO,HI and / or --randomize-goal ...: there is no range to put cells on")
    task_curriculum = TaskCurriculum(tuple(int(x) for x in parts[:4]), **({"every": int(parts[4])} if len(parts) > 4 else {}),
                                     **({"mode": parts[5]} if len(parts) > 5 else {}))
    del sys.argv[at:at + 2]
loss_shape = None
if huber is not None or pre_penalty:
    from ddpg_trucktrailer_amd.loss_shape import LossShape
    loss_shape = LossShape(huber, pre_penalty)
td3 = None
for at, arg in enumerate(sys.argv):
    if at and (arg == "--td3" or arg.startswith("--td3=")):
        from ddpg_trucktrailer_amd.td3 import TD3Config
        spec = arg[6:] if arg.startswith("--td3=") else ""
        if arg == "--td3" and at + 1 < len(sys.argv) and "," in sys.argv[at + 1]:
            spec = sys.argv.pop(at + 1)
        del sys.argv[at]
        parts = [x for x in spec.split(",") if x]
        td3 = TD3Config(*([int(parts[0])] + [float(x) for x in parts[1:3]])) if parts else TD3Config()
        break
n, slots, upd, batch, total, every = (int(x) for x in sys.argv[1:7])
seed = int(sys.argv[7]) if len(sys.argv) > 7 else 27
expert, labels = None, None
if expert_opt or label_lanes is not None:
    from ddpg_trucktrailer_amd.mpc import ExpertLabels, ExpertLanes, MPCConfig
    # horizon 64: what the planner's record supports from the env's own reset poses
    mpc_cfg = MPCConfig(horizon=expert_opt.get("horizon", 64), samples=expert_opt.get("samples", 256))
    if "lanes" in expert_opt:
        expert = ExpertLanes(expert_opt["lanes"], mpc_cfg, seed=expert_opt.get("seed", seed))
    if label_lanes is not None:
        labels = ExpertLabels(label_lanes, mpc_cfg, seed=expert_opt.get("seed", seed))
graph_steps = int(sys.argv[8]) if len(sys.argv) > 8 else (20 if slots <= 1024 else 0)      # (as before: no graphs past 1024 slots)
env = TruckTrailerVecEnv(n)
env.reset(seed=seed)
# the log holds a report block's episodes: at most one per env and step
loop = DDPGRollout(env, batch_size=batch, replay_slots=slots, seed=seed, updates_per_step=upd, graph_steps=graph_steps,
                   episode_log=min(n * every, 1 << 24), episode_log_detail=detail, n_step=n_step,
                   # the log holds a report block's records: one per learn_every updates
                   learn_log=None if learn_every is None else min(max(1, upd * every // learn_every + 1), 1 << 22),
                   learn_log_every=learn_every or 1, td3=td3, loss_shape=loss_shape, demo_loss=demo_loss, expert=expert, labels=labels,
                   grad_clip=grad_clip, curriculum=curriculum, randomize=randomize, task_curriculum=task_curriculum,
                   success_replay=success_replay)
if demos is not None:
    from ddpg_trucktrailer_amd.expert import load_transitions_npz
    d_obs, d_act, d_rew, d_obs2, d_done = load_transitions_npz(demos)
    loop.ring.load_side(d_obs, d_act[:, 0], d_rew, d_obs2, d_done)
print(f"N = {n}, ring {slots} steps ({slots * n:.2e} transitions), {upd} learn() per vector step = {n / upd:.1f} env-steps per update, "
      f"batch {batch}, pipeline={loop.pipeline}, graph_steps={loop.graph_steps}, n_step={loop.n_step}" + (f", {td3}" if td3 is not None else "") +
      (f", {loss_shape}" if loss_shape is not None else "") + (f", {grad_clip}" if grad_clip is not None else "") +
      (f", {demo_loss} on {loop.ring.side_count} demonstrations" if demo_loss is not None else "") +
      (f", {expert}" if expert is not None else "") + (f", {labels}" if labels is not None else "") +
      (f", {curriculum}" if curriculum is not None else "") + (f", {randomize}" if randomize is not None else "") +
      (f", {task_curriculum}" if task_curriculum is not None else "") +
      (f", {success_replay}" if success_replay is not None else ""), flush=True)


def learn_line(rec):
    """The latest record of a drained learn log and the block's non-finite total, for a report line."""
    if not len(rec["step"]):
        return "  learn log: no record"
    bad = int(rec["nonfinite"].sum())
    return (f"  update {int(rec['step'][-1])}: critic loss {rec['critic_loss'][-1]:.4g}  actor loss {rec['actor_loss'][-1]:.4g}  "
            f"Q mean {rec['q_mean'][-1]:.4g}  |TD| mean {rec['td_abs_mean'][-1]:.4g}  |grad| critic {rec['grad_norm_critic'][-1]:.4g} "
            f"actor {rec['grad_norm_actor'][-1]:.4g}  non-finite {bad}" + (f"  ({rec['dropped']} records overwritten)" if rec["dropped"] else ""))


clip_seen = {}


def clip_line(stats):
    """The block's clipped share per clipped network, from the learner's running counts."""
    parts = []
    for key, st in stats.items():
        updates0, clipped0 = clip_seen.get(key, (0, 0))
        parts.append(f"{st['clipped'] - clipped0} of {st['updates'] - updates0} {key}")
        clip_seen[key] = (st["updates"], st["clipped"])
    return "  clipped " + " / ".join(parts) + " updates"


def curriculum_line(st):
    return f"  curriculum: cells seen {100 * st['cells_seen']:5.1f} %, mean p {st['mean_p']:.3f}, top-decile weight {100 * st['top_decile_weight']:4.1f} %"


def randomize_line(st):
    spans = "  ".join(f"{k} {st[k][0]:.3f} / {st[k][1]:.3f} / {st[k][2]:.3f}" for k in ("L2", "goal_x", "goal_y", "goal_yaw"))
    return (f"  randomize: goal {st['goal_lo']} .. {st['goal_hi']}, L2 {st['L2_lo']} .. {st['L2_hi']}; lanes now (min / mean / max) "
            + spans)


def _bins(table):
    return " ".join(f"[{lo:.3g}, {hi:.3g}) {'-' if rate is None else f'{rate:.2f}'} ({seen})" for lo, hi, seen, rate in table)


def task_line(st):
    """The task curriculum's summary; the success rate per bin (episodes seen) of L2 on the line, of the goal's dimensions behind it."""
    head = (f"  task curriculum: cells seen {100 * st['cells_seen']:5.1f} %, mean p {st['mean_p']:.3f}, top-decile weight "
            f"{100 * st['top_decile_weight']:4.1f} %, success by L2: {_bins(st['by_L2'])}")
    return head + "".join(f"\n    success by {k}: {_bins(st['by_' + k])}" for k in ("goal_x", "goal_y", "goal_yaw") if len(st["by_" + k]) > 1)


def demo_line(st):
    lab = f", {st['labelled']} labelled" if "labelled" in st else ""
    return f"  demonstrations {st['demo_rows']} rows{lab}, {st['applied']} applied, bc loss {st['bc_loss']:.4g}"


def lanes_line(r, m_lanes, l_lanes=0):
    """The block's finished episodes and successes by lane group: the expert's lanes [0, M) and the policy's.  With labels the groups
    carry their lane ranges, the expert's group is left out when there is none, and the policy's lanes [M, M + L) that the expert
    labels are shown on their own as well."""
    ex = r["lane"] < m_lanes
    ok = r["success"]
    if not l_lanes:
        return (f"  expert lanes: episodes {int(ex.sum().item())} successes {int((ok & ex).sum().item())}"
                f"  policy lanes: episodes {int((~ex).sum().item())} successes {int((ok & ~ex).sum().item())}")
    lab = ~ex & (r["lane"] < m_lanes + l_lanes)
    out = f"  expert lanes [0, {m_lanes}): episodes {int(ex.sum().item())} successes {int((ok & ex).sum().item())}" if m_lanes else ""
    return (out + f"  policy lanes [{m_lanes}, {n}): episodes {int((~ex).sum().item())} successes {int((ok & ~ex).sum().item())}"
            f"  of them labelled lanes [{m_lanes}, {m_lanes + l_lanes}): episodes {int(lab.sum().item())} successes {int((ok & lab).sum().item())}")


tracker = BestModelTracker()
evaluator, best_eval, blocks = None, None, 0
if eval_every is not None:
    from ddpg_trucktrailer_amd.evaluation import Evaluator, summary
    evaluator = Evaluator(eval_lanes, seed=seed, device=env.device)
episodes = 0
t0 = time.time()
s = 0
while s < total:
    k = min(every, total - s)
    loop.run(k)
    s += k
    r = loop.drain_episodes()
    m = len(r["ret"])
    best, avg, rate = tracker.update_many(r, episodes)
    episodes += m
    e = max(1, m)
    lost = f"  ({r['dropped']} records past the log's capacity)" if r["dropped"] else ""
    objs = ""
    if detail:                 # viz_how_agent_learn.py's objectives, 100-episode averages
        running.update(r)
        objs = "  " + "  ".join(f"{k[:4]}100 {v if v is not None else float('nan'):8.1f}" for k, v in running.last().items())
    print(f"vector steps {s:7d} ({s * n:.2e} env-steps, {int(loop.learner.step_dev.item())} updates): episodes {m:7d}  "
          f"mean length {r['len'].double().sum().item() / e:6.1f}  mean return {r['ret'].sum().item() / e:9.1f}  "
          f"successes {int(r['success'].sum().item()):6d} ({100 * r['success'].double().sum().item() / e:4.1f} %)  "
          f"avg100 {avg if avg is not None else float('nan'):9.1f}  success100 {rate if rate is not None else float('nan'):5.2f}  "
          f"best x{len(best)}{objs}{lost}{learn_line(loop.drain_learn_log()) if learn_every is not None else ''}"
          f"{demo_line(loop.demo_stats()) if demo_loss is not None else ''}"
          f"{clip_line(loop.learner.clip_stats()) if grad_clip is not None else ''}"
          f"{curriculum_line(curriculum_summary(env.curriculum_state())) if curriculum is not None else ''}"
          f"{randomize_line(randomize_summary(env.randomization_ranges(), env.episode())) if randomize is not None else ''}"
          f"{task_line(task_summary(env.task_curriculum_state(), env.randomization_ranges())) if task_curriculum is not None else ''}"
          f"{'  ' + success_replay_summary(loop.success_replay_stats()) if success_replay is not None else ''}"
          f"{lanes_line(r, expert.lanes if expert is not None else 0, labels.lanes if labels is not None else 0) if expert is not None or labels is not None else ''}  "
          f"{time.time() - t0:.0f}s", flush=True)
    blocks += 1
    if evaluator is not None and blocks % eval_every == 0:
        e = summary(loop.evaluate(evaluator))
        key = (e["success_rate"], e["mean_return"])
        is_best = best_eval is None or key > best_eval
        if is_best:
            best_eval = key
            loop.agent.save_models()
        ends = "  ".join(f"{k} {v}" for k, v in e["flags"].items() if v)
        print(f"evaluation  vector steps {s:7d}: {eval_lanes} episodes  mean return {e['mean_return']:9.1f}  success rate "
              f"{e['success_rate']:5.2f}  mean length {e['mean_len']:6.1f}  {ends}  ({evaluator.steps_run} steps)"
              f"{'  BEST: networks saved' if is_best else ''}", flush=True)
