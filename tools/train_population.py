#!/usr/bin/env python3
"""GPU: tools/train_vector.py for a population of K agents (ddpg_trucktrailer_amd/population.py): one loop, K seeds, per agent a
progress line per block of vector steps from its own episode log and checkpoint.BestModelTracker (trainv2.py's 100-episode
average, success rate and "best" decisions; the best agent's networks are saved through agents[a].save_models()).  At the end one
training-state file per agent, with the keys of trainv2.py's save_training_state (training_states/<name>_training_state.pkl), so
the reference's multi_training_state_plotter.py overlays the K runs.  --objectives: the detailed episode log, and each agent's line
adds the 100-episode averages of viz_how_agent_learn.py's four objectives (episode_metrics.py).
Usage: train_population.py [--objectives] K n_envs_per_agent ring_slots updates_per_step batch vector_steps report_every [first_seed [graph_steps]]"""
import os
import pickle
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddpg_trucktrailer_amd.checkpoint import BestModelTracker  # noqa: E402
from ddpg_trucktrailer_amd.population import PopulationRollout  # noqa: E402

detail = "--objectives" in sys.argv[1:]
if detail:
    sys.argv.remove("--objectives")
    from ddpg_trucktrailer_amd.episode_metrics import RunningObjectives  # noqa: E402
K, n, slots, upd, batch, total, every = (int(x) for x in sys.argv[1:8])
seed0 = int(sys.argv[8]) if len(sys.argv) > 8 else 27
graph_steps = int(sys.argv[9]) if len(sys.argv) > 9 else 20
seeds = [seed0 + a for a in range(K)]
pop = PopulationRollout(n, seeds, batch_size=batch, replay_slots=slots, updates_per_step=upd, graph_steps=graph_steps,
                        episode_log=min(n * every, 1 << 24), episode_log_detail=detail)
print(f"K = {K} agents x N = {n} envs, ring {slots} steps, {upd} learn() per vector step = {n / upd:.1f} env-steps per update "
      f"per agent, batch {batch}, seeds {seeds}", flush=True)
for a, ag in enumerate(pop.agents):       # each agent saves its best networks into a directory of its own
    d = os.path.join("tmp", "ddpg", f"seed{seeds[a]}")
    os.makedirs(d, exist_ok=True)
    for net in ag._nets():
        net.checkpoint_dir, net.checkpoint_file = d, os.path.join(d, os.path.basename(net.checkpoint_file))
trackers = [BestModelTracker() for _ in range(K)]
running = [RunningObjectives() for _ in range(K)] if detail else None
episodes = [0] * K
t0 = time.time()
s = 0
while s < total:
    k = min(every, total - s)
    pop.run(k)
    s += k
    for a, r in enumerate(pop.drain_episodes()):
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
              f"{'BEST ' if best else ''}{objs}{lost}", flush=True)
        if best:
            pop.agents[a].save_models()
    print(f"  {time.time() - t0:8.1f} s, {s * n * K / max(1e-9, time.time() - t0):.3e} env-steps/s over the population", flush=True)

os.makedirs("training_states", exist_ok=True)
for a, tr in enumerate(trackers):
    name = f"population_seed{seeds[a]}"
    state = {"episode_num": episodes[a], "score_history": tr.score_history, "best_score": tr.best_score,
             "best_success_rate": tr.best_success_rate, "success_history": tr.success_history, "total_steps": tr.total_steps,
             "step_history": tr.step_history, "filename": name}
    with open(os.path.join("training_states", f"{name}_training_state.pkl"), "wb") as f:
        pickle.dump(state, f)
    print(f"training state of agent {a} -> training_states/{name}_training_state.pkl")
