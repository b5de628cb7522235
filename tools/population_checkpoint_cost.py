#!/usr/bin/env python3
"""GPU: what a whole-population checkpoint costs (checkpoint.save_population_checkpoint / load_population_checkpoint; DESIGN.md
section 21): the file's size and the seconds of one save and of one load into the same population, after a few steps.
Usage: population_checkpoint_cost.py [K [n_envs_per_agent [ring_slots [directory]]]]   (defaults 16, 4096, 64, the temporary one)"""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from ddpg_trucktrailer_amd.checkpoint import load_population_checkpoint, save_population_checkpoint  # noqa: E402
from ddpg_trucktrailer_amd.pbt import PBT  # noqa: E402
from ddpg_trucktrailer_amd.population import PopulationRollout  # noqa: E402

given = [int(x) for x in sys.argv[1:4]]
K, n, slots = given + [16, 4096, 64][len(given):]
where = sys.argv[4] if len(sys.argv) > 4 else tempfile.gettempdir()
pop = PopulationRollout(n, list(range(27, 27 + K)), replay_slots=slots, updates_per_step=2, graph_steps=4, episode_log=1 << 16)
pbt = PBT(K, 20)
pop.run(12)
torch.cuda.synchronize()
path = os.path.join(where, f"population_checkpoint_cost_{os.getpid()}.pt")
try:
    t0 = time.perf_counter()
    save_population_checkpoint(path, pop, pbt)
    t1 = time.perf_counter()
    size = os.path.getsize(path)
    load_population_checkpoint(path, pop, pbt)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
finally:
    if os.path.exists(path):
        os.remove(path)
pop.run(5)                             # (the loaded population goes on: the handle was made again, the graphs are captured again)
torch.cuda.synchronize()
print(f"K = {K} x {n} lanes x {slots} slots: file {size} bytes ({size / 2 ** 20:.1f} MiB), save {t1 - t0:.2f} s, load {t2 - t1:.2f} s")
