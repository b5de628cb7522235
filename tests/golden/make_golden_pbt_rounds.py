"""Writes tests/golden/pbt_rounds.json: the decisions of pbt.PBT over a fixed sequence of synthetic drained records, recorded from
the controller as it stood BEFORE PBT.step took `evaluation=` (run with that pbt.py given as argv[1]; default: the package's).
tests/test_hold_cpu.py replays the sequence through PBT.step(..., evaluation=None) and compares decision for decision."""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
K, ROUNDS = 6, 8
CONFIG = dict(ready=10, seed=11, quantile=0.34, metric="success", window=8, min_episodes=4, n_step_choices=(1, 3, 5, 8))
HYP = {"alpha": 1e-4, "beta": 1e-3, "tau": 1e-3, "gamma": 0.99}


def records(r):
    """Round r's drained records: per agent 3 to 6 episodes with returns and successes from a generator keyed by (r, agent)."""
    out = []
    for a in range(K):
        g = np.random.RandomState(1000 * r + a)
        m = 3 + int(g.randint(4))
        out.append({"ret": [float(x) for x in g.normal(10.0 * ((a * 7 + r) % K), 25.0, m)], "success": [bool(x) for x in g.rand(m) < 0.3]})
    return out


class Pop:
    """What PBT.step reads of a PopulationRollout, with exploit() applied on the host."""

    class Ag:
        pass

    def __init__(self):
        self.agents = []
        for a in range(K):
            ag = Pop.Ag()
            for k, v in HYP.items():
                setattr(ag, k, v * (1.0 + 0.05 * a) if k != "gamma" else v)
            self.agents.append(ag)
        self.n_steps = [(1, 3, 5, 8)[a % 4] for a in range(K)]
        self.vector_steps = 0
        self.exploits = []

    def exploit(self, pairs):
        for dst, src, new in pairs:
            for k in HYP:
                setattr(self.agents[dst], k, new[k])
            self.n_steps[dst] = new["n_step"]
        self.exploits.append([(d, s) for d, s, _ in pairs])


def play(PBT, step):
    """The decisions of ROUNDS rounds; step(pbt, pop, drained) makes one."""
    pbt, pop, out = PBT(K, **CONFIG), Pop(), []
    for r in range(ROUNDS):
        pop.vector_steps += 10 if r % 3 else 7       # (a round is not always due)
        out.append(step(pbt, pop, records(r)))
    return json.loads(json.dumps(out))              # (tuples as lists, as the stored table has them)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        spec = importlib.util.spec_from_file_location("pbt_before", sys.argv[1])
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    else:
        sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
        from ddpg_trucktrailer_amd import pbt as mod
    table = play(mod.PBT, lambda p, pop, d: p.step(pop, d))
    assert sum(len(x) for x in table) >= 6, table
    json.dump(table, open(os.path.join(HERE, "pbt_rounds.json"), "w"), indent=1)
    print(sum(len(x) for x in table), "decisions in", len(table), "rounds")
