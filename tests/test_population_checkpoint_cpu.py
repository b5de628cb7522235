"""CPU: whole-population checkpoints as far as no GPU is needed -- the PBT controller's state through the
file and torch.load(weights_only=True), every refusal of population.check_population_state, the atomic write of
checkpoint.save_population_checkpoint, and checkpoint.BestModelTracker's round trip."""
import copy
import os

import pytest
import torch

HYP = {"alpha": 1e-4, "beta": 1e-3, "tau": 1e-3, "gamma": 0.99}


class _Pop:
    """What the checkpoint layer asks of a population: state_dict() and load_state_dict()."""

    def __init__(self, sd=None):
        self.sd, self.loaded = sd or {"format": 1, "marker": 7}, None

    def state_dict(self):
        return self.sd

    def load_state_dict(self, sd):
        self.loaded = sd


def _rec(gen, m=3):
    return {"ret": (torch.rand(m, generator=gen, dtype=torch.float64) * 100), "success": torch.rand(m, generator=gen) < 0.3}


def test_pbt_state_goes_through_the_file_and_weights_only(tmp_path):
    """A controller with non-empty windows, history and a moved RandomState, saved by save_population_checkpoint's PBT path, read
    with weights_only=True into a controller built with another seed: the next rounds' decisions -- their draws of src and of
    every factor -- are the original's, decision for decision."""
    from ddpg_trucktrailer_amd.checkpoint import load_population_checkpoint, save_population_checkpoint
    from ddpg_trucktrailer_amd.pbt import PBT
    gen = torch.Generator().manual_seed(3)
    K = 6
    hypers = [dict(HYP) for _ in range(K)]
    batches = [[_rec(gen) for _ in range(K)] for _ in range(12)]
    kw = dict(window=5, metric="success", quantile=0.34, n_step_choices=(1, 3, 5))
    for h in hypers:
        h["n_step"] = 3
    a = PBT(K, 2, seed=9, **kw)
    for i in range(6):
        a.observe(batches[i])
        a.decide(2 * (i + 1), hypers)
    assert a.history and any(len(w) for w in a.windows)
    path = str(tmp_path / "pop.pt")
    save_population_checkpoint(path, _Pop(), pbt=a, training_state={"blocks": 6})
    raw = torch.load(path, map_location="cpu", weights_only=True)        # (the loader checkpoint.py uses everywhere)
    assert raw["pbt"]["rng"]["keys"].dtype == torch.uint32 and raw["pbt"]["rng"]["kind"] == "MT19937"
    b, pop = PBT(K, 2, seed=123, **kw), _Pop()
    assert load_population_checkpoint(path, pop, b) == {"blocks": 6} and pop.loaded == {"format": 1, "marker": 7}
    assert b.history == a.history and [list(w) for w in b.windows] == [list(w) for w in a.windows] and b.last_round == a.last_round
    out_a, out_b = [], []
    for i in range(6, 12):
        for p, out in ((a, out_a), (b, out_b)):
            p.observe(batches[i])
            out.append(p.decide(2 * (i + 1), hypers))
    assert any(out_a) and out_a == out_b and a.history == b.history
    assert a.rng.randint(1 << 30) == b.rng.randint(1 << 30)


def test_a_controller_needs_pbt_state_in_the_file_and_the_reverse_is_allowed(tmp_path):
    from ddpg_trucktrailer_amd.checkpoint import load_population_checkpoint, save_population_checkpoint
    from ddpg_trucktrailer_amd.pbt import PBT
    without, with_pbt = str(tmp_path / "a.pt"), str(tmp_path / "b.pt")
    save_population_checkpoint(without, _Pop())
    save_population_checkpoint(with_pbt, _Pop(), pbt=PBT(2, 5))
    pop = _Pop()
    with pytest.raises(ValueError, match="no PBT state"):
        load_population_checkpoint(without, pop, PBT(2, 5))
    assert pop.loaded is None                              # (refused before anything is loaded)
    assert load_population_checkpoint(with_pbt, pop) == {} and pop.loaded is not None


def _agent_state(td3=None, n_step=1, slots=8, lanes=64, batch=16):
    st = {"format": 2, "seed": 1, "vector_steps": 3, "handover_gave_up": [], "batch_size": batch, "updates_per_step": 2,
          "n_step": n_step, "nets": {}, "ring": {"k": 3, "slots": slots, "n": lanes, "side_count": 0, "obs": torch.zeros(1)},
          "ou": torch.zeros(lanes), "env": None, "fused_adam": {}, "hyper": dict(HYP)}
    if td3 is not None:
        st["td3"] = list(td3)
        st["hyper"].update(target_noise=td3[1], noise_clip=td3[2])
    return st


def _state(K=3, td3=None, **kw):
    return {"format": 1, "K": K, "n": 64, "batch_size": 16, "updates_per_step": 2, "vector_steps": 3, "seeds": list(range(K)),
            "n_step_table": False, "n_step_max": 1, "policy_delay": None if td3 is None else td3[0],
            "agents": [_agent_state(td3, **kw) for _ in range(K)]}


MINE = dict(K=3, lanes=64, slots=8, batch_size=16)


def test_a_matching_state_passes_and_returns_the_n_steps():
    from ddpg_trucktrailer_amd.population import check_population_state
    assert check_population_state(_state(), **MINE) == [1, 1, 1]
    sd = _state()
    sd["agents"][1]["n_step"] = 3
    assert check_population_state(sd, **MINE, n_step_max=3, n_step_table=True) == [1, 3, 1]
    assert check_population_state(_state(td3=(2, 0.2, 0.5)), **MINE, policy_delay=2) == [1, 1, 1]


@pytest.mark.parametrize("name, change, mine, words", [
    ("K", lambda sd: sd.update(K=4, agents=sd["agents"] + [copy.deepcopy(sd["agents"][0])]), {}, "K: the checkpoint holds 4 agents"),
    ("lanes", lambda sd: sd.update(n=128), {}, "n_envs_per_agent: the checkpoint was written with 128 lanes"),
    ("ring lanes", lambda sd: sd["agents"][2]["ring"].update(n=128), {}, "n_envs_per_agent: agent 2's ring was written with 128 lanes"),
    ("slots", lambda sd: sd["agents"][1]["ring"].update(slots=16), {}, "replay_slots: agent 1's ring was written with 16 slots"),
    ("batch", lambda sd: sd.update(batch_size=32), {}, "batch_size: the checkpoint was written with 32"),
    ("agent batch", lambda sd: sd["agents"][0].update(batch_size=32), {}, "batch_size: agent 0's state was written with 32"),
    ("td3 in file", None, {}, "td3: the checkpoint was written with td3, this population has none"),
    ("td3 in population", lambda sd: None, {"policy_delay": 2}, "td3: the checkpoint was written without td3"),
    ("policy_delay", None, {"policy_delay": 1}, "policy_delay: the checkpoint was written with 2, this population has 1"),
    ("n above n_step_max", lambda sd: sd["agents"][1].update(n_step=4), {"n_step_max": 3, "n_step_table": True},
     "n_step: agent 1 was saved with n_step = 4, above this population's n_step_max = 3"),
    ("n without the table", lambda sd: sd["agents"][2].update(n_step=2), {"n_step_max": 3},
     "n_step: agent 2 was saved with n_step = 2, but this population was built without n-step returns"),
    ("format", lambda sd: sd.update(format=9), {}, "format: the checkpoint has format 9"),
    ("agent format", lambda sd: sd["agents"][0].update(format=1), {}, "format: agent 0's state has format 1"),
    ("no ring contents", lambda sd: sd["agents"][0]["ring"].pop("obs"), {}, "ring: agent 0's ring was written without its contents"),
    ("no hyper", lambda sd: sd["agents"][1].pop("hyper"), {}, "hyper: agent 1's state lacks"),
])
def test_every_refusal_names_what_differs(name, change, mine, words):
    from ddpg_trucktrailer_amd.population import check_population_state
    sd = _state(td3=(2, 0.2, 0.5)) if change is None else _state()
    if change is not None:
        change(sd)
    with pytest.raises(ValueError) as e:
        check_population_state(sd, **dict(MINE, **mine))
    assert words in str(e.value), str(e.value)


def test_updates_per_step_must_be_a_multiple_of_the_delay():
    from ddpg_trucktrailer_amd.population import check_population_state
    sd = _state(td3=(2, 0.2, 0.5))
    sd["updates_per_step"] = 3
    with pytest.raises(ValueError, match="updates_per_step: the checkpoint's 3 is not a multiple of policy_delay = 2"):
        check_population_state(sd, **MINE, policy_delay=2)
    sd["updates_per_step"] = 4                             # (otherwise it follows the file)
    assert check_population_state(sd, **MINE, policy_delay=2) == [1, 1, 1]


def test_a_failed_write_keeps_the_previous_file_and_leaves_no_temporary(tmp_path, monkeypatch):
    from ddpg_trucktrailer_amd.checkpoint import save_population_checkpoint
    path = str(tmp_path / "pop.pt")
    save_population_checkpoint(path, _Pop({"format": 1, "marker": 1}))
    before = open(path, "rb").read()
    real = torch.save

    def dies_midway(obj, f, *a, **kw):
        with open(f, "wb") as out:                         # (half a file under the name it was given, then the failure)
            out.write(b"half")
        raise OSError("disk full")
    monkeypatch.setattr(torch, "save", dies_midway)
    with pytest.raises(OSError, match="disk full"):
        save_population_checkpoint(path, _Pop({"format": 1, "marker": 2}))
    monkeypatch.setattr(torch, "save", real)
    assert open(path, "rb").read() == before and os.listdir(tmp_path) == ["pop.pt"]
    assert torch.load(path, weights_only=True)["population"]["marker"] == 1
    save_population_checkpoint(path, _Pop({"format": 1, "marker": 2}))
    assert torch.load(path, weights_only=True)["population"]["marker"] == 2 and os.listdir(tmp_path) == ["pop.pt"]


def test_best_model_tracker_round_trip(tmp_path):
    """A tracker saved after 150 episodes and loaded into a fresh one, through a weights_only file: both make the same decisions
    and averages on the next 60."""
    from ddpg_trucktrailer_amd.checkpoint import BestModelTracker
    gen = torch.Generator().manual_seed(5)
    eps = [(float(torch.rand((), generator=gen)) * 100, bool(torch.rand((), generator=gen) < 0.3), int(torch.randint(1, 300, (), generator=gen)))
           for _ in range(210)]
    a = BestModelTracker()
    fired = [a.update(i, *e)[0] for i, e in enumerate(eps[:150])]
    assert any(fired)
    path = str(tmp_path / "t.pt")
    torch.save({"training_state": {"trackers": [a.state_dict()]}}, path)
    b = BestModelTracker(start_episode=99, best_score=1e9)
    b.load_state_dict(torch.load(path, weights_only=True)["training_state"]["trackers"][0])
    assert b.state_dict() == a.state_dict()
    for i, e in enumerate(eps[150:], 150):
        assert a.update(i, *e) == b.update(i, *e)
    assert b.training_state(210) == a.training_state(210)
