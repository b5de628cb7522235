"""CPU: what the loops' options accept and refuse, pinned to the text.  tests/golden/loop_refusals.json is a table of calls -- the six
option values (TD3Config, LossShape, DemoLoss, MPCConfig, ExpertLanes, ExpertLabels), the check_* functions, the option blocks of
DDPGRollout, VectorStepper, PopulationRollout, PopulationLearner and FusedLearner, and the checkpoint refusals -- each with what it
gave: the exception's type and full message, or "ok" with the result's repr and, for an option value, its as_tuple() with the types.
tests/golden/make_golden_loop_refusals.py wrote it once from the commit before the options moved onto one base, one refusal table
and one resolve step (ddpg_trucktrailer_amd/options.py); the table is replayed here on the tree and compared exactly.  Calls that
fail two checks pin the order of the checks.

A case is {"call": "module.name", "args": [...], "kwargs": {...}} with optional "env" (environment variables set for the call),
"set" (attributes set on what the call returned) and "method" / "margs" (a method then called on it: the outcome is the method's).
An argument is a JSON value; a dict is one of {"float": "nan"}, {"tuple": [...]}, {"cpu_env": true} (tests/cpu_env.py), {"dict": {...}} (a plain dict) or
{"new": "module.name", "args": [...], "kwargs": {...}, "set": {attribute: value}} (an object, spoiled after construction by "set"),
{"the": "module.name"} (the named thing itself: "torch.uint8") or {"bare": "module.name", "set": {...}} (an object of that class made
without its constructor, with nothing but the attributes of "set").  A case may be {"bare": ..., "set": ..., "method": ...} instead of
a call: FusedLearner's setters and checks that raise before they touch the device are reached on a bare learner.
A module is one of the package's, or any importable one ("types.SimpleNamespace")."""
import importlib
import json
import os

import pytest

from conftest import GOLDEN
from cpu_env import CpuEnv

TABLE = os.path.join(GOLDEN, "loop_refusals.json")


def _resolve(name):
    module, attr = name.rsplit(".", 1)
    try:
        return getattr(importlib.import_module("ddpg_trucktrailer_amd." + module), attr)
    except ModuleNotFoundError:
        return getattr(importlib.import_module(module), attr)


def _arg(v):
    if isinstance(v, list):
        return [_arg(x) for x in v]
    if not isinstance(v, dict):
        return v
    if "float" in v:
        return float(v["float"])
    if "tuple" in v:
        return tuple(_arg(x) for x in v["tuple"])
    if "cpu_env" in v:
        return CpuEnv()
    if "dict" in v:
        return {k: _arg(x) for k, x in v["dict"].items()}
    if "the" in v:
        return _resolve(v["the"])
    if "bare" in v:
        obj = _resolve(v["bare"]).__new__(_resolve(v["bare"]))
    else:
        obj = _resolve(v["new"])(*_arg(v.get("args", [])), **{k: _arg(x) for k, x in v.get("kwargs", {}).items()})
    for k, x in v.get("set", {}).items():
        setattr(obj, k, _arg(x))
    return obj


def _typed(x):
    """as_tuple() with the types spelled out: (2, 0.2) -> ["tuple", [["int", 2], ["float", 0.2]]]."""
    if isinstance(x, tuple):
        return ["tuple", [_typed(v) for v in x]]
    return [type(x).__name__, x]


def outcome(case):
    """Makes the call of one table entry; returns what the table holds of it: ["ValueError", message], or ["ok", repr, as_tuple]."""
    saved = {k: os.environ.get(k) for k in case.get("env", {})}
    os.environ.update(case.get("env", {}))
    try:
        made = {"bare": case["bare"]} if "bare" in case else {"new": case["call"], "args": case.get("args", []), "kwargs": case.get("kwargs", {})}
        got = _arg(dict(made, set=case.get("set", {})))
        if "method" in case:
            got = getattr(got, case["method"])(*_arg(case.get("margs", [])))
    except Exception as exc:
        return [type(exc).__name__, str(exc)]
    finally:
        for k, v in saved.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    own_repr = type(got).__repr__ is not object.__repr__                  # (a loop has none: its type's name stands for it)
    return ["ok", repr(got) if own_repr else type(got).__name__, _typed(got.as_tuple()) if hasattr(got, "as_tuple") else None]


def test_every_case_of_the_table_keeps_its_outcome():
    table = json.load(open(TABLE))["cases"]
    assert len(table) >= 80
    wrong = []
    for case in table:
        got = outcome(case)
        if got != case["outcome"]:
            wrong.append(({k: v for k, v in case.items() if k != "outcome"}, got, case["outcome"]))
    assert not wrong, wrong
    assert sum("bare" in c for c in table) >= 40
    assert sum(c["outcome"][0] == "ok" for c in table) >= 15 and sum(c["outcome"][0] != "ok" for c in table) >= 60


# ------------------------------------------------------------------------------------------------- the checkpoint's option entries
def _loop(**kw):
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    return DDPGRollout(CpuEnv(), batch_size=4, replay_slots=8, use_graph=False, **kw)


def test_a_cpu_loops_state_dict_holds_the_options_under_their_keys():
    """The literal values are what the commit before the move wrote (and what its load_state_dict reads)."""
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    from ddpg_trucktrailer_amd.loss_shape import LossShape
    from ddpg_trucktrailer_amd.td3 import TD3Config
    sd = _loop(td3=TD3Config(), updates_per_step=2).state_dict()
    assert sd["format"] == 2 and sd["td3"] == [2, 0.2, 0.5] and [type(v) for v in sd["td3"]] == [int, float, float]
    assert not {"loss_shape", "demo_loss", "expert", "labels", "expert_plan"} & set(sd)
    _loop(td3=TD3Config(), updates_per_step=2).load_state_dict(sd)
    loop = _loop(loss_shape=LossShape(2, 0.5), demo_loss=DemoLoss(3, q_filter=0))
    sd = loop.state_dict()
    assert sd["format"] == 2 and sd["loss_shape"] == [2.0, 0.5] and sd["demo_loss"] == [3.0, False] and type(sd["demo_loss"][1]) is bool
    assert not {"td3", "expert", "labels", "expert_plan"} & set(sd)
    loop.load_state_dict(sd)
    assert _loop(loss_shape=LossShape()).state_dict()["loss_shape"] == [None, 0.0]
    assert not {"td3", "loss_shape", "demo_loss", "expert", "labels"} & set(_loop().state_dict())


def test_a_steppers_acting_state_holds_expert_and_labels_under_their_keys():
    """A CPU stepper refuses expert lanes and labels (not in ring mode), so the options are set on a built one: acting_state() and
    check_expert_state() read nothing else of them but the plan."""
    import torch
    from ddpg_trucktrailer_amd.mpc import ExpertLabels, ExpertLanes, MPCConfig
    from ddpg_trucktrailer_amd.stepper import VectorStepper
    mpc = MPCConfig(horizon=5, samples=65)
    st = VectorStepper(CpuEnv(), batch_size=4, replay_slots=8)
    st.expert, st.expert_plan = ExpertLanes(2, mpc, seed=7), torch.zeros((2, 5))
    sd = st.acting_state()
    want = [5, 65, 0.3, 0.8, 10.0, 1.0, 20.0, 300.0]
    assert sd["expert"] == [2, tuple(want), 7] and type(sd["expert"][1]) is tuple and "labels" not in sd
    assert tuple(sd["expert_plan"].shape) == (2, 5)
    st.check_expert_state(sd)
    st.check_expert_state(dict(sd, expert=[2, want, 7]))            # (a file that went through JSON: lists all the way down)
    st.labels, st.expert_plan = ExpertLabels(1, mpc, seed=7), torch.zeros((3, 5))
    sd = st.acting_state()
    assert sd["expert"] == [2, tuple(want), 7] and sd["labels"] == [1, tuple(want), 7] and tuple(sd["expert_plan"].shape) == (3, 5)
    st.check_expert_state(sd)
    st.expert = None
    sd = st.acting_state()
    assert "expert" not in sd and sd["labels"] == [1, tuple(want), 7] and "expert_plan" in sd


def test_every_option_value_comes_back_from_its_tuple_equal_and_hashable():
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    from ddpg_trucktrailer_amd.loss_shape import LossShape
    from ddpg_trucktrailer_amd.mpc import ExpertLabels, ExpertLanes, MPCConfig
    from ddpg_trucktrailer_amd.td3 import TD3Config
    mpc = MPCConfig(horizon=5, samples=65)
    for v in (TD3Config(4, 0.1, 0.3), LossShape(2, 0.5), LossShape(), DemoLoss(0.5, False), mpc, ExpertLanes(3, mpc, 7),
              ExpertLabels(2, mpc, 9)):
        back = type(v).from_tuple(v.as_tuple())
        assert back == v and back is not v and hash(back) == hash(v) and len({v, back}) == 1 and repr(back) == repr(v)
        assert type(v).from_tuple(json.loads(json.dumps(v.as_tuple()))) == v          # (lists, as a file holds them)
        assert v != v.as_tuple()
    assert ExpertLanes(3, mpc, 7) != ExpertLabels(3, mpc, 7) and isinstance(ExpertLanes.from_tuple((3, mpc.as_tuple(), 7)).mpc, MPCConfig)
