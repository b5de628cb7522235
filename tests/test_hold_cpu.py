"""CPU: greedy evaluation with held lanes (include/ttenv.h: tt_env_set_hold .. tt_env_hold_read; evaluation.py; pbt.PBT.step's
`evaluation=`) as far as no GPU is needed:

* the new entry points refuse bad calls before any HIP call, each in its own name (handles and addresses are made up: a call
  that read one of them would crash here);
* Evaluator refuses lanes that are no multiple of 4, poses of another shape and a wrong number of actors;
* PBT.step(..., evaluation=None) makes the decisions the controller made before it took the argument (tests/golden/pbt_rounds.json,
  written by tests/golden/make_golden_pbt_rounds.py from that controller), draw for draw; with evaluation= the ranking is of the
  given records alone and the first pair's draws are those of a training-window round with the same scores;
* k_step_hold's two variants have no scratch and no vector spill, and the PER_ENV = false one reaches the waves per SIMD of
  k_step_log<false, false, false, false> in the same build."""
import ctypes as C
import importlib.util
import json
import math
import os

import pytest
import torch

from conftest import GOLDEN


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------- C ABI
FAKE = 0x1000      # never read: every call below is refused first


def _refused(lib, name, *args):
    dll = lib.load()
    rc = getattr(dll, name)(*args)
    msg = dll.tt_last_error(None).decode()
    assert rc == lib.TT_EINVAL and msg.startswith(name + ":"), (name, rc, msg)
    return msg


def test_entry_points_refuse_a_null_handle_in_their_own_name(lib):
    p = C.c_void_p
    assert "NULL handle" in _refused(lib, "tt_env_set_hold", None, 1, None)
    assert "NULL handle" in _refused(lib, "tt_env_hold_begin", None, None)
    assert "NULL handle" in _refused(lib, "tt_env_step_hold", None, p(FAKE), 1.0, p(FAKE), None)
    assert "NULL handle" in _refused(lib, "tt_env_hold_read", None, None, None, None, None, None, None, None)


def test_step_hold_refuses_null_arrays_and_a_non_finite_scale_before_it_reads_the_handle(lib):
    p = C.c_void_p
    h = p(FAKE)
    assert "mu and obs" in _refused(lib, "tt_env_step_hold", h, None, 1.0, p(FAKE), None)
    assert "mu and obs" in _refused(lib, "tt_env_step_hold", h, p(FAKE), 1.0, None, None)
    for bad in (math.nan, math.inf, -math.inf):
        assert "action_scale" in _refused(lib, "tt_env_step_hold", h, p(FAKE), bad, p(FAKE), None)
    # the order of the checks: the handle first, then the arrays, then the scale
    assert "NULL handle" in _refused(lib, "tt_env_step_hold", None, None, math.nan, None, None)
    assert "mu and obs" in _refused(lib, "tt_env_step_hold", h, None, math.nan, None, None)


def test_version_stays_three(lib):
    assert lib.load().tt_version() == 3


# ------------------------------------------------------------------------------------------------- Evaluator
def test_evaluator_refusals(lib):
    from ddpg_trucktrailer_amd.evaluation import Evaluator
    for lanes in (0, 1, 2, 6, 66, -4):
        with pytest.raises(ValueError, match="multiple of 4"):
            Evaluator(lanes)
    for shape in ((8,), (7, 3), (8, 2), (3, 8), (2, 8, 3)):
        with pytest.raises(ValueError, match=r"poses must be \[8,3\]"):
            Evaluator(8, poses=torch.zeros(shape))
    ev = Evaluator(8, agents=3, poses=torch.zeros((8, 3)))          # (no env yet: the first run() makes it)
    for actors in ([], [object()], [object()] * 2, [object()] * 4):
        with pytest.raises(ValueError, match="actors for 3 agents"):
            ev.run(actors)
    assert ev.env is None


def test_evaluator_draws_its_poses_once_from_the_reset_box_with_its_own_generator(lib):
    import numpy as np
    from ddpg_trucktrailer_amd.evaluation import Evaluator
    state = np.random.get_state()[1].copy()
    t = torch.random.get_rng_state().clone()
    a, b, c = Evaluator(12, agents=2, seed=5), Evaluator(12, agents=5, seed=5), Evaluator(12, seed=6)
    assert (np.random.get_state()[1] == state).all() and torch.equal(torch.random.get_rng_state(), t)
    assert a.poses.shape == (12, 3) and (a.poses == b.poses).all() and not (a.poses == c.poses).all()
    p = lib.default_params(0)
    for j in range(3):
        assert (a.poses[:, j] >= p.reset_lo[j]).all() and (a.poses[:, j] <= p.reset_hi[j]).all()


def test_summary_counts():
    from ddpg_trucktrailer_amd.evaluation import summary
    s = summary({"ret": torch.tensor([1.0, 3.0, -1.0], dtype=torch.float64), "success": torch.tensor([True, False, False]),
                 "flags": torch.tensor([0x48, 0x01, 0x05], dtype=torch.uint8), "len": torch.tensor([10, 20, 30], dtype=torch.int32)})
    assert s["episodes"] == 3 and s["mean_return"] == 1.0 and s["success_rate"] == pytest.approx(1 / 3) and s["mean_len"] == 20.0
    assert s["flags"] == {"jackknife": 2, "out_of_map": 0, "max_steps": 1, "goal_reached": 1, "goal_passed": 0, "excessive_back": 0,
                          "success_flag": 1}


# ------------------------------------------------------------------------------------------------- PBT
@pytest.fixture(scope="module")
def rounds():
    spec = importlib.util.spec_from_file_location("make_golden_pbt_rounds", os.path.join(GOLDEN, "make_golden_pbt_rounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pbt_step_without_an_evaluation_decides_as_before(rounds):
    from ddpg_trucktrailer_amd.pbt import PBT
    want = json.load(open(os.path.join(GOLDEN, "pbt_rounds.json")))
    assert sum(len(r) for r in want) >= 6 and any(not r for r in want)
    assert rounds.play(PBT, lambda p, pop, d: p.step(pop, d)) == want
    assert rounds.play(PBT, lambda p, pop, d: p.step(pop, d, None)) == want
    assert rounds.play(PBT, lambda p, pop, d: p.step(pop, d, evaluation=None)) == want


def _rec(rets, succ=None):
    rets = torch.tensor(rets, dtype=torch.float64)
    succ = torch.zeros(len(rets), dtype=torch.bool) if succ is None else torch.tensor(succ, dtype=torch.bool)
    return {"ret": rets, "success": succ}


HYP = {"alpha": 1e-4, "beta": 1e-3, "tau": 1e-3, "gamma": 0.99}


def test_pbt_ranks_on_the_evaluation_alone_with_the_draws_of_a_window_round():
    from ddpg_trucktrailer_amd.pbt import PBT
    K = 6
    hyp = [dict(HYP, n_step=3) for _ in range(K)]
    kw = dict(ready=10, seed=3, quantile=0.34, window=4, n_step_choices=(1, 3, 5))
    # the windows say agent a is worth 10 a; the evaluation says the opposite, with other episode counts
    windows = [_rec([10.0 * a] * 4) for a in range(K)]
    evaluation = [_rec([50.0 - 10.0 * a + d for d in (-1.0, 0.0, 1.0, 2.0, -2.0)]) for a in range(K)]
    p = PBT(K, **kw)
    p.observe(windows)
    d = p.decide(10, hyp, evaluation)
    assert [x["dst"] for x in d] == [5, 4] and all(x["src"] in (0, 1) for x in d)      # by the windows: dst 0, 1 from 5, 4
    assert d[0]["dst_score"] == (0.0,) and d[0]["src_score"] in ((50.0,), (40.0,))
    # a training-window round with the same scores: the first pair takes the same src, factors and n-step move
    q = PBT(K, **kw)
    q.observe([_rec([50.0 - 10.0 * a] * 4) for a in range(K)])
    w = q.decide(10, hyp)
    assert (d[0]["dst"], d[0]["src"], d[0]["new"]) == (w[0]["dst"], w[0]["src"], w[0]["new"])
    assert [(x["dst"], x["src"], x["new"]) for x in d] == [(x["dst"], x["src"], x["new"]) for x in w]
    # dst's window is cleared as in any round; the others' are untouched
    assert [len(x) for x in p.windows] == [4, 4, 4, 4, 0, 0]


def test_pbt_evaluation_eligibility_is_min_episodes_of_the_records_and_ignores_the_windows():
    from ddpg_trucktrailer_amd.pbt import PBT
    p = PBT(4, ready=1, window=8, min_episodes=3, metric="success")
    # no agent has a training episode; agents 0 and 3 have too few evaluation records
    ev = [_rec([9.0] * 2), _rec([1.0] * 3, [True, False, False]), _rec([5.0] * 3, [True, True, False]), _rec([])]
    assert p.evaluation_scores(ev) == [None, (1 / 3, 1.0), (2 / 3, 5.0), None]
    d = p.decide(1, [dict(HYP) for _ in range(4)], ev)
    assert [(x["dst"], x["src"]) for x in d] == [(1, 2)]
    assert p.decide(5, [dict(HYP) for _ in range(4)]) == []                  # the windows are still empty
    with pytest.raises(ValueError, match="evaluation records for 4 agents"):
        p.decide(9, [dict(HYP) for _ in range(4)], ev[:3])


# ------------------------------------------------------------------------------------------------- resources
def test_hold_kernels_keep_the_loop_kernels_occupancy(lib):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    ks = kr.kernels()
    hold = kr.find(ks, "11k_step_holdILb")
    assert len(hold) == 2, sorted(hold)
    for n, v in hold.items():
        assert v["scratch"] == 0 and v["vgpr_spills"] == 0, (n, v)
    (log,) = kr.find(ks, "10k_step_logILb0ELb0ELb0ELb0E").values()
    (plain,) = kr.find(ks, "11k_step_holdILb0E").values()
    assert kr.waves_per_simd(plain["vgpr"]) >= kr.waves_per_simd(log["vgpr"]) >= 4, (plain, log)
    for part in ("12k_hold_begin", "11k_hold_live", "11k_hold_read"):
        (v,) = kr.find(ks, part).values()
        assert v["scratch"] == 0 and v["vgpr_spills"] == 0, (part, v)
