"""CPU: episode randomisation without a GPU (ddpg_trucktrailer_amd/randomize.py; include/ttenv.h: tt_env_set_randomization;
csrc/ttenv_randomize.h: k_step_rnd, k_step_rnd_log, k_reset_rnd).

* EpisodeRandomization's validation, its tuple round trip, its repr and its checkpoint key;
* every row of its part of the refusal table, word for word and in order, and the loops refusing through the table;
* a plain loop's state_dict() has no "randomize" entry;
* the host model (tests/randomize_ref.py) against its own statement: values inside [lo, hi], a zero width gives lo exactly, and the
  task's words (third counter word 1) share no word with the start pose's (0) for the same (seed, env, episode);
* the new kernels' resources, read from the built library: no scratch, no vector or scalar spill, the observation tile's LDS, and every
  variant at no fewer waves per SIMD than k_step_log<PER_ENV = true, INFO, AUTO_RESET = true, RANDOM_POLICY> (the variant that, like
  the new kernels, carries a reset piece); every kernel of the golden tables keeps its row;
* the header, the exports and the ctypes table agree, and bad arguments are TT_EINVAL with a message before the handle is read."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import randomize_ref as ref
from conftest import GOLDEN, ROOT

GOAL = ((-10.0, -32.0, 1.3), (10.0, -28.0, 1.8))
L2 = (5.0, 10.0)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------------------- the option
def test_randomization_validates_its_fields():
    from ddpg_trucktrailer_amd.randomize import EpisodeRandomization as R
    r = R(goal=GOAL, L2=L2)
    assert (r.goal_lo, r.goal_hi, r.L2_lo, r.L2_hi) == (GOAL[0], GOAL[1], 5.0, 10.0)
    assert R(L2=[7, 7]).as_tuple() == (None, None, 7.0, 7.0) and R(goal=[[0, -30, 1], [0, -30, 1]]).L2_lo is None
    for kw, word in ((dict(), "both None"), (dict(goal=(GOAL[0],)), "goal"), (dict(goal=((0, 1), (0, 1))), "goal"),
                     (dict(goal=((0, 0, float("nan")), (0, 0, 1))), "goal"), (dict(goal=((0, 0, 0), (0, 0, float("inf")))), "goal"),
                     (dict(goal=((1.0, 0, 0), (0.0, 0, 0))), "goal: x"), (dict(goal=((0, 0, 2.0), (0, 0, 1.0))), "goal: yaw"),
                     (dict(goal=((0, True, 0), (0, 1, 0))), "goal"), (dict(L2=(5,)), "L2"), (dict(L2=(0.0, 5.0)), "0 < lo <= hi"),
                     (dict(L2=(-1.0, 5.0)), "0 < lo <= hi"), (dict(L2=(6.0, 5.0)), "0 < lo <= hi"),
                     (dict(L2=(5.0, float("inf"))), "L2"), (dict(L2="5,10"), "L2")):
        with pytest.raises(ValueError, match=word):
            R(**kw)


def test_tuple_round_trip_repr_and_checkpoint_key():
    from ddpg_trucktrailer_amd.options import CHECKPOINT_KEYS, _tupled, compare_options, write_options
    from ddpg_trucktrailer_amd.randomize import EpisodeRandomization as R
    for r in (R(goal=GOAL, L2=L2), R(L2=L2), R(goal=GOAL)):
        assert R.from_tuple(r.as_tuple()) == r and hash(R.from_tuple(r.as_tuple())) == hash(r)
    r = R(goal=GOAL, L2=L2)
    assert r.as_tuple() == (GOAL[0], GOAL[1], 5.0, 10.0)
    assert repr(r) == "EpisodeRandomization(goal_lo=(-10.0, -32.0, 1.3), goal_hi=(10.0, -28.0, 1.8), L2_lo=5.0, L2_hi=10.0)"
    assert repr(R(L2=L2)) == "EpisodeRandomization(goal_lo=None, goal_hi=None, L2_lo=5.0, L2_hi=10.0)"
    assert CHECKPOINT_KEYS[-1] == "randomize"
    sd = write_options({}, randomize=r)
    assert sd == {"randomize": [GOAL[0], GOAL[1], 5.0, 10.0]}
    as_file = {"randomize": [list(GOAL[0]), list(GOAL[1]), 5.0, 10.0]}            # (what a file gives back: lists)
    assert R.from_tuple(_tupled(as_file["randomize"])) == r
    compare_options(as_file, randomize=r)
    with pytest.raises(ValueError, match="written with randomize = None"):
        compare_options({}, randomize=r)
    with pytest.raises(ValueError, match="this loop has randomize = None"):
        compare_options(as_file, randomize=None)
    with pytest.raises(ValueError, match="written with randomize"):
        compare_options(as_file, randomize=R(goal=GOAL, L2=(5.0, 9.0)))


def test_nones_resolve_against_the_parameters(lib):
    from ddpg_trucktrailer_amd.randomize import EpisodeRandomization as R
    p = lib.default_params(0)
    r = R(L2=L2).resolved(p)
    assert r.goal_lo == r.goal_hi == tuple(p.goal) == (0.0, -30.0, math.pi / 2) and (r.L2_lo, r.L2_hi) == L2
    r = R(goal=GOAL).resolved(p)
    assert (r.goal_lo, r.goal_hi) == GOAL and r.L2_lo == r.L2_hi == p.L2 == 7.0
    c = R(goal=GOAL).c_struct(p)
    assert (tuple(c.goal_lo), tuple(c.goal_hi), c.L2_lo, c.L2_hi) == (GOAL[0], GOAL[1], 7.0, 7.0)


def test_every_refusal_row_has_its_wording():
    from ddpg_trucktrailer_amd.curriculum import Curriculum
    from ddpg_trucktrailer_amd.mpc import ExpertLabels, ExpertLanes
    from ddpg_trucktrailer_amd.options import TABLE
    from ddpg_trucktrailer_amd.randomize import EpisodeRandomization, check_randomization
    r = EpisodeRandomization(goal=GOAL, L2=L2)
    assert check_randomization(r) is r and check_randomization(r, device="cuda:0") is r
    with pytest.raises(ValueError, match="randomize = 3 is not an EpisodeRandomization"):
        check_randomization(3)
    rows = {
        "population": (dict(population=True), "episode randomisation in a population is not supported (a population's agents step envs "
                                              "of their own, and a randomisation per agent is not built)"),
        "data_parallel": (dict(data_parallel=True), "episode randomisation with data-parallel ranks (or the p2p exchange) is not supported"),
        "force_dp": (dict(force_dp=True), "episode randomisation with the data-parallel launch structure (TT_FORCE_DP) is not supported"),
        "curriculum": (dict(curriculum=Curriculum((3, 2, 2))), "episode randomisation with a curriculum is not supported (the two have "
                                                               "step kernels of their own, and the curriculum's cells would be counted "
                                                               "under a moving goal)"),
        "expert": (dict(expert=ExpertLanes(2)), "episode randomisation with expert lanes is not supported (the expert on randomised "
                                                "lanes is not checked here)"),
        "labels": (dict(labels=ExpertLabels(2)), "episode randomisation with expert labels is not supported (the planner on randomised "
                                                 "lanes is not checked here)"),
        "device": (dict(device="cpu"), "episode randomisation on device = 'cpu' is not supported: it exists only inside the HIP env step"),
        "episode_log_detail": (dict(episode_log_detail=True), "episode randomisation with episode_log_detail is not supported (the "
                                                              "randomised step kernels carry the plain episode log only)"),
    }
    names = [row if isinstance(row, str) else row[0] for row in TABLE["randomize"]["rows"]]
    assert names == list(rows)                   # every row, in the table's order
    for name, (kw, message) in rows.items():
        with pytest.raises(ValueError) as e:
            check_randomization(r, **kw)
        assert str(e.value) == message, name
    # the first row that applies speaks
    order = list(rows)
    for k in range(len(order) - 1):
        with pytest.raises(ValueError) as e:
            check_randomization(r, **rows[order[k]][0], **rows[order[k + 1]][0])
        assert str(e.value) == rows[order[k]][1]


def test_loops_refuse_through_the_table(monkeypatch):
    from cpu_env import CpuEnv
    from ddpg_trucktrailer_amd.curriculum import Curriculum
    from ddpg_trucktrailer_amd.population import PopulationRollout
    from ddpg_trucktrailer_amd.randomize import EpisodeRandomization
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    r = EpisodeRandomization(goal=GOAL, L2=L2)
    kw = dict(batch_size=4, replay_slots=8, use_graph=False)
    with pytest.raises(ValueError, match="episode randomisation in a population"):
        PopulationRollout(4, seeds=[1, 2], randomize=r)
    with pytest.raises(ValueError, match="episode randomisation on device = device\\(type='cpu'\\)"):
        DDPGRollout(CpuEnv(), randomize=r, **kw)
    with pytest.raises(ValueError, match="episode randomisation with data-parallel ranks"):
        DDPGRollout(CpuEnv(), randomize=r, world_size=2, **kw)
    with pytest.raises(ValueError, match="episode randomisation with data-parallel ranks"):
        DDPGRollout(CpuEnv(), randomize=r, dp_exchange="p2p", **kw)
    with pytest.raises(ValueError, match="is not an EpisodeRandomization"):
        DDPGRollout(CpuEnv(), randomize=(5.0, 10.0), **kw)
    # it is checked last: the curriculum's own refusal (the device) speaks before randomisation's refusal of the curriculum
    with pytest.raises(ValueError, match="a curriculum on device"):
        DDPGRollout(CpuEnv(), randomize=r, curriculum=Curriculum((3, 2, 2)), **kw)
    monkeypatch.setenv("TT_FORCE_DP", "1")
    with pytest.raises(ValueError, match="episode randomisation with the data-parallel launch structure"):
        DDPGRollout(CpuEnv(), randomize=r, **kw)


def test_a_plain_loops_state_dict_has_no_randomize_entry():
    from cpu_env import CpuEnv
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.stepper import VectorStepper
    loop = DDPGRollout(CpuEnv(), batch_size=4, replay_slots=8, use_graph=False)
    assert loop.randomize is None and "randomize" not in loop.state_dict()
    st = VectorStepper(CpuEnv(), batch_size=4, replay_slots=8)
    assert "randomize" not in st.acting_state() and len(st.graph_key()) == 4          # (the key of a plain stepper is the parent's)


# ------------------------------------------------------------------------------------------------------------- the model
RAND = (GOAL[0], GOAL[1], L2[0], L2[1])


def test_model_values_lie_inside_their_ranges():
    env, ep = np.arange(4096), np.arange(4096) % 7
    goal, l2 = ref.draw(27, env, ep, RAND)
    assert goal.shape == (4096, 3) and l2.shape == (4096,)
    for d in range(3):
        assert (goal[:, d] >= GOAL[0][d]).all() and (goal[:, d] <= GOAL[1][d]).all()
        assert goal[:, d].max() - goal[:, d].min() > 0.9 * (GOAL[1][d] - GOAL[0][d])
    assert (l2 >= L2[0]).all() and (l2 <= L2[1]).all() and l2.max() - l2.min() > 0.9 * (L2[1] - L2[0])
    # the extreme words stay inside too: u = (r + 0.5) / 2^32 is in (0, 1)
    u = ref.u01(np.array([0, 2 ** 32 - 1], dtype=np.uint64))
    assert 0.0 < u[0] < u[1] < 1.0
    assert (np.float64(L2[0]) + (np.float64(L2[1]) - np.float64(L2[0])) * u <= L2[1]).all()
    # a pure function of (seed, env, episode)
    again, l2_again = ref.draw(27, env[::-1].copy(), ep[::-1].copy(), RAND)
    assert (again[::-1] == goal).all() and (l2_again[::-1] == l2).all()
    other, _ = ref.draw(28, env, ep, RAND)
    assert (other != goal).any()


def test_model_zero_width_gives_lo_exactly():
    env, ep = np.arange(130), np.full(130, 3)
    lo = (0.1, -30.000000000000004, math.pi / 2)
    goal, l2 = ref.draw(5, env, ep, (lo, lo, 7.3, 7.3))
    assert (goal.view(np.uint64) == np.tile(np.array(lo, dtype=np.float64).view(np.uint64), (130, 1))).all()
    assert (l2.view(np.uint64) == np.float64(7.3).view(np.uint64)).all()


def test_task_words_share_nothing_with_the_start_poses():
    env = np.repeat(np.arange(130), 4)
    ep = np.tile(np.arange(4), 130)
    for seed in (0, 27, 2 ** 63 + 5):
        pose, task = ref.words(seed, env, ep, ref.POSE_WORD), ref.words(seed, env, ep, ref.TASK_WORD)
        for a in range(4):
            for b in range(4):
                assert not (pose[a] == task[b]).any(), (seed, a, b)
    assert (ref.POSE_WORD, ref.TASK_WORD, ref.RESET_TAG) == (0, 1, 0x7452)
    # the start pose is curriculum_ref's / loop_ref's: the reset's words with counter word 0
    from td3_ref import philox4x32
    r = philox4x32(env, ep, 0, 0x7452, 27, 0)
    assert all((r[k] == ref.words(27, env, ep, ref.POSE_WORD)[k]).all() for k in range(4))


def test_model_max_steps():
    start = np.array([[0.0, 10.0, 1.5], [3.0, 4.0, 1.0]])
    goal = np.array([[0.0, -30.0, 1.5], [0.0, 0.0, 1.0]])
    assert ref.max_steps(start, goal, 0.40096, 75).tolist() == [int(40.0 / 0.40096) + 75, int(5.0 / 0.40096) + 75]


# ------------------------------------------------------------------------------------------------------------- the library
def test_new_kernels_resources(lib):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    ks = kr.kernels()
    rnd, rnd_log = kr.find(ks, "10k_step_rndIL"), kr.find(ks, "14k_step_rnd_logIL")
    assert len(rnd) == 4 and len(rnd_log) == 4, (sorted(rnd), sorted(rnd_log))       # INFO x RANDOM_POLICY; per-env and auto-reset always
    for n, v in {**rnd, **rnd_log}.items():
        assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (n, v)
        assert v["lds"] == 256 * 23 * 4, (n, v)
    # against k_step_log<PER_ENV = true, INFO, AUTO_RESET = true, RANDOM_POLICY> with the same INFO / RANDOM_POLICY.  AN
    # INTERPRETATION of the issue, which names "the k_step_log<PER_ENV = true, ...> variant with the same INFO / RANDOM_POLICY" and
    # leaves AUTO_RESET open: two such variants exist, AUTO_RESET = true (141-149 registers, 3 waves per SIMD) and false (126, 4
    # waves).  The one with a reset piece is taken, like for like; it is the LOOSER reading -- the new kernels run at 3 waves where
    # the per-env kernels without a reset piece run at 4 (DESIGN.md section 39 says so).
    for info in (0, 1):
        for policy in (0, 1):
            log = kr.find(ks, f"10k_step_logILb1ELb{info}ELb1ELb{policy}E")
            assert len(log) == 1
            floor = kr.waves_per_simd(next(iter(log.values()))["vgpr"])
            for name in (f"10k_step_rndILb{info}ELb{policy}E", f"14k_step_rnd_logILb{info}ELb{policy}E"):
                mine = kr.find(ks, name)
                assert len(mine) == 1, name
                v = next(iter(mine.values()))
                assert kr.waves_per_simd(v["vgpr"]) >= floor, (name, v, floor)
    for name in ("11k_reset_rndE", "10k_rnd_seedE"):
        assert len(kr.find(ks, name)) == 1, name
    reset = next(iter(kr.find(ks, "11k_reset_rndE").values()))
    assert reset["scratch"] == 0 and reset["vgpr_spills"] == 0 and reset["lds"] == 0
    # every kernel of the golden tables keeps its row
    for table in ("kernel_resources_main.json", "kernel_resources_step_log.json"):
        before = json.load(open(os.path.join(GOLDEN, table)))
        moved = {n: (v, ks[n]) for n, v in before.items() if n in ks and ks[n] != v}
        assert not moved, moved
        assert all(n in ks for n in before)


def test_header_exports_and_ctypes_agree(lib):
    header = open(os.path.join(ROOT, "include", "ttenv.h")).read()
    dll = lib.load()
    for n in ("tt_env_set_randomization", "tt_env_randomization"):
        assert n in lib.EXPORTS and hasattr(dll, n), n
    assert re.search(r"\bint tt_env_set_randomization\(tt_env \*env, const tt_randomization \*cfg[^,]*, tt_stream_t stream\);", header)
    assert re.search(r"\bint tt_env_randomization\(const tt_env \*env, tt_randomization \*out\);", header)
    m = re.search(r"typedef struct tt_randomization \{(.*?)\} tt_randomization;", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"(\w+)(?:\[3\])?[,;]", body) == ["goal_lo", "goal_hi", "L2_lo", "L2_hi"]
    assert [f[0] for f in lib.TTRandomization._fields_] == ["goal_lo", "goal_hi", "L2_lo", "L2_hi"]
    assert C.sizeof(lib.TTRandomization) == 8 * 8
    from ddpg_trucktrailer_amd.randomize import EpisodeRandomization
    assert EpisodeRandomization.FIELDS == ("goal_lo", "goal_hi", "L2_lo", "L2_hi")
    assert re.search(r"#define TT_VERSION 3\b", header)            # the state blob's layout did not change


def test_arguments_are_refused_before_the_handle_is_read(lib):
    dll = lib.load()
    fake = C.c_void_p(0x1000)           # never read: the refusals below hold for any handle

    def refused(goal_lo=GOAL[0], goal_hi=GOAL[1], l2_lo=5.0, l2_hi=10.0):
        cfg = lib.TTRandomization((C.c_double * 3)(*goal_lo), (C.c_double * 3)(*goal_hi), l2_lo, l2_hi)
        assert dll.tt_env_set_randomization(fake, C.byref(cfg), None) == lib.TT_EINVAL
        return dll.tt_last_error(None).decode()

    nan, inf = float("nan"), float("inf")
    assert "the goal x range has a bound that is not finite" in refused(goal_lo=(nan, -32.0, 1.3))
    assert "the goal y range has a bound that is not finite" in refused(goal_hi=(10.0, inf, 1.8))
    assert "the goal yaw range has a bound that is not finite" in refused(goal_lo=(-10.0, -32.0, -inf))
    assert "the goal x range has lo = 10 > hi = -10" in refused(goal_lo=(10.0, -32.0, 1.3), goal_hi=(-10.0, -28.0, 1.8))
    assert "the goal yaw range has lo = 2 > hi = 1" in refused(goal_lo=(-10.0, -32.0, 2.0), goal_hi=(10.0, -28.0, 1.0))
    assert "the L2 range has a bound that is not finite" in refused(l2_hi=inf)
    assert "the L2 range has a bound that is not finite" in refused(l2_lo=nan)
    assert "the L2 range has lo = 10 > hi = 5" in refused(l2_lo=10.0, l2_hi=5.0)
    assert "L2_lo = 0 is not > 0" in refused(l2_lo=0.0)
    assert "L2_lo = -1 is not > 0" in refused(l2_lo=-1.0)
    cfg = lib.TTRandomization((C.c_double * 3)(*GOAL[0]), (C.c_double * 3)(*GOAL[1]), 5.0, 10.0)
    assert dll.tt_env_set_randomization(None, C.byref(cfg), None) == lib.TT_EINVAL
    assert b"tt_env_set_randomization: NULL handle" in dll.tt_last_error(None)
    assert dll.tt_env_randomization(None, None) == lib.TT_EINVAL
    assert b"tt_env_randomization: NULL handle" in dll.tt_last_error(None)
