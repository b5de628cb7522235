"""CPU: the task curriculum without a GPU (ddpg_trucktrailer_amd/task_curriculum.py; include/ttenv.h: tt_env_set_task_curriculum;
csrc/ttenv_task.h: k_step_task, k_step_task_log, k_reset_task).

* TaskCurriculum's validation, its tuple round trip, its repr and its checkpoint key (directly before "randomize");
* every row of its part of the refusal table, word for word and in order, and the loops refusing through the table; a plain loop's
  state_dict() has no "task_curriculum" entry and a plain stepper's graph key keeps its length;
* the host model (tests/task_curriculum_ref.py) against its own statement: cell shares over all 2^16 leading values of the pick word
  equal q / cum[-1] to the integer; bins (1, 1, 1, 1) give randomize_ref.draw bit for bit; values inside [lo, hi] with the extreme
  words in the first and the last of 4096 cells; a zero width gives lo exactly; the pick's words share none with the pose's and the
  task's;
* the new kernels' resources, read from the built library;
* the header, the exports and the ctypes table agree, and bad arguments are TT_EINVAL with a message before the handle is read."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import randomize_ref
import task_curriculum_ref as ref
from conftest import GOLDEN, ROOT

GOAL = ((-10.0, -32.0, 1.3), (10.0, -28.0, 1.8))
L2 = (5.0, 10.0)
RAND = (GOAL[0], GOAL[1], L2[0], L2[1])
BINS = (3, 2, 2, 2)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib as L
    return L


def _rand():
    from ddpg_trucktrailer_amd.randomize import EpisodeRandomization
    return EpisodeRandomization(goal=GOAL, L2=L2)


# ------------------------------------------------------------------------------------------------------------- the option
def test_task_curriculum_validates_its_fields():
    from ddpg_trucktrailer_amd.task_curriculum import TaskCurriculum as T, cell_index, cell_of
    t = T(BINS)
    assert (t.bins, t.every, t.mode, t.alpha, t.uniform, t.cells) == (BINS, 64, "frontier", 0.1, 0.1, 24)
    assert T([8, 8, 8, 8]).cells == 4096 and T((1, 1, 1, 1), every=1, mode="hard", alpha=1, uniform=0).uniform == 0.0
    for args, kw, word in (((3,), {}, "bins"), (((3, 2, 2),), {}, "four whole numbers"), (((3, 2, 2, 0),), {}, "bins: nl2"),
                           (((3, 2.0, 2, 2),), {}, "bins: ngy"), (((True, 2, 2, 2),), {}, "bins: ngx"),
                           (((8, 8, 8, 9),), {}, "at most 4096 cells \\(it has 4608\\)"), ((BINS,), dict(every=0), "every"),
                           ((BINS,), dict(mode="easy"), "mode"), ((BINS,), dict(alpha=0.0), "alpha"), ((BINS,), dict(alpha=1.5), "alpha"),
                           ((BINS,), dict(uniform=-0.1), "uniform"), ((BINS,), dict(uniform=float("nan")), "uniform"),
                           ((BINS,), dict(uniform=1.5), "uniform")):
        with pytest.raises(ValueError, match=word):
            T(*args, **kw)
    for c in range(24):
        assert cell_of(BINS, *cell_index(BINS, c)) == c
    assert cell_index(BINS, 23) == (2, 1, 1, 1) and cell_of(BINS, 1, 0, 0, 0) == 1 and cell_of(BINS, 0, 0, 0, 1) == 12
    assert [int(v) for v in ref.cell_index(BINS, 17)] == list(cell_index(BINS, 17)) and ref.cell_of(BINS, 2, 1, 0, 1) == cell_of(BINS, 2, 1, 0, 1)


def test_tuple_round_trip_repr_and_checkpoint_key():
    from ddpg_trucktrailer_amd.options import CHECKPOINT_KEYS, _tupled, compare_options, write_options
    from ddpg_trucktrailer_amd.task_curriculum import TaskCurriculum as T
    t = T(BINS, every=4, mode="hard", alpha=0.25, uniform=0.5)
    assert T.from_tuple(t.as_tuple()) == t and hash(T.from_tuple(t.as_tuple())) == hash(t)
    assert t.as_tuple() == (BINS, 4, "hard", 0.25, 0.5)
    assert repr(t) == "TaskCurriculum(bins=(3, 2, 2, 2), every=4, mode='hard', alpha=0.25, uniform=0.5)"
    assert CHECKPOINT_KEYS[-2:] == ("task_curriculum", "randomize")
    sd = write_options({}, task_curriculum=t, randomize=_rand())
    assert list(sd) == ["task_curriculum", "randomize"] and sd["task_curriculum"] == [BINS, 4, "hard", 0.25, 0.5]
    as_file = {"task_curriculum": [list(BINS), 4, "hard", 0.25, 0.5]}
    assert T.from_tuple(_tupled(as_file["task_curriculum"])) == t
    compare_options(as_file, task_curriculum=t)
    with pytest.raises(ValueError, match="written with task_curriculum = None"):
        compare_options({}, task_curriculum=t)
    with pytest.raises(ValueError, match="this loop has task_curriculum = None"):
        compare_options(as_file, task_curriculum=None)


def test_more_than_one_bin_on_a_zero_width_range_is_refused(lib):
    from ddpg_trucktrailer_amd.randomize import EpisodeRandomization as R
    from ddpg_trucktrailer_amd.task_curriculum import TaskCurriculum as T
    p = lib.default_params(0)
    T(BINS).check_ranges(_rand().resolved(p))
    T((1, 1, 1, 4)).check_ranges(R(L2=L2).resolved(p))                  # (the goal is None: width 0, one bin each)
    with pytest.raises(ValueError, match="3 bins on the goal_x range \\[0.0, 0.0\\], which has width 0"):
        T(BINS).check_ranges(R(L2=L2).resolved(p))
    with pytest.raises(ValueError, match="2 bins on the L2 range \\[7.0, 7.0\\], which has width 0"):
        T(BINS).check_ranges(R(goal=GOAL).resolved(p))
    with pytest.raises(ValueError, match="2 bins on the goal_yaw range"):
        T((1, 1, 2, 1)).check_ranges(R(goal=((-1.0, -31.0, 1.5), (1.0, -29.0, 1.5)), L2=L2))


def test_every_refusal_row_has_its_wording():
    from ddpg_trucktrailer_amd.options import TABLE
    from ddpg_trucktrailer_amd.task_curriculum import TaskCurriculum, check_task_curriculum
    t, r = TaskCurriculum(BINS), _rand()
    assert check_task_curriculum(t, randomize=r) is t and check_task_curriculum(t, randomize=r, device="cuda:0") is t
    with pytest.raises(ValueError, match="task_curriculum = 3 is not a TaskCurriculum"):
        check_task_curriculum(3, randomize=r)
    rows = {
        "randomize": (dict(randomize=None), "a task curriculum without randomize is not supported: there is no range to put cells on"),
        "population": (dict(population=True), "a task curriculum in a population is not supported (a population's agents step envs of "
                                              "their own, and a task curriculum per agent is not built)"),
        "data_parallel": (dict(data_parallel=True), "a task curriculum with data-parallel ranks (or the p2p exchange) is not supported"),
        "force_dp": (dict(force_dp=True), "a task curriculum with the data-parallel launch structure (TT_FORCE_DP) is not supported"),
        "device": (dict(device="cpu"), "a task curriculum on device = 'cpu' is not supported: it exists only inside the HIP env step"),
    }
    names = [row if isinstance(row, str) else row[0] for row in TABLE["task_curriculum"]["rows"]]
    assert names == list(rows)                   # every row, in the table's order
    for name, (kw, message) in rows.items():
        with pytest.raises(ValueError) as e:
            check_task_curriculum(t, **{"randomize": r, **kw})
        assert str(e.value) == message, name
    order = list(rows)                           # the first row that applies speaks
    for k in range(len(order) - 1):
        with pytest.raises(ValueError) as e:
            check_task_curriculum(t, **{"randomize": r, **rows[order[k]][0], **rows[order[k + 1]][0]})
        assert str(e.value) == rows[order[k]][1]


def test_loops_refuse_through_the_table(monkeypatch):
    from cpu_env import CpuEnv
    from ddpg_trucktrailer_amd.population import PopulationRollout
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.task_curriculum import TaskCurriculum
    t, r = TaskCurriculum(BINS), _rand()
    kw = dict(batch_size=4, replay_slots=8, use_graph=False)
    with pytest.raises(ValueError, match="a task curriculum without randomize"):
        PopulationRollout(4, seeds=[1, 2], task_curriculum=t)
    with pytest.raises(ValueError, match="episode randomisation in a population"):          # (randomisation's own row comes first)
        PopulationRollout(4, seeds=[1, 2], task_curriculum=t, randomize=r)
    with pytest.raises(ValueError, match="a task curriculum without randomize is not supported: there is no range to put cells on"):
        DDPGRollout(CpuEnv(), task_curriculum=t, **kw)
    with pytest.raises(ValueError, match="episode randomisation on device"):
        DDPGRollout(CpuEnv(), task_curriculum=t, randomize=r, **kw)
    with pytest.raises(ValueError, match="is not a TaskCurriculum"):
        DDPGRollout(CpuEnv(), task_curriculum=BINS, **kw)
    monkeypatch.setenv("TT_FORCE_DP", "1")
    with pytest.raises(ValueError, match="a task curriculum without randomize"):
        DDPGRollout(CpuEnv(), task_curriculum=t, **kw)


def test_a_plain_loops_state_dict_has_no_task_curriculum_entry():
    from cpu_env import CpuEnv
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.stepper import VectorStepper
    loop = DDPGRollout(CpuEnv(), batch_size=4, replay_slots=8, use_graph=False)
    assert loop.task_curriculum is None and "task_curriculum" not in loop.state_dict()
    st = VectorStepper(CpuEnv(), batch_size=4, replay_slots=8)
    assert "task_curriculum" not in st.acting_state() and len(st.graph_key()) == 4
    st.vector_steps = 5
    assert st.curriculum_room(9) == 9 and st.task_curriculum_tick() is None


# ------------------------------------------------------------------------------------------------------------- the model
def test_model_cell_shares_equal_the_weights_to_the_integer():
    # q with the extremes 1 and 65536; all 2^16 leading values of s[0] (the low 16 bits zero): 2^16 divides every share's denominator
    q = np.array([1, 65536, 300, 65536, 7, 1, 4096, 1, 1, 20000, 65535, 2] * 2, dtype=np.uint64)
    cum = np.cumsum(q).astype(np.uint32)
    s0 = (np.arange(2 ** 16, dtype=np.uint64) << np.uint64(16))
    c = ref.curriculum_ref.pick(s0, cum)
    counts = np.bincount(c, minlength=q.size)
    # t = floor(k * 2^16 * S / 2^32) = floor(k S / 2^16): cell c holds the k with cum[c-1] <= t < cum[c], i.e. k in
    # [ceil(2^16 cum[c-1] / S), ceil(2^16 cum[c] / S)) -- its share is q / S to the integer
    S = int(cum[-1])
    edges = [0] + [-((-(1 << 16) * int(v)) // S) for v in cum]
    assert counts.tolist() == [edges[k + 1] - edges[k] for k in range(q.size)]
    assert counts.sum() == 2 ** 16 and all(abs(int(n) - (1 << 16) * int(w) / S) < 1 for n, w in zip(counts, q))


def test_model_one_bin_is_plain_randomisation_bit_for_bit():
    env, ep = np.arange(4096), np.arange(4096) % 5
    for seed in (0, 27, 2 ** 63 + 5):
        c, goal, l2 = ref.draw(seed, env, ep, np.array([65536], dtype=np.uint32), (1, 1, 1, 1), RAND)
        g0, l0 = randomize_ref.draw(seed, env, ep, RAND)
        assert (c == 0).all()
        assert (goal.view(np.uint64) == g0.view(np.uint64)).all() and (l2.view(np.uint64) == l0.view(np.uint64)).all()


def test_model_values_lie_inside_their_ranges_and_cells():
    env, ep = np.arange(4096), np.arange(4096) % 7
    q, cum = ref.weights(np.full(24, 0.5), "frontier", 0.1)
    c, goal, l2 = ref.draw(27, env, ep, cum, BINS, RAND)
    lo, hi = (*GOAL[0], L2[0]), (*GOAL[1], L2[1])
    vals = [goal[:, 0], goal[:, 1], goal[:, 2], l2]
    idx = ref.cell_index(BINS, c)
    assert set(c.tolist()) == set(range(24))
    for d in range(4):
        w = (hi[d] - lo[d]) / BINS[d]
        assert (vals[d] >= lo[d]).all() and (vals[d] <= hi[d]).all()
        assert (vals[d] >= lo[d] + idx[d] * w - 1e-12).all() and (vals[d] <= lo[d] + (idx[d] + 1) * w + 1e-12).all()
    # the extreme words 0 and 2^32 - 1 in the first and the last of 4096 cells of one dimension, each dimension in turn
    r = [np.array([0, 2 ** 32 - 1], dtype=np.uint64)] * 4
    for d in range(4):
        bins = tuple(4096 if k == d else 1 for k in range(4))
        cells = np.array([0, 4095]) * 1                     # (the other dimensions have one bin: c is this dimension's index)
        g, l = ref.place(r, cells, bins, RAND)
        v = [g[:, 0], g[:, 1], g[:, 2], l][d]
        w = (hi[d] - lo[d]) / 4096
        assert lo[d] < v[0] < lo[d] + w and hi[d] - w < v[1] <= hi[d], (d, v)
        for k, other in enumerate([g[:, 0], g[:, 1], g[:, 2], l]):
            assert (other >= lo[k]).all() and (other <= hi[k]).all(), (d, k)
    # a pure function of (seed, env, episode, cum)
    c2, g2, l2b = ref.draw(27, env[::-1].copy(), ep[::-1].copy(), cum, BINS, RAND)
    assert (c2[::-1] == c).all() and (g2[::-1] == goal).all() and (l2b[::-1] == l2).all()


def test_model_zero_width_gives_lo_exactly():
    env, ep = np.arange(130), np.full(130, 3)
    lo = (0.1, -30.000000000000004, math.pi / 2)
    q, cum = ref.weights(np.full(4, 0.5), "hard", 0.0)
    c, goal, l2 = ref.draw(5, env, ep, cum, (1, 1, 1, 4), (lo, lo, 5.0, 10.0))
    assert (goal.view(np.uint64) == np.tile(np.array(lo, dtype=np.float64).view(np.uint64), (130, 1))).all()
    assert set(c.tolist()) == {0, 1, 2, 3}
    c, goal, l2 = ref.draw(5, env, ep, np.array([9], dtype=np.uint32), (1, 1, 1, 1), (GOAL[0], GOAL[1], 7.3, 7.3))
    assert (l2.view(np.uint64) == np.float64(7.3).view(np.uint64)).all()


def test_pick_words_share_nothing_with_the_poses_and_the_tasks():
    env = np.repeat(np.arange(130), 4)
    ep = np.tile(np.arange(4), 130)
    assert (randomize_ref.POSE_WORD, randomize_ref.TASK_WORD, ref.PICK_WORD) == (0, 1, 2)
    for seed in (0, 27, 2 ** 63 + 5):
        pick = randomize_ref.words(seed, env, ep, ref.PICK_WORD)
        for other in (randomize_ref.POSE_WORD, randomize_ref.TASK_WORD):
            w = randomize_ref.words(seed, env, ep, other)
            for a in range(4):
                for b in range(4):
                    assert not (pick[a] == w[b]).any(), (seed, other, a, b)


# ------------------------------------------------------------------------------------------------------------- the library
def test_new_kernels_resources(lib):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    ks = kr.kernels()
    task, task_log = kr.find(ks, "11k_step_taskIL"), kr.find(ks, "15k_step_task_logIL")
    assert len(task) == 4 and len(task_log) == 4, (sorted(task), sorted(task_log))      # INFO x RANDOM_POLICY
    for n, v in {**task, **task_log}.items():
        assert v["scratch"] == 0 and v["vgpr_spills"] == 0, (n, v)                      # (scalar spills: recorded, no condition)
        assert v["lds"] == 256 * 23 * 4, (n, v)
    for info in (0, 1):
        for policy in (0, 1):
            for mine, theirs in ((f"11k_step_taskILb{info}ELb{policy}E", f"10k_step_rndILb{info}ELb{policy}E"),
                                 (f"15k_step_task_logILb{info}ELb{policy}E", f"14k_step_rnd_logILb{info}ELb{policy}E")):
                a, b = kr.find(ks, mine), kr.find(ks, theirs)
                assert len(a) == 1 and len(b) == 1, (mine, theirs)
                assert kr.waves_per_simd(next(iter(a.values()))["vgpr"]) >= kr.waves_per_simd(next(iter(b.values()))["vgpr"]), (mine, a, b)
    reset = kr.find(ks, "12k_reset_taskE")
    assert len(reset) == 1
    reset = next(iter(reset.values()))
    assert reset["scratch"] == 0 and reset["vgpr_spills"] == 0 and reset["lds"] == 0
    # every kernel of the golden tables keeps its row
    for table in ("kernel_resources_main.json", "kernel_resources_step_log.json"):
        before = json.load(open(os.path.join(GOLDEN, table)))
        moved = {n: (v, ks[n]) for n, v in before.items() if n in ks and ks[n] != v}
        assert not moved, moved
        assert all(n in ks for n in before)


NAMES = ("tt_env_set_task_curriculum", "tt_env_task_curriculum_update", "tt_env_task_curriculum_read", "tt_env_task_curriculum_write",
         "tt_env_task_curriculum")


def test_header_exports_and_ctypes_agree(lib):
    header = open(os.path.join(ROOT, "include", "ttenv.h")).read()
    dll = lib.load()
    for n in NAMES:
        assert n in lib.EXPORTS and hasattr(dll, n), n
        assert re.search(r"\bint " + n + r"\((const )?tt_env \*env,", header), n
    m = re.search(r"typedef struct tt_task_curriculum \{(.*?)\} tt_task_curriculum;", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"(\w+)(?:\[4\])?[,;]", body) == ["bins", "mode", "alpha", "uniform"]
    assert [f[0] for f in lib.TTTaskCurriculum._fields_] == ["bins", "mode", "alpha", "uniform"]
    assert C.sizeof(lib.TTTaskCurriculum) == 4 * 4 + 4 + 4 + 2 * 8 and lib.TTTaskCurriculum.alpha.offset == 24
    assert re.search(r"#define TT_VERSION 3\b", header)            # the state blob's layout did not change
    src = open(os.path.join(ROOT, "ddpg-trucktrailer_amd", "csrc", "ttenv_task.h")).read()
    assert "#pragma clang fp contract(off)" in src


def test_arguments_are_refused_before_the_handle_is_read(lib):
    dll = lib.load()
    fake = C.c_void_p(0x1000)           # never read: the refusals below hold for any handle

    def refused(bins=BINS, mode=0, alpha=0.1, uniform=0.1):
        cfg = lib.TTTaskCurriculum((C.c_int32 * 4)(*bins), mode, alpha, uniform)
        assert dll.tt_env_set_task_curriculum(fake, C.byref(cfg), None, None) == lib.TT_EINVAL
        return dll.tt_last_error(None).decode()

    assert "tt_env_set_task_curriculum: bins (3, 2, 0, 2): a bin count below 1" in refused(bins=(3, 2, 0, 2))
    assert "bins (-1, 2, 2, 2): a bin count below 1" in refused(bins=(-1, 2, 2, 2))
    assert "bins (8, 8, 8, 9) make more than 4096 cells" in refused(bins=(8, 8, 8, 9))
    assert "make more than 4096 cells" in refused(bins=(65536, 65536, 65536, 65536))
    assert "unknown mode 2" in refused(mode=2)
    assert "alpha is outside (0, 1]" in refused(alpha=0.0)
    assert "alpha is outside (0, 1]" in refused(alpha=float("nan"))
    assert "uniform is outside [0, 1] or not finite" in refused(uniform=1.5)
    assert "uniform is outside [0, 1] or not finite" in refused(uniform=float("nan"))
    cfg = lib.TTTaskCurriculum((C.c_int32 * 4)(*BINS), 0, 0.1, 0.1)
    part = lib.TTCurriculumArrays(0x10, 0x10, 0x10, None, 0x10, 0x10, 0x10)
    assert dll.tt_env_set_task_curriculum(fake, C.byref(cfg), C.byref(part), None) == lib.TT_EINVAL
    assert b"place names every array or is NULL" in dll.tt_last_error(None)
    assert dll.tt_env_set_task_curriculum(None, C.byref(cfg), None, None) == lib.TT_EINVAL
    assert b"tt_env_set_task_curriculum: NULL handle" in dll.tt_last_error(None)
    for n in NAMES[1:]:
        args = (None, None) if n in ("tt_env_task_curriculum_update", "tt_env_task_curriculum") else (None, None, None)
        assert getattr(dll, n)(*args) == lib.TT_EINVAL, n
        assert (n + ": NULL handle").encode() in dll.tt_last_error(None), n
