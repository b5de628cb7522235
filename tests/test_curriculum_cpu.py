"""CPU: the start-pose curriculum without a GPU (ddpg_trucktrailer_amd/curriculum.py; include/ttenv.h: tt_env_set_curriculum;
csrc/ttenv_curriculum.h: k_step_cur, k_step_cur_log, k_curriculum_update).

* Curriculum's validation, its tuple round trip, and every row of its part of the refusal table, word for word;
* the host model (tests/curriculum_ref.py) against its own statement: draw shares to the integer, cum[-1] == sum(q), equal weights at
  p = 0.5 in both modes, alpha = 1 replaces p, a cell with no episodes keeps its p;
* the new kernels' resources, read from the built library: no scratch, no vector spill, and the loop's variants at k_step_log's four
  waves per SIMD; every kernel the library had keeps its row of the golden tables;
* the header, the exports and the ctypes table agree, and bad arguments are TT_EINVAL with a message before the handle is read;
* the counting test's condition on the C oracle: the small box around the goal with three steps gives successes AND failures;
* a plain loop's state_dict() has no "curriculum" entry."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import curriculum_ref as ref
from conftest import GOLDEN, ROOT

# the counting test's env (tests/test_gpu_curriculum.py uses the same numbers): a box around the goal pose, episodes of three steps
COUNT_LO = (-0.3, -29.8, np.pi / 2 - 0.1)
COUNT_HI = (0.3, -28.0, np.pi / 2 + 0.1)
COUNT_MAX_STEPS = 3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------------------- the option
def test_curriculum_validates_its_fields():
    from ddpg_trucktrailer_amd.curriculum import Curriculum
    c = Curriculum((3, 2, 2), every=4)
    assert (c.bins, c.every, c.mode, c.alpha, c.uniform, c.cells) == ((3, 2, 2), 4, "frontier", 0.1, 0.1, 12)
    assert Curriculum((16, 16, 16)).cells == 4096 and Curriculum([1, 1, 1], mode="hard", alpha=1, uniform=0).cells == 1
    for kw, word in ((dict(bins=(3, 2)), "bins"), (dict(bins=(0, 2, 2)), "nx"), (dict(bins=(3, 2.0, 2)), "ny"),
                     (dict(bins=(3, 2, True)), "nyaw"), (dict(bins=(17, 16, 16)), "4096"), (dict(bins=(3, 2, 2), every=0), "every"),
                     (dict(bins=(3, 2, 2), every=1.5), "every"), (dict(bins=(3, 2, 2), mode="easy"), "mode"),
                     (dict(bins=(3, 2, 2), alpha=0), "alpha"), (dict(bins=(3, 2, 2), alpha=1.01), "alpha"),
                     (dict(bins=(3, 2, 2), alpha=float("nan")), "alpha"), (dict(bins=(3, 2, 2), uniform=-0.1), "uniform"),
                     (dict(bins=(3, 2, 2), uniform=1.5), "uniform"), (dict(bins=(3, 2, 2), uniform=float("inf")), "uniform")):
        with pytest.raises(ValueError, match=word):
            Curriculum(**kw)


def test_tuple_round_trip_and_checkpoint_key():
    from ddpg_trucktrailer_amd.curriculum import Curriculum
    from ddpg_trucktrailer_amd.options import CHECKPOINT_KEYS, _tupled, compare_options, write_options
    c = Curriculum((3, 2, 2), every=4, mode="hard", alpha=0.25, uniform=0.5)
    assert c.as_tuple() == ((3, 2, 2), 4, "hard", 0.25, 0.5)
    assert Curriculum.from_tuple(c.as_tuple()) == c and hash(Curriculum.from_tuple(c.as_tuple())) == hash(c)
    assert repr(c) == "Curriculum(bins=(3, 2, 2), every=4, mode='hard', alpha=0.25, uniform=0.5)"
    assert "curriculum" in CHECKPOINT_KEYS
    sd = write_options({}, curriculum=c)
    assert sd == {"curriculum": [(3, 2, 2), 4, "hard", 0.25, 0.5]}
    as_file = {"curriculum": [[3, 2, 2], 4, "hard", 0.25, 0.5]}           # (what a file gives back: lists)
    assert Curriculum.from_tuple(_tupled(as_file["curriculum"])) == c
    compare_options(as_file, curriculum=c)
    with pytest.raises(ValueError, match="written with curriculum = None"):
        compare_options({}, curriculum=c)
    with pytest.raises(ValueError, match="this loop has curriculum = None"):
        compare_options(as_file, curriculum=None)
    with pytest.raises(ValueError, match="written with curriculum"):
        compare_options(as_file, curriculum=Curriculum((3, 2, 2), every=8, mode="hard", alpha=0.25, uniform=0.5))


def test_every_refusal_row_has_its_wording():
    from ddpg_trucktrailer_amd.curriculum import Curriculum, check_curriculum
    from ddpg_trucktrailer_amd.mpc import ExpertLabels, ExpertLanes
    from ddpg_trucktrailer_amd.options import TABLE
    c = Curriculum((3, 2, 2))
    assert check_curriculum(c) is c and check_curriculum(c, device="cuda:0") is c
    with pytest.raises(ValueError, match="curriculum = 3 is not a Curriculum"):
        check_curriculum(3)
    rows = {
        "population": (dict(population=True), "a curriculum in a population is not supported (a population's agents step envs of their "
                                              "own, and a curriculum per agent is not built)"),
        "data_parallel": (dict(data_parallel=True), "a curriculum with data-parallel ranks (or the p2p exchange) is not supported"),
        "force_dp": (dict(force_dp=True), "a curriculum with the data-parallel launch structure (TT_FORCE_DP) is not supported"),
        "expert": (dict(expert=ExpertLanes(2)), "a curriculum with expert lanes is not supported (the expert's launch steps and resets "
                                                "its lanes itself)"),
        "labels": (dict(labels=ExpertLabels(2)), "a curriculum with expert labels is not supported (the planner's launch steps and "
                                                 "resets its lanes itself)"),
        "device": (dict(device="cpu"), "a curriculum on device = 'cpu' is not supported: it exists only inside the HIP env step"),
        "episode_log_detail": (dict(episode_log_detail=True), "a curriculum with episode_log_detail is not supported (the curriculum's "
                                                              "step kernels carry the plain episode log only)"),
    }
    names = [r if isinstance(r, str) else r[0] for r in TABLE["curriculum"]["rows"]]
    assert names == list(rows)                   # every row, in the table's order
    for name, (kw, message) in rows.items():
        with pytest.raises(ValueError) as e:
            check_curriculum(c, **kw)
        assert str(e.value) == message, name
    # the first row that applies speaks
    with pytest.raises(ValueError, match="in a population"):
        check_curriculum(c, population=True, device="cpu")


def test_loops_refuse_through_the_table(monkeypatch):
    from cpu_env import CpuEnv
    from ddpg_trucktrailer_amd.curriculum import Curriculum
    from ddpg_trucktrailer_amd.population import PopulationRollout
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    c = Curriculum((3, 2, 2), every=4)
    kw = dict(batch_size=4, replay_slots=8, use_graph=False)
    with pytest.raises(ValueError, match="in a population"):
        PopulationRollout(4, seeds=[1, 2], curriculum=c)
    with pytest.raises(ValueError, match="device = device\\(type='cpu'\\)"):
        DDPGRollout(CpuEnv(), curriculum=c, **kw)
    with pytest.raises(ValueError, match="data-parallel ranks"):
        DDPGRollout(CpuEnv(), curriculum=c, world_size=2, **kw)
    with pytest.raises(ValueError, match="data-parallel ranks"):
        DDPGRollout(CpuEnv(), curriculum=c, dp_exchange="p2p", **kw)
    with pytest.raises(ValueError, match="is not a Curriculum"):
        DDPGRollout(CpuEnv(), curriculum=(3, 2, 2), **kw)
    monkeypatch.setenv("TT_FORCE_DP", "1")
    with pytest.raises(ValueError, match="TT_FORCE_DP"):
        DDPGRollout(CpuEnv(), curriculum=c, **kw)


def test_a_plain_loops_state_dict_has_no_curriculum_entry():
    from cpu_env import CpuEnv
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.stepper import VectorStepper
    loop = DDPGRollout(CpuEnv(), batch_size=4, replay_slots=8, use_graph=False)
    assert loop.curriculum is None and "curriculum" not in loop.state_dict()
    assert "curriculum" not in VectorStepper(CpuEnv(), batch_size=4, replay_slots=8).acting_state()
    assert loop.curriculum_room(7) == 7
    loop.curriculum_tick()          # nothing to do, and no env call


# ------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("bins", [(3, 2, 2), (16, 16, 16), (1, 1, 1), (5, 1, 7)])
def test_cell_map_round_trips(bins):
    from ddpg_trucktrailer_amd.curriculum import cell_index, cell_of
    nx, ny, nyaw = bins
    c = np.arange(nx * ny * nyaw)
    ix, iy, iyaw = ref.cell_index(bins, c)
    assert (ix < nx).all() and (iy < ny).all() and (iyaw < nyaw).all()
    assert (ref.cell_of(bins, ix, iy, iyaw) == c).all()
    assert all(cell_index(bins, int(k)) == (int(ix[k]), int(iy[k]), int(iyaw[k])) and cell_of(bins, ix[k], iy[k], iyaw[k]) == k
               for k in (0, len(c) // 2, len(c) - 1))
    assert ref.cell_of(bins, nx - 1, ny - 1, nyaw - 1) == len(c) - 1


@pytest.mark.parametrize("cells, heavy", [(12, 5), (4096, 4095), (4096, 0), (1, 0)])
def test_draw_shares_equal_the_weights_to_the_integer(cells, heavy):
    """Planted weights, one cell at 65536 and the rest at 1: over all 2^16 leading values of r[3] (r[3] = v << 16) the draws of a
    cell are the integers t = (r3 * total) >> 32 that fall in [cum[c - 1], cum[c])."""
    q = np.ones(cells, dtype=np.int64)
    q[heavy] = 65536
    cum = np.cumsum(q)
    r3 = np.arange(65536, dtype=np.uint64) << np.uint64(16)
    got = np.bincount(ref.pick(r3, cum), minlength=cells)
    t = (r3 * np.uint64(cum[-1])) >> np.uint64(32)
    lo = np.concatenate(([0], cum[:-1]))
    want = np.array([np.count_nonzero((t >= a) & (t < b)) for a, b in zip(lo, cum)]) if cells <= 12 else \
        np.histogram(t.astype(np.int64), bins=np.concatenate(([0], cum)))[0]
    assert (got == want).all() and got.sum() == 65536
    # ... and that is q / cum[-1] of the 2^16 values, to the integer
    share = 65536 * q / cum[-1]
    assert (np.abs(got - share) < 1.0 + 1e-9).all()
    assert got[heavy] in (int(np.floor(share[heavy])), int(np.ceil(share[heavy])))


@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("uniform", [0.0, 0.1, 1.0])
def test_weights_rule(mode, uniform):
    rng = np.random.RandomState(3)
    p = rng.uniform(0, 1, 4096)
    p[:3] = (0.0, 0.5, 1.0)
    q, cum = ref.weights(p, mode, uniform)
    assert q.min() >= 1 and q.max() <= 65536 and int(cum[-1]) == int(q.astype(np.int64).sum())
    assert (np.diff(cum.astype(np.int64)) == q[1:]).all() and cum[0] == q[0]
    # p = 0.5 everywhere: equal weights in both modes
    qh, _ = ref.weights(np.full(12, 0.5), mode, uniform)
    assert len(set(qh.tolist())) == 1
    if uniform == 1.0:
        assert (q == 65536).all()
    if uniform == 0.0:
        assert q[0] == (1 if mode == "frontier" else 65536) and q[2] == 1
        assert q[1] == (65536 if mode == "frontier" else 1 + 32767)


def test_update_rule():
    rng = np.random.RandomState(5)
    C_ = 12
    p0 = rng.uniform(0, 1, C_)
    att = rng.randint(0, 50, C_).astype(np.uint32)
    att[[1, 7]] = 0
    suc = (att * rng.uniform(0, 1, C_)).astype(np.uint32)
    seen0 = rng.randint(0, 2 ** 40, C_).astype(np.uint64)
    # alpha = 1 replaces p by the rate; a cell with no episodes keeps its p, bit for bit
    p, seen, q, cum = ref.update(p0, seen0, att, suc, "frontier", 1.0, 0.1)
    hit = att > 0
    assert (p[hit] == suc[hit].astype(np.float64) / att[hit].astype(np.float64)).all()
    assert (p[~hit] == p0[~hit]).all() and (seen == seen0 + att).all()
    assert (q == ref.weights(p, "frontier", 0.1)[0]).all() and (cum == np.cumsum(q)).all()
    # alpha = 0.1: the running mean, one rounding per operation
    p, _, _, _ = ref.update(p0, seen0, att, suc, "hard", 0.1, 0.0)
    want = np.float64(0.9) * p0[hit] + np.float64(0.1) * (suc[hit].astype(np.float64) / att[hit].astype(np.float64))
    assert (p[hit] == want).all() and (p[~hit] == p0[~hit]).all()


def test_draw_is_inside_its_cell_and_uses_the_resets_words():
    from td3_ref import philox4x32
    bins, lo, hi = (3, 2, 2), (-27.0, 0.0, np.pi / 4), (27.0, 27.0, 2 * np.pi / 3)
    q = np.array([1, 65536, 1, 7, 9, 1, 300, 1, 1, 65536, 2, 1])
    cum = np.cumsum(q)
    env, ep = np.arange(130), np.full(130, 2)
    c, pose = ref.draw(27, env, ep, cum, bins, lo, hi)
    idx = ref.cell_index(bins, c)
    for d in range(3):
        w = (hi[d] - lo[d]) / bins[d]
        assert (pose[:, d] >= lo[d] + idx[d] * w - 1e-12).all() and (pose[:, d] <= lo[d] + (idx[d] + 1) * w + 1e-12).all()
    r = philox4x32(env, ep, 0, 0x7452, 27, 0)
    assert (c == np.searchsorted(cum, (r[3] * np.uint64(cum[-1])) >> np.uint64(32), side="right")).all()
    assert len(set(c.tolist())) > 1 and np.bincount(c, minlength=12)[[1, 9]].sum() > 100


# ------------------------------------------------------------------------------------------------------------- the library
def test_new_kernels_resources(lib):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    ks = kr.kernels()
    cur, cur_log = kr.find(ks, "10k_step_curIL"), kr.find(ks, "14k_step_cur_logIL")
    assert len(cur) == 8 and len(cur_log) == 8, (sorted(cur), sorted(cur_log))       # PER_ENV x INFO x RANDOM_POLICY, auto-reset always
    for n, v in {**cur, **cur_log}.items():
        assert v["scratch"] == 0 and v["vgpr_spills"] == 0, (n, v)
        assert v["lds"] == 256 * 23 * 4, (n, v)
    # the forms the loop launches (PER_ENV = false): the occupancy of k_step_log's
    log_waves = {kr.waves_per_simd(v["vgpr"]) for v in kr.find(ks, "10k_step_logILb0E").values()}
    assert log_waves == {4}
    loop = {**kr.find(ks, "10k_step_curILb0E"), **kr.find(ks, "14k_step_cur_logILb0E")}
    assert len(loop) == 8
    for n, v in loop.items():
        assert v["vgpr"] <= 128 and kr.waves_per_simd(v["vgpr"]) == 4, (n, v)
    for name in ("19k_curriculum_update", "18k_reset_curriculum", "18k_curriculum_unset", "17k_curriculum_seed"):
        assert len(kr.find(ks, name)) == 1, name
    up = next(iter(kr.find(ks, "19k_curriculum_update").values()))
    assert up["scratch"] == 0 and up["vgpr_spills"] == 0 and up["lds"] == 1024
    # every kernel of the golden tables keeps its row
    for table in ("kernel_resources_main.json", "kernel_resources_step_log.json"):
        before = json.load(open(os.path.join(GOLDEN, table)))
        moved = {n: (v, ks[n]) for n, v in before.items() if n in ks and ks[n] != v}
        assert not moved, moved


def test_header_exports_and_ctypes_agree(lib):
    names = ("tt_env_set_curriculum", "tt_env_curriculum_update", "tt_env_curriculum_read", "tt_env_curriculum_write")
    header = open(os.path.join(ROOT, "include", "ttenv.h")).read()
    dll = lib.load()
    for n in names:
        assert n in lib.EXPORTS and hasattr(dll, n) and re.search(r"\bint " + n + r"\(tt_env \*env,", header), n
    assert C.sizeof(lib.TTCurriculum) == 32 and C.sizeof(lib.TTCurriculumArrays) == 7 * 8
    assert [f[0] for f in lib.TTCurriculumArrays._fields_] == list(lib.CURRICULUM_ARRAYS)
    m = re.search(r"typedef struct tt_curriculum_arrays \{(.*?)\} tt_curriculum_arrays;", header, re.S)
    assert re.findall(r"\*(\w+)", m.group(1)) == list(lib.CURRICULUM_ARRAYS)
    for macro, value in (("TT_CURRICULUM_MAX_CELLS", lib.CURRICULUM_MAX_CELLS), ("TT_CURRICULUM_NO_CELL", lib.CURRICULUM_NO_CELL),
                         ("TT_CURRICULUM_FRONTIER", lib.CURRICULUM_MODES.index("frontier")),
                         ("TT_CURRICULUM_HARD", lib.CURRICULUM_MODES.index("hard"))):
        got = re.search(r"#define " + macro + r" (\w+)", header).group(1).rstrip("u")
        assert int(got, 0) == value, macro
    assert ref.NO_CELL == lib.CURRICULUM_NO_CELL and ref.MODES == lib.CURRICULUM_MODES


def test_arguments_are_refused_before_the_handle_is_read(lib):
    dll = lib.load()
    fake = C.c_void_p(0x1000)           # never read: the refusals below hold for any handle

    def refused(nx=3, ny=2, nyaw=2, mode=0, alpha=0.1, uniform=0.1):
        cfg = lib.TTCurriculum(nx, ny, nyaw, mode, alpha, uniform)
        assert dll.tt_env_set_curriculum(fake, C.byref(cfg), None, None) == lib.TT_EINVAL
        return dll.tt_last_error(None).decode()

    assert "a bin count below 1" in refused(nx=0) and "a bin count below 1" in refused(nyaw=-2)
    assert "4352 cells, outside [1, 4096]" in refused(17, 16, 16)
    assert "unknown mode 2" in refused(mode=2)
    for a in (0.0, -0.5, 1.5, float("nan")):
        assert "alpha is outside (0, 1]" in refused(alpha=a)
    for u in (-0.1, 1.1, float("nan"), float("inf")):
        assert "uniform is outside [0, 1] or not finite" in refused(uniform=u)
    cfg = lib.TTCurriculum(3, 2, 2, 0, 0.1, 0.1)
    part = lib.TTCurriculumArrays(0x2000, 0x2000, 0x2000, 0x2000, 0x2000, 0x2000, None)
    assert dll.tt_env_set_curriculum(fake, C.byref(cfg), C.byref(part), None) == lib.TT_EINVAL
    assert b"place names every array or is NULL" in dll.tt_last_error(None)
    for fn, args in (("tt_env_set_curriculum", (None, C.byref(cfg), None, None)), ("tt_env_curriculum_update", (None, None)),
                     ("tt_env_curriculum_read", (None, C.byref(part), None)), ("tt_env_curriculum_write", (None, C.byref(part), None))):
        assert getattr(dll, fn)(*args) == lib.TT_EINVAL
        assert (fn + ": NULL handle").encode() in dll.tt_last_error(None)
    assert dll.tt_env_curriculum_read(fake, None, None) == lib.TT_EINVAL and b"NULL argument" in dll.tt_last_error(None)


def test_counting_box_gives_successes_and_failures_on_the_oracle():
    """The condition tests/test_gpu_curriculum.py's counting test stands on, checked where it can be without a GPU: starts spread
    over the small box around the goal, three steps of uniform random steering -- some episodes succeed, some end without."""
    from oracle import c_oracle
    n = 256
    rng = np.random.RandomState(11)
    start = np.stack([rng.uniform(COUNT_LO[d], COUNT_HI[d], n) for d in range(3)], axis=1)
    ora = c_oracle.COracle(n)
    ora.params.fixed_max_steps = COUNT_MAX_STEPS
    ora.place(start)
    alive, success = np.ones(n, bool), np.zeros(n, bool)
    for _ in range(COUNT_MAX_STEPS):
        a = (rng.uniform(-1, 1, n) * np.pi / 4).astype(np.float32)
        _, _, done, info = ora.step(a)
        success |= alive & done & (info[:, c_oracle.INFO_KEYS.index("final_success_bonus")] > 0)
        alive &= ~done
    assert not alive.any()                                  # every episode is over within the three steps
    assert 20 < success.sum() < n - 20, int(success.sum())
