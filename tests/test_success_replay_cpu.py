"""CPU: success replay without a GPU (ddpg_trucktrailer_amd/success_replay.py; include/ttenv.h: tt_ring_harvest, tt_env_harvest;
csrc/ttenv_harvest.h: k_harvest_plan, k_harvest_copy).

* the host model (tests/harvest_ref.py) against a second statement of the rule, made row by row from the side region's end of things:
  side row x holds the newest global row g = x (mod capacity) -- on random planted logs with failures, expired and malformed
  records, wraps, oversized harvests, tails and early rings; a permuted log gives the same result;
* SuccessReplay's validation, its tuple round trip and its checkpoint key; every row of its part of the refusal table, word for
  word and in order; the loops refusing through the table; a plain loop carries nothing of the option;
* the ring's part: the region behind loaded demonstrations, load_side refused after it, the exposed count and the epoch, the state
  dict's round trip and its refusal of another region;
* the ctypes struct's layout against the header, the exports, and the C refusals with their messages before any HIP call;
* the two kernels' resources, and every kernel of the golden tables keeping its row;
* the pose pool of the GPU loop test (harvest_ref.POSE_POOL): with the C oracle every pose ends in success within 8 steps under
  constant steering -1, 0, +1 and one fixed random sequence."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import harvest_ref as ref
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------------------- the model
def random_log(rng, n_envs, slots, k, count, step_base=0):
    """`count` records with unique (end_step, lane): successes and failures around the window's edges, some expired, some malformed."""
    W, lo = ref.window(k, slots)
    steps = np.arange(max(0, lo - 4), k + 2)
    pairs = rng.permutation(len(steps) * n_envs)[:count]
    s, lane = steps[pairs // n_envs], (pairs % n_envs).astype(np.int32)
    recs = dict(lane=lane, end_step=(s - step_base).astype(np.int64), len=rng.randint(1, 2 * slots, count).astype(np.int32),
                success=(rng.rand(count) < 0.6).astype(np.uint8))
    bad = rng.rand(count) < 0.08
    recs["lane"][bad & (lane % 2 == 0)] = n_envs + 3                 # malformed: a lane the ring does not have
    recs["len"][bad & (lane % 2 == 1)] = 0                           # malformed: an empty episode
    return recs


def restated(state, side, ring, k, recs, written, record_capacity, capacity, tail=0, step_base=0):
    """The rule once more, from the side row's point of view: the rows of the harvest as one list in (s, lane, step) order; side row
    x holds the last listed row whose global number is x modulo the capacity, if the harvest has one."""
    state = np.array(state, dtype=np.int64)
    side = {name: np.array(a) for name, a in side.items()}
    slots, n = ring["act"].shape
    k = max(int(k), 0)
    lo = k - min(k, slots - 1)
    m = min(int(written), int(record_capacity))
    mark = min(max(int(state[0]), 0), m)
    idx = np.arange(mark, m)
    lane, L = recs["lane"][idx].astype(np.int64), recs["len"][idx].astype(np.int64)
    s = recs["end_step"][idx].astype(np.int64) + step_base
    ok = (recs["success"][idx] != 0) & (lane >= 0) & (lane < n) & (L >= 1) & (s < k)
    expired = ok & (s < lo)
    elig = ok & ~expired
    want = L if tail == 0 else np.minimum(L, tail)
    first = np.maximum(s - want + 1, lo)
    order = np.lexsort((lane[elig], s[elig]))
    rows = []                                                      # (ring step, lane) of global row written_rows + len(rows)
    for q in order:
        rows += [(j, int(lane[elig][q])) for j in range(int(first[elig][q]), int(s[elig][q]) + 1)]
    R = len(rows)
    for x in range(capacity):
        g = int(state[1]) + R - 1 - ((int(state[1]) + R - 1 - x) % capacity)      # the newest g <= written_rows + R - 1 with g % capacity == x
        if g < int(state[1]):
            continue
        j, e = rows[g - int(state[1])]
        side["obs"][x], side["obs2"][x] = ring["obs"][j % slots, e], ring["obs"][(j + 1) % slots, e]
        side["act"][x], side["rew"][x], side["done"][x] = ring["act"][j % slots, e], ring["rew"][j % slots, e], ring["done"][j % slots, e]
    state[0] = m
    state[1] += R
    state[2] += int(elig.sum())
    state[3] += int((want[elig] - (s[elig] - first[elig] + 1)).sum())
    state[4] += int(expired.sum())
    return state, side


def same(a, b):
    return (a[0] == b[0]).all() and all(a[1][name].tobytes() == b[1][name].tobytes() for name in a[1])


@pytest.mark.parametrize("n_envs,slots,k,count,capacity,tail", [
    (130, 8, 21, 40, 1000, 0), (130, 8, 21, 60, 37, 0), (130, 8, 21, 90, 16, 0), (130, 8, 21, 40, 1000, 3), (130, 8, 3, 30, 64, 0),
    (5, 3, 2, 8, 4, 1), (7, 16, 100, 70, 50, 5), (64, 4, 0, 10, 8, 0)])
def test_model_equals_its_restatement(n_envs, slots, k, count, capacity, tail):
    rng = np.random.RandomState(n_envs * 1000 + k)
    ring = ref.planted(n_envs, slots, seed=k)
    for step_base in (0, 5):
        recs = random_log(rng, n_envs, slots, k, count, step_base)
        state = np.zeros(8, np.int64)
        state[1] = 30
        args = (ring, k, recs, count, count + 3, capacity, tail, step_base)
        a, b = ref.harvest(state, ref.empty_region(capacity), *args), restated(state, ref.empty_region(capacity), *args)
        assert same(a, b), (a[0], b[0])
        assert a[0][0] == count and (a[0][5:] == 0).all()
        p = rng.permutation(count)                                 # the log's order does not show
        assert same(a, ref.harvest(state, ref.empty_region(capacity), ring, k, {n: v[p] for n, v in recs.items()}, *args[3:]))
        # a second harvest of the same log finds nothing: the mark is at the window's end
        again = ref.harvest(a[0], a[1], *args)
        assert same(a, again)
        # the capacity of the log cuts the window
        cut = ref.harvest(state, ref.empty_region(capacity), ring, k, recs, count, count // 2, capacity, tail, step_base)
        assert cut[0][0] == count // 2 and same(cut, restated(state, ref.empty_region(capacity), ring, k, recs, count, count // 2,
                                                                capacity, tail, step_base))


def test_model_on_a_hand_made_log():
    # slots 8, k = 21: W = 7, intact steps 14 .. 20
    recs = dict(lane=np.array([2, 0, 2, 1, 3], np.int32), end_step=np.array([20, 14, 16, 13, 18], np.int64),
                len=np.array([3, 9, 2, 2, 30], np.int32), success=np.array([1, 1, 1, 1, 0], np.uint8))
    episodes, tot = ref.plan(0, recs, 5, 8, 21, 4, 8)
    assert episodes == [(14, 0, 14, 1), (16, 2, 15, 2), (20, 2, 18, 3)]
    assert tot == dict(m=5, rows=6, episodes=3, rows_cut=8, expired=1)
    episodes, tot = ref.plan(0, recs, 5, 8, 21, 4, 8, tail=1)
    assert [e[2:] for e in episodes] == [(14, 1), (16, 1), (20, 1)] and tot["rows_cut"] == 0
    ring = ref.planted(4, 8)
    state, side = ref.harvest(np.zeros(8, np.int64), ref.empty_region(4), ring, 21, recs, 5, 8, 4)
    assert state.tolist() == [5, 6, 3, 8, 1, 0, 0, 0]
    # rows 2 .. 5 of the six are kept, at side rows 2, 3, 0, 1: steps 16 | 18, 19, 20 of lane 2
    for at, j in ((2, 16), (3, 18), (0, 19), (1, 20)):
        assert (side["obs"][at] == ring["obs"][j % 8, 2]).all() and (side["obs2"][at] == ring["obs"][(j + 1) % 8, 2]).all()
        assert side["act"][at] == ring["act"][j % 8, 2] and side["done"][at] == ring["done"][j % 8, 2]


# ------------------------------------------------------------------------------------------------------------- the option
def test_success_replay_validates_its_fields_and_round_trips():
    from ddpg_trucktrailer_amd.options import CHECKPOINT_KEYS, _tupled, compare_options, write_options
    from ddpg_trucktrailer_amd.success_replay import SuccessReplay as S, summary
    s = S(64)
    assert (s.capacity, s.every, s.tail) == (64, 32, 0) and s.as_tuple() == (64, 32, 0)
    for args, kw, word in (((0,), {}, "capacity"), ((1.5,), {}, "capacity"), ((True,), {}, "capacity"), ((2 ** 31,), {}, "capacity"),
                           ((64,), dict(every=0), "every"), ((64,), dict(tail=-1), "tail"), ((64,), dict(tail=2.0), "tail")):
        with pytest.raises(ValueError, match=word):
            S(*args, **kw)
    t = S(1000, every=4, tail=3)
    assert S.from_tuple(t.as_tuple()) == t and hash(S.from_tuple(t.as_tuple())) == hash(t) and t != s
    assert repr(t) == "SuccessReplay(capacity=1000, every=4, tail=3)"
    assert "success_replay" in CHECKPOINT_KEYS and CHECKPOINT_KEYS[-2:] == ("task_curriculum", "randomize")
    assert CHECKPOINT_KEYS.index("success_replay") == len(CHECKPOINT_KEYS) - 3        # behind every key a test does not pin to the end
    sd = write_options({}, success_replay=t)
    assert sd == {"success_replay": [1000, 4, 3]}
    assert S.from_tuple(_tupled(json.loads(json.dumps(sd))["success_replay"])) == t
    compare_options(sd, success_replay=t)
    with pytest.raises(ValueError, match="written with success_replay = None"):
        compare_options({}, success_replay=t)
    with pytest.raises(ValueError, match="this loop has success_replay = None"):
        compare_options(sd, success_replay=None)
    line = summary(dict(episodes=3, rows=17, rows_cut=2, expired=1, exposed=16))
    assert line == "success replay: 3 episodes, 17 rows harvested, 16 in the draw, 2 rows cut, 1 episodes expired"


def test_every_refusal_row_has_its_wording():
    from ddpg_trucktrailer_amd.options import TABLE
    from ddpg_trucktrailer_amd.success_replay import SuccessReplay, check_success_replay
    s = SuccessReplay(64)
    assert check_success_replay(s, episode_log=16) is s and check_success_replay(s, episode_log=16, device="cuda:0") is s
    with pytest.raises(ValueError, match="success_replay = 64 is not a SuccessReplay"):
        check_success_replay(64, episode_log=16)
    rows = {
        "episode_log": (dict(episode_log=None), "success replay without episode_log is not supported: the harvest reads the episode "
                                                "log's records (DDPGRollout(episode_log=...))"),
        "td3": (dict(td3=object()), "success replay with td3 is not supported (the TD3 draw refuses side buffers)"),
        "n_step": (dict(n_step=3), "success replay with n_step = 3 is not supported: side tuples are single steps, and the ring "
                                   "refuses them in an n-step draw"),
        "population": (dict(population=True), "success replay in a population is not supported (a population's agents have rings of "
                                              "their own, and a harvest per agent is not built)"),
        "data_parallel": (dict(data_parallel=True), "success replay with data-parallel ranks (or the p2p exchange) is not supported"),
        "force_dp": (dict(force_dp=True), "success replay with the data-parallel launch structure (TT_FORCE_DP) is not supported"),
        "expert": (dict(expert=object()), "success replay with expert lanes is not supported (the expert's lanes are demonstrations "
                                          "already, and their successes would be harvested as the agent's)"),
        "labels": (dict(labels=object()), "success replay with expert labels is not supported (the side region's rows carry no label)"),
        "device": (dict(device="cpu"), "success replay on device = 'cpu' is not supported: the harvest exists only as HIP kernels"),
    }
    names = [row if isinstance(row, str) else row[0] for row in TABLE["success_replay"]["rows"]]
    assert names == list(rows)                   # every row, in the table's order
    for name, (kw, message) in rows.items():
        with pytest.raises(ValueError) as e:
            check_success_replay(s, **{"episode_log": 16, **kw})
        assert str(e.value) == message, name
    order = list(rows)                           # the first row that applies speaks
    for a in range(len(order) - 1):
        with pytest.raises(ValueError) as e:
            check_success_replay(s, **{"episode_log": 16, **rows[order[a]][0], **rows[order[a + 1]][0]})
        assert str(e.value) == rows[order[a]][1]
    assert list(TABLE)[-1] == "success_replay"   # a part of its own, behind the others: no existing row moved


def test_loops_refuse_through_the_table(monkeypatch):
    from cpu_env import CpuEnv
    from ddpg_trucktrailer_amd.population import PopulationRollout
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.success_replay import SuccessReplay
    from ddpg_trucktrailer_amd.td3 import TD3Config
    s = SuccessReplay(64)
    kw = dict(batch_size=4, replay_slots=8, use_graph=False)
    with pytest.raises(ValueError, match="success replay without episode_log"):
        PopulationRollout(4, seeds=[1, 2], success_replay=s)
    with pytest.raises(ValueError, match="success replay in a population is not supported"):
        PopulationRollout(4, seeds=[1, 2], success_replay=s, episode_log=16)
    with pytest.raises(ValueError, match="success replay without episode_log"):
        DDPGRollout(CpuEnv(), success_replay=s, **kw)
    with pytest.raises(ValueError, match="success replay with td3"):
        DDPGRollout(CpuEnv(), success_replay=s, episode_log=16, td3=TD3Config(), updates_per_step=2, **kw)
    with pytest.raises(ValueError, match="success replay with n_step = 2"):
        DDPGRollout(CpuEnv(), success_replay=s, episode_log=16, n_step=2, **kw)
    with pytest.raises(ValueError, match="success replay on device = device\\(type='cpu'\\)"):
        DDPGRollout(CpuEnv(), success_replay=s, episode_log=16, **kw)
    with pytest.raises(ValueError, match="is not a SuccessReplay"):
        DDPGRollout(CpuEnv(), success_replay=64, episode_log=16, **kw)
    monkeypatch.setenv("TT_FORCE_DP", "1")
    with pytest.raises(ValueError, match="success replay with the data-parallel launch structure"):
        DDPGRollout(CpuEnv(), success_replay=s, episode_log=16, **kw)


def test_a_plain_loop_carries_nothing_of_the_option():
    from cpu_env import CpuEnv
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.stepper import VectorStepper
    loop = DDPGRollout(CpuEnv(), batch_size=4, replay_slots=8, use_graph=False)
    sd = loop.state_dict()
    assert loop.success_replay is None and "success_replay" not in sd and "harvest" not in sd["ring"]
    assert loop.ring.side is None and loop.ring.harvest is None
    st = VectorStepper(CpuEnv(), batch_size=4, replay_slots=8)
    assert "success_replay" not in st.acting_state() and len(st.graph_key()) == 4
    st.vector_steps = 5
    assert st.curriculum_room(9) == 9 and st.success_replay_tick() is None
    with pytest.raises(ValueError, match="success replay is off"):
        st.success_replay_stats()


# ------------------------------------------------------------------------------------------------------------- the ring
def test_ring_region_lies_behind_loaded_demonstrations():
    from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing
    ring = TrajectoryRing(4, 8, 23, "cpu")
    demo = np.arange(3 * 23, dtype=np.float32).reshape(3, 23)
    ring.load_side(demo, [1, 2, 3], [4, 5, 6], demo + 1, [0, 1, 0], capacity=5)
    epoch = ring.side_epoch
    hv = ring.enable_success_replay(10)
    assert (hv["base"], hv["capacity"]) == (3, 10) and hv["state"].tolist() == [0] * 8
    assert ring.side["obs"].shape == (13, 23) and ring.side["done"].shape == (13,) and ring.side_count == 3
    assert (ring.side["obs"][:3].numpy() == demo).all() and ring.side["act"][:3].tolist() == [1, 2, 3] and ring.side_epoch == epoch + 1
    with pytest.raises(ValueError, match="load_side after enable_success_replay is not supported"):
        ring.load_side(demo, [1, 2, 3], [4, 5, 6], demo, [0, 0, 0])
    with pytest.raises(ValueError, match="already enabled"):
        ring.enable_success_replay(4)
    # the exposed count follows the written rows up to the capacity; the epoch moves only while it does
    assert ring.expose_successes(0) == 0 and ring.side_epoch == epoch + 1
    assert ring.expose_successes(7) == 7 and ring.side_count == 10 and ring.side_epoch == epoch + 2
    assert ring.expose_successes(7) == 7 and ring.side_epoch == epoch + 2
    assert ring.expose_successes(25) == 10 and ring.side_count == 13 and ring.side_epoch == epoch + 3
    assert ring.expose_successes(400) == 10 and ring.side_epoch == epoch + 3
    h = ring.harvest_struct(record_capacity=16, tail=2, step_base=7)
    assert h.obs == ring.side["obs"].data_ptr() + 3 * 23 * 4 and h.done == ring.side["done"].data_ptr() + 3
    assert (h.capacity, h.tail, h.step_base) == (10, 2, 7) and ring.harvest["work"].shape == (16,)


def test_ring_state_dict_round_trip_and_refusal():
    from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing
    a = TrajectoryRing(4, 8, 23, "cpu")
    a.enable_success_replay(6)
    a.side["obs"][2] = 5.0
    a.harvest["state"][:5] = torch.tensor([2, 9, 3, 1, 4])
    a.expose_successes(9)
    sd = a.state_dict()
    assert sd["harvest"]["base"] == 0 and sd["harvest"]["capacity"] == 6 and sd["harvest"]["exposed"] == 6 and sd["side_count"] == 6
    b = TrajectoryRing(4, 8, 23, "cpu")
    b.enable_success_replay(6)
    b.load_state_dict(sd)
    assert b.harvest["state"].tolist() == [2, 9, 3, 1, 4, 0, 0, 0] and b.side_count == 6 and (b.side["obs"][2] == 5.0).all()
    plain = TrajectoryRing(4, 8, 23, "cpu")
    with pytest.raises(ValueError, match="success-replay region \\(base, capacity\\) is None and the checkpoint's ring has \\(0, 6\\)"):
        plain.load_state_dict(sd)
    c = TrajectoryRing(4, 8, 23, "cpu")
    c.enable_success_replay(7)
    with pytest.raises(ValueError, match="is \\(0, 7\\) and the checkpoint's ring has \\(0, 6\\)"):
        c.load_state_dict(sd)
    with pytest.raises(ValueError, match="is \\(0, 7\\) and the checkpoint's ring has None"):
        c.load_state_dict(plain.state_dict())


# ------------------------------------------------------------------------------------------------------------- the library
NAMES = ("tt_ring_harvest", "tt_env_harvest")


def test_header_exports_and_struct_layout_agree(lib):
    header = open(os.path.join(ROOT, "include", "ttenv.h")).read()
    dll = lib.load()
    for n in NAMES:
        assert n in lib.EXPORTS and hasattr(dll, n), n
        assert re.search(r"\bint " + n + r"\(", header), n
    m = re.search(r"typedef struct tt_harvest \{(.*?)\} tt_harvest;", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"\*?(\w+)\s*[,;]", body)
    assert fields == ["state", "obs", "act", "rew", "obs2", "done", "capacity", "tail", "step_base", "work"]
    assert [f[0] for f in lib.TTHarvest._fields_] == fields
    H = lib.TTHarvest
    assert C.sizeof(H) == 6 * 8 + 2 * 4 + 8 + 8
    assert (H.state.offset, H.done.offset, H.capacity.offset, H.tail.offset, H.step_base.offset, H.work.offset) == (0, 40, 48, 52, 56, 64)
    assert lib.HARVEST_STATE == ref.STATE
    assert re.search(r"#define TT_VERSION 3\b", header)            # the state blob's layout did not change
    src = open(os.path.join(ROOT, "ddpg-trucktrailer_amd", "csrc", "ttenv_harvest.h")).read()
    assert "float" not in re.sub(r"(const )?float \*", "", re.sub(r"//.*", "", src))      # integer arithmetic only: floats are copied


def test_arguments_are_refused_before_any_hip_call(lib):
    dll = lib.load()
    X = 0x1000                          # never read: the refusals below come before any launch

    def refused(fn="tt_ring_harvest", capacity=8, tail=0, record_capacity=16, slots=8, n_envs=4, null=None):
        h = lib.TTHarvest(X, X, X, X, X, X, capacity, tail, 0, X)
        view = lib.TTRingView(None, X, X, X, X, n_envs, slots)
        cols = [X, X, X, X, X]
        if null in ("state", "obs", "act", "rew", "obs2", "done", "work"):
            setattr(h, null, None)
        if null in ("ring.obs", "ring.act", "ring.rew", "ring.done"):
            setattr(view, null[5:], None)
        if isinstance(null, int):
            cols[null] = None
        hp, vp, kp = (None if null == "h" else C.byref(h)), (None if null == "ring" else C.byref(view)), (None if null == "k_dev" else X)
        assert dll.tt_ring_harvest(hp, vp, kp, *cols, record_capacity, None) == lib.TT_EINVAL
        return dll.tt_last_error(None).decode()

    for null in ("h", "ring", "k_dev"):
        assert refused(null=null) == "tt_ring_harvest: h, ring and k_dev are required"
    for null in ("state", "obs", "act", "rew", "obs2", "done", "work"):
        assert "tt_ring_harvest: a NULL pointer in tt_harvest" in refused(null=null), null
    for null in ("ring.obs", "ring.act", "ring.rew", "ring.done"):
        assert "tt_ring_harvest: a NULL pointer in the ring view" in refused(null=null), null
    for null in range(5):
        assert "tt_ring_harvest: a NULL record column" in refused(null=null), null
    assert "tt_ring_harvest: capacity = 0 is below 1 or tail = 0 is negative" in refused(capacity=0)
    assert "capacity = 8 is below 1 or tail = -1 is negative" in refused(tail=-1)
    assert "tt_ring_harvest: record_capacity = 0 is below 1" in refused(record_capacity=0)
    assert "tt_ring_harvest: a ring of 2 slots and 4 envs" in refused(slots=2)
    assert "a ring of 8 slots and 0 envs" in refused(n_envs=0)
    assert "record_capacity = 400000000 with 8 slots: work[] holds 32-bit row counts" in refused(record_capacity=400000000)
    assert dll.tt_env_harvest(None, None, None, None, None) == lib.TT_EINVAL
    assert b"tt_env_harvest: NULL handle" in dll.tt_last_error(None)


def test_new_kernels_resources(lib):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    ks = kr.kernels()
    # LDS: the plan's tile of 256 (key, rows) pairs, its totals and the workgroup's votes, under 4 KiB; the copy has none
    for name, lds in (("14k_harvest_planE", 4096), ("14k_harvest_copyE", 0)):
        found = kr.find(ks, name)
        assert len(found) == 1, (name, sorted(found))
        v = next(iter(found.values()))
        assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (name, v)
        assert (256 * 12 <= v["lds"] <= lds if lds else v["lds"] == 0) and v["max_threads"] == 256 and kr.waves_per_simd(v["vgpr"]) == 8, (name, v)
    # every kernel of the golden tables keeps its row
    for table in ("kernel_resources_main.json", "kernel_resources_step_log.json"):
        before = json.load(open(os.path.join(GOLDEN, table)))
        moved = {n: (v, ks[n]) for n, v in before.items() if n in ks and ks[n] != v}
        assert not moved, moved
        assert all(n in ks for n in before)


# ------------------------------------------------------------------------------------------------------------- the pose pool
def test_pose_pool_ends_in_success_within_8_steps_whatever_the_steering():
    """What tests/test_gpu_success_replay.py's loop test relies on: from every pose of the pool the episode ends in success (the final
    bonus is paid) after at most 8 steps under constant steering -1, 0, +1 (times pi / 4) and one fixed random sequence -- so the loop's
    policy, whatever it does, produces successful episodes shorter than its ring's window."""
    from ddpg_trucktrailer_amd import _lib as L
    from oracle import c_oracle
    final = L.INFO_ROWS.index("final_success_bonus")
    high = np.float32(np.pi / 4)
    sequences = [np.full(8, c, np.float32) * high for c in (-1.0, 0.0, 1.0)]
    sequences.append(np.random.RandomState(41).uniform(-1, 1, 8).astype(np.float32) * high)
    m = len(ref.POSE_POOL)
    for actions in sequences:
        ora = c_oracle.COracle(m)
        ora.place(ref.POSE_POOL)
        ended, success, steps = np.zeros(m, bool), np.zeros(m, bool), np.zeros(m, int)
        for t in range(8):
            _, _, done, info = ora.step(np.full(m, actions[t], np.float32))
            fresh = done & ~ended
            success |= fresh & (info[:, final] > 0)
            steps[fresh] = t + 1
            ended |= done
        assert ended.all() and success.all(), (actions, ended, success)
        assert steps.max() <= 8 and steps.min() >= 1
