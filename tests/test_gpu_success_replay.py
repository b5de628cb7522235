"""GPU (-m gpu): success replay on the device (include/ttenv.h: tt_ring_harvest, tt_env_harvest; csrc/ttenv_harvest.h:
k_harvest_plan, k_harvest_copy) against the host model tests/harvest_ref.py.

Base shape: N = 130 (two tiles and a ragged tail), slots = 8.  Every comparison is exact: the harvest copies bits and counts in
integers.  The loop test runs on the pose pool tests/test_success_replay_cpu.py has shown to end in success within 8 steps whatever
the policy does, and fails -- it does not skip -- if fewer than 4 episodes were harvested."""
import ctypes as C

import numpy as np
import pytest

import harvest_ref as ref

pytestmark = pytest.mark.gpu

N, SLOTS, K = 130, 8, 21
NAMES = ("obs", "act", "rew", "obs2", "done")


def planted_log():
    """40 records at k = 21 (W = 7: intact steps 14 .. 20), unique in (end_step, lane): what the issue lists, then filler."""
    rows = [  # lane, end_step, len, success
        (0, 17, 2, 1), (129, 19, 4, 1),                   # the first and the last lane
        (5, 15, 2, 1), (5, 19, 3, 1),                     # two successes of one lane
        (7, 16, 1, 1),                                    # len = 1
        (9, 20, 3, 1), (11, 14, 2, 1),                    # s = k - 1 and s = k - W (the second loses a row)
        (13, 12, 3, 1),                                   # an expired success
        (15, 18, 30, 1),                                  # an episode longer than the window
        (17, 18, 3, 0), (19, 20, 5, 0), (0, 15, 2, 0), (129, 14, 1, 0),      # failures
    ]
    rng = np.random.RandomState(3)
    used = {(r[1], r[0]) for r in rows}
    while len(rows) < 40:
        lane, s = int(rng.randint(N)), int(rng.randint(10, K))
        if (s, lane) not in used:
            used.add((s, lane))
            rows.append((lane, s, int(rng.randint(1, 12)), int(rng.rand() < 0.6)))
    a = np.array(rows)
    return dict(lane=a[:, 0].astype(np.int32), end_step=a[:, 1].astype(np.int64), len=a[:, 2].astype(np.int32),
                success=a[:, 3].astype(np.uint8))


class Planted:
    """Ring, record columns and a harvest's buffers on the device; `arena`: where the buffers the launches write come from."""

    def __init__(self, device, recs, record_capacity, capacity, k=K, n=N, slots=SLOTS, arena=None, ring=None):
        import torch
        import fenced
        from ddpg_trucktrailer_amd import _lib as L
        self.L, self.device, self.capacity, self.record_capacity, self.n, self.slots = L, device, capacity, record_capacity, n, slots
        self.ring = ring if ring is not None else ref.planted(n, slots, seed=1)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.ring_dev = {name: t(a) for name, a in self.ring.items()}
        pad = lambda a: np.concatenate([a, np.zeros(record_capacity - len(a), a.dtype)])
        self.recs_dev = {name: t(pad(a)) for name, a in recs.items()}
        self.k_dev = torch.tensor(k, dtype=torch.int64, device=device)
        self.written = torch.zeros(1, dtype=torch.int64, device=device)
        arena = arena if arena is not None else fenced.Plain(device)
        self.arena = arena
        region = ref.empty_region(capacity)
        self.side = {name: arena.inp("side_" + name, t(region[name])) for name in NAMES}
        self.state = arena.inp("state", torch.zeros(8, dtype=torch.int64, device=device))
        self.work = arena.out("work", record_capacity, dtype=torch.int32)

    def harvest(self, written, tail=0, step_base=0):
        import torch
        L = self.L
        self.written.fill_(written)
        p = lambda x: C.c_void_p(x.data_ptr())
        h = L.TTHarvest(*(self.side[name].data_ptr() if name != "state" else self.state.data_ptr()
                          for name in ("state",) + NAMES), self.capacity, tail, step_base, self.work.data_ptr())
        view = L.TTRingView(None, *(self.ring_dev[name].data_ptr() for name in ("obs", "act", "rew", "done")), self.n, self.slots)
        r = self.recs_dev
        L.check(L.load().tt_ring_harvest(C.byref(h), C.byref(view), p(self.k_dev), p(r["lane"]), p(r["end_step"]), p(r["len"]),
                                         p(r["success"]), p(self.written), self.record_capacity, L.stream(self.device)))
        torch.cuda.synchronize(self.device)
        return self.state.cpu().numpy().copy(), {name: self.side[name].cpu().numpy().copy() for name in NAMES}


def same(a, b):
    assert a[0].tolist() == b[0].tolist(), (a[0], b[0])
    for name in NAMES:
        assert a[1][name].tobytes() == b[1][name].tobytes(), name
    return True


def model(p, state, side, recs, written, tail=0, step_base=0, k=K):
    return ref.harvest(state, side, p.ring, k, recs, written, p.record_capacity, p.capacity, tail, step_base)


def test_planted_log_equals_the_model_in_any_order(gpu_device):
    recs = planted_log()
    episodes, tot = ref.plan(0, recs, 40, 64, K, N, SLOTS)
    assert tot["expired"] >= 1 and tot["rows_cut"] >= 24 and tot["episodes"] >= 9 and tot["rows"] < 1000
    assert {0, 129} <= {e[1] for e in episodes} and sum(e[1] == 5 for e in episodes) == 2
    assert {14, 20} <= {e[0] for e in episodes} and any(e[3] == 1 for e in episodes) and any(e[3] == 7 for e in episodes)
    p = Planted(gpu_device, recs, 64, 1000)
    got = p.harvest(40)
    want = model(p, np.zeros(8, np.int64), ref.empty_region(1000), recs, 40)
    assert same(got, want) and got[0][1] == tot["rows"] and got[0][0] == 40
    perm = np.random.RandomState(5).permutation(40)
    q = Planted(gpu_device, {name: a[perm] for name, a in recs.items()}, 64, 1000)
    assert same(q.harvest(40), got)
    # the same log once more: nothing new, nothing moves
    assert same(p.harvest(40), got)


def test_wrap_and_oversized_harvest(gpu_device):
    import torch
    recs = planted_log()
    _, tot = ref.plan(0, recs, 40, 64, K, N, SLOTS)
    assert tot["rows"] > 37                                        # both regions are smaller than the harvest
    for capacity, start in ((37, 30), (16, 0), (16, 5)):
        p = Planted(gpu_device, recs, 64, capacity)
        state = np.zeros(8, np.int64)
        state[1] = start
        p.state.copy_(torch.from_numpy(state))
        got = p.harvest(40)
        assert same(got, model(p, state, ref.empty_region(capacity), recs, 40))
        assert got[0][1] == start + tot["rows"] and all(got[1]["act"] != 0)      # every row of the region was written
    # a harvest smaller than the region that wraps: the first 6 records only, from written_rows = 30 of 37
    _, small = ref.plan(0, recs, 6, 64, K, N, SLOTS)
    assert 7 < small["rows"] < 37
    p = Planted(gpu_device, recs, 64, 37)
    state = np.zeros(8, np.int64)
    state[1] = 30
    p.state.copy_(torch.from_numpy(state))
    got = p.harvest(6)
    assert same(got, model(p, state, ref.empty_region(37), recs, 6)) and (got[1]["act"] == 0).sum() == 37 - small["rows"]


def test_tail_early_ring_and_the_mark(gpu_device):
    recs = planted_log()
    # tail = 3
    p = Planted(gpu_device, recs, 64, 1000)
    got = p.harvest(40, tail=3)
    assert same(got, model(p, np.zeros(8, np.int64), ref.empty_region(1000), recs, 40, tail=3))
    assert got[0][1] < ref.plan(0, recs, 40, 64, K, N, SLOTS)[1]["rows"]
    # step_base moves the records' steps: the same harvest from end_step - 4
    shifted = dict(recs, end_step=recs["end_step"] - 4)
    q = Planted(gpu_device, shifted, 64, 1000)
    assert same(q.harvest(40, tail=3, step_base=4), got)
    # k = 3: the window is bounded by k (steps 0 .. 2)
    early = dict(lane=np.array([0, 129, 4, 4, 6, 8], np.int32), end_step=np.array([0, 2, 1, 2, 3, 1], np.int64),
                 len=np.array([1, 3, 2, 1, 2, 9], np.int32), success=np.array([1, 1, 1, 1, 1, 0], np.uint8))
    e = Planted(gpu_device, early, 8, 64, k=3)
    got = e.harvest(6)
    assert same(got, model(e, np.zeros(8, np.int64), ref.empty_region(64), early, 6, k=3))
    assert got[0].tolist() == [6, 1 + 3 + 2 + 1, 4, 0, 0, 0, 0, 0]          # (the record of step 3 is not this ring's yet)
    # two calls with records appended between them: the mark moves; then the rewind a drain makes
    m = Planted(gpu_device, recs, 64, 1000)
    first = m.harvest(25)
    want = model(m, np.zeros(8, np.int64), ref.empty_region(1000), recs, 25)
    assert same(first, want) and first[0][0] == 25
    second = m.harvest(40)
    want = model(m, *want, recs, 40)
    assert same(second, want) and second[0][0] == 40
    stale = m.harvest(10)                                          # the log was emptied and refilled behind the harvest's back
    assert stale[0][0] == 10 and same(stale, model(m, *want, recs, 10)) and stale[0][1] == second[0][1]
    m.state[0] = 0                                                 # the rewind: records [0, 10) are new ones
    again = m.harvest(10)
    want = model(m, np.concatenate([[0], stale[0][1:]]), stale[1], recs, 10)
    assert same(again, want) and again[0][1] > second[0][1]


def test_a_long_log_over_several_workgroups_and_tiles(gpu_device):
    """600 records in a log of 700: three workgroups in the plan launch, three LDS tiles, a mark inside a tile, and the last
    workgroup's totals over all of them."""
    import torch
    from test_success_replay_cpu import random_log
    recs = random_log(np.random.RandomState(11), N, SLOTS, K, 600)
    for mark, capacity in ((0, 4000), (300, 4000), (517, 100)):
        p = Planted(gpu_device, recs, 700, capacity)
        state = np.zeros(8, np.int64)
        state[:2] = mark, 77
        p.state.copy_(torch.from_numpy(state))
        got = p.harvest(600)
        assert same(got, model(p, state, ref.empty_region(capacity), recs, 600)) and got[0][0] == 600
        assert got[0][2] >= 20, got[0]
    # a log written past its capacity: the window ends at the capacity
    p = Planted(gpu_device, {name: a[:300] for name, a in recs.items()}, 300, 4000)
    got = p.harvest(100000)
    assert same(got, model(p, np.zeros(8, np.int64), ref.empty_region(4000), recs, 100000)) and got[0][0] == 300


@pytest.mark.parametrize("surround", ["nan", "huge"])
def test_nothing_outside_the_region_work_and_state_is_written(gpu_device, surround):
    import fenced
    recs = planted_log()
    plain = Planted(gpu_device, recs, 40, 16)
    want = plain.harvest(40)
    arena = fenced.Arena(gpu_device, surround=surround)
    p = Planted(gpu_device, recs, 40, 16, arena=arena)             # a log filled to its capacity, a region smaller than the harvest
    got = p.harvest(40)
    arena.assert_clean("tt_ring_harvest")
    assert same(got, want) and same(got, model(p, np.zeros(8, np.int64), ref.empty_region(16), recs, 40))
    assert (p.work.cpu().numpy() == plain.work.cpu().numpy()).all() and (p.work.cpu().numpy() >= 0).all()
    ring_before = {name: a.clone() for name, a in p.ring_dev.items()}
    p.harvest(40, tail=2)
    arena.assert_clean("tt_ring_harvest, second call")
    for name, a in ring_before.items():
        assert (p.ring_dev[name] == a).all(), name


# ================================================================================================================ the live env
def _env(device, n=N):
    import torch
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    env = TruckTrailerVecEnv(n, device=device)
    env.set_reset_pool(torch.from_numpy(ref.POSE_POOL).to(device))
    env.reset(seed=27)
    return env


def _stepped(device, steps=12):
    """An env on the pose pool with the log on, stepped `steps` times into a ring under fixed actions."""
    import torch
    from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing
    env = _env(device)
    env.enable_episode_log(4096)
    ring = TrajectoryRing(N, SLOTS, 23, device)
    ring.attach(env)
    env.observe(out=ring.obs[0])
    action = torch.from_numpy(np.random.RandomState(8).uniform(-np.pi / 4, np.pi / 4, N).astype(np.float32)).to(device)
    for k in range(steps):
        ring.cursor_dev[0], ring.cursor_dev[1] = k % SLOTS, (k + 1) % SLOTS
        ring.act[k % SLOTS] = action
        env.step_ring(action, ring.view(), auto_reset=True)
        ring.advance()
    return env, ring


def test_live_env_harvest_equals_the_model_and_leaves_the_log_alone(gpu_device):
    import torch
    env, ring = _stepped(gpu_device)
    twin, _ = _stepped(gpu_device)
    ring.enable_success_replay(1000)
    env.harvest(ring.harvest_struct(env.episode_log_capacity), ring.view(), ring.k_dev)
    torch.cuda.synchronize()
    assert int(ring.k_dev.item()) == 12
    rec, rec_twin = env.drain_episodes(), twin.drain_episodes()
    for name in ("ret", "len", "flags", "success", "lane", "end_step"):
        assert torch.equal(rec[name], rec_twin[name]), name
    assert rec["written"] == rec_twin["written"] and rec["counts"] == rec_twin["counts"] and rec["dropped"] == 0
    recs = {name: rec[name].cpu().numpy() for name in ("lane", "end_step", "len")}
    recs["success"] = rec["success"].cpu().numpy().astype(np.uint8)
    host_ring = {name: getattr(ring, name).cpu().numpy() for name in ("obs", "act", "rew", "done")}
    want = ref.harvest(np.zeros(8, np.int64), ref.empty_region(1000), host_ring, 12, recs, rec["written"], 4096, 1000)
    got = (ring.harvest["state"].cpu().numpy(), {name: ring.side[name].cpu().numpy() for name in NAMES})
    assert same(got, want)
    # the pool makes every episode a success; some ended before the window and some reach out of it
    assert got[0][2] >= 4 and got[0][4] >= 1 and got[0][1] >= got[0][2] and int(rec["success"].sum()) == got[0][2] + got[0][4]
    done_rows = got[1]["done"][:got[0][1]]
    assert done_rows.sum() == got[0][2]                             # one done transition per harvested episode
    env.close(); twin.close()


def test_library_refusals_that_read_the_handle(gpu_device):
    from ddpg_trucktrailer_amd import _lib as L
    from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing
    env = _env(gpu_device)
    ring = TrajectoryRing(N, SLOTS, 23, gpu_device)
    ring.enable_success_replay(8)
    with pytest.raises(L.TTError, match="tt_env_harvest: the episode log is off"):
        env.harvest(ring.harvest_struct(16), ring.view(), ring.k_dev)
    env.enable_episode_log(16)
    other = TrajectoryRing(N + 1, SLOTS, 23, gpu_device)
    with pytest.raises(L.TTError, match="tt_env_harvest: the ring view has 131 envs, this handle 130"):
        env.harvest(ring.harvest_struct(16), other.view(), ring.k_dev)
    h = ring.harvest_struct(16)
    h.capacity = 0
    with pytest.raises(L.TTError, match="tt_env_harvest: capacity = 0 is below 1"):
        env.harvest(h, ring.view(), ring.k_dev)
    env.harvest(ring.harvest_struct(16), ring.view(), ring.k_dev)      # an empty log: nothing happens
    assert ring.harvest["state"].tolist() == [0] * 8
    env.close()


# ================================================================================================================ the loop
def _loop(device, seed=27, success_replay="default", **kw):
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.success_replay import SuccessReplay
    env = _env(device)
    if success_replay == "default":
        success_replay = SuccessReplay(capacity=64, every=4)
    return DDPGRollout(env, batch_size=32, replay_slots=16, seed=seed, episode_log=4096, demo_loss=DemoLoss(0.5),
                       success_replay=success_replay, **kw)


def _flat(loop):
    import torch
    return torch.cat([p.detach().reshape(-1) for net in loop.agent._nets() for p in net.parameters()])


def _assert_same_loop(a, b):
    import torch
    torch.cuda.synchronize()
    assert torch.equal(_flat(a), _flat(b))
    for name in ("obs", "act", "rew", "done"):
        assert torch.equal(getattr(a.ring, name), getattr(b.ring, name)), name
    assert torch.equal(a.noise.x, b.noise.x) and torch.equal(a.env.state, b.env.state)
    assert torch.equal(a.ring.harvest["state"], b.ring.harvest["state"])
    for name in NAMES:
        assert torch.equal(a.ring.side[name], b.ring.side[name]), name
    assert a.ring.side_count == b.ring.side_count


def test_graphs_and_eager_agree_and_a_resumed_run_continues(gpu_device, tmp_path):
    from ddpg_trucktrailer_amd import checkpoint
    a, b = _loop(gpu_device, graph_steps=4), _loop(gpu_device, graph_steps=0)
    assert a.graph_steps == 4 and b.graph_steps == 0 and a.ring.side_count == 0
    epoch = a.ring.side_epoch
    a.run(8)
    for _ in range(8):
        b.step()
    # nothing is in the draw until a drain (or the stats) exposes it
    assert a.ring.side_count == 0 and a.ring.side_epoch == epoch
    ra, rb = a.drain_episodes(), b.drain_episodes()
    assert ra["written"] == rb["written"] > 0 and int(a.ring.harvest["state"][0]) == 0
    assert a.ring.side_count > 0 and a.ring.side_epoch == epoch + 1
    a.run(9)
    for _ in range(9):
        b.step()
    _assert_same_loop(a, b)
    stats = a.success_replay_stats()
    assert stats == b.success_replay_stats()
    assert stats["episodes"] >= 4, stats                           # the test means something: episodes were harvested
    assert stats["exposed"] == 64 == a.ring.side_count and stats["rows"] > 64 and a.ring.side_epoch <= epoch + 2
    # the harvested rows are successes' transitions: one done row per episode that still lies in the region, each with the bonus
    done = a.ring.side["done"].bool()
    assert int(done.sum()) >= 4 and (a.ring.side["rew"][done] > 100).all()
    # a saved and resumed run equals the continuous one (saved between two harvests, behind a drain)
    c = _loop(gpu_device, graph_steps=4)
    c.run(8)
    c.drain_episodes()
    c.run(2)
    path = checkpoint.save_loop_checkpoint(str(tmp_path / "loop.pt"), c)
    d = _loop(gpu_device, seed=99, graph_steps=4)
    d.run(5)
    checkpoint.load_loop_checkpoint(path, d)
    assert d.vector_steps == 10 and d.ring.side_count == c.ring.side_count
    d.run(7)
    d.success_replay_stats()
    _assert_same_loop(a, d)
    # a loop without the option refuses the file; its ring has no side buffer at all
    e = _loop(gpu_device, success_replay=None, graph_steps=0)
    with pytest.raises(ValueError, match="success_replay"):
        checkpoint.load_loop_checkpoint(path, e)
    e.run(6)
    assert e.ring.side is None and e.ring.harvest is None and e.ring.side_count == 0
    for lp in (a, c, d, e):
        lp.env.close()
    # a later update clones harvested rows: 64 of about 1750 rows in the draw are the region's, 32 rows a batch
    seen = 0
    for _ in range(12):
        b.step()
        seen += int(b.demo_stats()["demo_rows"])
    assert seen > 0
    path2 = str(tmp_path / "successes.npz")
    assert b.export_successes(path2) == 64
    z = np.load(path2)
    assert z["obs"].shape == (64, 23) and z["act"].shape == (64, 1) and z["done"].dtype == np.bool_
    b.env.close()
