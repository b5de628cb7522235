"""GPU (-m gpu): the start-pose curriculum on the device (include/ttenv.h: tt_env_set_curriculum; csrc/ttenv_curriculum.h: k_step_cur,
k_step_cur_log, k_reset_curriculum, k_curriculum_update) against the host model tests/curriculum_ref.py.

Sizes: N = 130 (two tiles and a ragged tail) and N = 1; bins (3, 2, 2) and (16, 16, 16).  Everything is compared bit for bit: cells and
counters are integers, and the poses and success rates are f64 formed with one rounding per operation on both sides."""
import ctypes as C
import math

import numpy as np
import pytest

import curriculum_ref as ref
from test_curriculum_cpu import COUNT_HI, COUNT_LO, COUNT_MAX_STEPS

pytestmark = pytest.mark.gpu

BINS = [(3, 2, 2), (16, 16, 16)]


def _env(n, device, lo=None, hi=None, max_steps=0):
    from ddpg_trucktrailer_amd import _lib as L
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    p = L.default_params(0)
    if lo is not None:
        p.reset_lo, p.reset_hi = (C.c_double * 3)(*lo), (C.c_double * 3)(*hi)
    p.fixed_max_steps = max_steps
    return TruckTrailerVecEnv(n, device=device, params=p)


def _box(env):
    return tuple(env.params.reset_lo), tuple(env.params.reset_hi)


def _skewed(cells, seed=1):
    """Planted weights: most cells at 1, a few at 65536, a few in between; (q, cum) as the model forms the scan."""
    rng = np.random.RandomState(seed)
    q = np.ones(cells, dtype=np.int64)
    q[rng.choice(cells, max(1, cells // 6), replace=False)] = 65536
    q[rng.choice(cells, max(1, cells // 6), replace=False)] = rng.randint(2, 5000, max(1, cells // 6))
    return q.astype(np.uint32), np.cumsum(q).astype(np.uint32)


def _plant(env, **arrays):
    env.load_curriculum_state({k: np.asarray(v).astype(np.int64) if k == "seen" else
                               (np.asarray(v, dtype=np.float64) if k == "p" else np.asarray(v).astype(np.uint32).view(np.int32))
                               for k, v in arrays.items()})


def _state(env):
    """curriculum_state() as numpy with the unsigned views back."""
    s = {k: v.cpu().numpy().reshape(-1) for k, v in env.curriculum_state().items()}
    for k in ("attempts", "successes", "q", "cum", "cell"):
        s[k] = s[k].view(np.uint32)
    s["seen"] = s["seen"].view(np.uint64)
    return s


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and (a.view(np.uint64) == b.view(np.uint64)).all()


# ================================================================================================================ the draw
@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("n", [130, 1])
def test_draw_gives_the_models_cell_and_pose(gpu_device, n, bins):
    import torch
    from ddpg_trucktrailer_amd.curriculum import Curriculum
    env = _env(n, gpu_device, max_steps=2)
    lo, hi = _box(env)
    env.enable_curriculum(Curriculum(bins))
    fresh = _state(env)
    assert (fresh["p"] == 0.5).all() and len(set(fresh["q"].tolist())) == 1 and (fresh["cell"] == ref.NO_CELL).all()
    assert (fresh["cum"] == np.cumsum(fresh["q"].astype(np.int64))).all() and not fresh["seen"].any()
    q, cum = _skewed(env.curriculum.cells)
    _plant(env, q=q, cum=cum)
    lanes, seed = np.arange(n), 27
    episode = np.zeros(n, dtype=np.int64)

    def check(what):
        cells, pose = ref.draw(seed, lanes, episode, cum, bins, lo, hi)
        assert (_state(env)["cell"] == cells.astype(np.uint32)).all(), what
        assert _same_bits(env.episode()["start"].cpu().numpy(), pose), what

    env.reset(seed=seed)
    check("reset")
    # auto-resets up to episode 2 (episodes of two steps; the host follows the done flags)
    while episode.min() < 2:
        _, _, done, _ = env.step_random(policy_seed=5)
        episode += done.cpu().numpy().astype(np.int64)
        check(f"auto-reset, episodes {episode.min()}..{episode.max()}")
    assert len(set(_state(env)["cell"].tolist())) > (1 if n > 1 else 0)
    # the masked reset moves the chosen lanes on by one episode, the same draw
    mask = (lanes % 3 == 0)
    env.reset(seed=seed, mask=torch.from_numpy(mask.astype(np.uint8)))
    episode += mask
    check("masked reset")
    # set_pose and set_state: the lanes they touch have no cell, the others keep theirs
    before = _state(env)["cell"].copy()
    idx = np.array([0] if n == 1 else [1, 64, 129], dtype=np.int32)
    env.set_pose(np.tile([0.0, 10.0, math.pi / 2], (len(idx), 1)), idx=torch.from_numpy(idx))
    after = _state(env)["cell"]
    assert (after[idx] == ref.NO_CELL).all() and (np.delete(after, idx) == np.delete(before, idx)).all()
    if n > 1:
        env.set_state(np.tile([1.5, 1.5, 0.0, 17.0, 0.0, 10.0], (1, 1)), idx=torch.tensor([5], dtype=torch.int32))
        assert _state(env)["cell"][5] == ref.NO_CELL
    env.close()


# ================================================================================================================ counting
def _expected_counts(rec, seed, cum, bins, lo, hi, cells):
    """attempts and successes per cell from the log's records (sorted by (end_step, lane)): a lane's j-th record is its episode j."""
    lane = rec["lane"].cpu().numpy().astype(np.int64)
    succ = rec["success"].cpu().numpy().astype(bool)
    ep = np.zeros(len(lane), dtype=np.int64)
    seen = {}
    for j, i in enumerate(lane):
        ep[j] = seen.get(int(i), 0)
        seen[int(i)] = ep[j] + 1
    cell, _ = ref.draw(seed, lane, ep, cum, bins, lo, hi)
    return np.bincount(cell, minlength=cells), np.bincount(cell[succ], minlength=cells), len(lane), int(succ.sum())


@pytest.mark.parametrize("ring", [False, True], ids=["plain", "ring"])
@pytest.mark.parametrize("bins", BINS)
def test_counters_equal_the_logs_records(gpu_device, bins, ring):
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    from ddpg_trucktrailer_amd.curriculum import Curriculum
    n, seed, steps = 130, 9, 20
    env = _env(n, gpu_device, COUNT_LO, COUNT_HI, COUNT_MAX_STEPS)
    env.enable_episode_log(4096)
    env.enable_curriculum(Curriculum(bins))
    q, cum = _skewed(env.curriculum.cells, seed=2)
    _plant(env, q=q, cum=cum)
    env.reset(seed=seed)
    if not ring:
        for _ in range(steps):
            env.step_random(policy_seed=5)
    else:       # tt_env_step_ring: obs / reward / done addressed through a device cursor
        slots = 4
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=gpu_device)
        bufs = dict(obs=z(slots, n, 23), act=z(slots, n), rew=z(slots, n), done=z(slots, n, dt=torch.uint8))
        cursor = torch.zeros(32, dtype=torch.int32, device=gpu_device)
        view = L.TTRingView(cursor.data_ptr(), bufs["obs"].data_ptr(), bufs["act"].data_ptr(), bufs["rew"].data_ptr(),
                            bufs["done"].data_ptr(), n, slots)
        for k in range(steps):
            cursor[:4] = torch.tensor([k % slots, (k + 1) % slots, (k - 1) % slots, int(k > 0)], dtype=torch.int32)
            env.step_ring(env.random_actions(5, k), view)
        assert bufs["done"].any() and bufs["obs"].abs().sum() > 0          # (the ring's rows were written)
    rec = env.drain_episodes()
    want_a, want_s, total, wins = _expected_counts(rec, seed, cum, bins, *_box(env), env.curriculum.cells)
    got = _state(env)
    assert rec["dropped"] == 0 and total >= n * (steps // COUNT_MAX_STEPS) and 0 < wins < total, (total, wins)
    assert (got["attempts"] == want_a).all() and (got["successes"] == want_s).all()
    assert int(got["attempts"].sum()) == total and int(got["successes"].sum()) == wins
    assert not got["seen"].any() and (got["q"] == q).all()           # no update ran
    env.close()


# ================================================================================================================ the update
def _planted_cells(cells, seed):
    rng = np.random.RandomState(seed)
    p = rng.uniform(0, 1, cells)
    p[:3] = (0.0, 0.5, 1.0)[:min(3, cells)]
    att = rng.randint(0, 200, cells).astype(np.uint32)
    att[rng.choice(cells, max(1, cells // 4), replace=False)] = 0
    att[-1] = 3000000000             # (a count past 2^31: the counters are unsigned)
    suc = (att * rng.uniform(0, 1, cells)).astype(np.uint32)
    seen = rng.randint(0, 2 ** 40, cells).astype(np.uint64)
    return p, att, suc, seen


@pytest.mark.parametrize("uniform", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("alpha", [0.1, 1.0])
@pytest.mark.parametrize("mode", ref.MODES)
def test_update_equals_the_model(gpu_device, mode, alpha, uniform):
    from ddpg_trucktrailer_amd.curriculum import Curriculum
    for bins, n in (((16, 16, 16), 130), ((3, 2, 2), 1)):
        env = _env(n, gpu_device)
        env.enable_curriculum(Curriculum(bins, mode=mode, alpha=alpha, uniform=uniform))
        p, att, suc, seen = _planted_cells(env.curriculum.cells, 7)
        _plant(env, p=p, attempts=att, successes=suc, seen=seen)
        env.curriculum_update()
        wp, wseen, wq, wcum = ref.update(p, seen, att, suc, mode, alpha, uniform)
        got = _state(env)
        assert _same_bits(got["p"], wp) and (got["seen"] == wseen).all()
        assert (got["q"] == wq).all() and (got["cum"] == wcum).all()
        assert not got["attempts"].any() and not got["successes"].any()
        env.close()


def test_update_inside_a_captured_graph_replayed_twice(gpu_device):
    import torch
    from ddpg_trucktrailer_amd.curriculum import Curriculum
    bins = (16, 16, 16)
    env = _env(130, gpu_device)
    env.enable_curriculum(Curriculum(bins, mode="frontier", alpha=0.1, uniform=0.1))
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.curriculum_update()           # (warm-up: nothing counted, the weights are formed again)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        env.curriculum_update()
    p, att, suc, seen = _planted_cells(4096, 8)
    _plant(env, p=p, attempts=att, successes=suc, seen=seen)
    for round_ in range(2):
        g.replay()
        p, seen, wq, wcum = ref.update(p, seen, att, suc, "frontier", 0.1, 0.1)
        got = _state(env)
        assert _same_bits(got["p"], p) and (got["seen"] == seen).all() and (got["q"] == wq).all() and (got["cum"] == wcum).all()
        assert not got["attempts"].any() and not got["successes"].any()
        _, att, suc, _ = _planted_cells(4096, 9 + round_)
        _plant(env, attempts=att, successes=suc)
    env.close()


# ================================================================================================================ fences
@pytest.mark.parametrize("bins", BINS)
def test_every_array_between_fences(gpu_device, bins):
    """The curriculum's arrays as caller-owned buffers between fences (tests/fenced.py): the enable, a reset, a masked reset,
    auto-resetting steps with the log on and off, set_pose and the update write nothing outside the stated extents -- and the
    arrays end with the bits a handle-owned curriculum has."""
    import torch
    from ddpg_trucktrailer_amd.curriculum import Curriculum
    from fenced import Arena
    n, cells = 130, bins[0] * bins[1] * bins[2]
    npad = (n + 63) // 64 * 64
    results = []
    for fenced in (True, False):
        env = _env(n, gpu_device, COUNT_LO, COUNT_HI, COUNT_MAX_STEPS)
        place = arena = None
        if fenced:
            arena = Arena(gpu_device)
            kw = dict(full=True, also_input=True)
            place = dict(p=arena.out("p", cells, torch.float64, **kw), seen=arena.out("seen", cells, torch.int64, **kw),
                         attempts=arena.out("attempts", cells, torch.int32, **kw), successes=arena.out("successes", cells, torch.int32, **kw),
                         q=arena.out("q", cells, torch.int32, **kw), cum=arena.out("cum", cells, torch.int32, **kw),
                         cell=arena.out("cell", npad, torch.int32, **kw))
        env.enable_curriculum(Curriculum(bins, every=4, alpha=0.5), place=place)
        if fenced:
            arena.assert_clean("enable")
            assert (place["cell"] == -1).all()
        env.reset(seed=3)
        for k in range(8):
            if k == 4:
                env.enable_episode_log(1024)
            env.step_random(policy_seed=7)
            if k % 4 == 3:
                env.curriculum_update()
        env.reset(seed=3, mask=(torch.arange(n, device=gpu_device) % 2).to(torch.uint8))
        env.set_pose(np.array([[0.0, -29.0, math.pi / 2]]), idx=torch.tensor([n - 1], dtype=torch.int32))
        env.step_random(policy_seed=7)
        env.curriculum_update()
        torch.cuda.synchronize()
        if fenced:
            arena.assert_clean("reset, steps, update")
            assert (place["cell"][n:] == -1).all()            # the padding lanes never draw
        s = _state(env)
        assert s["seen"].sum() > 0 and (s["cell"][:n - 1] != ref.NO_CELL).all()
        results.append(s)
        env.close()
    for k in results[0]:
        assert (results[0][k] == results[1][k]).all() if k != "p" else _same_bits(results[0][k], results[1][k]), k


# ================================================================================================================ the loop
def _loop(device, seed=27, curriculum="default", **kw):
    from ddpg_trucktrailer_amd.curriculum import Curriculum
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    env = _env(130, device, COUNT_LO, COUNT_HI, COUNT_MAX_STEPS)
    env.reset(seed=seed)
    if curriculum == "default":
        curriculum = Curriculum((3, 2, 2), every=4, alpha=0.5)
    return DDPGRollout(env, batch_size=64, replay_slots=16, seed=seed, curriculum=curriculum, **kw)


def _flat(loop):
    import torch
    return torch.cat([p.detach().reshape(-1) for net in loop.agent._nets() for p in net.parameters()])


def _assert_same_loop(a, b, curriculum=True):
    import torch
    torch.cuda.synchronize()
    assert torch.equal(_flat(a), _flat(b))
    for name in ("obs", "act", "rew", "done"):
        assert torch.equal(getattr(a.ring, name), getattr(b.ring, name)), name
    assert torch.equal(a.noise.x, b.noise.x) and torch.equal(a.env.state, b.env.state)
    ea, eb = a.env.episode(), b.env.episode()
    assert torch.equal(ea["steps"], eb["steps"]) and torch.equal(ea["start"], eb["start"])
    if curriculum:
        sa, sb = _state(a.env), _state(b.env)
        for k in sa:
            assert (sa[k] == sb[k]).all() if k != "p" else _same_bits(sa[k], sb[k]), k
        return sa


def _td3(on):
    from ddpg_trucktrailer_amd.td3 import TD3Config
    return dict(td3=TD3Config(), updates_per_step=2) if on else {}        # (the delay is counted inside a vector step)


@pytest.mark.parametrize("td3", [False, True], ids=["ddpg", "td3"])
def test_graphs_and_eager_agree_and_a_resumed_run_continues(gpu_device, tmp_path, td3):
    from ddpg_trucktrailer_amd import checkpoint
    steps = 2 * 4 + 3
    a, b = _loop(gpu_device, graph_steps=4, **_td3(td3)), _loop(gpu_device, graph_steps=0, **_td3(td3))
    assert a.graph_steps == 4 and b.graph_steps == 0
    a.run(steps)
    for _ in range(steps):
        b.step()
    s = _assert_same_loop(a, b)
    # two updates ran (after steps 4 and 8), the episodes since wait in the counters, and the weights moved off the fresh ones
    assert s["seen"].sum() > 0 and s["attempts"].sum() > 0 and len(set(s["q"].tolist())) > 1
    assert (s["p"] != 0.5).any() and "curriculum" in a.state_dict() and "curriculum" in a.state_dict()["env"]
    # save at step 5 (between two updates: counters are part of the state), resume in a fresh loop
    c = _loop(gpu_device, graph_steps=4, **_td3(td3))
    c.run(5)
    path = checkpoint.save_loop_checkpoint(str(tmp_path / "loop.pt"), c)
    d = _loop(gpu_device, seed=99, graph_steps=4, **_td3(td3))
    d.run(6)
    checkpoint.load_loop_checkpoint(path, d)
    assert d.vector_steps == 5
    d.run(steps - 5)
    _assert_same_loop(a, d)
    # a loop without the option refuses the file, and the other way round
    e = _loop(gpu_device, curriculum=None, graph_steps=0, **_td3(td3))
    with pytest.raises(ValueError, match="curriculum"):
        checkpoint.load_loop_checkpoint(path, e)
    for lp in (a, b, c, d, e):
        lp.env.close()


def test_off_is_off(gpu_device):
    from ddpg_trucktrailer_amd.curriculum import Curriculum
    a, b = _loop(gpu_device, curriculum=None, graph_steps=4), _loop(gpu_device, curriculum=None, graph_steps=4)
    a.run(11)
    b.run(5)
    epoch = b.env.graph_epoch
    b.env.enable_curriculum(Curriculum((3, 2, 2), every=4))
    b.env.disable_curriculum()
    assert b.env.graph_epoch == epoch + 2 and b.env.curriculum is None and "curriculum" not in b.env.state_dict()
    b.run(6)
    _assert_same_loop(a, b, curriculum=False)
    with pytest.raises(RuntimeError, match="curriculum is off"):
        b.env.curriculum_update()
    a.env.close(); b.env.close()


def test_library_refusals_that_read_the_handle(gpu_device):
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    from ddpg_trucktrailer_amd.curriculum import Curriculum
    cur = Curriculum((3, 2, 2))
    env = _env(4, gpu_device)
    env.set_reset_pool(torch.tensor([[0.0, 10.0, 1.5]], dtype=torch.float64))
    with pytest.raises(L.TTError, match="a curriculum with a reset pool is not supported"):
        env.enable_curriculum(cur)
    env.set_reset_pool(None)
    env.enable_curriculum(cur)
    with pytest.raises(L.TTError, match="a reset pool with a curriculum is not supported"):
        env.set_reset_pool(torch.tensor([[0.0, 10.0, 1.5]], dtype=torch.float64))
    with pytest.raises(L.TTError, match="the detailed episode log with a curriculum is not supported"):
        env.enable_episode_log(64, detail=True)
    env.disable_curriculum()
    env.enable_episode_log(64, detail=True)
    with pytest.raises(ValueError, match="episode_log_detail"):
        env.enable_curriculum(cur)
    cfg = cur.c_struct()
    assert env.lib.tt_env_set_curriculum(env._h, C.byref(cfg), None, None) == L.TT_EINVAL
    assert b"a curriculum with the detailed episode log is not supported" in env.lib.tt_last_error(env._h)
    env.close()
    bad = _env(4, gpu_device, lo=(1.0, 0.0, 0.0), hi=(-1.0, 1.0, 1.0))
    with pytest.raises(L.TTError, match=r"reset_hi\[0\] < reset_lo\[0\]"):
        bad.enable_curriculum(cur)
    bad.close()
