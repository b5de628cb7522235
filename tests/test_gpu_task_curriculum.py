"""GPU (-m gpu): the task curriculum on the device (include/ttenv.h: tt_env_set_task_curriculum; csrc/ttenv_task.h: k_step_task,
k_step_task_log, k_reset_task) against the host model tests/task_curriculum_ref.py, against a plain randomised
env and against an env placed with set_pose.

Sizes: N = 130 (one ragged workgroup), 300 (two workgroups, counts from both) and 1; bins (3, 2, 2, 2) and (8, 8, 8, 8) = 4096 cells.
Everything is compared bit for bit: cells and counters are integers, and goals, lengths and success rates are f64 formed with one
rounding per operation on both sides.  The env of most tests is the counting test's of tests/test_gpu_curriculum.py -- a reset box
around the goal -- with goals drawn from a small box around the default goal, so that episodes are short and end both ways."""
import ctypes as C
import math

import numpy as np
import pytest

import randomize_ref
import task_curriculum_ref as ref
from test_curriculum_cpu import COUNT_HI, COUNT_LO, COUNT_MAX_STEPS

pytestmark = pytest.mark.gpu

BINS = [(3, 2, 2, 2), (8, 8, 8, 8)]
GOAL = ((-0.3, -30.2, math.pi / 2 - 0.1), (0.3, -29.6, math.pi / 2 + 0.1))        # around the default goal (0, -30, pi / 2)
L2 = (6.0, 8.0)
WIDE_GOAL = ((-10.0, -32.0, 1.3), (10.0, -28.0, 1.8))                               # tests/test_gpu_randomize.py's ranges
WIDE_L2 = (5.0, 10.0)


def _env(n, device, max_steps=COUNT_MAX_STEPS, extra_steps=None, lo=COUNT_LO, hi=COUNT_HI):
    from ddpg_trucktrailer_amd import _lib as L
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    p = L.default_params(0)
    if lo is not None:
        p.reset_lo, p.reset_hi = (C.c_double * 3)(*lo), (C.c_double * 3)(*hi)
    p.fixed_max_steps = max_steps
    if extra_steps is not None:
        p.extra_steps = extra_steps
    return TruckTrailerVecEnv(n, device=device, params=p)


def _rand(goal=GOAL, l2=L2):
    from ddpg_trucktrailer_amd.randomize import EpisodeRandomization
    return EpisodeRandomization(goal=goal, L2=l2)


def _task(bins, **kw):
    from ddpg_trucktrailer_amd.task_curriculum import TaskCurriculum
    return TaskCurriculum(bins, **kw)


def _on(env, bins, rand=None, place=None, **kw):
    env.enable_randomization(rand if rand is not None else _rand())
    env.enable_task_curriculum(_task(bins, **kw), place=place)
    return env


def _model(env):
    r = env.randomization_ranges()
    return (r.goal_lo, r.goal_hi, r.L2_lo, r.L2_hi)


def _skewed(cells, seed=1):
    """Planted weights: most cells at 1, a few at 65536, a few in between; (q, cum) as the model forms the scan."""
    rng = np.random.RandomState(seed)
    q = np.ones(cells, dtype=np.int64)
    q[rng.choice(cells, max(1, cells // 6), replace=False)] = rng.randint(2, 5000, max(1, cells // 6))
    q[rng.choice(cells, max(1, cells // 6), replace=False)] = 65536
    assert (q == 1).any() and (q == 65536).any()
    return q.astype(np.uint32), np.cumsum(q).astype(np.uint32)


def _plant(env, **arrays):
    env.load_task_curriculum_state({k: np.asarray(v).astype(np.int64) if k == "seen" else
                                    (np.asarray(v, dtype=np.float64) if k == "p" else np.asarray(v).astype(np.uint32).view(np.int32))
                                    for k, v in arrays.items()})


def _state(env):
    """task_curriculum_state() as flat numpy arrays with the unsigned views back."""
    s = {k: v.cpu().numpy().reshape(-1) for k, v in env.task_curriculum_state().items()}
    for k in ("attempts", "successes", "q", "cum", "cell"):
        s[k] = s[k].view(np.uint32)
    s["seen"] = s["seen"].view(np.uint64)
    return s


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and (a == b).all()


def _ep(env):
    return {k: v.cpu().numpy() for k, v in env.episode().items()}


# ================================================================================================================ the draw
@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("n", [130, 1])
def test_draw_gives_the_models_cell_goal_and_length(gpu_device, n, bins):
    """Episodes of int(|goal - start| / step_length) + 1 steps (extra_steps = 1, no fixed length): one to seven, so max_episode_steps is
    the drawn goal's at every reset and the lanes' episode numbers spread.  Under planted weights that hold 1 and 65536."""
    import torch
    env, plain = _env(n, gpu_device, max_steps=0, extra_steps=1), _env(n, gpu_device, max_steps=1)
    _on(env, bins)
    shaped = env.task_curriculum_state()
    assert shaped["p"].shape == (bins[3], bins[2], bins[1], bins[0]) and shaped["cell"].shape == (n,)
    fresh = _state(env)
    assert (fresh["p"] == 0.5).all() and len(set(fresh["q"].tolist())) == 1 and (fresh["cell"] == ref.NO_CELL).all()
    assert (fresh["cum"] == np.cumsum(fresh["q"].astype(np.int64))).all() and not fresh["seen"].any()
    cells = env.task_curriculum.cells
    q, cum = _skewed(cells)
    _plant(env, q=q, cum=cum)
    lanes, seed = np.arange(n), 27
    episode = np.zeros(n, dtype=np.int64)
    # a plain env's start poses of the same seed, per episode number: episodes of one step, so step k leaves every lane in episode k + 1
    plain.reset(seed=seed)
    plain_start = [_ep(plain)["start"]]
    for _ in range(3 * 8 + 2):
        assert bool(plain.step_random(policy_seed=5)[2].all())
        plain_start.append(_ep(plain)["start"])
    plain_start = np.stack(plain_start)
    assert len({tuple(r) for r in plain_start[:, 0].tolist()}) == len(plain_start)

    def check(what):
        c, goal, l2 = ref.draw(seed, lanes, episode, cum, bins, _model(env))
        e = _ep(env)
        assert (_state(env)["cell"] == c.astype(np.uint32)).all(), what
        assert _same_bits(e["goal"], goal) and _same_bits(e["L2"], l2), what
        assert _same_bits(e["start"], plain_start[episode, lanes]), what         # counter word 0 keeps its words
        want = randomize_ref.max_steps(e["start"], goal, env.params.step_length, 1)
        assert (e["max_episode_steps"] == want).all(), what
        return c, want

    env.reset(seed=seed)
    c, want = check("reset")
    assert n == 1 or (len(set(want.tolist())) > 2 and len(set(c.tolist())) > 2)
    assert (q[c] > 1).mean() > 0.9                                      # the heavy cells are the ones drawn
    steps = 0
    while episode.min() < 2:        # auto-resets up to episode 2 (the host follows the done flags)
        _, _, done, _ = env.step_random(policy_seed=5)
        episode += done.cpu().numpy().astype(np.int64)
        steps += 1
        assert steps <= 3 * 8
        check(f"auto-reset, episodes {episode.min()}..{episode.max()}")
    # the masked reset moves the chosen lanes on by one episode, the same draw
    mask = (lanes % 3 == 0)
    env.reset(seed=seed, mask=torch.from_numpy(mask.astype(np.uint8)))
    episode += mask
    check("masked reset")
    # set_pose and set_state: the lanes they touch have no cell, the others keep theirs
    before = _state(env)["cell"].copy()
    idx = np.array([0] if n == 1 else [1, 64, 129], dtype=np.int32)
    env.set_pose(np.tile([0.0, -29.0, math.pi / 2], (len(idx), 1)), idx=torch.from_numpy(idx))
    after = _state(env)["cell"]
    assert (after[idx] == ref.NO_CELL).all() and (np.delete(after, idx) == np.delete(before, idx)).all()
    if n > 1:
        env.set_state(np.tile([1.5, 1.5, 0.0, 17.0, 0.0, 10.0], (1, 1)), idx=torch.tensor([5], dtype=torch.int32))
        assert _state(env)["cell"][5] == ref.NO_CELL
    env.close(); plain.close()


# ================================================================================================================ one bin is plain
def test_one_bin_is_plain_randomisation_bit_for_bit(gpu_device):
    """A (1, 1, 1, 1) env against a randomised env that never had the option, through two auto-resets of every lane (episodes of three
    steps, seven steps): every state word, observation, reward, done flag and info column."""
    import torch
    n = 130
    a, b = _env(n, gpu_device, lo=None), _env(n, gpu_device, lo=None)
    _on(a, (1, 1, 1, 1), rand=_rand(WIDE_GOAL, WIDE_L2))
    b.enable_randomization(_rand(WIDE_GOAL, WIDE_L2))
    assert torch.equal(a.reset(seed=11), b.reset(seed=11)) and torch.equal(a.state, b.state)
    resets = 0
    for k in range(7):
        act = a.random_actions(seed=5, step=k)
        oa, ra, da, ia = a.step(act, auto_reset=True, info=True)
        oa, ra, da, ia = oa.clone(), ra.clone(), da.clone(), {key: v.clone() for key, v in ia.items()}
        ob, rb, db, ib = b.step(act, auto_reset=True, info=True)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), k
        assert torch.equal(ia["flags"], ib["flags"]) and torch.equal(ia["violation"], ib["violation"]), k
        assert (_bits(ia["comp"]) == _bits(ib["comp"])).all(), k
        assert torch.equal(a.state, b.state), k
        ea, eb = a.episode(), b.episode()
        for key in ea:
            assert torch.equal(ea[key], eb[key]), (k, key)
        resets += int(da.sum())
    assert resets >= 2 * n
    s = _state(a)
    assert (s["cell"] == 0).all() and s["attempts"].tolist() == [resets]
    # ... and the random-policy step, with the log on
    a.enable_episode_log(1024); b.enable_episode_log(1024)
    for k in range(3):
        xa, xb = a.step_random(policy_seed=3), b.step_random(policy_seed=3)
        assert all(torch.equal(u, v) for u, v in zip(xa[:3], xb[:3])) and torch.equal(a.state, b.state), k
    a.close(); b.close()


# ================================================================================================================ a placed lane
@pytest.mark.parametrize("n", [130, 1])
def test_a_task_curriculum_lane_is_a_placed_lane(gpu_device, n):
    """tests/test_gpu_randomize.py's placed-lane test with the task curriculum on in env A: env B has no option and is placed with
    set_pose(start, goal, L2) from what A reports.  B steps with auto_reset on, for the reason DESIGN.md section 39 records (the
    plain kernels without auto-reset are no reference for bits)."""
    import torch
    a, b = _env(n, gpu_device, lo=None), _env(n, gpu_device, lo=None)
    _on(a, (3, 2, 2, 2), rand=_rand(WIDE_GOAL, WIDE_L2))
    q, cum = _skewed(24, seed=3)
    _plant(a, q=q, cum=cum)
    obs_a = a.reset(seed=11).clone()
    e = a.episode()
    obs_b = b.set_pose(e["start"], goal=e["goal"], L2=e["L2"]).clone()
    assert torch.equal(obs_a, obs_b)
    resets = 0
    for k in range(7):          # two whole rounds of three steps and one step more
        act = a.random_actions(seed=5, step=k)
        oa, ra, da, ia = a.step(act, auto_reset=True, info=True)
        oa, ra, da = oa.clone(), ra.clone(), da.clone()
        ia = {key: v.clone() for key, v in ia.items()}
        ob, rb, db, ib = b.step(act, auto_reset=True, info=True)
        assert torch.equal(ra, rb) and torch.equal(da, db), k
        assert torch.equal(ia["flags"], ib["flags"]) and torch.equal(ia["violation"], ib["violation"]), k
        assert (_bits(ia["comp"]) == _bits(ib["comp"])).all(), k
        live = ~da.bool()
        assert torch.equal(oa[live], ob[live]), k
        if da.any():
            idx = da.bool().nonzero().reshape(-1).to(torch.int32)
            e = a.episode()
            j = idx.long()
            placed = b.set_pose(e["start"][j], goal=e["goal"][j], L2=e["L2"][j], idx=idx, out=torch.zeros_like(ob))
            assert torch.equal(placed[j], oa[j]), k
            resets += int(da.sum())
        assert torch.equal(a.state, b.state), k
    assert resets >= 2 * n
    a.close(); b.close()


def test_a_lane_placed_from_outside_counts_nothing(gpu_device):
    import torch
    n = 130
    env = _on(_env(n, gpu_device), (3, 2, 2, 2))
    env.reset(seed=4)
    e = env.episode()
    env.set_pose(e["start"][5:6], goal=e["goal"][5:6], L2=e["L2"][5:6], idx=torch.tensor([5], dtype=torch.int32))
    assert _state(env)["cell"][5] == ref.NO_CELL and (np.delete(_state(env)["cell"], 5) < 24).all()
    finished = np.zeros(n, dtype=np.int64)
    for _ in range(COUNT_MAX_STEPS):        # every lane finishes exactly one episode within three steps?  the host counts
        finished += env.step_random(policy_seed=5)[2].cpu().numpy().astype(np.int64)
    s = _state(env)
    first = np.minimum(finished, 1)
    # lane 5's first episode counts nothing; every other finished episode counts once (a lane's later episodes are draws again)
    assert finished[5] >= 1 and int(s["attempts"].sum()) == int(finished.sum()) - 1 and first.all()
    assert s["cell"][5] < 24                                     # its next episode is a draw's again
    env.close()


# ================================================================================================================ counting
def _expected_counts(rec, seed, cum, bins, rand, cells):
    """attempts and successes per cell from the log's records (sorted by (end_step, lane)): a lane's j-th record is its episode j."""
    lane = rec["lane"].cpu().numpy().astype(np.int64)
    succ = rec["success"].cpu().numpy().astype(bool)
    ep = np.zeros(len(lane), dtype=np.int64)
    seen = {}
    for j, i in enumerate(lane):
        ep[j] = seen.get(int(i), 0)
        seen[int(i)] = ep[j] + 1
    cell, _, _ = ref.draw(seed, lane, ep, cum, bins, rand)
    return np.bincount(cell, minlength=cells), np.bincount(cell[succ], minlength=cells), len(lane), int(succ.sum())


@pytest.mark.parametrize("ring", [False, True], ids=["plain", "ring"])
@pytest.mark.parametrize("bins", BINS)
def test_counters_equal_the_logs_records(gpu_device, bins, ring):
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    n, seed, steps = 300, 9, 20
    env = _env(n, gpu_device)
    env.enable_episode_log(8192)
    _on(env, bins)
    cells = env.task_curriculum.cells
    q, cum = _skewed(cells, seed=2)
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
    want_a, want_s, total, wins = _expected_counts(rec, seed, cum, bins, _model(env), cells)
    got = _state(env)
    print(f"episodes {total}, successes {wins}")
    assert rec["dropped"] == 0 and total >= n * (steps // COUNT_MAX_STEPS) and 0 < wins < total, (total, wins)      # both outcomes occurred
    assert (got["attempts"] == want_a).all() and (got["successes"] == want_s).all()
    assert int(got["attempts"].sum()) == total and int(got["successes"].sum()) == wins
    lanes = rec["lane"].cpu().numpy()
    assert (lanes < 256).any() and (lanes >= 256).any()                    # counts from both workgroups
    assert not got["seen"].any() and (got["q"] == q).all()                 # no update ran
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
    for bins, n in (((8, 8, 8, 8), 130), ((3, 2, 2, 2), 1)):
        env = _on(_env(n, gpu_device), bins, mode=mode, alpha=alpha, uniform=uniform)
        p, att, suc, seen = _planted_cells(env.task_curriculum.cells, 7)
        _plant(env, p=p, attempts=att, successes=suc, seen=seen)
        env.task_curriculum_update()
        wp, wseen, wq, wcum = ref.update(p, seen, att, suc, mode, alpha, uniform)
        got = _state(env)
        assert _same_bits(got["p"], wp) and (got["seen"] == wseen).all()
        assert (got["q"] == wq).all() and (got["cum"] == wcum).all()
        assert not got["attempts"].any() and not got["successes"].any()
        env.close()


def test_update_inside_a_captured_graph_replayed_twice(gpu_device):
    import torch
    env = _on(_env(130, gpu_device), (8, 8, 8, 8), mode="frontier", alpha=0.1, uniform=0.1)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.task_curriculum_update()           # (warm-up: nothing counted, the weights are formed again)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        env.task_curriculum_update()
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
    """The task curriculum's arrays as caller-owned buffers between fences (tests/fenced.py): the enable, a reset, a masked reset,
    auto-resetting steps with the log on and off, set_pose and the update write nothing outside the stated extents -- and the arrays
    end with the bits a handle-owned task curriculum has."""
    import torch
    from fenced import Arena
    n, cells = 130, bins[0] * bins[1] * bins[2] * bins[3]
    npad = (n + 63) // 64 * 64
    results = []
    for fenced in (True, False):
        env = _env(n, gpu_device)
        place = arena = None
        if fenced:
            arena = Arena(gpu_device)
            kw = dict(full=True, also_input=True)
            place = dict(p=arena.out("p", cells, torch.float64, **kw), seen=arena.out("seen", cells, torch.int64, **kw),
                         attempts=arena.out("attempts", cells, torch.int32, **kw), successes=arena.out("successes", cells, torch.int32, **kw),
                         q=arena.out("q", cells, torch.int32, **kw), cum=arena.out("cum", cells, torch.int32, **kw),
                         cell=arena.out("cell", npad, torch.int32, **kw))
        _on(env, bins, place=place, every=4, alpha=0.5)
        if fenced:
            arena.assert_clean("enable")
            assert (place["cell"] == -1).all()
        env.reset(seed=3)
        for k in range(8):
            if k == 4:
                env.enable_episode_log(1024)
            env.step_random(policy_seed=7)
            if k % 4 == 3:
                env.task_curriculum_update()
        env.reset(seed=3, mask=(torch.arange(n, device=gpu_device) % 2).to(torch.uint8))
        env.set_pose(np.array([[0.0, -29.0, math.pi / 2]]), idx=torch.tensor([n - 1], dtype=torch.int32))
        env.step_random(policy_seed=7)
        env.task_curriculum_update()
        torch.cuda.synchronize()
        if fenced:
            arena.assert_clean("reset, steps, update")
            assert (place["cell"][n:] == -1).all()            # the padding lanes never draw
        s = _state(env)
        assert s["seen"].sum() > 0 and (s["cell"][:n - 1] != ref.NO_CELL).all() and (s["cell"][:n - 1] < cells).all()
        results.append(s)
        env.close()
    for k in results[0]:
        assert (results[0][k] == results[1][k]).all() if k != "p" else _same_bits(results[0][k], results[1][k]), k


# ================================================================================================================ the reset pool
POOL = [[-20.0, 5.0, 1.0], [-10.0, 20.0, 1.4], [0.0, 12.0, 1.6], [12.5, 25.0, 2.0], [25.0, 3.0, 0.9]]      # (far from every goal)


def test_the_reset_pool_works_in_both_orders(gpu_device):
    """tests/test_gpu_randomize.py's pool test with the task curriculum on: an env that set the pool BEFORE enabling and one that set
    it AFTER start, at reset() and at every auto-reset, where a plain env with the same pool and seed starts, on rows of the pool;
    cells, goals and lengths stay the model's.  After set_reset_pool(None) the starts are the box's again."""
    import torch
    n, seed, bins = 130, 27, (3, 2, 2, 2)
    lanes = np.arange(n)
    pool = torch.tensor(POOL, dtype=torch.float64)
    before, after, plain = (_env(n, gpu_device, max_steps=2) for _ in range(3))
    before.set_reset_pool(pool)
    _on(before, bins)
    _on(after, bins)
    after.set_reset_pool(pool)
    plain.set_reset_pool(pool)
    q, cum = _skewed(24, seed=5)
    for env in (before, after):
        _plant(env, q=q, cum=cum)
    envs = [before, after, plain]
    episode = np.zeros(n, dtype=np.int64)
    rows = {tuple(r) for r in POOL}

    def check(what, from_pool):
        want = _ep(plain)["start"]
        assert ({tuple(r) for r in want.tolist()} <= rows) == from_pool, what
        c, goal, l2 = ref.draw(seed, lanes, episode, cum, bins, _model(before))
        for name, env in zip(("pool before enable", "pool after enable"), envs[:2]):
            e = _ep(env)
            assert _same_bits(e["start"], want), (what, name)
            assert _same_bits(e["goal"], goal) and _same_bits(e["L2"], l2), (what, name)
            assert (_state(env)["cell"] == c.astype(np.uint32)).all(), (what, name)

    def step():     # episodes of exactly two steps in all three envs (fixed_max_steps = 2, and no lane reaches its goal in one)
        dones = [env.step_random(policy_seed=5)[2].cpu().numpy().astype(np.int64) for env in envs]
        return dones

    for env in envs:
        env.reset(seed=seed)
    check("reset", True)
    for k in range(4):
        dones = step()
        if not all((d == dones[0]).all() for d in dones):       # (an early end in some env: the episode numbers part ways)
            pytest.fail(f"the envs' episodes ended at different steps at step {k}")
        episode += dones[0]
        check(f"auto-reset, episodes {episode.min()}..{episode.max()}", True)
    assert episode.min() >= 1
    for env in envs:
        env.set_reset_pool(None)
    for env in envs:
        env.reset(seed=seed + 1)
    episode[:] = 0
    seed += 1
    check("pool cleared, reset", False)
    for env in envs:
        env.set_reset_pool(pool)
    for env in envs:
        env.reset(seed=seed)
    check("pool set again", True)
    for env in envs:
        env.close()


# ================================================================================================================ the loop
def _loop(device, seed=27, task="default", randomize="default", **kw):
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    env = _env(130, device)
    env.reset(seed=seed)
    if randomize == "default":
        randomize = _rand()
    if task == "default":
        task = _task((3, 2, 2, 2), every=4, alpha=0.5)
    return DDPGRollout(env, batch_size=64, replay_slots=16, seed=seed, randomize=randomize, task_curriculum=task, **kw)


def _flat(loop):
    import torch
    return torch.cat([p.detach().reshape(-1) for net in loop.agent._nets() for p in net.parameters()])


def _assert_same_loop(a, b, task=True):
    import torch
    torch.cuda.synchronize()
    assert torch.equal(_flat(a), _flat(b))
    for name in ("obs", "act", "rew", "done"):
        assert torch.equal(getattr(a.ring, name), getattr(b.ring, name)), name
    assert torch.equal(a.noise.x, b.noise.x) and torch.equal(a.env.state, b.env.state)
    ea, eb = a.env.episode(), b.env.episode()
    for key in ("steps", "max_episode_steps", "start", "goal", "L2"):
        assert torch.equal(ea[key], eb[key]), key
    if task:
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
    assert a.graph_steps == 4 and b.graph_steps == 0 and a.env.task_curriculum == _task((3, 2, 2, 2), every=4, alpha=0.5)
    assert a.graph_key()[-2:] == (_rand().as_tuple(), a.task_curriculum.as_tuple())
    # episode 0 is a draw of the fresh task curriculum: every lane has a cell, and the goals are the model's under equal weights
    fresh_q, fresh_cum = ref.weights(np.full(24, 0.5), "frontier", 0.1)
    c, goal, l2 = ref.draw(27, np.arange(130), np.zeros(130, dtype=np.int64), fresh_cum, (3, 2, 2, 2), _model(a.env))
    assert (_state(a.env)["cell"] == c.astype(np.uint32)).all() and _same_bits(a.env.episode()["goal"], goal)
    a.run(steps)
    for _ in range(steps):
        b.step()
    s = _assert_same_loop(a, b)
    # two updates ran (after steps 4 and 8), the episodes since wait in the counters, and the weights moved off the fresh ones
    assert s["seen"].sum() > 0 and s["attempts"].sum() > 0 and len(set(s["q"].tolist())) > 1
    sd = a.state_dict()
    assert (s["p"] != 0.5).any() and "task_curriculum" in sd and "task_curriculum" in sd["env"] and "randomize" in sd["env"]
    # save at step 5 (between two updates: counters are part of the state), resume in a fresh loop with another seed
    c_ = _loop(gpu_device, graph_steps=4, **_td3(td3))
    c_.run(5)
    path = checkpoint.save_loop_checkpoint(str(tmp_path / "loop.pt"), c_)
    d = _loop(gpu_device, seed=99, graph_steps=4, **_td3(td3))
    d.run(6)
    checkpoint.load_loop_checkpoint(path, d)
    assert d.vector_steps == 5
    d.run(steps - 5)
    _assert_same_loop(a, d)
    # a loop without the option refuses the file
    e = _loop(gpu_device, task=None, graph_steps=0, **_td3(td3))
    with pytest.raises(ValueError, match="task_curriculum"):
        checkpoint.load_loop_checkpoint(path, e)
    for lp in (a, b, c_, d, e):
        lp.env.close()


# ================================================================================================================ off and refusals
def test_off_is_off(gpu_device):
    """After disabling, the env equals a randomised env that never had the option: the loop continues bit for bit."""
    a, b = _loop(gpu_device, task=None, graph_steps=4), _loop(gpu_device, task=None, graph_steps=4)
    a.run(11)
    b.run(5)
    epoch = b.env.graph_epoch
    b.env.enable_task_curriculum(_task((3, 2, 2, 2), every=4))
    assert b.env.lib.tt_env_task_curriculum(b.env._h, None) == 1
    b.env.disable_task_curriculum()
    assert b.env.graph_epoch == epoch + 2 and b.env.task_curriculum is None and "task_curriculum" not in b.env.state_dict()
    assert b.env.lib.tt_env_task_curriculum(b.env._h, None) == 0 and b.env.randomization == _rand()
    b.run(6)
    _assert_same_loop(a, b, task=False)
    with pytest.raises(RuntimeError, match="task curriculum is off"):
        b.env.task_curriculum_update()
    a.env.close(); b.env.close()


def test_library_refusals_that_read_the_handle(gpu_device):
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    from ddpg_trucktrailer_amd.curriculum import Curriculum
    env = _env(4, gpu_device)
    lib, h, st = env.lib, env._h, L.stream(env.device)
    cfg = _task((3, 2, 2, 2)).c_struct()

    def refused(rc, words):
        assert rc == L.TT_EINVAL
        for who in (h, None):                       # fail_both: the handle's message and the library's
            assert words in lib.tt_last_error(who).decode(), lib.tt_last_error(who)

    def usable():
        env.reset(seed=1)
        _, _, done, _ = env.step_random(policy_seed=3)
        torch.cuda.synchronize()
        assert done.shape == (4,) and torch.isfinite(env.obs).all()

    # randomisation not on
    refused(lib.tt_env_set_task_curriculum(h, C.byref(cfg), None, st), "there is no range to put cells on")
    with pytest.raises(ValueError, match="a task curriculum without randomize is not supported: there is no range to put cells on"):
        env.enable_task_curriculum(_task((3, 2, 2, 2)))
    assert lib.tt_env_task_curriculum(h, None) == 0
    refused(lib.tt_env_task_curriculum_update(h, st), "the task curriculum is off")
    arrays = L.TTCurriculumArrays()
    refused(lib.tt_env_task_curriculum_read(h, C.byref(arrays), st), "the task curriculum is off")
    refused(lib.tt_env_task_curriculum_write(h, C.byref(arrays), st), "the task curriculum is off")
    usable()
    # more than one bin on a range of width 0: a None of the option resolved against the parameters
    env.enable_randomization(_rand(goal=None))
    refused(lib.tt_env_set_task_curriculum(h, C.byref(cfg), None, st), "3 bins on the goal x range, which has width 0")
    with pytest.raises(ValueError, match="3 bins on the goal_x range"):
        env.enable_task_curriculum(_task((3, 2, 2, 2)))
    env.enable_task_curriculum(_task((1, 1, 1, 4)))             # one bin there is fine
    out = L.TTTaskCurriculum()
    assert lib.tt_env_task_curriculum(h, C.byref(out)) == 1 and (tuple(out.bins), out.mode, out.alpha) == ((1, 1, 1, 4), 0, 0.1)
    usable()
    # while it is on, randomisation stays as it is
    rnd = _rand().c_struct(env.params)
    refused(lib.tt_env_set_randomization(h, C.byref(rnd), st), "turn the task curriculum off first")
    refused(lib.tt_env_set_randomization(h, None, st), "turn the task curriculum off first")
    with pytest.raises(L.TTError, match="turn the task curriculum off first"):
        env.disable_randomization()
    assert env.randomization == _rand(goal=None)
    # what randomisation refuses is refused with it
    refused(lib.tt_env_set_episode_log2(h, 64, L.LOG_DETAIL, st), "the detailed episode log with episode randomisation is not supported")
    cur = Curriculum((3, 2, 2)).c_struct()
    refused(lib.tt_env_set_curriculum(h, C.byref(cur), None, st), "a curriculum with episode randomisation is not supported")
    refused(lib.tt_env_rollout_random(h, 3, 7, None, None, None, st), "episode randomisation does not follow k_rollout")
    env.set_reset_pool(torch.tensor([[0.0, -29.0, 1.5]], dtype=torch.float64))      # a reset pool stays allowed
    usable()
    env.set_reset_pool(None)
    env.enable_episode_log(64)                                  # the plain log composes
    usable()
    env.disable_task_curriculum()
    env.disable_randomization()
    usable()
    env.close()
