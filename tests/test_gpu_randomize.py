"""GPU (-m gpu): episode randomisation on the device (include/ttenv.h: tt_env_set_randomization; csrc/ttenv_randomize.h: k_step_rnd,
k_step_rnd_log, k_reset_rnd) against the host model tests/randomize_ref.py, against an env placed with
set_pose, and against the C oracle.

Sizes: N = 130 (two tiles and a ragged tail) and N = 1; episodes of two or three steps (fixed_max_steps), so that every lane
resets within a few steps.  Goals and lengths are compared bit for bit: f64 formed with one rounding per operation on both sides."""
import ctypes as C

import numpy as np
import pytest

import randomize_ref as ref

pytestmark = pytest.mark.gpu

GOAL = ((-10.0, -32.0, 1.3), (10.0, -28.0, 1.8))
L2 = (5.0, 10.0)
OBS_TOL = 1e-5          # tests/test_gpu_parity.py: TOL


def _env(n, device, max_steps=0):
    from ddpg_trucktrailer_amd import _lib as L
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    p = L.default_params(0)
    p.fixed_max_steps = max_steps
    return TruckTrailerVecEnv(n, device=device, params=p)


def _rand(goal=GOAL, l2=L2):
    from ddpg_trucktrailer_amd.randomize import EpisodeRandomization
    return EpisodeRandomization(goal=goal, L2=l2)


def _model(env):
    """The model's `rand` of what the env draws from: the resolved ranges, read back from the library."""
    r = env.randomization_ranges()
    return (r.goal_lo, r.goal_hi, r.L2_lo, r.L2_hi)


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and (a == b).all()


def _ep(env):
    return {k: v.cpu().numpy() for k, v in env.episode().items()}


# ================================================================================================================ the draw
@pytest.mark.parametrize("n", [130, 1])
def test_draw_equals_the_model_and_starts_are_a_plain_envs(gpu_device, n):
    import torch
    env, plain = _env(n, gpu_device, max_steps=2), _env(n, gpu_device, max_steps=2)
    env.enable_randomization(_rand())
    assert _model(env) == (GOAL[0], GOAL[1], L2[0], L2[1]) and plain.randomization_ranges() is None
    lanes, seed = np.arange(n), 27
    episode, episode_plain = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)

    def check(what):
        goal, l2 = ref.draw(seed, lanes, episode, _model(env))
        e = _ep(env)
        assert _same_bits(e["goal"], goal), what
        assert _same_bits(e["L2"], l2), what
        assert (episode == episode_plain).all(), what
        assert _same_bits(e["start"], _ep(plain)["start"]), what            # counter word 0 keeps its words

    env.reset(seed=seed)
    plain.reset(seed=seed)
    check("reset")
    assert n == 1 or len(set(_ep(env)["L2"].tolist())) == n
    # auto-resets up to episode 2 (episodes of two steps; the host follows the done flags of both envs)
    while episode.min() < 2:
        _, _, done, _ = env.step_random(policy_seed=5)
        _, _, done_plain, _ = plain.step_random(policy_seed=5)
        episode += done.cpu().numpy().astype(np.int64)
        episode_plain += done_plain.cpu().numpy().astype(np.int64)
        check(f"auto-reset, episodes {episode.min()}..{episode.max()}")
    assert episode.max() == 2
    # the masked reset moves the chosen lanes on by one episode, the same draw
    mask = (lanes % 3 == 0)
    m = torch.from_numpy(mask.astype(np.uint8))
    env.reset(seed=seed, mask=m)
    plain.reset(seed=seed, mask=m)
    episode += mask
    episode_plain += mask
    check("masked reset")
    # another seed, other draws; a full reset starts from episode 0 again
    env.reset(seed=seed + 1)
    goal, l2 = ref.draw(seed + 1, lanes, np.zeros(n, dtype=np.int64), _model(env))
    assert _same_bits(_ep(env)["goal"], goal) and _same_bits(_ep(env)["L2"], l2)
    env.close(); plain.close()


def test_max_steps_come_from_the_drawn_goal(gpu_device):
    n = 130
    env = _env(n, gpu_device, max_steps=0)
    env.enable_randomization(_rand(goal=((-30.0, -35.0, 1.0), (30.0, -5.0, 2.0))))
    env.reset(seed=3)
    e = _ep(env)
    want = ref.max_steps(e["start"], e["goal"], env.params.step_length, env.params.extra_steps)
    assert (e["max_episode_steps"] == want).all() and len(set(want.tolist())) > 10
    # ... and not from the parameters' goal
    default = ref.max_steps(e["start"], np.tile(np.array(tuple(env.params.goal)), (n, 1)), env.params.step_length, env.params.extra_steps)
    assert (want != default).any()
    env.close()


# ================================================================================================================ the reset pool
POOL = [[-20.0, 5.0, 1.0], [-10.0, 20.0, 1.4], [0.0, 12.0, 1.6], [12.5, 25.0, 2.0], [25.0, 3.0, 0.9]]


def test_the_reset_pool_works_with_randomisation_in_both_orders(gpu_device):
    """random_pose's pool branch in the randomised reset and step kernels, which read the pool from the descriptor's copy: an env that
    set the pool BEFORE enabling and one that set it AFTER start, at reset() and at every auto-reset, where a plain env with the same
    pool and seed starts, bit for bit, on rows of the pool; goal and L2 stay the model's.  A state dict carries both to a fresh env
    (re-enable, import, then the pool).  After set_reset_pool(None) the starts are the box's again."""
    import torch
    n, seed = 130, 27
    lanes = np.arange(n)
    pool = torch.tensor(POOL, dtype=torch.float64)
    before, after, plain = (_env(n, gpu_device, max_steps=2) for _ in range(3))
    before.set_reset_pool(pool)
    before.enable_randomization(_rand())
    after.enable_randomization(_rand())
    after.set_reset_pool(pool)
    plain.set_reset_pool(pool)
    envs = [before, after, plain]
    episode = np.zeros(n, dtype=np.int64)
    rows = {tuple(r) for r in POOL}

    def check(what, from_pool):
        want = _ep(plain)["start"]
        assert ({tuple(r) for r in want.tolist()} <= rows) == from_pool, what
        assert not from_pool or len({tuple(r) for r in want.tolist()}) == len(POOL), what
        goal, l2 = ref.draw(seed, lanes, episode, _model(before))
        for name, env in zip(("pool before enable", "pool after enable", "restored")[:len(envs) - 1], envs):
            if env is plain:
                continue
            e = _ep(env)
            assert _same_bits(e["start"], want), (what, name)
            assert _same_bits(e["goal"], goal) and _same_bits(e["L2"], l2), (what, name)

    def step():
        dones = [env.step_random(policy_seed=5)[2].cpu().numpy().astype(np.int64) for env in envs]
        assert all((d == dones[0]).all() for d in dones)
        return dones[0]

    for env in envs:
        env.reset(seed=seed)
    check("reset", True)
    while episode.min() < 2:        # episodes of two steps: auto-resets up to episode 2
        episode += step()
        check(f"auto-reset, episodes {episode.min()}..{episode.max()}", True)
    # a fresh env from the state dict: the option is re-enabled, the blob imported, the pool set behind them
    sd = before.state_dict()
    assert sd["pool"] is not None and "randomize" in sd
    restored = _env(n, gpu_device, max_steps=2)
    restored.load_state_dict(sd)
    assert restored.randomization == _rand()
    envs = [before, after, restored, plain]
    for _ in range(2):
        episode += step()
        check(f"after load_state_dict, episodes {episode.min()}..{episode.max()}", True)
    assert torch.equal(restored.state, before.state)
    # the pool cleared after enable: the box's starts again, at auto-resets and at a reset
    for env in envs:
        env.set_reset_pool(None)
    for _ in range(2):              # (one whole episode: every lane resets once, at the second step)
        episode += step()
    check(f"pool cleared, episodes {episode.min()}..{episode.max()}", False)
    for env in envs:
        env.reset(seed=seed + 1)
    episode[:] = 0
    seed += 1
    check("pool cleared, reset", False)
    lo, hi = tuple(plain.params.reset_lo), tuple(plain.params.reset_hi)
    start = _ep(before)["start"]
    assert all((start[:, d] >= lo[d]).all() and (start[:, d] <= hi[d]).all() for d in range(3))
    # ... and set again after enable
    for env in envs:
        env.set_reset_pool(pool)
    for _ in range(2):
        episode += step()
    check("pool set again", True)
    for env in envs:
        env.close()


# ================================================================================================================ a placed lane
@pytest.mark.parametrize("n", [130, 1])
def test_a_randomised_lane_is_a_placed_lane(gpu_device, n):
    """Env B has no randomisation and is placed with set_pose(start, goal, L2) from what env A reports; both are driven with the same
    actions.  Reward, done, flags and every info column agree bit for bit at every step, observations on every lane that is not done;
    a lane that A auto-resets is placed again in B from A's report -- and set_pose's observation is the auto-reset's, bit for bit.
    B steps with auto_reset on, as A does: the plain step kernel that the randomised one stands in for (B's own reset of a finished
    lane is overwritten by the placement).  The plain kernels without auto-reset are no reference for bits: they round psi2 of
    one lane in 130 one ulp apart from the plain kernels with it (recorded in profiles/randomize_twin_probe.txt by
    tools/randomize_twin_probe.py)."""
    import torch
    a, b = _env(n, gpu_device, max_steps=3), _env(n, gpu_device, max_steps=3)
    a.enable_randomization(_rand())
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
            placed = b.set_pose(e["start"][j], goal=e["goal"][j], L2=e["L2"][j], idx=idx,
                                out=torch.zeros_like(ob))
            assert torch.equal(placed[j], oa[j]), k
            resets += int(da.sum())
        assert torch.equal(a.state, b.state), k
    assert resets >= 2 * n
    a.close(); b.close()


# ================================================================================================================ oracle
def test_first_observation_against_the_c_oracle(gpu_device):
    from oracle import c_oracle
    n = 130
    env = _env(n, gpu_device, max_steps=3)
    env.enable_randomization(_rand())
    obs = env.reset(seed=19).cpu().numpy()
    e = _ep(env)
    ora = c_oracle.COracle(n)
    want = ora.place(e["start"], e["goal"], e["L2"])
    assert np.abs(obs - want).max() <= OBS_TOL
    for i in (0, 63, 64, 129):
        assert np.abs(obs[i] - ora.observe(i)).max() <= OBS_TOL
    # after the auto-reset of every lane (three steps) likewise
    for k in range(3):
        obs, _, done, _ = env.step(env.random_actions(seed=2, step=k))
    assert bool(done.all())
    e = _ep(env)
    want = c_oracle.COracle(n).place(e["start"], e["goal"], e["L2"])
    assert np.abs(obs.cpu().numpy() - want).max() <= OBS_TOL
    env.close()


# ================================================================================================================ ring and log
@pytest.mark.parametrize("ring", [False, True], ids=["plain", "ring"])
def test_log_records_equal_the_hosts_tally(gpu_device, ring):
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    n, seed, steps = 130, 9, 10
    env = _env(n, gpu_device, max_steps=3)
    env.enable_episode_log(4096)
    env.enable_randomization(_rand())
    env.reset(seed=seed)
    lanes = np.arange(n)
    episode, length = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    want = []           # (end_step, lane, episode, length) of every finished episode, in the drain's order
    if ring:            # tt_env_step_ring: obs / reward / done addressed through a device cursor
        slots = 4
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=gpu_device)
        bufs = dict(obs=z(slots, n, 23), act=z(slots, n), rew=z(slots, n), done=z(slots, n, dt=torch.uint8))
        cursor = torch.zeros(32, dtype=torch.int32, device=gpu_device)
        view = L.TTRingView(cursor.data_ptr(), bufs["obs"].data_ptr(), bufs["act"].data_ptr(), bufs["rew"].data_ptr(),
                            bufs["done"].data_ptr(), n, slots)
    for k in range(steps):
        if ring:
            cursor[:4] = torch.tensor([k % slots, (k + 1) % slots, (k - 1) % slots, int(k > 0)], dtype=torch.int32)
            env.step_ring(env.random_actions(5, k), view)
            done = bufs["done"][k % slots].cpu().numpy().astype(bool)
        else:
            done = env.step_random(policy_seed=5)[2].cpu().numpy().astype(bool)
        length += 1
        want += [(k, int(i), int(episode[i]), int(length[i])) for i in lanes[done]]
        episode += done
        length[done] = 0
        # the running episodes' goals and lengths are the model's at the host's episode numbers
        goal, l2 = ref.draw(seed, lanes, episode, _model(env))
        e = _ep(env)
        assert _same_bits(e["goal"], goal) and _same_bits(e["L2"], l2), k
    rec = env.drain_episodes()
    assert rec["dropped"] == 0 and rec["written"] == len(want) >= n * (steps // 3)
    assert rec["lane"].cpu().tolist() == [w[1] for w in want]
    assert rec["end_step"].cpu().tolist() == [w[0] for w in want]
    assert rec["len"].cpu().tolist() == [w[3] for w in want]
    # a lane's j-th record is its episode j: the episode number from the DRAINED records (the count of the lane's earlier records)
    # against the host's tally
    seen, got_episode = {}, []
    for lane in rec["lane"].cpu().tolist():
        got_episode.append(seen.get(lane, 0))
        seen[lane] = got_episode[-1] + 1
    assert got_episode == [w[2] for w in want]
    assert [seen.get(int(i), 0) for i in lanes] == episode.tolist()
    if ring:
        assert bufs["obs"].abs().sum() > 0 and bufs["rew"].abs().sum() > 0
    env.close()


# ================================================================================================================ fences
def test_every_array_between_fences(gpu_device):
    """Every array the randomised reset and step paths are handed, at N = 130, between fences (tests/fenced.py): nothing is written
    outside the stated extents, every element that is to be written is, and the values are those of a run on plain tensors."""
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    from fenced import Arena, Plain
    n = 130

    def run(alloc):
        dev = alloc.device
        env = _env(n, dev, max_steps=2)
        env.enable_randomization(_rand())
        h, lib, st, p = env._h, env.lib, L.stream(dev), L.ptr
        chk = lambda rc: L.check(rc, h)
        T = dict(tile_rows=256)
        soa = lambda rows, width=8: dict(tile_bytes=rows * 256 * width)
        f64, i32, u8 = torch.float64, torch.int32, torch.uint8
        lanes = torch.arange(n, device=dev)
        chk(lib.tt_env_reset(h, None, 11, p(alloc.out("reset.obs", (n, 23), **T)), st))
        mask = alloc.inp("mask", (lanes % 3 == 0).to(u8), **T)
        chk(lib.tt_env_reset(h, p(mask), 11, p(alloc.out("~reset_masked.obs", (n, 23), full=False, **T)), st))
        g = torch.Generator(device=dev).manual_seed(n)
        action = alloc.inp("action", (torch.rand(n, device=dev, generator=g) * 2 - 1) * 0.7, **T)

        def step(tag, log):
            if log:
                env.enable_episode_log(1024)
            for rep in range(2):            # episodes of two steps: the second step resets every lane
                o = dict(obs=alloc.out(f"{tag}{rep}.obs", (n, 23), **T), rew=alloc.out(f"{tag}{rep}.reward", (n,), **T),
                         done=alloc.out(f"{tag}{rep}.done", (n,), u8, **T),
                         comp=alloc.out(f"{tag}{rep}.comp", (L.NINFO, n), f64, **soa(L.NINFO)),
                         viol=alloc.out(f"{tag}{rep}.violation", (n,), u8, **T), flags=alloc.out(f"{tag}{rep}.flags", (n,), u8, **T))
                info = L.TTInfo(o["comp"].data_ptr(), o["viol"].data_ptr(), o["flags"].data_ptr())
                chk(lib.tt_env_step(h, p(action), p(o["obs"]), p(o["rew"]), p(o["done"]), C.byref(info), 1, st))
                chk(lib.tt_env_step_random(h, 99, p(alloc.out(f"{tag}{rep}.r.action", (n,), **T)),
                                           p(alloc.out(f"{tag}{rep}.r.obs", (n, 23), **T)),
                                           p(alloc.out(f"{tag}{rep}.r.reward", (n,), **T)),
                                           p(alloc.out(f"{tag}{rep}.r.done", (n,), u8, **T)), None, 1, st))
        step("step", False)
        step("log", True)
        chk(lib.tt_env_get_episode(h, p(alloc.out("episode.steps", (n,), i32, **T)), p(alloc.out("episode.max_steps", (n,), i32, **T)),
                                   p(alloc.out("episode.start", (3, n), f64, **soa(3))), p(alloc.out("episode.goal", (3, n), f64, **soa(3))),
                                   p(alloc.out("episode.L2", (n,), f64, **T)), st))
        torch.cuda.synchronize()
        alloc.assert_clean("randomised reset and steps")
        assert alloc["step1.r.done"].all() and alloc["log1.r.done"].all()           # the reset piece ran on every lane
        out = {name: t.clone() for name, t in alloc.items()}
        env.close()
        return out

    fenced, plain = run(Arena(gpu_device)), run(Plain(gpu_device))
    assert fenced.keys() == plain.keys()
    for name in fenced:
        assert torch.equal(fenced[name].view(torch.uint8), plain[name].view(torch.uint8)), name


# ================================================================================================================ the loop
def _loop(device, seed=27, randomize="default", **kw):
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    env = _env(130, device, max_steps=3)
    env.reset(seed=seed)
    if randomize == "default":
        randomize = _rand()
    return DDPGRollout(env, batch_size=64, replay_slots=16, seed=seed, randomize=randomize, **kw)


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
    ea, eb = a.env.episode(), b.env.episode()
    for key in ("steps", "max_episode_steps", "start", "goal", "L2"):
        assert torch.equal(ea[key], eb[key]), key


def _td3(on):
    from ddpg_trucktrailer_amd.td3 import TD3Config
    return dict(td3=TD3Config(), updates_per_step=2) if on else {}        # (the delay is counted inside a vector step)


@pytest.mark.parametrize("td3", [False, True], ids=["ddpg", "td3"])
def test_graphs_and_eager_agree_and_a_resumed_run_continues(gpu_device, tmp_path, td3):
    from ddpg_trucktrailer_amd import checkpoint
    steps = 2 * 4 + 3
    a, b = _loop(gpu_device, graph_steps=4, **_td3(td3)), _loop(gpu_device, graph_steps=0, **_td3(td3))
    assert a.graph_steps == 4 and b.graph_steps == 0 and a.env.randomization == _rand()
    # slot 0 of the ring holds the observation of a randomised episode 0: columns 12-15 are the drawn goal's, not the default's
    goal, _ = ref.draw(27, np.arange(130), np.zeros(130, dtype=np.int64), _model(a.env))
    slot0 = a.ring.obs[0].cpu().numpy()
    p = a.env.params
    half_x, half_y = (p.map_max_x - p.map_min_x) / 2, (p.map_max_y - p.map_min_y) / 2
    cx, cy = (p.map_max_x + p.map_min_x) / 2, (p.map_max_y + p.map_min_y) / 2
    assert (slot0[:, 12] == ((goal[:, 0] - cx) * (1.0 / half_x)).astype(np.float32)).all()
    assert (slot0[:, 13] == ((goal[:, 1] - cy) * (1.0 / half_y)).astype(np.float32)).all()
    assert np.abs(slot0[:, 14] - np.sin(goal[:, 2])).max() <= 1e-6 and np.abs(slot0[:, 15] - np.cos(goal[:, 2])).max() <= 1e-6
    assert (slot0[:, 13] != np.float32((p.goal[1] - cy) / half_y)).all() and len(set(slot0[:, 12].tolist())) == 130
    a.run(steps)
    for _ in range(steps):
        b.step()
    _assert_same_loop(a, b)
    sd = a.state_dict()
    assert "randomize" in sd and "randomize" in sd["env"] and int(a.ring.done.sum()) >= 3 * 130
    # the lanes run the model's episodes: every lane has finished floor(11 / 3) = 3
    goal, l2 = ref.draw(27, np.arange(130), np.full(130, 3), _model(a.env))
    assert _same_bits(a.env.episode()["goal"], goal) and _same_bits(a.env.episode()["L2"], l2)
    # save at step 5, resume in a fresh loop with another seed
    c = _loop(gpu_device, graph_steps=4, **_td3(td3))
    c.run(5)
    path = checkpoint.save_loop_checkpoint(str(tmp_path / "loop.pt"), c)
    d = _loop(gpu_device, seed=99, graph_steps=4, **_td3(td3))
    d.run(6)
    checkpoint.load_loop_checkpoint(path, d)
    assert d.vector_steps == 5
    d.run(steps - 5)
    _assert_same_loop(a, d)
    # a loop without the option refuses the file, and so does one with other ranges
    e = _loop(gpu_device, randomize=None, graph_steps=0, **_td3(td3))
    with pytest.raises(ValueError, match="randomize"):
        checkpoint.load_loop_checkpoint(path, e)
    f = _loop(gpu_device, randomize=_rand(l2=(5.0, 9.0)), graph_steps=0, **_td3(td3))
    with pytest.raises(ValueError, match="randomize"):
        checkpoint.load_loop_checkpoint(path, f)
    for lp in (a, b, c, d, e, f):
        lp.env.close()


# ================================================================================================================ off is off
def _trajectory(env, steps=8, policy_seed=7):
    import torch
    out = []
    for _ in range(steps):
        obs, rew, done, _ = env.step_random(policy_seed=policy_seed)
        out.append((obs.clone(), rew.clone(), done.clone(), env.state))
    torch.cuda.synchronize()
    return out


def _assert_same_trajectory(a, b):
    import torch
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        for name, s, t in zip(("obs", "reward", "done", "state"), x, y):
            assert torch.equal(s, t), (k, name)


def test_off_is_off(gpu_device):
    n, seed = 130, 27
    plain, toggled = _env(n, gpu_device, max_steps=3), _env(n, gpu_device, max_steps=3)
    epoch = toggled.graph_epoch
    toggled.enable_randomization(_rand())
    toggled.disable_randomization()
    assert toggled.graph_epoch == epoch + 2 and toggled.randomization is None and toggled.randomization_ranges() is None
    assert "randomize" not in toggled.state_dict() and "randomize" not in plain.state_dict()
    o1, o2 = plain.reset(seed=seed).clone(), toggled.reset(seed=seed).clone()
    import torch
    assert torch.equal(o1, o2)
    _assert_same_trajectory(_trajectory(plain), _trajectory(toggled))
    ea, eb = plain.episode(), toggled.episode()
    for key in ea:
        assert torch.equal(ea[key], eb[key]), key
    plain.close(); toggled.close()


def test_zero_width_ranges_are_the_per_env_path(gpu_device):
    """Ranges of zero width at the parameters' own values: the trajectories of a plain env on which set_pose(goal = default,
    L2 = default) turned the per-env path on, bit for bit."""
    import torch
    n, seed = 130, 27
    z, q = _env(n, gpu_device, max_steps=3), _env(n, gpu_device, max_steps=3)
    p = z.params
    default = tuple(p.goal)
    z.enable_randomization(_rand(goal=(default, default), l2=(p.L2, p.L2)))
    oz = z.reset(seed=seed).clone()
    q.reset(seed=seed)
    oq = q.set_pose(q.episode()["start"], goal=torch.tensor(default, dtype=torch.float64).repeat(n, 1),
                    L2=torch.full((n,), float(p.L2), dtype=torch.float64)).clone()
    assert torch.equal(oz, oq)
    ez = z.episode()
    assert _same_bits(ez["goal"], np.tile(np.array(default), (n, 1))) and _same_bits(ez["L2"], np.full(n, float(p.L2)))
    _assert_same_trajectory(_trajectory(z), _trajectory(q))
    z.close(); q.close()


# ================================================================================================================ refusals
def test_library_refusals_that_read_the_handle(gpu_device):
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    from ddpg_trucktrailer_amd.curriculum import Curriculum
    env = _env(4, gpu_device, max_steps=3)
    lib, h, st = env.lib, env._h, L.stream(env.device)
    rnd = _rand().c_struct(env.params)
    cur = Curriculum((3, 2, 2)).c_struct()

    def refused(rc, words):
        assert rc == L.TT_EINVAL
        for who in (h, None):                       # fail_both: the handle's message and the library's
            assert words in lib.tt_last_error(who).decode(), lib.tt_last_error(who)

    def usable():
        env.reset(seed=1)
        _, _, done, _ = env.step_random(policy_seed=3)
        torch.cuda.synchronize()
        assert done.shape == (4,) and torch.isfinite(env.obs).all()

    # with a curriculum on, and the converse
    env.enable_curriculum(Curriculum((3, 2, 2)))
    refused(lib.tt_env_set_randomization(h, C.byref(rnd), st), "episode randomisation with a curriculum is not supported")
    assert lib.tt_env_randomization(h, None) == 0
    with pytest.raises(ValueError, match="episode randomisation with a curriculum"):
        env.enable_randomization(_rand())
    usable()
    env.disable_curriculum()
    env.enable_randomization(_rand())
    out = L.TTRandomization()
    assert lib.tt_env_randomization(h, C.byref(out)) == 1 and (tuple(out.goal_lo), out.L2_hi) == (GOAL[0], L2[1])
    refused(lib.tt_env_set_curriculum(h, C.byref(cur), None, st), "a curriculum with episode randomisation is not supported")
    with pytest.raises(L.TTError, match="a curriculum with episode randomisation"):
        env.enable_curriculum(Curriculum((3, 2, 2)))
    usable()
    # with the detailed log, both directions
    refused(lib.tt_env_set_episode_log2(h, 64, L.LOG_DETAIL, st), "the detailed episode log with episode randomisation is not supported")
    with pytest.raises(L.TTError, match="the detailed episode log with episode randomisation"):
        env.enable_episode_log(64, detail=True)
    env.enable_episode_log(64)                      # the plain log composes
    usable()
    assert env.drain_episodes()["written"] >= 0
    env.disable_episode_log()
    refused(lib.tt_env_rollout_random(h, 3, 7, None, None, None, st), "episode randomisation does not follow k_rollout")
    usable()
    env.disable_randomization()
    env.rollout_random(3)
    env.enable_episode_log(64, detail=True)
    refused(lib.tt_env_set_randomization(h, C.byref(rnd), st), "episode randomisation with the detailed episode log is not supported")
    with pytest.raises(ValueError, match="episode_log_detail"):
        env.enable_randomization(_rand())
    env.disable_episode_log()
    # ranges that only the handle's parameters can judge
    far = _rand(goal=((-10.0, -45.0, 1.3), (10.0, -28.0, 1.8))).c_struct(env.params)
    refused(lib.tt_env_set_randomization(h, C.byref(far), st), "leaves the map")
    short = _rand(l2=(1.0, 10.0)).c_struct(env.params)
    refused(lib.tt_env_set_randomization(h, C.byref(short), st), "rad per step exceeds the 0.25 rad")
    assert lib.tt_env_randomization(h, None) == 0
    usable()
    env.close()
