"""GPU: the episode log written by the env step kernel (include/ttenv.h: tt_env_set_episode_log; DESIGN.md "Episode log").

Every env that finishes an episode appends its f64 return, length, flags, success (trainv2.py's final_success_bonus > 0), lane
and end step; exact counters by outcome sit beside the records.  Checked here against a host recomputation from the step's
info (bitwise), the C oracle, the trajectory ring of the fast loop, graph replays against eager steps, overflow, resume, and
that the log changes nothing it observes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def host_log(env, steps, seed, n_events=None):
    """Step `env` (log on) with seeded random actions, info and auto-reset, and rebuild its episode log on the host from
    info.comp[TT_I_TOTAL] (f64), info.flags, info.comp[TT_I_FINAL] and done, summed in step order.  n_events: {step:
    callable(env) -> lanes whose episode it restarted} run before that step."""
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    n = env.n_envs
    rng = np.random.RandomState(seed)
    acc = np.zeros(n, np.float64)
    length = np.zeros(n, np.int64)
    recs = []
    for t in range(steps):
        if n_events and t in n_events:
            lanes = n_events[t](env)
            acc[lanes] = 0.0
            length[lanes] = 0
        a = torch.from_numpy((rng.uniform(-1, 1, n) * np.pi / 4).astype(np.float32)).to(env.device)
        _, _, done, info = env.step(a, auto_reset=True, info=True)
        comp = info["comp"].cpu().numpy()
        flags = info["flags"].cpu().numpy()
        d = done.cpu().numpy().astype(bool)
        acc = acc + comp[0]                       # TT_I_TOTAL, the f64 reward
        length += 1
        for i in np.nonzero(d)[0]:
            recs.append((acc[i], length[i], flags[i], comp[L.INFO_ROWS.index("final_success_bonus"), i] > 0, i, t))
        acc[d] = 0.0
        length[d] = 0
    return recs


def as_lists(r):
    return (r["ret"].cpu().numpy(), r["len"].cpu().numpy(), r["flags"].cpu().numpy(), r["success"].cpu().numpy(),
            r["lane"].cpu().numpy(), r["end_step"].cpu().numpy())


def check_exact(got, recs):
    ret, ln, fl, su, lane, end = as_lists(got)
    assert got["written"] == len(recs) and got["dropped"] == 0
    assert len(ret) == len(recs)
    want_ret = np.array([r[0] for r in recs], np.float64)
    assert np.array_equal(ret.view(np.int64), want_ret.view(np.int64)), "returns differ in their bits"
    assert ln.tolist() == [int(r[1]) for r in recs]
    assert fl.tolist() == [int(r[2]) for r in recs]
    assert su.tolist() == [bool(r[3]) for r in recs]
    assert lane.tolist() == [int(r[4]) for r in recs]
    assert end.tolist() == [int(r[5]) for r in recs]


def host_counts(recs):
    c = {"episodes": len(recs), "successes": sum(bool(r[3]) for r in recs)}
    from ddpg_trucktrailer_amd import _lib as L
    for b, name in enumerate(L.LOG_COUNTS[2:]):
        c[name] = sum((int(r[2]) >> b) & 1 for r in recs)
    return c


@pytest.mark.parametrize("per_env", [False, True])
def test_log_equals_host_recomputation_bitwise(gpu_device, per_env):
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    n, steps = 4096, 600
    env = TruckTrailerVecEnv(n, device=gpu_device)
    env.enable_episode_log(65536)
    env.reset(seed=11)
    rs = np.random.RandomState(3)
    if per_env:          # per-env goals: the PER_ENV kernel variant
        start = np.stack([rs.uniform(-20, 20, n), rs.uniform(5, 25, n), rs.uniform(0.9, 2.0, n)], 1)
        goal = np.stack([rs.uniform(-5, 5, n), rs.uniform(-32, -25, n), rs.uniform(1.2, 1.9, n)], 1)
        env.set_pose(start, goal=goal)

    def set_pose_some(e):          # a new episode for some lanes mid-run: their returns restart at 0
        idx = np.arange(5, n, 37, dtype=np.int32)
        st = np.stack([rs.uniform(-20, 20, len(idx)), rs.uniform(5, 25, len(idx)), rs.uniform(0.9, 2.0, len(idx))], 1)
        e.set_pose(st, idx=idx)
        return idx

    def masked_reset(e):
        m = np.zeros(n, np.uint8)
        m[3::29] = 1
        e.reset(seed=11, mask=m)
        return np.nonzero(m)[0]

    def set_state_some(e):         # continues the episode: no restart
        e.set_state(e.state[:64].cpu().numpy())
        return np.array([], np.int64)

    recs = host_log(env, steps, seed=7, n_events={100: set_pose_some, 250: masked_reset, 400: set_state_some})
    assert len(recs) > 1000
    got = env.drain_episodes()
    check_exact(got, recs)
    assert got["counts"] == host_counts(recs)
    again = env.drain_episodes()               # drained: no records, the counters stay
    assert again["written"] == 0 and len(again["ret"]) == 0 and again["counts"] == got["counts"]
    env.close()


def test_log_returns_match_the_c_oracle(gpu_device):
    """The first episode of each of a handful of lanes, stepped with the same actions by the C restatement: the returns agree
    to the suite's reward parity tolerance (1e-5 per step)."""
    import torch
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    from oracle import c_oracle
    n = 16
    env = TruckTrailerVecEnv(n, device=gpu_device)
    env.reset(seed=5)
    env.enable_episode_log(4096)
    ora = c_oracle.COracle(n)
    ora.place(env.episode()["start"].cpu().numpy())
    rng = np.random.RandomState(1)
    acc = np.zeros(n)
    first = {}
    for t in range(1500):
        a = (rng.uniform(-1, 1, n) * np.pi / 4).astype(np.float32)
        env.step(torch.from_numpy(a).to(gpu_device), auto_reset=False)
        _, o_rew, o_done, _ = ora.step(a)
        for i in range(n):
            if i not in first:
                acc[i] += o_rew[i]
                if o_done[i]:
                    first[i] = (acc[i], t)
        if len(first) == n:
            break
    assert len(first) == n
    got = env.drain_episodes()
    ret, ln, _, _, lane, end = as_lists(got)
    for i, (r, t) in first.items():
        j = np.nonzero(lane == i)[0][0]           # the lane's first record (sorted by end step)
        assert end[j] == t and ln[j] == t + 1
        assert abs(ret[j] - r) <= 1e-5 * (t + 1), (i, ret[j], r)
    env.close()


def _short_episodes(env, seed):
    """First episodes of 3..40 steps (max_episode_steps), so that a short run has many finishers."""
    env.set_max_steps(np.random.RandomState(seed).randint(3, 41, env.n_envs).astype(np.int32))


def _loop(n, graph_steps, seed=27, log=1 << 20):
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    env = TruckTrailerVecEnv(n)
    env.reset(seed=seed)
    _short_episodes(env, seed)
    return DDPGRollout(env, batch_size=256, replay_slots=64, seed=seed, graph_steps=graph_steps, episode_log=log)


def _flat(loop):
    import torch
    return torch.cat([p.detach().reshape(-1) for net in loop.agent._nets() for p in net.parameters()])


def _records(r):
    return [x.cpu().numpy() for x in (r["ret"], r["len"], r["flags"], r["success"], r["lane"], r["end_step"])]


@pytest.mark.parametrize("graph_steps", [20, 4])
def test_fast_loop_log_graphs_equal_eager_and_the_ring(gpu_device, graph_steps):
    """DDPGRollout at N = 65536, pipelined: the records of graph replays == those of eager steps, bit for bit; each record
    matches a shadow rebuilt from ring.rew / ring.done (lengths, lanes, end steps exact; returns to f32 summation)."""
    import torch
    steps = 48
    out = []
    for g in (graph_steps, 0):
        loop = _loop(65536, g)
        assert loop.pipeline
        loop.run(steps)
        torch.cuda.synchronize()
        if g:
            assert loop.graphG is not None
        r = loop.drain_episodes()
        assert r["dropped"] == 0
        out.append((_records(r), loop.ring.rew[:steps].double().cpu().numpy(),
                    loop.ring.done[:steps].cpu().numpy().astype(bool)))
        loop.env.close()
        del loop
    (ra, rew, done), (rb, _, _) = out
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)
    ret, ln, _, _, lane, end = ra
    assert len(ret) > 1000
    acc = np.zeros(rew.shape[1])
    length = np.zeros(rew.shape[1], np.int64)
    shadow = []
    for t in range(steps):
        acc += rew[t]
        length += 1
        for i in np.nonzero(done[t])[0]:
            shadow.append((t, i, length[i], acc[i]))
        acc[done[t]] = 0.0
        length[done[t]] = 0
    assert [(s[0], s[1]) for s in shadow] == list(zip(end.tolist(), lane.tolist()))
    assert [s[2] for s in shadow] == ln.tolist()
    sret = np.array([s[3] for s in shadow])
    assert np.all(np.abs(sret - ret) <= 1e-4 * ln + 1e-6 * np.abs(ret))


def test_log_only_observes(gpu_device):
    """Weights, observations, ring contents and env state after K steps are bitwise those of the same loop without the log."""
    import torch
    res = []
    for log in (1 << 20, None):
        loop = _loop(65536, 20, log=log)
        loop.run(28)
        torch.cuda.synchronize()
        res.append([_flat(loop).clone(), loop.ring.obs[:29].clone(), loop.ring.act[:28].clone(), loop.ring.rew[:28].clone(),
                    loop.ring.done[:28].clone(), loop.env.state.clone(), loop.noise.x.clone()])
        loop.env.close()
        del loop
    for x, y in zip(*res):
        assert torch.equal(x, y)


def test_turning_the_log_on_and_off_recaptures(gpu_device):
    import torch
    loop = _loop(8192, 4, log=None)
    loop.run(12)                                   # warm-up + captured graphs without the log
    g_before = loop.graphG
    assert g_before is not None
    loop.env.enable_episode_log(1 << 16)
    loop.env.set_max_steps(np.ones(8192, np.int32))     # every lane's episode ends at the next step
    loop.run(8)
    r = loop.drain_episodes()
    assert loop.graphG is not g_before and r["written"] >= 8192 and r["counts"]["max_steps"] >= 8192
    assert r["end_step"].min().item() >= 0 and r["end_step"].max().item() <= 7   # launches counted since enable
    g_on = loop.graphG
    loop.env.disable_episode_log()
    loop.run(8)
    torch.cuda.synchronize()
    assert loop.graphG is not g_on
    with pytest.raises(RuntimeError):
        loop.drain_episodes()
    loop.env.close()


def test_overflow_keeps_counting(gpu_device):
    import torch
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    full = {}
    for cap in (65536, 64):
        env = TruckTrailerVecEnv(4096, device=gpu_device)
        env.enable_episode_log(cap)
        env.reset(seed=2)
        _short_episodes(env, 2)
        for t in range(120):
            env.step_random(policy_seed=9, auto_reset=True)
        full[cap] = env.drain_episodes()
        env.close()
    a, b = full[65536], full[64]
    assert a["dropped"] == 0 and a["written"] > 64
    assert b["written"] == a["written"] and b["dropped"] == b["written"] - 64 and len(b["ret"]) == 64
    assert b["counts"] == a["counts"]
    # what was stored is the full run's prefix, up to the order inside the launch where the log filled up (set by atomics)
    ka = (a["end_step"] * 4096 + a["lane"]).cpu().numpy()
    kb = (b["end_step"] * 4096 + b["lane"]).cpu().numpy()
    last = int(b["end_step"].max().item())
    before = ka[a["end_step"].cpu().numpy() < last]
    assert np.array_equal(kb[:len(before)], before)
    assert set(kb[len(before):].tolist()) <= set(ka[a["end_step"].cpu().numpy() == last].tolist())
    pos = {k: j for j, k in enumerate(ka.tolist())}
    for j, k in enumerate(kb.tolist()):
        assert torch.equal(b["ret"][j], a["ret"][pos[k]]) and int(b["len"][j]) == int(a["len"][pos[k]])


def test_resume_continues_the_log(gpu_device, tmp_path):
    """Checkpoint mid-run (records not drained yet), load into a fresh loop, continue: the records equal an uninterrupted
    run's."""
    import torch
    from ddpg_trucktrailer_amd import checkpoint
    a = _loop(4096, 4, seed=21, log=1 << 17)
    a.run(10)
    path = checkpoint.save_loop_checkpoint(str(tmp_path / "loop.pt"), a)
    a.run(30)
    da = a.drain_episodes()
    assert da["dropped"] == 0
    ra = _records(da)
    b = _loop(4096, 4, seed=99, log=1 << 17)
    b.run(6)
    checkpoint.load_loop_checkpoint(path, b)
    b.run(30)
    torch.cuda.synchronize()
    db = b.drain_episodes()
    assert db["counts"] == da["counts"] and db["written"] == da["written"]
    rb = _records(db)
    assert len(ra[0]) > 100
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)
    assert torch.equal(_flat(a), _flat(b))
    a.env.close(); b.env.close()


def test_rollout_random_refuses_while_logging(gpu_device):
    from ddpg_trucktrailer_amd import _lib as L
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    env = TruckTrailerVecEnv(256, device=gpu_device)
    env.reset(seed=1)
    env.enable_episode_log(128)
    with pytest.raises(L.TTError):
        env.rollout_random(4)
    env.disable_episode_log()
    env.rollout_random(4)
    env.close()
