"""GPU: the detailed episode log (include/ttenv.h: tt_env_set_episode_log2 with TT_LOG_DETAIL; DESIGN.md "Episode log").

Every record of a detailed log also carries its episode's sum of each reward term (TT_I_PROGRESS .. TT_I_SMOOTH) and its start
pose.  Checked against a host rebuild from the step's info (bitwise), the C oracle, the plain log of the same run, graph replays
against eager steps in the fast loop, resume from a checkpoint, and a population against lone loops."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COMP_ROWS = slice(1, 10)       # info.comp rows TT_I_PROGRESS .. TT_I_SMOOTH


def _events(env, n, rs):
    """Mid-run changes at steps 100 / 250 / 400: set_pose and a masked reset restart episodes, set_state continues them."""
    def set_pose_some(e):
        idx = np.arange(5, n, 37, dtype=np.int32)
        st = np.stack([rs.uniform(-20, 20, len(idx)), rs.uniform(5, 25, len(idx)), rs.uniform(0.9, 2.0, len(idx))], 1)
        e.set_pose(st, idx=idx)
        return idx

    def masked_reset(e):
        m = np.zeros(n, np.uint8)
        m[3::29] = 1
        e.reset(seed=11, mask=m)
        return np.nonzero(m)[0]

    def set_state_some(e):
        e.set_state(e.state[:64].cpu().numpy())
        return np.array([], np.int64)
    return {100: set_pose_some, 250: masked_reset, 400: set_state_some}


def _run(per_env, detail, steps=600, n=4096, host=False):
    """The run of tests/test_gpu_episode_log.py's bitwise test with the log plain or detailed; host=True also rebuilds the
    detailed records on the host: the nine term sums from info.comp in step order, the start pose env.episode() showed when
    the episode began."""
    import torch
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    env = TruckTrailerVecEnv(n)
    env.enable_episode_log(65536, detail=detail)
    env.reset(seed=11)
    rs = np.random.RandomState(3)
    if per_env:
        start = np.stack([rs.uniform(-20, 20, n), rs.uniform(5, 25, n), rs.uniform(0.9, 2.0, n)], 1)
        goal = np.stack([rs.uniform(-5, 5, n), rs.uniform(-32, -25, n), rs.uniform(1.2, 1.9, n)], 1)
        env.set_pose(start, goal=goal)
    events = _events(env, n, rs)
    rng = np.random.RandomState(7)
    acc = np.zeros((9, n))
    pose = env.episode()["start"].cpu().numpy() if host else None
    recs = []
    for t in range(steps):
        if t in events:
            lanes = events[t](env)
            if host:
                acc[:, lanes] = 0.0
                pose[lanes] = env.episode()["start"].cpu().numpy()[lanes]
        a = torch.from_numpy((rng.uniform(-1, 1, n) * np.pi / 4).astype(np.float32)).to(env.device)
        _, _, done, info = env.step(a, auto_reset=True, info=True)
        if host:
            comp = info["comp"].cpu().numpy()
            d = done.cpu().numpy().astype(bool)
            acc = acc + comp[COMP_ROWS]
            for i in np.nonzero(d)[0]:
                recs.append((t, i, acc[:, i].copy(), pose[i].copy()))
            acc[:, d] = 0.0
            if d.any():
                pose[d] = env.episode()["start"].cpu().numpy()[d]
    got = env.drain_episodes()
    env.close()
    return got, recs


PLAIN_KEYS = ("ret", "len", "flags", "success", "lane", "end_step")


@pytest.mark.parametrize("per_env", [False, True])
def test_detail_equals_host_rebuild_and_the_plain_log(gpu_device, per_env):
    import torch
    got, recs = _run(per_env, True, host=True)
    assert got["written"] == len(recs) > 1000 and got["dropped"] == 0
    assert [(int(t), int(i)) for t, i, _, _ in recs] == list(zip(got["end_step"].tolist(), got["lane"].tolist()))
    comp = got["components"].cpu().numpy()
    assert comp.shape == (len(recs), 9) and got["start"].shape == (len(recs), 3)
    want = np.stack([r[2] for r in recs])
    assert np.array_equal(comp.view(np.int64), want.view(np.int64)), "term sums differ in their bits"
    assert np.array_equal(got["start"].cpu().numpy(), np.stack([r[3] for r in recs]))
    plain, _ = _run(per_env, False)
    assert "components" not in plain and "start" not in plain
    for k in PLAIN_KEYS:
        assert torch.equal(got[k], plain[k]), k
    assert got["counts"] == plain["counts"] and got["written"] == plain["written"]


def test_detail_sums_match_the_c_oracle(gpu_device):
    """The first episode of 16 lanes stepped with the same actions by the C restatement: each term sum agrees to the suite's
    reward parity tolerance (1e-5 per step)."""
    import torch
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    from oracle import c_oracle
    n = 16
    env = TruckTrailerVecEnv(n, device=gpu_device)
    env.reset(seed=5)
    env.enable_episode_log(4096, detail=True)
    start = env.episode()["start"].cpu().numpy()
    ora = c_oracle.COracle(n)
    ora.place(start)
    rng = np.random.RandomState(1)
    acc = np.zeros((n, 9))
    first = {}
    for t in range(1500):
        a = (rng.uniform(-1, 1, n) * np.pi / 4).astype(np.float32)
        env.step(torch.from_numpy(a).to(gpu_device), auto_reset=False)
        _, _, o_done, o_info = ora.step(a)
        for i in range(n):
            if i not in first:
                acc[i] += o_info[i, COMP_ROWS]
                if o_done[i]:
                    first[i] = (acc[i].copy(), t)
        if len(first) == n:
            break
    assert len(first) == n
    got = env.drain_episodes()
    lane, end = got["lane"].cpu().numpy(), got["end_step"].cpu().numpy()
    comp, st = got["components"].cpu().numpy(), got["start"].cpu().numpy()
    for i, (sums, t) in first.items():
        j = np.nonzero(lane == i)[0][0]
        assert end[j] == t
        assert np.all(np.abs(comp[j] - sums) <= 1e-5 * (t + 1)), (i, comp[j], sums)
        assert np.array_equal(st[j], start[i])
    env.close()


def _loop(n, graph_steps, seed=27, log=1 << 20, detail=True):
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    env = TruckTrailerVecEnv(n)
    env.reset(seed=seed)
    env.set_max_steps(np.random.RandomState(seed).randint(3, 41, n).astype(np.int32))
    return DDPGRollout(env, batch_size=256, replay_slots=64, seed=seed, graph_steps=graph_steps, episode_log=log,
                       episode_log_detail=detail)


def test_fast_loop_detail_graphs_equal_eager_and_only_observe(gpu_device):
    import torch
    steps = 48
    out = {}
    for name, g, detail in (("graph", 20, True), ("eager", 0, True), ("plain", 20, False)):
        loop = _loop(65536, g, detail=detail)
        assert loop.pipeline
        loop.run(steps)
        torch.cuda.synchronize()
        if g:
            assert loop.graphG is not None
        r = loop.drain_episodes()
        assert r["dropped"] == 0
        out[name] = (r, [loop.ring.obs[:steps + 1].clone(), loop.ring.act[:steps].clone(), loop.ring.rew[:steps].clone(),
                         loop.ring.done[:steps].clone(), loop.env.state.clone()])
        loop.env.close()
        del loop
    (rg, ring_g), (re_, _), (rp, ring_p) = out["graph"], out["eager"], out["plain"]
    assert len(rg["ret"]) > 1000
    for k in PLAIN_KEYS + ("components", "start"):
        assert torch.equal(rg[k], re_[k]), k
    for k in PLAIN_KEYS:
        assert torch.equal(rg[k], rp[k]), k
    assert rg["counts"] == rp["counts"]
    for x, y in zip(ring_g, ring_p):
        assert torch.equal(x, y)
    # each record's term sums add up to its return (to summation order)
    tot = rg["components"].sum(1)
    assert torch.all((tot - rg["ret"]).abs() <= 1e-9 * (1 + rg["ret"].abs()))


def test_turning_detail_on_and_off_recaptures(gpu_device):
    import torch
    loop = _loop(8192, 4, log=1 << 16, detail=False)
    loop.run(12)
    g_plain = loop.graphG
    assert g_plain is not None
    loop.env.enable_episode_log(1 << 16, detail=True)
    loop.env.set_max_steps(np.ones(8192, np.int32))
    loop.run(8)
    r = loop.drain_episodes()
    assert loop.graphG is not g_plain and r["written"] >= 8192 and r["components"].shape == (r["written"], 9)
    g_detail = loop.graphG
    loop.env.enable_episode_log(1 << 16, detail=False)
    loop.run(8)
    torch.cuda.synchronize()
    assert loop.graphG is not g_detail and "components" not in loop.drain_episodes()
    loop.env.close()


def test_resume_continues_the_sums_and_kinds_do_not_mix(gpu_device):
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv, _ptr

    def make(detail=True):
        e = TruckTrailerVecEnv(4096, device=gpu_device)
        e.enable_episode_log(1 << 17, detail=detail)
        return e

    def go(e, k):
        for _ in range(k):
            e.step_random(policy_seed=9, auto_reset=True)

    a = make()
    a.reset(seed=2)
    go(a, 40)
    sd = a.state_dict()                       # mid-episode for most lanes, records not drained
    assert sd["episode_log"]["detail"] is True
    go(a, 200)
    ra = a.drain_episodes()
    b = TruckTrailerVecEnv(4096, device=gpu_device)
    b.load_state_dict(sd)
    assert b.episode_log_detail
    go(b, 200)
    rb = b.drain_episodes()
    assert len(ra["ret"]) > 1000 and ra["counts"] == rb["counts"]
    for k in PLAIN_KEYS + ("components", "start"):
        assert torch.equal(ra[k], rb[k]), k

    # a detailed blob does not go into a plain log, nor a plain blob into a detailed one
    plain = make(detail=False)
    psd = plain._episode_log_state()
    for dst, blob, kind in ((plain, sd["episode_log"], b"detailed"), (b, psd, b"plain")):
        before = dst._episode_log_state()["blob"]
        meta = (C.c_uint64 * 2)(*blob["meta"])
        src = blob["blob"].to(gpu_device)
        assert dst.lib.tt_env_import_episode_log(dst._h, _ptr(src), C.byref(meta), dst._stream()) == L.TT_EINVAL
        assert b"the blob is of a " + kind in dst.lib.tt_last_error(dst._h)
        assert torch.equal(dst._episode_log_state()["blob"], before)

    # comp / start from a plain log, and unknown flag bits on a live handle, are refused and change nothing
    out = torch.zeros((9, 1 << 17), dtype=torch.float64, device=gpu_device)
    rc = plain.lib.tt_env_drain_episode_log2(plain._h, None, None, None, None, None, None, _ptr(out), None, None, None,
                                             plain._stream())
    assert rc == L.TT_EINVAL and b"plain episode log" in plain.lib.tt_last_error(plain._h)
    assert plain.lib.tt_env_set_episode_log2(plain._h, 64, 6, plain._stream()) == L.TT_EINVAL
    assert b"unknown flag bits 0x6" in plain.lib.tt_last_error(plain._h)
    assert plain.lib.tt_env_episode_log_bytes(plain._h) == psd["blob"].numel()
    for e in (a, b, plain):
        e.close()


def test_population_detail_logs_equal_lone_loops(gpu_device):
    import torch
    from ddpg_trucktrailer_amd.population import PopulationRollout
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    seeds, n, steps = [31, 32], 2048, 40
    kw = dict(batch_size=256, replay_slots=16, updates_per_step=2, episode_log=1 << 16, episode_log_detail=True)
    pop = PopulationRollout(n, seeds, graph_steps=4, **kw)
    pop.run(steps)
    torch.cuda.synchronize()
    logs = pop.drain_episodes()
    old = os.environ.get("TT_ACTOR_TAIL")
    os.environ["TT_ACTOR_TAIL"] = "1"          # the lone loop's tail in one launch, as the population's
    try:
        for a, s in enumerate(seeds):
            env = TruckTrailerVecEnv(n, device=gpu_device)
            env.reset(seed=s)
            lp = DDPGRollout(env, seed=s, pipeline=False, **kw)
            lp.run(steps)
            want = lp.drain_episodes()
            got = logs[a]
            assert len(want["ret"]) > 0 and "components" in got and set(got) == set(want)
            for key in want:
                x, y = got[key], want[key]
                assert (torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y), (a, key)
            env.close()
    finally:
        if old is None:
            os.environ.pop("TT_ACTOR_TAIL")
        else:
            os.environ["TT_ACTOR_TAIL"] = old
