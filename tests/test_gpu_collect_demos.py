"""GPU (-m gpu): collect_demonstrations (ddpg_trucktrailer_amd/mpc.py) on the 8 lanes of
mpc_ref.COLLECT_START -- 8.2 to 11.7 m in front of the default goal, yaw offsets up to 6 degrees -- with H = 16, S = 128 and the
other defaults of MPCConfig.  tests/test_mpc_cpu.py asserts that mpc_ref's closed loop on the C oracle succeeds in all 8 from
these poses with this config and ends within half of both goal thresholds (at most 0.19 m and 5.6 degrees), so at least 6 must
succeed here: 2 lanes are the cap on what GPU-against-oracle drift may cost a free-running closed loop.

    success     >= 6 of 8; keep="success" keeps exactly the episodes that end in TT_F_SUCCESS
    tuples      obs2[k] is obs[k + 1] bit for bit inside an episode, done on the last tuple only, actions in [-1, 1]
    replay      the stored actions through env.step from the same poses give the stored rewards bit for bit
    statistics  add up
    file        save_transitions_npz / load_transitions_npz round-trips the arrays
    loop        four steps of DDPGRollout(demo_loss=DemoLoss(1.0)), N = 64, B = 33, the file in the side buffer: demo_rows > 0"""
import functools

import numpy as np
import pytest

import mpc_ref as M

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _collected(keep):
    """(arrays, stats) of one collection; made once per process: do not write to it."""
    from ddpg_trucktrailer_amd.mpc import collect_demonstrations
    return collect_demonstrations(8, M.collect_cfg(), poses=M.COLLECT_START, seed=M.COLLECT_SEED, keep=keep)


def _episodes(arrays, stats):
    """[(lane, slice of the lane's rows)] of the kept episodes."""
    ends = np.cumsum(stats["lengths"])
    return [(lane, slice(int(e - k), int(e))) for lane, k, e in zip(stats["lanes"], stats["lengths"], ends)]


def test_most_lanes_succeed_and_success_keeps_only_successes(gpu_device):
    from ddpg_trucktrailer_amd import _lib as L
    (obs, act, rew, obs2, done), st = _collected("success")
    _, st_all = _collected("all")
    print("success:", st)
    print("all:", st_all)
    assert st["episodes"] == 8 and st["successes"] >= 6, st
    assert st["kept_episodes"] == st["successes"] == len(st["lanes"]) and st_all["kept_episodes"] == 8
    assert st["successes"] == st_all["successes"] and st["flags"] == st_all["flags"]
    assert st["flags"]["success"] == st["successes"]
    # the kept episodes are the successful ones of the full collection, tuple for tuple
    all_arrays, _ = _collected("all")
    by_lane = dict(_episodes(all_arrays, st_all))
    for lane, rows in _episodes((obs, act, rew, obs2, done), st):
        for kept, full in zip((obs, act, rew, obs2, done), all_arrays):
            assert np.array_equal(kept[rows], full[by_lane[lane]])
    assert len(st["end_flags"]) == st["kept_episodes"] and all(f & L.F_SUCCESS for f in st["end_flags"])
    assert sum(1 for f in st_all["end_flags"] if f & L.F_SUCCESS) == st["successes"]
    assert all(rew[rows][-1] > 200.0 for _, rows in _episodes((obs, act, rew, obs2, done), st)), "the last step pays the final bonus"


def test_tuples_chain_inside_an_episode(gpu_device):
    (obs, act, rew, obs2, done), st = _collected("all")
    assert obs.dtype == np.float32 and act.dtype == np.float32 and rew.dtype == np.float32 and obs2.dtype == np.float32
    assert done.dtype == np.bool_ and obs.shape == obs2.shape == (len(rew), 23) and act.shape == (len(rew), 1) and done.shape == rew.shape
    assert np.all(np.abs(act) <= 1.0) and np.isfinite(obs).all() and np.isfinite(rew).all()
    for lane, rows in _episodes((obs, act, rew, obs2, done), st):
        o, o2, d = obs[rows], obs2[rows], done[rows]
        assert np.array_equal(o2[:-1].view(np.int32), o[1:].view(np.int32)), lane
        assert d[-1] and not d[:-1].any(), lane


def test_replaying_the_actions_reproduces_the_rewards(gpu_device):
    import torch
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    (obs, act, rew, obs2, done), st = _collected("all")
    eps = _episodes((obs, act, rew, obs2, done), st)
    assert [lane for lane, _ in eps] == list(range(8))
    env = TruckTrailerVecEnv(8, device=gpu_device)
    first = env.set_pose(M.COLLECT_START).cpu().numpy()
    steps = max(st["lengths"])
    a = np.zeros((steps, 8), np.float32)
    for lane, rows in eps:
        a[:rows.stop - rows.start, lane] = act[rows, 0]
        assert np.array_equal(first[lane].view(np.int32), obs[rows][0].view(np.int32))
    high = torch.tensor(float(M.HIGH), dtype=torch.float32, device=gpu_device)
    got = np.zeros((steps, 8), np.float32)
    for t in range(steps):
        _, r, _, _ = env.step(torch.from_numpy(a[t]).to(gpu_device) * high, auto_reset=False)
        got[t] = r.cpu().numpy()
    for lane, rows in eps:
        k = rows.stop - rows.start
        assert np.array_equal(got[:k, lane].view(np.int32), rew[rows].view(np.int32)), lane
    env.close()


def test_statistics_add_up(gpu_device):
    for keep in ("success", "all"):
        (obs, act, rew, obs2, done), st = _collected(keep)
        assert st["transitions"] == len(rew) == sum(st["lengths"]) and st["kept_episodes"] == len(st["lengths"]) == int(done.sum())
        assert st["finished"] == 8 and sum(st["flags"].values()) >= st["finished"]
        assert st["vector_steps"] == max(_collected("all")[1]["lengths"]) and st["seconds"] > 0
        assert st["mean_length"] == pytest.approx(np.mean(st["lengths"]))
        rets = [rew[rows].astype(np.float64).sum() for _, rows in _episodes((obs, act, rew, obs2, done), st)]
        assert st["mean_return"] == pytest.approx(np.mean(rets), rel=1e-12)
        assert set(st["flags"]) == {"jackknife", "out_of_map", "max_steps", "goal_reached", "goal_passed", "excessive_back", "success"}


def test_file_round_trip_and_the_vector_loop_draws_demonstrations(gpu_device, tmp_path):
    import torch
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    from ddpg_trucktrailer_amd.expert import load_transitions_npz, save_transitions_npz
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    arrays, st = _collected("success")
    path = str(tmp_path / "demos.npz")
    assert save_transitions_npz(path, *arrays) == st["transitions"]
    back = load_transitions_npz(path)
    for x, y in zip(arrays, back):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    env = TruckTrailerVecEnv(64, device=gpu_device)
    env.reset(seed=6)
    loop = DDPGRollout(env, batch_size=33, replay_slots=8, seed=6, graph_steps=0, demo_loss=DemoLoss(1.0))
    d_obs, d_act, d_rew, d_obs2, d_done = back
    assert loop.ring.load_side(d_obs, d_act[:, 0], d_rew, d_obs2, d_done) == st["transitions"]
    loop.run(4)
    torch.cuda.synchronize()
    stats = loop.demo_stats()
    print(stats, int(loop.learner.step_dev.item()))
    assert stats["demo_rows"] > 0, stats
    env.close()
