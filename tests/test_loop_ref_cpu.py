"""CPU: the host model of the vector loop (tests/loop_ref.py) held to its own statement, so that the GPU lock-step test
(tests/test_gpu_loop_lockstep.py) cannot pass through a wrong model: the draw reaches exactly its window and is uniform over it,
the OU normals have N(0, 1)'s moments, poses and actions lie in their boxes and depend on each argument, and COracle.place_lanes
leaves the other lanes alone."""
import math

import numpy as np
import pytest

import loop_ref as M

ROWS = 50000
N_ENVS = (1, 77, 200)


def _cases():
    """(slots, reserve, lag, n_step) over the issue's grid where the ring allows the draw: a base step with its n steps inside a
    window that leaves out the slot being written and the reserve (replay_buffer.slots_needed: 3 + reserve + n - 1 slots)."""
    from ddpg_trucktrailer_amd.replay_buffer import slots_needed
    return [(slots, reserve, lag, n_step) for slots in (3, 5, 6, 8) for reserve, lag in ((0, 0), (2, 1)) for n_step in (1, 3)
            if slots >= slots_needed(n_step, reserve)]


def _draw(seed, k, n_envs, slots, reserve, lag, n_step):
    if n_step > 1:
        return M.draw_nstep(seed, k, ROWS, n_envs, slots, n_step, reserve, lag)
    return M.draw(seed, k, ROWS, n_envs, slots, reserve, lag)


def _within(share, p, rows, what):
    """|share - p| <= 5 standard errors of a binomial share of `rows` draws (computed here); returns the worst in standard errors."""
    se = np.sqrt(p * (1.0 - p) / rows)
    dev = np.abs(share - p)
    assert (dev <= 5.0 * se).all(), (what, share, p, se)
    return float((dev / np.maximum(se, 1e-300)).max()) if (se > 0).any() else 0.0


@pytest.mark.parametrize("slots,reserve,lag,n_step", _cases())
def test_draw_reaches_exactly_its_window_and_is_uniform(slots, reserve, lag, n_step):
    """Every counter 0 .. 3 slots, 50,000 rows: the steps drawn are exactly window(...) -- the oldest included, none outside --,
    every env is reached, and each step's and each env decile's share is within 5 standard errors of uniform.  Where the window is
    empty (an early counter: the loop makes no draw there) the rows are only in bounds."""
    worst, seen_nonempty = 0.0, 0
    for k in range(3 * slots + 1):
        win = M.window(k, slots, reserve, lag, n_step)
        for n_envs in N_ENVS:
            idx = _draw(1000 + k, k, n_envs, slots, reserve, lag, n_step)
            assert idx.shape == (ROWS, 2) and idx.dtype == np.int64
            assert idx[:, 0].min() >= 0 and idx[:, 0].max() < slots and idx[:, 1].min() >= 0 and idx[:, 1].max() < n_envs
            if len(win) == 0:
                continue
            seen_nonempty += 1
            steps = M.step_of_slot(idx[:, 0], k, slots, lag)
            got = np.unique(steps)
            assert got.tolist() == list(win), (k, n_envs, got, win)
            assert np.unique(idx[:, 1]).size == n_envs
            share = np.bincount(steps - win[0], minlength=len(win)) / ROWS
            worst = max(worst, _within(share, np.full(len(win), 1.0 / len(win)), ROWS, ("step", k, n_envs)))
            decile = idx[:, 1] * 10 // n_envs
            p = np.bincount(np.arange(n_envs) * 10 // n_envs, minlength=10) / n_envs
            worst = max(worst, _within(np.bincount(decile, minlength=10) / ROWS, p, ROWS, ("env decile", k, n_envs)))
    assert seen_nonempty >= 3 * (2 * slots)
    print(f"slots {slots} reserve {reserve} lag {lag} n_step {n_step}: worst share off uniform {worst:.2f} standard errors")


def test_window_is_the_range_the_docstrings_give():
    """Spot values: the serial order after step t (counter t + 1) holds the steps t - (slots - 2) .. t, the pipelined order of step t
    (counter t, lag 1, reserve 2) the steps up to t - 2, slots - 3 of them; an n-step base step ends n - 1 steps earlier."""
    assert list(M.window(0, 6)) == [] and list(M.window(1, 6)) == [0] and list(M.window(5, 6)) == [0, 1, 2, 3, 4]
    assert list(M.window(9, 6)) == [4, 5, 6, 7, 8]
    assert list(M.window(1, 6, 2, 1)) == [] and list(M.window(2, 6, 2, 1)) == [0] and list(M.window(9, 6, 2, 1)) == [5, 6, 7]
    assert list(M.window(9, 8, 2, 1, n_step=3)) == [3, 4, 5] and list(M.window(3, 8, 2, 1, n_step=3)) == []
    assert list(M.window(4, 8, 2, 1, n_step=3)) == [0]
    ref = M.LoopRef(1, 1, 4, 6, 8, pipelined=False)
    assert [t for t in range(5) if ref.learns(t)] == [1, 2, 3, 4] and ref.updates_after(4) == 4
    ref = M.LoopRef(1, 1, 4, 8, 8, pipelined=True, updates_per_step=2, n_step=3)
    assert [t for t in range(7) if ref.learns(t)] == [4, 5, 6] and ref.updates_after(6) == 6
    assert len(ref.window(4)) == 1 and len(ref.window(3)) == 0          # the first learning step is the first with a window


def test_update_seeds_and_counter_words_enter_the_draw():
    a = M.draw(5, 9, 513, 200, 6)
    assert not np.array_equal(a, M.draw(M.update_seed(5, 1), 9, 513, 200, 6))
    assert not np.array_equal(a, M.draw(5 + 2 ** 32, 9, 513, 200, 6))                   # the key's high word
    assert not np.array_equal(a[:, 1], M.draw(5, 10, 513, 200, 6)[:, 1])                 # the step counter
    assert np.array_equal(M.draw(5, 9, 513, 200, 6, 2, 1)[:, 1], M.draw(5, 8, 513, 200, 6, 2, 0)[:, 1])    # the counter word is k - lag
    assert M.update_seed(2 ** 64 - 1, 1) == M.SEED_STRIDE - 1


def test_ou_normals_have_the_normal_moments():
    """10^6 normals (1000 steps x 1000 rows): mean, variance and fourth moment within 5 standard errors of N(0, 1)'s (standard
    errors 1 / sqrt(n), sqrt(2 / n), sqrt(96 / n)), the lag-1 correlation across consecutive steps within 5 / sqrt(n) of 0."""
    x = M.ou_normal(27, np.arange(1000), 1000)
    assert x.shape == (1000, 1000) and np.isfinite(x).all()
    n = x.size
    assert abs(x.mean()) <= 5.0 / math.sqrt(n), x.mean()
    assert abs((x ** 2).mean() - 1.0) <= 5.0 * math.sqrt(2.0 / n), (x ** 2).mean()
    assert abs((x ** 4).mean() - 3.0) <= 5.0 * math.sqrt(96.0 / n), (x ** 4).mean()
    lag1 = (x[:-1] * x[1:]).mean()
    assert abs(lag1) <= 5.0 / math.sqrt(x[1:].size), lag1
    assert np.array_equal(x[7], M.ou_normal(27, 7, 1000))                        # the array form is the scalar form
    assert not np.array_equal(x[7], M.ou_normal(28, 7, 1000)) and not np.array_equal(x[7, :999], x[8, 1:])
    # a step count beyond 2^32 reaches the second counter word
    assert not np.array_equal(M.ou_normal(27, 7 + 2 ** 32, 1000), x[7])


def test_ou_next_and_its_constants():
    assert M.OU_DECAY == float(np.float32(1.0) - np.float32(0.2 * 0.01)) and M.OU_SCALE == float(np.float32(0.015))
    x = M.ou_next([0.5, 0.5], [False, True], [2.0, 2.0])
    assert x[0] == 0.5 * M.OU_DECAY + 2.0 * M.OU_SCALE and x[1] == 2.0 * M.OU_SCALE


def test_poses_and_actions():
    lo, hi = M.reset_box()
    lanes = np.arange(4096)
    p = M.reset_pose(27, lanes, 0)
    assert p.shape == (4096, 3) and (p >= lo).all() and (p <= hi).all()
    assert (p.max(0) - p.min(0) > 0.9 * (hi - lo)).all()                          # ... and fills it
    assert not np.array_equal(p, M.reset_pose(28, lanes, 0)) and not np.array_equal(p, M.reset_pose(27, lanes, 1))
    assert not np.array_equal(p[:-1], p[1:]) and not np.array_equal(p, M.reset_pose(27 + 2 ** 32, lanes, 0))
    assert np.array_equal(M.reset_pose(27, 5, 3), M.reset_pose(27, lanes, np.full(4096, 3))[5])
    a = M.random_action(123, lanes, 4)
    assert a.dtype == np.float32 and np.abs(a).max() <= np.float32(math.pi / 4) and a.max() - a.min() > 0.9 * math.pi / 2
    assert not np.array_equal(a, M.random_action(124, lanes, 4)) and not np.array_equal(a, M.random_action(123, lanes, 5))
    assert not np.array_equal(a[:-1], a[1:]) and not np.array_equal(a, M.random_action(123, lanes, 4 + 2 ** 32))


def test_place_lanes_leaves_the_other_lanes_alone():
    """Lanes {1, 3} of a 5-lane oracle that has taken six steps are placed anew: lanes {0, 2, 4} keep their state bit for bit and
    their reward carry -- the next steps' outputs equal an untouched twin's --, the placed lanes are what place() makes of the pose."""
    from oracle import c_oracle
    start = M.reset_pose(3, np.arange(5), 0)
    a, b = c_oracle.COracle(5), c_oracle.COracle(5)
    for ora in (a, b):
        ora.place(start)
        for t in range(6):
            ora.step(M.random_action(9, np.arange(5), t))
    new = M.reset_pose(3, np.array([1, 3]), 1)
    obs = a.place_lanes([1, 3], new)
    fresh = c_oracle.COracle(2)
    assert np.array_equal(obs, fresh.place(new))
    keep = [0, 2, 4]
    assert np.array_equal(a.state()[keep], b.state()[keep]) and not np.array_equal(a.state()[[1, 3]], b.state()[[1, 3]])
    assert np.array_equal(a.state()[[1, 3]], fresh.state())
    for t in range(6, 10):
        act = M.random_action(9, np.arange(5), t)
        oa, ob, of = a.step(act), b.step(act), fresh.step(act[[1, 3]])
        for x, y, z in zip(oa, ob, of):
            assert np.array_equal(x[keep], y[keep]), t
            assert np.array_equal(x[[1, 3]], z), t
    assert [a.envs[i].steps for i in range(5)] == [10, 4, 10, 4, 10]
