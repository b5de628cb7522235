"""The plain host model of a success-replay harvest (include/ttenv.h: tt_ring_harvest; csrc/ttenv_harvest.h):
which rows of the trajectory ring a harvest copies into its region of the side buffer, and where.  Integer arithmetic and bit copies
only, so the kernels agree with it exactly.

    plan(...)      the eligible records in (s, lane) order with their rows, and the harvest's totals
    harvest(...)   the state and the region after the harvest
    planted(...)   a ring filled with distinct bit patterns, for tests that plant their own records"""
import numpy as np

STATE = ("mark", "written_rows", "episodes", "rows_cut", "expired")
OBS = 23


def window(k, slots):
    """(W, lo): the intact transitions per lane and the oldest intact ring step."""
    k = max(int(k), 0)
    W = min(k, slots - 1)
    return W, k - W


def plan(mark, recs, written, record_capacity, k, n_envs, slots, tail=0, step_base=0):
    """recs: dict of lane, end_step, len, success (arrays of at least min(written, record_capacity) entries).  Returns (episodes,
    totals): episodes a list of (s, lane, first, rows) in ascending (s, lane) order -- the episode's rows are the ring steps first ..
    s --, totals a dict of m (the window's end), rows, episodes, rows_cut, expired."""
    m = min(int(written), int(record_capacity))
    mark = min(max(int(mark), 0), m)
    k = max(int(k), 0)
    W, lo = window(k, slots)
    out, cut, expired = [], 0, 0
    for j in range(mark, m):
        if not recs["success"][j]:
            continue
        e, L, s = int(recs["lane"][j]), int(recs["len"][j]), int(recs["end_step"][j]) + int(step_base)
        if e < 0 or e >= n_envs or L < 1 or s >= k:          # not a record of this ring
            continue
        if s < lo:
            expired += 1
            continue
        want = L if tail == 0 else min(L, tail)
        first = max(s - want + 1, lo)
        rows = s - first + 1
        cut += want - rows
        out.append((s, e, first, rows))
    out.sort()
    return out, dict(m=m, rows=sum(r for _, _, _, r in out), episodes=len(out), rows_cut=cut, expired=expired)


def harvest(state, side, ring, k, recs, written, record_capacity, capacity, tail=0, step_base=0):
    """state int64 [8], side a dict of the REGION's arrays (obs [capacity, 23], act, rew, obs2, done), ring a dict of obs
    [slots, n, 23], act, rew, done [slots, n]: returns (state, side) after the harvest, both new arrays."""
    state = np.array(state, dtype=np.int64)
    side = {name: np.array(a) for name, a in side.items()}
    slots, n = ring["act"].shape
    episodes, tot = plan(state[0], recs, written, record_capacity, k, n, slots, tail, step_base)
    R, r = tot["rows"], 0
    for s, e, first, rows in episodes:
        for j in range(first, s + 1):
            if r >= R - capacity:
                at = (int(state[1]) + r) % capacity
                t, t1 = j % slots, (j + 1) % slots
                side["obs"][at], side["obs2"][at] = ring["obs"][t, e], ring["obs"][t1, e]
                side["act"][at], side["rew"][at], side["done"][at] = ring["act"][t, e], ring["rew"][t, e], ring["done"][t, e]
            r += 1
    state[0] = tot["m"]
    state[1] += R
    state[2] += tot["episodes"]
    state[3] += tot["rows_cut"]
    state[4] += tot["expired"]
    state[5:] = 0
    return state, side


def empty_region(capacity):
    return dict(obs=np.zeros((capacity, OBS), np.float32), act=np.zeros(capacity, np.float32), rew=np.zeros(capacity, np.float32),
                obs2=np.zeros((capacity, OBS), np.float32), done=np.zeros(capacity, np.uint8))


def planted(n_envs, slots, seed=0):
    """A ring whose every word is a distinct finite f32 bit pattern (so a misplaced copy shows), done flags from the seed."""
    rng = np.random.RandomState(seed)
    words = slots * n_envs * (OBS + 2)
    assert words < 2 ** 23
    bits = np.arange(words, dtype=np.uint32) + np.uint32(0x3F000000)       # 0.5 and up, one ulp apart
    rng.shuffle(bits)
    f = bits.view(np.float32)
    o = slots * n_envs * OBS
    return dict(obs=f[:o].reshape(slots, n_envs, OBS).copy(), act=f[o:o + slots * n_envs].reshape(slots, n_envs).copy(),
                rew=f[o + slots * n_envs:].reshape(slots, n_envs).copy(),
                done=rng.randint(0, 2, (slots, n_envs)).astype(np.uint8))


# The reset pool of the loop tests: the trailer straight above the goal (0, -30, pi / 2), which the truck backs onto in 0.4 m steps.
# tests/test_success_replay_cpu.py shows with the C oracle that every pose ends in success within 8 steps whatever the steering.
POSE_POOL = np.array([[0.0, -30.0 + d, np.pi / 2] for d in (0.9, 1.3, 1.7, 2.1)], dtype=np.float64)
