"""The start-pose curriculum's host model (include/ttenv.h: tt_env_set_curriculum): numpy on
td3_ref.philox4x32, written from the rules of the header and not from the kernels' control flow.

    cell_of / cell_index      c = (iyaw * ny + iy) * nx + ix and back
    weights(p, mode, uniform) q = min(65536, 1 + floor(65535 (u + (1 - u) f))), f = 4 p (1 - p) or 1 - p;  cum = cumsum(q)
    update(...)               p, seen, q, cum after tt_env_curriculum_update
    draw(...)                 the cell and the pose of (seed, env, episode) under a cum

f64 throughout, one rounding per operation (numpy does not contract), integers for everything that decides a draw."""
import numpy as np

from td3_ref import philox4x32

RESET_TAG = 0x7452          # csrc/ttenv_state.h: the Philox domain of the reset's draw
NO_CELL = 0xFFFFFFFF
MODES = ("frontier", "hard")


def cell_of(bins, ix, iy, iyaw):
    nx, ny, _ = bins
    return (iyaw * ny + iy) * nx + ix


def cell_index(bins, c):
    nx, ny, _ = bins
    c = np.asarray(c)
    return c % nx, (c // nx) % ny, c // (nx * ny)


def weights(p, mode, uniform):
    """(q, cum) as uint32 arrays from the success rates p."""
    assert mode in MODES
    p = np.asarray(p, dtype=np.float64)
    u = np.float64(uniform)
    f = np.float64(4.0) * p * (np.float64(1.0) - p) if mode == "frontier" else np.float64(1.0) - p
    w = u + (np.float64(1.0) - u) * f
    q = np.minimum(65536, 1 + np.floor(w * np.float64(65535.0)).astype(np.int64))
    cum = np.cumsum(q)
    assert cum[-1] < 2 ** 32
    return q.astype(np.uint32), cum.astype(np.uint32)


def update(p, seen, attempts, successes, mode, alpha, uniform):
    """The arrays after one update: (p, seen, q, cum); the counters are zero afterwards."""
    p = np.array(p, dtype=np.float64)
    n = np.asarray(attempts).astype(np.uint32).astype(np.float64)
    s = np.asarray(successes).astype(np.uint32).astype(np.float64)
    a = np.float64(alpha)
    hit = n > 0
    rate = s[hit] / n[hit]
    p[hit] = (np.float64(1.0) - a) * p[hit] + a * rate
    seen = np.asarray(seen).astype(np.uint64) + np.asarray(attempts).astype(np.uint32).astype(np.uint64)
    q, cum = weights(p, mode, uniform)
    return p, seen, q, cum


def pick(r3, cum):
    """The cell of the fourth Philox word(s) r3 under cum: t = (r3 * cum[-1]) >> 32, the smallest c with cum[c] > t."""
    cum = np.asarray(cum).astype(np.uint64)
    t = (np.asarray(r3, dtype=np.uint64) * cum[-1]) >> np.uint64(32)
    return np.searchsorted(cum, t, side="right").astype(np.int64)


def draw(seed, env, episode, cum, bins, lo, hi):
    """(cell [k] int64, pose [k, 3] f64) of lanes `env` at episode numbers `episode` under reset seed `seed`."""
    seed = int(seed) & (2 ** 64 - 1)
    r = philox4x32(np.asarray(env), np.asarray(episode), 0, RESET_TAG, seed & 0xFFFFFFFF, seed >> 32)
    c = pick(r[3], cum)
    idx = cell_index(bins, c)
    pose = np.empty((c.shape[0], 3), dtype=np.float64)
    for d in range(3):
        u = (r[d].astype(np.float64) + np.float64(0.5)) * np.float64(1.0 / 4294967296.0)
        width = (np.float64(hi[d]) - np.float64(lo[d])) / np.float64(bins[d])
        pose[:, d] = np.float64(lo[d]) + (idx[d].astype(np.float64) + u) * width
    return c, pose
