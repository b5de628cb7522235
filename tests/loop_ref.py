"""What tests/test_loop_ref_cpu.py (CPU) and tests/test_gpu_loop_lockstep.py (GPU) share: a plain host model of one vector step of
the DDPG loop (rollout.py's docstring has the step), in numpy / torch on the CPU, with no HIP in it.

Every random number of the library is a pure function of (seed, counters) through Philox4x32-10, so each stream is restated here
from its definition -- reset poses, the env's random actions, the OU normals, the replay draw -- on td3_ref's numpy Philox (pinned
to Random123's known-answer vectors by tests/test_td3_cpu.py).  LoopRef holds what the model knows at vector step t: the lanes'
episode numbers, a C oracle of the N lanes, and the order rule (which steps learn, and from which window).

Nothing here follows the kernels' control flow: each function is the rule as the docstrings state it, in f64 or exact integers."""
import math
import types

import numpy as np

from nstep_ref import walk64
from td3_ref import philox4x32

MASK32, MASK64 = 0xFFFFFFFF, 2 ** 64 - 1
POSE_TAG, ACTION_TAG, OU_TAG, DRAW_TAG = 0x7452, 0xAC71, 0x0A5E, 0x5A3D      # the Philox domains (counter word 3)
SEED_STRIDE = 0x9E3779B97F4A7C15       # update u of a vector step draws with seed + u * SEED_STRIDE (mod 2^64)
PIPE_RESERVE, PIPE_LAG = 2, 1          # the pipelined order's window (rollout.py's docstring)
# OU noise (noise.py): theta 0.2, sigma 0.15, dt 0.01, as the f32 numbers the policy launch is given
OU_DECAY = float(np.float32(1.0 - 0.2 * 0.01))
OU_SCALE = float(np.float32(0.15 * math.sqrt(0.01)))
HIGH = np.float32(math.pi / 4)         # action_space.high


def _key(seed):
    seed = int(seed) & MASK64
    return seed & MASK32, seed >> 32


def _lo_hi(x):
    x = np.asarray(x, dtype=np.uint64)
    return x & np.uint64(MASK32), x >> np.uint64(32)


def u01(x):
    """A 32-bit word as a uniform in (0, 1), f64: (x + 0.5) / 2^32."""
    return (np.asarray(x, dtype=np.uint64).astype(np.float64) + 0.5) / 4294967296.0


# ---- the env's streams ------------------------------------------------------------------------------------------------
def reset_box():
    """(lo [3], hi [3]) of the default reset box (x, y, yaw), read from the library's default parameters."""
    from ddpg_trucktrailer_amd import _lib as L
    p = L.default_params(0)
    return np.array(list(p.reset_lo), np.float64), np.array(list(p.reset_hi), np.float64)


def reset_pose(seed, env, episode):
    """Start pose (x, y, yaw) of episode number `episode` of lane `env` under reset seed `seed`, f64 [..., 3].  episode is 0 after a
    full reset(seed) and goes up by one with every auto-reset or masked reset of the lane."""
    r = philox4x32(env, episode, 0, POSE_TAG, *_key(seed))
    lo, hi = reset_box()
    return np.stack([lo[i] + (hi[i] - lo[i]) * u01(r[i]) for i in range(3)], axis=-1)


def random_action(seed, env, step):
    """tt_env_random_actions: the steering of lane `env` at step `step` under policy seed `seed`, f32, uniform in +-pi/4."""
    r = philox4x32(env, *_lo_hi(step), ACTION_TAG, *_key(seed))
    return ((2.0 * u01(r[0]) - 1.0) * (math.pi / 4)).astype(np.float32)


# ---- OU noise ---------------------------------------------------------------------------------------------------------
def ou_normal(seed, st, rows):
    """The standard normal of rows 0 .. rows - 1 at vector step st (a number, or an array [m]: the result is then [m, rows]): Philox
    (row, st, OU_TAG, seed), the two uniforms ((r >> 8) + 0.5) 2^-24 and the angle 2 pi u2 formed exactly in f32, then log, sqrt and
    cos in f64 (Box-Muller)."""
    st = np.asarray(st, dtype=np.uint64)
    row = np.arange(rows, dtype=np.uint64)
    if st.ndim:
        st, row = st[:, None], row[None, :]
    r0, r1, _, _ = philox4x32(row, *_lo_hi(st), OU_TAG, *_key(seed))
    f32 = np.float32
    u1 = ((r0 >> np.uint64(8)).astype(f32) + f32(0.5)) * f32(1.0 / 16777216.0)
    u2 = ((r1 >> np.uint64(8)).astype(f32) + f32(0.5)) * f32(1.0 / 16777216.0)
    angle = (f32(6.28318530717958647692) * u2).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(angle)


def ou_next(x_prev, restart, normal):
    """x <- x (1 - theta dt) + sigma sqrt(dt) N in f64, from 0 for a lane whose episode ended at the previous step."""
    x0 = np.where(np.asarray(restart, dtype=bool), 0.0, np.asarray(x_prev, dtype=np.float64))
    return x0 * OU_DECAY + OU_SCALE * np.asarray(normal, dtype=np.float64)


# ---- the replay draw --------------------------------------------------------------------------------------------------
def update_seed(seed, u):
    return (int(seed) + u * SEED_STRIDE) & MASK64


def _draw_words(seed, k_counter, batch, slots, reserve, lag):
    k = max(int(k_counter) - lag, 0)
    avail = min(k, slots - 1 - reserve)
    r = philox4x32(np.arange(batch), k & MASK32, k >> 32, DRAW_TAG, *_key(seed))
    return k, avail, r


def draw(seed, k_counter, batch, n_envs, slots, reserve=0, lag=0):
    """The (slot, env) of rows 0 .. batch - 1 of a one-step draw with no side tuples, int64 [batch, 2], when the device counter the
    draw reads holds k_counter."""
    k, avail, r = _draw_words(seed, k_counter, batch, slots, reserve, lag)
    back = ((r[0] * np.uint64(avail)) >> np.uint64(32)).astype(np.int64)
    env = ((r[1] * np.uint64(n_envs)) >> np.uint64(32)).astype(np.int64)
    return np.stack([(k - 1 - back) % slots, env], axis=1)


def draw_nstep(seed, k_counter, batch, n_envs, slots, n_step, reserve=0, lag=0):
    """The base (slot, env) of an n-step draw: the same words over the base steps that have their n steps inside the window (their
    number counts as 1 when there is none: an early draw's rows are in bounds and meaningless)."""
    k, avail, r = _draw_words(seed, k_counter, batch, slots, reserve, lag)
    avail_n = max(avail - (n_step - 1), 1)
    back = (n_step - 1) + ((r[0] * np.uint64(avail_n)) >> np.uint64(32)).astype(np.int64)
    env = ((r[1] * np.uint64(n_envs)) >> np.uint64(32)).astype(np.int64)
    return np.stack([(k - 1 - back) % slots, env], axis=1)


def draw_side(seed, k_counter, batch, n_envs, slots, side_count, reserve=0, lag=0):
    """A one-step draw from a ring with side_count stand-alone tuples (TrajectoryRing.load_side): every one of the avail * n_envs
    ring transitions and the side tuples is as likely.  Row b is side tuple j -- the pair (-1, j), j = (r0 * side_count) >> 32 --
    when (u * (avail * n_envs + side_count)) >> 64 < side_count with u the 64-bit word r2 : r3, and draw()'s ring row otherwise."""
    k, avail, r = _draw_words(seed, k_counter, batch, slots, reserve, lag)
    idx = draw(seed, k_counter, batch, n_envs, slots, reserve, lag)
    total = avail * n_envs + side_count
    for b in range(batch):
        u = (int(r[2][b]) << 32) | int(r[3][b])
        if (u * total) >> 64 < side_count:
            idx[b] = (-1, (int(r[0][b]) * side_count) >> 32)
    return idx


def gather_side(ring, side, idx):
    """gather() where idx may hold side rows (-1, j): those come from side = dict of numpy obs, act, rew, obs2, done [M, ...]."""
    is_side, j = idx[:, 0] < 0, idx[:, 1]
    out = [x.copy() for x in gather(ring, np.where(is_side[:, None], 0, idx))]
    for i, key in enumerate(("obs", "act", "rew", "obs2", "done")):
        out[i][is_side] = side[key][j[is_side]].reshape(out[i][is_side].shape)
    return out


def window(k_counter, slots, reserve=0, lag=0, n_step=1):
    """The vector steps a draw may return as base steps, oldest to newest (a range, empty when there is none), when the counter holds
    k_counter: the newest complete step is the one `lag` steps before the counter's; the ring keeps slots - 1 complete steps (the
    slot being written holds none) of which the `reserve` oldest are being overwritten; a base step needs its n steps inside."""
    newest = max(int(k_counter) - lag, 0) - 1
    kept = slots - 1 - reserve
    oldest = max(0, newest + 1 - kept)
    return range(oldest, newest - (n_step - 1) + 1)


def step_of_slot(slot, k_counter, slots, lag=0):
    """The newest vector step before the draw's counter that lives in ring slot `slot`."""
    newest = max(int(k_counter) - lag, 0) - 1
    return newest - (newest - np.asarray(slot, dtype=np.int64)) % slots


def gather(ring, idx):
    """The one-step batch (s, a [B, 1], r, s2, done u8) of rows idx [B, 2] = (slot, env) from ring = dict of numpy obs [T, N, 23],
    act, rew, done [T, N]."""
    t, e = idx[:, 0], idx[:, 1]
    slots = ring["obs"].shape[0]
    return ring["obs"][t, e], ring["act"][t, e][:, None], ring["rew"][t, e], ring["obs"][(t + 1) % slots, e], ring["done"][t, e]


def gather_nstep(ring, idx, n_step, gamma):
    """nstep_ref.walk64 on the same dict: s, a, R (f64) with its bound, s2, D, m."""
    import torch
    view = types.SimpleNamespace(**{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in ring.items()})
    return walk64(view, torch.from_numpy(np.ascontiguousarray(idx)), n_step, gamma)


# ---- the loop ---------------------------------------------------------------------------------------------------------
class LoopRef:
    """The host's knowledge of a lone vector loop at step t.

    Order rule (rollout.py's docstring, replay_buffer.learn_start): learn() runs once 1 + n_step steps are counted.  The serial order
    counts after its env step, so learn() of step t runs when t + 1 >= 1 + n_step, and draws with the ring counter t + 1 and the
    whole window.  The pipelined order counts the steps opened before the running one, so learn() of step t runs when t >= 1 + n_step,
    and draws with the counter t, lag 1 and reserve 2: from the steps up to t - 2.  Each learning step makes updates_per_step
    updates, update u with the seed seed + u * SEED_STRIDE.

    k0, u0: the loop starts (a loaded checkpoint) with k0 vector steps and u0 learn steps already made; every method takes the
    ABSOLUTE vector step number t >= k0, and with k0 = u0 = 0 every answer is that of a loop started fresh."""

    def __init__(self, seed, env_seed, n_envs, slots, batch, pipelined, updates_per_step=1, n_step=1, oracle=None, k0=0, u0=0):
        self.seed, self.env_seed, self.n, self.slots, self.batch = int(seed), int(env_seed), n_envs, slots, batch
        self.pipelined, self.updates_per_step, self.n_step = bool(pipelined), int(updates_per_step), int(n_step)
        self.k0, self.u0 = int(k0), int(u0)
        self.episode = np.zeros(n_envs, np.int64)
        self.oracle = oracle

    # -- env
    def start_poses(self, lanes=None):
        lanes = np.arange(self.n) if lanes is None else np.asarray(lanes)
        return reset_pose(self.env_seed, lanes, self.episode[lanes])

    def restart(self, lanes):
        """The lanes move on to their next episode: its pose, and the oracle lanes placed there.  Returns (poses, first observations)."""
        lanes = np.asarray(lanes)
        self.episode[lanes] += 1
        poses = self.start_poses(lanes)
        obs = self.oracle.place_lanes(lanes, poses) if self.oracle is not None else None
        return poses, obs

    # -- noise
    def noise(self, t, x_before, done_prev):
        """(x after the policy launch of step t, the normals): done_prev [N] = the done flags of step t - 1 (None at t = 0)."""
        nrm = ou_normal(self.seed, t, self.n)
        restart = np.zeros(self.n, bool) if done_prev is None else np.asarray(done_prev) != 0
        return ou_next(x_before, restart, nrm), nrm

    # -- learn()
    def learns(self, t):
        counted = t if self.pipelined else t + 1
        return counted >= 1 + self.n_step

    def updates_after(self, t):
        """learn() calls made once step t is over: u0, and updates_per_step for each of the steps k0 .. t that learn -- those from
        the first learning step on, 1 + n_step (pipelined) or n_step (serial)."""
        first = max(self.k0, 1 + self.n_step if self.pipelined else self.n_step)
        return self.u0 + self.updates_per_step * max(0, int(t) - first + 1)

    def draw_window(self, t):
        """(counter, reserve, lag) of the draws of step t."""
        return (t, PIPE_RESERVE, PIPE_LAG) if self.pipelined else (t + 1, 0, 0)

    def draws(self, t):
        """[(slot, env) rows of update u for u in 0 .. updates_per_step - 1] of step t."""
        counter, reserve, lag = self.draw_window(t)
        out = []
        for u in range(self.updates_per_step):
            s = update_seed(self.seed, u)
            if self.n_step > 1:
                out.append(draw_nstep(s, counter, self.batch, self.n, self.slots, self.n_step, reserve, lag))
            else:
                out.append(draw(s, counter, self.batch, self.n, self.slots, reserve, lag))
        return out

    def window(self, t):
        counter, reserve, lag = self.draw_window(t)
        return window(counter, self.slots, reserve, lag, self.n_step)

    def steps_of(self, t, idx):
        counter, _, lag = self.draw_window(t)
        return step_of_slot(idx[:, 0], counter, self.slots, lag)
