"""Episode randomisation's host model (include/ttenv.h: tt_env_set_randomization): numpy on
td3_ref.philox4x32, written from the rule of the header and not from the kernels.

    words(seed, env, episode, word2)   the reset's Philox words with third counter word `word2`: 0 the start pose's, 1 the task's
    draw(seed, env, episode, rand)     (goal [k, 3], L2 [k]) of lanes `env` at episode numbers `episode`
    start(seed, env, episode, lo, hi)  the start pose [k, 3] of a plain reset from the box lo .. hi
    max_steps(start, goal, step_length, extra_steps)   int(|goal - start| / step_length) + extra_steps

`rand` is (goal_lo, goal_hi, L2_lo, L2_hi), every entry given.  f64 throughout, one rounding per operation (numpy does not contract):
value = lo + (hi - lo) * u, u = (r + 0.5) / 2^32 (exact in f64)."""
import numpy as np

from td3_ref import philox4x32

RESET_TAG = 0x7452          # csrc/ttenv_state.h: the Philox domain of the reset's draws
POSE_WORD, TASK_WORD = 0, 1  # the third counter word of the start pose's draw and of the task's


def words(seed, env, episode, word2):
    seed = int(seed) & (2 ** 64 - 1)
    return philox4x32(np.asarray(env), np.asarray(episode), word2, RESET_TAG, seed & 0xFFFFFFFF, seed >> 32)


def u01(r):
    return (np.asarray(r).astype(np.float64) + np.float64(0.5)) * np.float64(1.0 / 4294967296.0)


def _uniform(lo, hi, r):
    width = np.float64(hi) - np.float64(lo)
    return np.float64(lo) + width * u01(r)


def draw(seed, env, episode, rand):
    goal_lo, goal_hi, l2_lo, l2_hi = rand
    r = words(seed, env, episode, TASK_WORD)
    goal = np.stack([_uniform(goal_lo[d], goal_hi[d], r[d]) for d in range(3)], axis=1)
    return goal, _uniform(l2_lo, l2_hi, r[3])


def start(seed, env, episode, lo, hi):
    """The plain reset's start pose from the box: the same words a randomised env uses for its start pose."""
    r = words(seed, env, episode, POSE_WORD)
    return np.stack([_uniform(lo[d], hi[d], r[d]) for d in range(3)], axis=1)


def max_steps(start_pose, goal, step_length, extra_steps):
    dx, dy = goal[:, 0] - start_pose[:, 0], goal[:, 1] - start_pose[:, 1]
    return (np.sqrt(dx * dx + dy * dy) / np.float64(step_length)).astype(np.int64) + int(extra_steps)
