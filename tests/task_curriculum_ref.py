"""The task curriculum's host model (include/ttenv.h: tt_env_set_task_curriculum): numpy on
td3_ref.philox4x32, built on randomize_ref (the words, u01) and curriculum_ref (pick, update, weights), written from the rule of
the header and not from the kernels.

    cell_of / cell_index             c = ((il2 * ngyaw + igyaw) * ngy + igy) * ngx + igx and back
    place(r, c, bins, rand)          (goal [k, 3], L2 [k]) of task words r [4][k] inside cells c
    draw(seed, env, episode, cum, bins, rand)   (cell [k], goal [k, 3], L2 [k]) of lanes `env` at episode numbers `episode`

`rand` is randomize_ref's (goal_lo, goal_hi, L2_lo, L2_hi).  value = lo + (i + u) * ((hi - lo) / n), f64 with one rounding per
operation; the cell from the words with third counter word PICK_WORD: t = (s[0] * cum[-1]) >> 32, the smallest c with cum[c] > t."""
import numpy as np

import curriculum_ref
import randomize_ref
from curriculum_ref import MODES, NO_CELL, update, weights      # (the update is the start-pose curriculum's) # noqa: F401

PICK_WORD = 2        # the third counter word of the cell pick (randomize_ref: 0 the start pose's, 1 the task's)


def cell_of(bins, igx, igy, igyaw, il2):
    ngx, ngy, ngyaw, _ = bins
    return ((il2 * ngyaw + igyaw) * ngy + igy) * ngx + igx


def cell_index(bins, c):
    ngx, ngy, ngyaw, _ = bins
    c = np.asarray(c)
    return c % ngx, (c // ngx) % ngy, (c // (ngx * ngy)) % ngyaw, c // (ngx * ngy * ngyaw)


def place(r, c, bins, rand):
    goal_lo, goal_hi, l2_lo, l2_hi = rand
    lo, hi = (*goal_lo, l2_lo), (*goal_hi, l2_hi)
    idx = cell_index(bins, c)
    cols = []
    for d in range(4):
        width = (np.float64(hi[d]) - np.float64(lo[d])) / np.float64(bins[d])
        cols.append(np.float64(lo[d]) + (np.asarray(idx[d]).astype(np.float64) + randomize_ref.u01(r[d])) * width)
    return np.stack(cols[:3], axis=1), cols[3]


def draw(seed, env, episode, cum, bins, rand):
    r = randomize_ref.words(seed, env, episode, randomize_ref.TASK_WORD)
    s = randomize_ref.words(seed, env, episode, PICK_WORD)
    c = curriculum_ref.pick(s[0], cum)
    goal, l2 = place(r, c, bins, rand)
    return c, goal, l2
