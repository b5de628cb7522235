"""Task curriculum of the vector loop (include/ttenv.h: tt_env_set_task_curriculum; csrc/ttenv_task.h: k_step_task, k_step_task_log,
k_reset_task): with episode randomisation on, the env counts, per cell of a grid over the ranges of goal x,
goal y, goal yaw and L2, how the episodes whose task was drawn there end, and draws the next task by weights made from those counts
-- on the device, inside the env step and one small launch every `every` vector steps.  The cells' success rates are the per-task
statistic; the weighted draw is the curriculum.

    TaskCurriculum         bins (ngx, ngy, ngyaw, nl2), every, mode, alpha, uniform
    check_task_curriculum  every combination a loop refuses with it, as one pure function
    cell_of, cell_index    the cell <-> (igx, igy, igyaw, il2) map: c = ((il2 * ngyaw + igyaw) * ngy + igy) * ngx + igx
    task_summary           what tools/train_vector.py prints of its state, with the success rate per bin of each dimension

The update rule and the two modes are the start-pose curriculum's (curriculum.py)."""
import math

from ddpg_trucktrailer_amd import _lib as L
from ddpg_trucktrailer_amd.options import Option, is_number, refuse, refuse_value, whole_number

DIMENSIONS = ("goal_x", "goal_y", "goal_yaw", "L2")       # the order of bins, and of the cell index from its lowest digit up


class TaskCurriculum(Option):
    """bins: (ngx, ngy, ngyaw, nl2), whole numbers >= 1 with at most 4096 cells, one bin on every range of width 0; every: vector
    steps between updates, >= 1; mode: "frontier" or "hard"; alpha: the running rate's step, in (0, 1]; uniform: the share of the
    weight every cell keeps, in [0, 1]."""
    FIELDS = ("bins", "every", "mode", "alpha", "uniform")

    def __init__(self, bins, every=64, mode="frontier", alpha=0.1, uniform=0.1):
        if not (isinstance(bins, (tuple, list)) and len(bins) == 4):
            refuse_value("bins", bins, "four whole numbers (ngx, ngy, ngyaw, nl2)")
        for n, b in zip(("ngx", "ngy", "ngyaw", "nl2"), bins):
            whole_number(f"bins: {n}", b, 1)
        cells = bins[0] * bins[1] * bins[2] * bins[3]
        if cells > L.CURRICULUM_MAX_CELLS:
            refuse_value("bins", tuple(bins), f"a grid of at most {L.CURRICULUM_MAX_CELLS} cells (it has {cells})")
        whole_number("every", every, 1)
        if mode not in L.CURRICULUM_MODES:
            refuse_value("mode", mode, "one of " + ", ".join(repr(m) for m in L.CURRICULUM_MODES))
        if not (is_number(alpha) and math.isfinite(alpha) and 0 < alpha <= 1):
            refuse_value("alpha", alpha, "a number in (0, 1]")
        if not (is_number(uniform) and math.isfinite(uniform) and 0 <= uniform <= 1):
            refuse_value("uniform", uniform, "a finite number in [0, 1]")
        self.bins, self.every, self.mode = tuple(int(b) for b in bins), int(every), mode
        self.alpha, self.uniform = float(alpha), float(uniform)

    @property
    def cells(self):
        return self.bins[0] * self.bins[1] * self.bins[2] * self.bins[3]

    def c_struct(self):
        return L.TTTaskCurriculum((L.C.c_int32 * 4)(*self.bins), L.CURRICULUM_MODES.index(self.mode), self.alpha, self.uniform)

    def check_ranges(self, rand):
        """ValueError when a range of `rand` (a resolved EpisodeRandomization) with width 0 has more than one bin: its cells could
        not be told apart."""
        lo, hi = (*rand.goal_lo, rand.L2_lo), (*rand.goal_hi, rand.L2_hi)
        for name, n, a, b in zip(DIMENSIONS, self.bins, lo, hi):
            if n > 1 and not b - a > 0:
                raise ValueError(f"task_curriculum: {n} bins on the {name} range [{a}, {b}], which has width 0 (its cells could not be "
                                 "told apart)")


def check_task_curriculum(cur, randomize=None, population=False, data_parallel=False, force_dp=False, device=None):
    """What is refused with a task curriculum, each a ValueError, in this order: no `randomize`, a population, data-parallel ranks
    (or the p2p exchange), the TT_FORCE_DP launch structure, an env that is not on a GPU (device None: not known yet).  What
    episode randomisation refuses (randomize.check_randomization) is refused there.  Returns cur."""
    TaskCurriculum.expect("task_curriculum", cur)
    return refuse("task_curriculum", cur, randomize=randomize, population=population, data_parallel=data_parallel, force_dp=force_dp,
                  device=device)


def cell_of(bins, igx, igy, igyaw, il2):
    ngx, ngy, ngyaw, _ = bins
    return ((il2 * ngyaw + igyaw) * ngy + igy) * ngx + igx


def cell_index(bins, c):
    """(igx, igy, igyaw, il2) of cell c."""
    ngx, ngy, ngyaw, _ = bins
    return c % ngx, (c // ngx) % ngy, (c // (ngx * ngy)) % ngyaw, c // (ngx * ngy * ngyaw)


def task_summary(state, randomize):
    """Of TruckTrailerVecEnv.task_curriculum_state() and the resolved EpisodeRandomization its cells lie on
    (TruckTrailerVecEnv.randomization_ranges()): the share of cells with an episode counted, the mean p, the share of the draw weight
    the top decile of cells holds (0.1 for equal weights), and per dimension "by_<name>": a list over its bins of (lo, hi, episodes
    seen, the seen-weighted mean of p -- None where nothing was seen), e.g. by_L2, the success by trailer length."""
    seen, p, q = (state[k].double() for k in ("seen", "p", "q"))           # [nl2, ngyaw, ngy, ngx]
    flat = q.reshape(-1)
    top = max(1, -(-flat.numel() // 10))
    out = {"cells_seen": float((seen > 0).double().mean()), "mean_p": float(p.mean()),
           "top_decile_weight": float(flat.sort(descending=True).values[:top].sum() / flat.sum())}
    lo, hi = (*randomize.goal_lo, randomize.L2_lo), (*randomize.goal_hi, randomize.L2_hi)
    for d, name in enumerate(DIMENSIONS):
        axis = 3 - d                                                         # (goal_x is the last axis)
        others = tuple(a for a in range(4) if a != axis)
        n, ps = seen.sum(dim=others), (seen * p).sum(dim=others)
        w = (hi[d] - lo[d]) / n.numel()
        out["by_" + name] = [(lo[d] + k * w, lo[d] + (k + 1) * w, int(n[k]), float(ps[k] / n[k]) if n[k] > 0 else None)
                             for k in range(n.numel())]
    return out
