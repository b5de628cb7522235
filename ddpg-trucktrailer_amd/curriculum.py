"""Start-pose curriculum of the vector loop (include/ttenv.h: tt_env_set_curriculum; csrc/ttenv_curriculum.h: k_step_cur, k_curriculum_update;
DESIGN.md section 37): the env counts, per cell of a grid over its reset box, how the episodes started there end, and draws the next
start pose by weights made from those counts -- all of it on the device, inside the env step and one small launch every `every`
vector steps.

    Curriculum         bins (nx, ny, nyaw), every, mode, alpha, uniform
    check_curriculum   every combination a loop refuses with a curriculum, as one pure function
    cell_of, cell_index   the cell <-> (ix, iy, iyaw) map: c = (iyaw * ny + iy) * nx + ix
    summary            what tools/train_vector.py prints of a curriculum's state

The rule: per cell with n > 0 episodes since the last update, p <- (1 - alpha) p + alpha (successes / n); then for every cell
f = 4 p (1 - p) ("frontier": the cells the policy solves about half the time) or 1 - p ("hard"), w = uniform + (1 - uniform) f and the
integer draw weight q = min(65536, 1 + floor(65535 w)).  p starts at 0.5, where both modes give every cell the same weight."""
import math

from ddpg_trucktrailer_amd import _lib as L
from ddpg_trucktrailer_amd.options import Option, is_number, refuse, refuse_value, whole_number


class Curriculum(Option):
    """bins: (nx, ny, nyaw), whole numbers >= 1 with at most 4096 cells; every: vector steps between updates, >= 1; mode: "frontier" or
    "hard"; alpha: the running rate's step, in (0, 1]; uniform: the share of the weight every cell keeps, in [0, 1]."""
    FIELDS = ("bins", "every", "mode", "alpha", "uniform")

    def __init__(self, bins, every=64, mode="frontier", alpha=0.1, uniform=0.1):
        if not (isinstance(bins, (tuple, list)) and len(bins) == 3):
            refuse_value("bins", bins, "three whole numbers (nx, ny, nyaw)")
        for n, b in zip(("nx", "ny", "nyaw"), bins):
            whole_number(f"bins: {n}", b, 1)
        cells = bins[0] * bins[1] * bins[2]
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
        return self.bins[0] * self.bins[1] * self.bins[2]

    def c_struct(self):
        nx, ny, nyaw = self.bins
        return L.TTCurriculum(nx, ny, nyaw, L.CURRICULUM_MODES.index(self.mode), self.alpha, self.uniform)


def check_curriculum(cur, population=False, data_parallel=False, force_dp=False, expert=None, labels=None, device=None,
                     episode_log_detail=False):
    """What is refused with a curriculum, each a ValueError: a population, data-parallel ranks (or the p2p exchange), the TT_FORCE_DP
    launch structure, expert lanes, expert labels, an env that is not on a GPU (device None: not known yet), the detailed episode
    log.  Returns cur."""
    Curriculum.expect("curriculum", cur)
    return refuse("curriculum", cur, population=population, data_parallel=data_parallel, force_dp=force_dp, expert=expert, labels=labels,
                  device=device, episode_log_detail=bool(episode_log_detail))


def cell_of(bins, ix, iy, iyaw):
    nx, ny, _ = bins
    return (iyaw * ny + iy) * nx + ix


def cell_index(bins, c):
    """(ix, iy, iyaw) of cell c."""
    nx, ny, _ = bins
    return c % nx, (c // nx) % ny, c // (nx * ny)


def summary(state):
    """Of TruckTrailerVecEnv.curriculum_state(): the share of cells with an episode counted, the mean p, and the share of the draw
    weight the top decile of cells holds (0.1 for equal weights)."""
    seen, p, q = (state[k].reshape(-1).double() for k in ("seen", "p", "q"))
    top = max(1, -(-q.numel() // 10))
    return {"cells_seen": float((seen > 0).double().mean()), "mean_p": float(p.mean()),
            "top_decile_weight": float(q.sort(descending=True).values[:top].sum() / q.sum())}
