"""Episode randomisation of the vector loop (include/ttenv.h: tt_env_set_randomization; csrc/ttenv_randomize.h: k_step_rnd,
k_step_rnd_log, k_reset_rnd): at every reset of a lane -- reset(), the masked reset, the step's auto-reset --
the env draws the new episode's goal (x, y, yaw) and trailer length L2 uniformly from configured ranges, on the device, as a pure
function of (reset seed, lane, episode number).  The start pose is drawn as without the option.

    EpisodeRandomization   goal ((lo3, hi3) or None: the parameters' goal), L2 ((lo, hi) or None: the parameters' L2)
    check_randomization    every combination a loop refuses with it, as one pure function
    summary                what tools/train_vector.py prints: the ranges and the lanes' current goals and lengths

The draw: r = philox4x32(lane, episode, 1, 0x7452, seed);  value = lo + (hi - lo) * ((r[k] + 0.5) / 2^32) with k = 0, 1, 2 for the
goal's x, y, yaw and 3 for L2, in f64 with every operation rounded on its own: a range of width 0 gives its bound exactly."""
import math

from ddpg_trucktrailer_amd import _lib as L
from ddpg_trucktrailer_amd.options import Option, is_number, refuse, refuse_value


def _finite(x):
    return is_number(x) and math.isfinite(x)


class EpisodeRandomization(Option):
    """goal: ((x_lo, y_lo, yaw_lo), (x_hi, y_hi, yaw_hi)), finite with lo <= hi, or None (the env's parameters' goal, not drawn);
    L2: (lo, hi), finite with 0 < lo <= hi, or None (the parameters' L2).  At least one is given.  A None is resolved against the
    env's parameters when the option is enabled (resolved()); the option itself, and a checkpoint, keep it as given."""
    FIELDS = ("goal_lo", "goal_hi", "L2_lo", "L2_hi")
    A = "an"

    def __init__(self, goal=None, L2=None):
        if goal is None and L2 is None:
            raise ValueError("EpisodeRandomization: goal and L2 are both None (nothing would be drawn)")
        self.goal_lo = self.goal_hi = self.L2_lo = self.L2_hi = None
        if goal is not None:
            if not (isinstance(goal, (tuple, list)) and len(goal) == 2 and
                    all(isinstance(b, (tuple, list)) and len(b) == 3 and all(_finite(v) for v in b) for b in goal)):
                refuse_value("goal", goal, "a pair (lo, hi) of three finite numbers (x, y, yaw) each")
            lo, hi = (tuple(float(v) for v in b) for b in goal)
            for name, a, b in zip(("x", "y", "yaw"), lo, hi):
                if a > b:
                    refuse_value(f"goal: {name}", (a, b), "a range with lo <= hi")
            self.goal_lo, self.goal_hi = lo, hi
        if L2 is not None:
            if not (isinstance(L2, (tuple, list)) and len(L2) == 2 and all(_finite(v) for v in L2)):
                refuse_value("L2", L2, "a pair (lo, hi) of finite numbers")
            lo, hi = float(L2[0]), float(L2[1])
            if not 0 < lo <= hi:
                refuse_value("L2", (lo, hi), "a range with 0 < lo <= hi")
            self.L2_lo, self.L2_hi = lo, hi

    @classmethod
    def from_tuple(cls, t):
        goal_lo, goal_hi, l2_lo, l2_hi = t
        return cls(goal=None if goal_lo is None else (tuple(goal_lo), tuple(goal_hi)), L2=None if l2_lo is None else (l2_lo, l2_hi))

    def resolved(self, params):
        """The option with every None replaced by the value of `params` (a tt_params): ranges of width 0 there."""
        goal = (self.goal_lo, self.goal_hi) if self.goal_lo is not None else (tuple(params.goal),) * 2
        l2 = (self.L2_lo, self.L2_hi) if self.L2_lo is not None else (float(params.L2),) * 2
        return EpisodeRandomization(goal=goal, L2=l2)

    def c_struct(self, params):
        r = self.resolved(params)
        return L.TTRandomization((L.C.c_double * 3)(*r.goal_lo), (L.C.c_double * 3)(*r.goal_hi), r.L2_lo, r.L2_hi)


def check_randomization(rand, population=False, data_parallel=False, force_dp=False, curriculum=None, expert=None, labels=None,
                        device=None, episode_log_detail=False):
    """What is refused with episode randomisation, each a ValueError, in this order: a population, data-parallel ranks (or the p2p
    exchange), the TT_FORCE_DP launch structure, a curriculum, expert lanes, expert labels, an env that is not on a GPU (device
    None: not known yet), the detailed episode log.  Returns rand."""
    EpisodeRandomization.expect("randomize", rand)
    return refuse("randomize", rand, population=population, data_parallel=data_parallel, force_dp=force_dp, curriculum=curriculum,
                  expert=expert, labels=labels, device=device, episode_log_detail=bool(episode_log_detail))


def summary(rand, episode):
    """Of an EpisodeRandomization (resolved or not) and TruckTrailerVecEnv.episode(): the ranges, and the min / mean / max over the
    lanes of their current episode's L2 and goal x, y, yaw."""
    out = {"goal_lo": rand.goal_lo, "goal_hi": rand.goal_hi, "L2_lo": rand.L2_lo, "L2_hi": rand.L2_hi}
    cols = {"L2": episode["L2"].double().reshape(-1)}
    goal = episode["goal"].double().reshape(-1, 3)
    for k, name in enumerate(("goal_x", "goal_y", "goal_yaw")):
        cols[name] = goal[:, k]
    for name, v in cols.items():
        out[name] = (float(v.min()), float(v.mean()), float(v.max()))
    return out
