"""Success replay of the vector loop (include/ttenv.h: tt_ring_harvest, tt_env_harvest; csrc/ttenv_harvest.h: k_harvest_plan,
k_harvest_copy): every `every` vector steps, between graph replays, the transitions of the episodes that ended
in success since the last look are copied from the trajectory ring into a region of the ring's side buffer, first in first out.
They take part in every uniform draw with the ring's transitions, and with demo_loss they are demonstration rows, cloned behind the
Q-filter: the agent as its own demonstrator.

    SuccessReplay         capacity (rows of the region), every, tail
    check_success_replay  every combination a loop refuses with it, as one pure function
    summary               what tools/train_vector.py prints of DDPGRollout.success_replay_stats()"""
from ddpg_trucktrailer_amd.options import Option, refuse, whole_number


class SuccessReplay(Option):
    """capacity: rows of the side buffer's region, >= 1 (the oldest rows are overwritten); every: vector steps between harvests,
    >= 1 -- a successful episode is harvested whole when it is no longer than replay_slots - 1 - every steps, else its newest rows;
    tail: 0 = whole episodes, n >= 1 = the last n transitions of each."""
    FIELDS = ("capacity", "every", "tail")

    def __init__(self, capacity, every=32, tail=0):
        whole_number("capacity", capacity, 1, 2 ** 31 - 1)
        whole_number("every", every, 1)
        whole_number("tail", tail, 0, 2 ** 31 - 1)
        self.capacity, self.every, self.tail = int(capacity), int(every), int(tail)


def check_success_replay(value, episode_log=None, td3=None, n_step=1, population=False, data_parallel=False, force_dp=False,
                         expert=None, labels=None, device=None):
    """What is refused with success replay, each a ValueError, in this order: no episode_log, td3, n_step > 1, a population,
    data-parallel ranks (or the p2p exchange), the TT_FORCE_DP launch structure, expert lanes, expert labels, an env that is not on
    a GPU (device None: not known yet).  Returns value."""
    SuccessReplay.expect("success_replay", value)
    return refuse("success_replay", value, episode_log=episode_log, td3=td3, n_step=n_step, population=population,
                  data_parallel=data_parallel, force_dp=force_dp, expert=expert, labels=labels, device=device)


def summary(stats):
    """One line of DDPGRollout.success_replay_stats(): episodes and rows harvested, rows in the draw, what was lost."""
    return (f"success replay: {stats['episodes']} episodes, {stats['rows']} rows harvested, {stats['exposed']} in the draw, "
            f"{stats['rows_cut']} rows cut, {stats['expired']} episodes expired")
