"""Gradient-norm clipping in learn(): torch.nn.utils.clip_grad_norm_ in front of each optimizer step (include/ttenv.h: tt_grad_clip;
csrc/ttclip.hip).

    GradClip          critic and actor: each None (that network's step is the plain one) or max_norm, a finite number > 0
    check_grad_clip   every combination a loop or a learner refuses with a clip, as one pure function

    norm = sqrt(sum of squares over every element of the network's gradient)
    coef = max_norm / (norm + 1e-6), 1 where that is greater than 1            (clip_grad_norm_'s formula)
    the optimizer sees coef * grad; weight decay is added after the clip, as torch.optim.Adam adds it inside step()

The norm is GLOBAL, so a clipped network's update cannot ride in the weight-gradient launch: with a clip the lone learner runs the
separate-optimizer order (weight gradients with no optimizer step, then tt_adam_soft_update[_clipped]) at both sites.

The torch form is Agent(grad_clip=).learn_batch (agent.py): the CPU path, and the twin the kernels are tested against."""
from ddpg_trucktrailer_amd.options import Option, finite_number, refuse, refuse_value


class GradClip(Option):
    """critic, actor: None, or max_norm, a finite number > 0.  At least one has a value."""
    FIELDS = ("critic", "actor")

    def __init__(self, critic=None, actor=None):
        finite_number("critic", critic, "> 0", or_none=True)
        finite_number("actor", actor, "> 0", or_none=True)
        if critic is None and actor is None:
            refuse_value("grad_clip", (critic, actor), "a clip of at least one network (no clip is grad_clip=None)")
        self.critic = None if critic is None else float(critic)
        self.actor = None if actor is None else float(actor)


def check_grad_clip(clip, td3=None, population=False, data_parallel=False, force_dp=False, demo_loss=None, expert=None, labels=None):
    """What is refused with a clip, each a ValueError that names grad_clip: the paths with optimizer launches of their own (TD3,
    populations, data-parallel ranks, the p2p exchange, the TT_FORCE_DP launch structure) and the demonstration entry points
    (demo_loss, expert lanes, expert labels), whose tails carry the optimizer step."""
    GradClip.expect("grad_clip", clip)
    return refuse("grad_clip", clip, td3=td3, population=population, data_parallel=data_parallel, force_dp=force_dp, demo_loss=demo_loss,
                  expert=expert, labels=labels)
