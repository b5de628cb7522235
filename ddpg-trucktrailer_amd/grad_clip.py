"""Gradient-norm clipping in learn(): torch.nn.utils.clip_grad_norm_ in front of each optimizer step (include/ttenv.h: tt_grad_clip;
csrc/ttclip.hip).

    GradClip          critic and actor: each None (that network's step is the plain one) or max_norm, a finite number > 0
    check_grad_clip   every combination a loop or a learner refuses with a clip, as one pure function
    check_population_grad_clip   a population's own per-agent clip: its forms, and what it is refused with

    norm = sqrt(sum of squares over every element of the network's gradient)
    coef = max_norm / (norm + 1e-6), 1 where that is greater than 1            (clip_grad_norm_'s formula)
    the optimizer sees coef * grad; weight decay is added after the clip, as torch.optim.Adam adds it inside step()

The norm is GLOBAL, so a clipped network's update cannot ride in the weight-gradient launch: with a clip the lone learner runs the
separate-optimizer order (weight gradients with no optimizer step, then tt_adam_soft_update[_clipped]) at both sites.

A population clips per agent (PopulationLearner(grad_clips=), PopulationRollout(grad_clip=); include/ttenv.h: tt_pop_clip): its
launches read each agent's two max_norm values from a table in device memory, where 0 stands for "this network is not clipped".

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


def check_population_grad_clip(clips, K, td3=None, data_parallel=False, device=None):
    """A population's own clip: None, one GradClip for every agent, or a list with one GradClip or None per agent.  Returns None (no
    clip table: the population's launches are the ones they were) or the K entries; any entry that is not None makes the table.
    Refused, each a ValueError that names grad_clip: TD3 populations, by name, and what a population refuses anyway."""
    if clips is None:
        return None
    if isinstance(clips, (list, tuple)):
        if len(clips) != K:
            raise ValueError(f"grad_clip: {len(clips)} values for {K} agents")
        clips = list(clips)
    else:
        clips = [clips] * K
    for c in clips:
        if c is not None:
            GradClip.expect("grad_clip", c)
    if all(c is None for c in clips):
        return None
    return refuse("population_grad_clip", clips, td3=td3, data_parallel=data_parallel, device=device)


def clip_values(clip):
    """(max_norm critic, max_norm actor) of a GradClip or None as the population's table holds them: 0.0 = not clipped."""
    return (0.0, 0.0) if clip is None else (float(clip.critic or 0.0), float(clip.actor or 0.0))


def clip_of_values(critic, actor):
    """The GradClip of two table values (None when both are 0)."""
    return None if not critic and not actor else GradClip(critic or None, actor or None)
