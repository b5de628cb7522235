"""What the loops' options share: the base of the option values (td3.TD3Config, loss_shape.LossShape,
demo_loss.DemoLoss, mpc.MPCConfig, mpc.ExpertLanes, mpc.ExpertLabels, grad_clip.GradClip, curriculum.Curriculum,
randomize.EpisodeRandomization, task_curriculum.TaskCurriculum, success_replay.SuccessReplay) with the validators
their constructors use, the one table of "not supported with" refusals behind the check_* functions, and the options' entries of a checkpoint.

    Option                        a value named by its FIELDS: repr, ==, hash, as_tuple(), from_tuple(); a nested Option nests
    finite_number, whole_number   the constructors' tests, with their wording; refuse_value for any other bound
    refuse                        raises the first row of an option's part of the table that the context meets
    write_options, compare_options   the options' tuples in a state dict, under CHECKPOINT_KEYS"""
import math


class Option:
    FIELDS = ()          # the attributes, in the constructor's and the tuple's order
    NESTED = {}          # field -> the Option class of a nested value
    A = "a"              # the article before the class's name

    def __repr__(self):
        return f"{type(self).__name__}(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in self.FIELDS) + ")"

    def __eq__(self, other):
        return type(other) is type(self) and self.as_tuple() == other.as_tuple()

    def __hash__(self):
        return hash(self.as_tuple())

    def as_tuple(self):
        """What a checkpoint holds of the value (as lists): the fields' numbers, a nested option as a tuple of its own."""
        return tuple(v.as_tuple() if isinstance(v, Option) else v for v in (getattr(self, n) for n in self.FIELDS))

    @classmethod
    def from_tuple(cls, t):
        return cls(*[cls.NESTED[n].from_tuple(v) if n in cls.NESTED else v for n, v in zip(cls.FIELDS, t)])

    @classmethod
    def expect(cls, name, x):
        if not isinstance(x, cls):
            raise ValueError(f"{name} = {x!r} is not {cls.A} {cls.__name__}")
        return x


def is_number(x, or_bool=False):
    return isinstance(x, (int, float)) and (or_bool or not isinstance(x, bool))


def is_whole(x):
    return isinstance(x, int) and not isinstance(x, bool)


def refuse_value(what, x, wording):
    raise ValueError(f"{what} = {x!r} is not {wording}")


def finite_number(what, x, bound, or_none=False, or_bool=False):
    """x is a finite number within bound, ">= 0" or "> 0" (or_none: or None; or_bool: True and False count as numbers)."""
    if x is None and or_none:
        return
    if not (is_number(x, or_bool) and math.isfinite(x) and (x > 0 or (x == 0 and bound == ">= 0"))):
        refuse_value(what, x, ("None or " if or_none else "") + "a finite number " + bound)


def whole_number(what, x, lo, hi=None, bound=None):
    """x is a whole number in [lo, hi] (hi None: >= lo); bound: the wording of the range when it is not the plain one."""
    if not (is_whole(x) and x >= lo and (hi is None or x <= hi)):
        refuse_value(what, x, "a whole number " + (bound or (f">= {lo}" if hi is None else f"in [{lo}, {hi}]")))


# ---- the refusal table.  A row: (the context field it reads, when it refuses, the message); the context is a dict of DEFAULTS,
# what the caller knows, and "value", the option itself.  A message is a template over the option's words, or a function of the context.
# Beyond DEFAULTS an option's own rows read what its check_* passes: labels "first" (the expert lanes before the labelled ones);
# grad_clip "demo_loss", "expert" and "labels" (each None or the loop's option); population_grad_clip "device" (None: not known yet); td3 "updates_per_step" and "delay"; population_td3 those two and "n_steps", "n_step_max", "device".
UNSET = object()
DEFAULTS = dict(td3=None, population=False, data_parallel=False, force_dp=False, n_step=1, ring_mode=None, n_envs=None, pipeline=None,
                learn_log=None, demo_loss=UNSET)
_SHARED = {
    "td3": (lambda c: c["td3"] is not None, "{what} with td3 is not supported (the TD3 launches have no {form} form)"),
    "population": (lambda c: c["population"], "{what} in a population {be} not supported ({population})"),
    "data_parallel": (lambda c: c["data_parallel"], "{what} with data-parallel ranks (or the p2p exchange) {be} not supported"),
    "force_dp": (lambda c: c["force_dp"], "{what} with the data-parallel launch structure (TT_FORCE_DP) {be} not supported"),
    "ring_mode": (lambda c: c["ring_mode"] is not None and not c["ring_mode"],
                  "{what} need a stepper in ring mode (the reference-shaped actor on a GPU): the {launch} launch finds the step's "
                  "{row} row through the device cursor"),
}
def _device_type(device):
    import torch
    return torch.device(device).type


_TD3_MULTIPLE = ("updates_per_step", lambda c: int(c["updates_per_step"]) % c["delay"] != 0,
                 lambda c: f"td3: updates_per_step = {c['updates_per_step']} is not a multiple of policy_delay = {c['delay']} (the delay "
                           "is counted inside a vector step)")
_TD3_LEARN_LOG = ("learn_log", lambda c: c["learn_log"] is not None, "td3: learn_log is not supported")
_IN_POPULATION = "PopulationRollout / PopulationLearner"
TABLE = {
    "loss_shape": dict(what="loss_shape", be="is", form="shaped", population="the population's launches have no shaped form",
                       rows=("td3", "population", "data_parallel", "force_dp")),
    "demo_loss": dict(what="demo_loss", be="is", form="demonstration", population="the population's launches have no demonstration form",
                      rows=("td3", "population", "data_parallel", "force_dp",
                            ("n_step", lambda c: int(c["n_step"]) > 1,
                             lambda c: f"demo_loss with n_step = {int(c['n_step'])} is not supported: side tuples are single steps, and "
                                       "the ring refuses them in an n-step draw"))),
    "expert": dict(what="expert lanes", be="are", population=_IN_POPULATION, launch="expert's", row="ring",
                   rows=(("n_envs", lambda c: c["n_envs"] is not None and c["value"].lanes > int(c["n_envs"]),
                          lambda c: f"expert: lanes = {c['value'].lanes} is outside [1, {int(c['n_envs'])}], the env's lanes"),
                         "ring_mode", "population", "data_parallel", "force_dp")),
    "labels": dict(what="expert labels", be="are", population=_IN_POPULATION, launch="planner's", row="label",
                   rows=(("n_envs", lambda c: c["n_envs"] is not None and c["first"] + c["value"].lanes > int(c["n_envs"]),
                          lambda c: f"labels: {c['first']} expert lanes + {c['value'].lanes} labelled lanes are more than the env's "
                                    f"{int(c['n_envs'])} lanes"),
                         "ring_mode", "population", "data_parallel", "force_dp",
                         ("demo_loss", lambda c: c["demo_loss"] is None, "expert labels without demo_loss: no learner would read the "
                                                                         "labels (DDPGRollout(demo_loss=DemoLoss(...)))"))),
    "grad_clip": dict(what="grad_clip", be="is", form="clipped", population="the population's launches have no clipped optimizer step",
                      rows=("td3", "population", "data_parallel", "force_dp",
                            ("demo_loss", lambda c: c["demo_loss"] is not None,
                             "grad_clip with demo_loss is not supported (the demonstration entry points have no clipped optimizer step)"),
                            ("expert", lambda c: c["expert"] is not None,
                             "grad_clip with expert lanes is not supported (they train through the demonstration entry points)"),
                            ("labels", lambda c: c["labels"] is not None,
                             "grad_clip with expert labels is not supported (they train through the demonstration entry points)"))),
    # a population's OWN clip (PopulationLearner(grad_clips=) / PopulationRollout(grad_clip=)); "value": the list of per-agent entries
    "population_grad_clip": dict(rows=(
        ("td3", lambda c: c["td3"] is not None,
         "grad_clip in a TD3 population (PopulationTD3Learner / PopulationRollout(td3=...)) is not supported: the shared TD3 launches "
         "have no clipped optimizer step"),
        ("data_parallel", lambda c: c["data_parallel"], "grad_clip in a data-parallel population is not supported (populations run on one GPU)"),
        ("device", lambda c: c["device"] is not None and _device_type(c["device"]) != "cuda",
         lambda c: f"grad_clip in a population on device = {c['device']!r} is not supported: the per-agent clip exists only as HIP kernels"))),
    "td3": dict(rows=(_TD3_MULTIPLE, ("n_step", lambda c: int(c["n_step"]) > 1, lambda c: f"td3: n_step = {c['n_step']} > 1 is not supported"),
                      ("data_parallel", lambda c: c["data_parallel"], "td3: data_parallel ranks (and the p2p exchange) are not supported"),
                      ("pipeline", lambda c: c["pipeline"], "td3: pipeline=True is not supported (TD3 runs in the serial order)"),
                      _TD3_LEARN_LOG)),
    "population_td3": dict(rows=(
        _TD3_MULTIPLE,
        ("n_steps", lambda c: any(int(n) > 1 for n in c["n_steps"]), lambda c: f"td3: n_step = {list(c['n_steps'])} > 1 is not supported"),
        ("n_step_max", lambda c: int(c["n_step_max"]) > 1, lambda c: f"td3: n_step_max = {c['n_step_max']} > 1 is not supported"),
        _TD3_LEARN_LOG,
        ("device", lambda c: _device_type(c["device"]) != "cuda", lambda c: f"td3: device = {c['device']!r} is not supported: a population's "
                                                                             "TD3 update exists only as HIP kernels"))),
    # the env's start-pose curriculum (curriculum.check_curriculum passes expert, labels, device -- None: not known yet -- and
    # episode_log_detail)
    "curriculum": dict(what="a curriculum", be="is", population="a population's agents step envs of their own, and a curriculum per agent "
                                                                "is not built",
                       rows=("population", "data_parallel", "force_dp",
                             ("expert", lambda c: c["expert"] is not None,
                              "a curriculum with expert lanes is not supported (the expert's launch steps and resets its lanes itself)"),
                             ("labels", lambda c: c["labels"] is not None,
                              "a curriculum with expert labels is not supported (the planner's launch steps and resets its lanes itself)"),
                             ("device", lambda c: c["device"] is not None and _device_type(c["device"]) != "cuda",
                              lambda c: f"a curriculum on device = {c['device']!r} is not supported: it exists only inside the HIP env step"),
                             ("episode_log_detail", lambda c: c["episode_log_detail"],
                              "a curriculum with episode_log_detail is not supported (the curriculum's step kernels carry the plain "
                              "episode log only)"))),
    # the env's episode randomisation (randomize.check_randomization passes curriculum, expert, labels, device -- None: not known
    # yet -- and episode_log_detail)
    "randomize": dict(what="episode randomisation", be="is", population="a population's agents step envs of their own, and a "
                                                                          "randomisation per agent is not built",
                      rows=("population", "data_parallel", "force_dp",
                            ("curriculum", lambda c: c["curriculum"] is not None,
                             "episode randomisation with a curriculum is not supported (the two have step kernels of their own, and the "
                             "curriculum's cells would be counted under a moving goal)"),
                            ("expert", lambda c: c["expert"] is not None,
                             "episode randomisation with expert lanes is not supported (the expert on randomised lanes is not checked here)"),
                            ("labels", lambda c: c["labels"] is not None,
                             "episode randomisation with expert labels is not supported (the planner on randomised lanes is not checked here)"),
                            ("device", lambda c: c["device"] is not None and _device_type(c["device"]) != "cuda",
                             lambda c: f"episode randomisation on device = {c['device']!r} is not supported: it exists only inside the HIP "
                                       "env step"),
                            ("episode_log_detail", lambda c: c["episode_log_detail"],
                             "episode randomisation with episode_log_detail is not supported (the randomised step kernels carry the plain "
                             "episode log only)"))),
    # the env's task curriculum (task_curriculum.check_task_curriculum passes randomize and device -- None: not known yet; what
    # randomisation refuses is refused by its own rows first: the option is on only with it)
    "task_curriculum": dict(what="a task curriculum", be="is", population="a population's agents step envs of their own, and a task "
                                                                          "curriculum per agent is not built",
                            rows=(("randomize", lambda c: c["randomize"] is None,
                                   "a task curriculum without randomize is not supported: there is no range to put cells on"),
                                  "population", "data_parallel", "force_dp",
                                  ("device", lambda c: c["device"] is not None and _device_type(c["device"]) != "cuda",
                                   lambda c: f"a task curriculum on device = {c['device']!r} is not supported: it exists only inside the HIP "
                                             "env step"))),
    # success replay (success_replay.check_success_replay passes episode_log -- None or the log's capacity --, td3, n_step, expert,
    # labels and device -- None: not known yet)
    "success_replay": dict(what="success replay", be="is", population="a population's agents have rings of their own, and a harvest "
                                                                     "per agent is not built",
                           rows=(("episode_log", lambda c: not c["episode_log"],
                                  "success replay without episode_log is not supported: the harvest reads the episode log's records "
                                  "(DDPGRollout(episode_log=...))"),
                                 ("td3", lambda c: c["td3"] is not None,
                                  "success replay with td3 is not supported (the TD3 draw refuses side buffers)"),
                                 ("n_step", lambda c: int(c["n_step"]) > 1,
                                  lambda c: f"success replay with n_step = {int(c['n_step'])} is not supported: side tuples are single "
                                            "steps, and the ring refuses them in an n-step draw"),
                                 "population", "data_parallel", "force_dp",
                                 ("expert", lambda c: c["expert"] is not None,
                                  "success replay with expert lanes is not supported (the expert's lanes are demonstrations already, and "
                                  "their successes would be harvested as the agent's)"),
                                 ("labels", lambda c: c["labels"] is not None,
                                  "success replay with expert labels is not supported (the side region's rows carry no label)"),
                                 ("device", lambda c: c["device"] is not None and _device_type(c["device"]) != "cuda",
                                  lambda c: f"success replay on device = {c['device']!r} is not supported: the harvest exists only as HIP "
                                            "kernels"))),
}


def refuse(option, value=None, **context):
    """ValueError with the message of the first row of `option`'s part of TABLE that the context meets; else returns value."""
    words = TABLE[option]
    c = dict(DEFAULTS, value=value, **context)
    for row in words["rows"]:
        refuses, message = _SHARED[row] if isinstance(row, str) else row[1:]
        if refuses(c):
            raise ValueError(message(c) if callable(message) else message.format(**words))
    return value


# ---- the options' entries of a checkpoint: each present option's as_tuple() as a list, under its key
CHECKPOINT_KEYS = ("td3", "loss_shape", "demo_loss", "expert", "labels", "grad_clip", "curriculum", "success_replay", "task_curriculum", "randomize")


def write_options(sd, **options):
    for key in CHECKPOINT_KEYS:
        if options.get(key) is not None:
            sd[key] = list(options[key].as_tuple())
    return sd


def _tupled(x):
    return tuple(_tupled(v) for v in x) if isinstance(x, (list, tuple)) else x


def compare_options(sd, who="loop", **options):
    """ValueError when state dict `sd` was written with another value than `who` has of one of the options passed (None: without
    it), in the order of CHECKPOINT_KEYS.  Of td3 only the presence counts: its numbers are hyperparameters a file may change."""
    for key in CHECKPOINT_KEYS:
        if key not in options:
            continue
        have = _tupled(sd[key]) if sd.get(key) is not None else None
        mine = options[key].as_tuple() if options[key] is not None else None
        if key == "td3":
            if (key in sd) != (mine is not None):
                raise ValueError(f"the checkpoint was written with td3, this {who} has none" if key in sd else
                                 f"the checkpoint was written without td3, this {who} has td3 (no second critic in it)")
        elif have != mine:
            raise ValueError(f"the checkpoint was written with {key} = {have}, this {who} has {key} = {mine}")
