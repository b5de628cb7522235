"""A population of K independent DDPG agents trained in one loop on one GPU (include/ttenv.h: tt_pop_learn_*).

Agent a is a VectorStepper (stepper.py) built with agent a's arguments -- the acting half of a lone loop: its own env of n lanes,
networks, replay ring, OU noise, policy launch and env step -- stepped in the lone loop's serial order.  The learn() launches are
shared: one population update is four launches (csrc/ttpop.hip) that run every agent's workgroups.  Each agent's results are the
bits of its lone serial-order loop (rollout.py, pipeline=False) with the actor tail in one launch (TT_ACTOR_TAIL=1).  Seeds,
learning rates, tau and gamma are per agent; the network shape (23-400-300-1) and the batch size B are shared.

exploit() is population-based training's exploit/explore step (pbt.py decides it): between vector steps one launch copies an
agent's networks, Adam moments and fc2 images over another's and sets new hyperparameters in the descriptors, in place.

N-step returns are per agent too (n_steps= / n_step=): agent a draws n-step tuples with its own n and
gamma inside the shared first launch (csrc/ttpop_nstep.hip), from a table in device memory beside the descriptors; its TD
discount gamma ** n travels by value (fused_learn.nstep_discount, the lone learner's expression).  Once a population has the
table its first launch is the n-step kernel for good -- also at n = 1, the one-step draw bit for bit -- so exploit() may change
an agent's n under captured graphs.  A population built without n-step arguments launches the four one-step kernels.

Gradient-norm clipping is per agent as well (grad_clips= / grad_clip=; include/ttenv.h: tt_pop_clip): one
GradClip for all, or one GradClip or None per agent.  Any entry makes a table of the agents' max_norm values in device memory (0 =
that network is not clipped), and a population update is then eight launches for good: the weight-gradient launches leave the
gradients, and a norm launch and a clipped optimizer launch (csrc/ttclip.hip) follow each.  exploit() carries the clip with the
weights, or sets a new one ("clip_critic" / "clip_actor"), under captured graphs.  An agent's bits are those of a lone
FusedLearner(grad_clip=); an agent with no clip in such a population has the bits of the lone separate-optimizer chain.

With td3= (one td3.TD3Config, or one per agent with equal policy_delay) every agent is a TD3 agent -- six networks, its own
target_noise and noise_clip -- and a population update is the shared TD3 launches of csrc/ttpop_td3.hip (td3.PopulationTD3Learner,
DESIGN.md section 17): update u of a vector step is a full one when (u + 1) % policy_delay == 0, as in a lone TD3 loop, whose bits
agent a keeps.  exploit() then also copies the second critic and carries the two noise values.  Not with n-step returns or a learn log.

PopulationRollout.state_dict() / load_state_dict() (checkpoint.save_population_checkpoint) save and resume
the whole population bit for bit -- every agent's networks, Adam state, ring, env, OU state and the hyperparameters and n that
exploit() has moved -- and one agent of the file loads into a lone DDPGRollout.  The load makes the handle again from the restored
host state, so the device holds the file's seeds, hyperparameters, n-step table and TD3 noise values.

Out of scope: the pipelined order, data-parallel populations, expert side buffers (with any n), checkpoints without the rings'
contents, the learn log's records in a checkpoint."""
import ctypes as C

import torch

from ddpg_trucktrailer_amd import _lib as L
from ddpg_trucktrailer_amd.demo_loss import check_demo_loss
from ddpg_trucktrailer_amd.fused_learn import FusedLearner, LearnLog, check_learn_log, nstep_discount
from ddpg_trucktrailer_amd.grad_clip import check_grad_clip, check_population_grad_clip, clip_values
from ddpg_trucktrailer_amd.loss_shape import check_loss_shape
from ddpg_trucktrailer_amd.mpc import check_expert_lanes
from ddpg_trucktrailer_amd.options import write_options
from ddpg_trucktrailer_amd.replay_buffer import check_n_step, learn_start, slots_needed
from ddpg_trucktrailer_amd.rollout import _CAPTURE_MODE, _SEED_STRIDE, _gc_off
from ddpg_trucktrailer_amd.stepper import VectorStepper


def _refuse_lone_options(loss_shape, demo_loss, expert, agents=()):
    """A population has no loss shape, demonstration loss or expert lanes (the options' own checks, with population=True): neither
    as an option nor, of the first two, on an agent it is given; nor an agent that carries a gradient clip (Agent(grad_clip=))."""
    for name, check, value in (("loss_shape", check_loss_shape, loss_shape), ("demo_loss", check_demo_loss, demo_loss),
                               ("expert", check_expert_lanes, expert), ("grad_clip", check_grad_clip, None)):
        for v in [value] + [getattr(ag, name, None) for ag in agents if name != "expert"]:
            if v is not None:
                check(v, population=True)


class _PopulationLearnerBase:
    """What the population learners of DDPG (PopulationLearner) and TD3 (td3.PopulationTD3Learner) share: K agents, each with the
    state of a fused learner of its own, whose updates are launched together through one handle of the library.  The handle is made
    at the first eager learn(); every buffer and parameter storage must stay where it is from then on.  A subclass names its C
    entry points and its hyperparameters, makes the handle (_create), launches (learn(), after _ready()) and fills in exploit()'s
    three hooks."""

    HYPERS = ("alpha", "beta", "tau", "gamma")         # what a pair of exploit() may set and hyper() reads, in the C order
    _DESTROY, _HYPER = "tt_pop_learn_destroy", "tt_pop_hyper"

    def __init__(self, agents, batch_size, rings, seeds):
        self.K, self.B = len(agents), int(batch_size)
        if not 1 <= self.K <= L.POP_MAX_AGENTS:
            raise ValueError(f"a population has 1 to {L.POP_MAX_AGENTS} agents, not {self.K}")
        if rings is None or seeds is None or len(rings) != self.K or len(seeds) != self.K:
            raise ValueError("one ring and one seed per agent")
        self.agents, self.rings, self.seeds = list(agents), list(rings), [int(s) for s in seeds]
        self._h = self._key = None

    def _adopt(self, learners):
        self.lib = L.load()
        self.learners = list(learners)
        for ag, fl in zip(self.agents, self.learners):
            ag.fused_learner = fl          # (checkpoint.py exports the moments through it)

    def __del__(self):
        if getattr(self, "_h", None) is not None and L._lib is not None:
            torch.cuda.synchronize()
            getattr(L._lib, self._DESTROY)(self._h)
        self._h = None

    def _storage_key(self):
        return tuple(p.data_ptr() for fl in self.learners for n in fl._nets() for p in n.parameters())

    def _need_handle(self, what):
        if self._h is None:
            raise RuntimeError(f"{type(self).__name__}.{what}: no learn() has made the population's descriptors yet")

    def refresh_images(self):
        for fl in self.learners:
            FusedLearner.refresh_images(fl)        # (the images alone: TD3Learner's own would make a lone descriptor)

    def _ready(self):
        """What learn() does before its launches: the handle at the first eager call, and the images of fc2 tensors someone else
        wrote.  A capture holds launches only."""
        capturing, name = torch.cuda.is_current_stream_capturing(), type(self).__name__
        if self._h is None:
            if capturing:
                raise RuntimeError(f"{name}: run one eager learn() before capturing it")
            self._create()
            self._key = self._storage_key()
        elif self._key != self._storage_key():
            raise RuntimeError(f"{name}: a network's parameter storage moved since the descriptors were made")
        if not capturing:
            self.refresh_images()

    def tail_gave_up(self):
        """[agent: 0, or the step whose tail hand-over was abandoned] (host memory only)."""
        return [fl.tail_gave_up() for fl in self.learners]

    def state_dict(self, a):
        """Agent a's Adam moments and step count(s), in the format of its learner's state_dict()."""
        return self.learners[a].state_dict()

    def _hyper_of(self, a):
        """Agent a's HYPERS as the host holds them."""
        return {k: getattr(self.agents[a], k) for k in self.HYPERS}

    def exploit(self, pairs):
        """Population-based training's exploit/explore step, one launch on the current stream: pairs = [(dst, src, {HYPERS})].
        dst != src: dst's networks, Adam moments and fc2 images become src's; every dst then takes the given hyperparameters (a
        missing key: src's value).  The host mirrors -- agent.alpha / beta / tau / gamma, the torch optimizers' lr, the learner's
        hyp_actor / hyp_critic and what the subclass adds -- follow, so a checkpoint sees the new values.  Captured launches stay
        valid: the descriptors change in place."""
        self._need_handle("exploit")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{type(self).__name__}.exploit: not while capturing (it runs between vector steps)")
        pairs = list(pairs)
        if not 1 <= len(pairs) <= self.K:
            raise ValueError(f"exploit: 1 to {self.K} pairs, not {len(pairs)}")
        self.refresh_images()          # (src's images must hold its weights: they are copied with them)
        new = []
        for i, (dst, src, hyp) in enumerate(pairs):
            dst, src = int(dst), int(src)
            if not (0 <= dst < self.K and 0 <= src < self.K):
                raise ValueError(f"exploit: pair {i} ({dst} <- {src}) names an agent outside [0, {self.K})")
            n = self._pair_n_step(i, dst, src, hyp)
            of_src = self._hyper_of(src)
            new.append((dst, src, {k: float(hyp.get(k, of_src[k])) for k in self.HYPERS}, n))
        clips = self._pair_clips(pairs)
        self._launch_exploit(new)
        self._launch_clip_write(clips)
        for dst, _, h, n in new:
            self._set_mirrors(dst, h, n)

    def _pair_clips(self, pairs):
        """What exploit()'s pairs say about the clip, checked before anything is launched: [(dst, max_norm critic, max_norm
        actor)], or None for a population without a clip table, which refuses the keys."""
        for i, (_, _, hyp) in enumerate(pairs):
            if "clip_critic" in hyp or "clip_actor" in hyp:
                raise ValueError(f"exploit: pair {i} sets clip_critic / clip_actor, but this population was built without a gradient clip "
                                 "(PopulationLearner(grad_clips=...) / PopulationRollout(grad_clip=...))")
        return None

    def _launch_clip_write(self, clips):
        pass

    def _set_mirrors(self, a, h, n):
        """Agent a's host mirrors of the hyperparameters h ({HYPERS}) and of its n: what exploit() and a checkpoint's load leave
        on the host, and what _create() reads."""
        ag, fl = self.agents[a], self.learners[a]
        ag.alpha, ag.beta, ag.tau, ag.gamma = h["alpha"], h["beta"], h["tau"], h["gamma"]
        ag.actor.optimizer.param_groups[0]["lr"] = h["alpha"]
        ag.critic.optimizer.param_groups[0]["lr"] = h["beta"]
        fl.hyp_actor = (h["alpha"],) + tuple(fl.hyp_actor[1:])
        fl.hyp_critic = (h["beta"],) + tuple(fl.hyp_critic[1:])
        self._mirror(a, h, n)

    def _set_seed(self, a, seed):
        self.seeds[a] = int(seed)

    @property
    def has_handle(self):
        return self._h is not None

    def restore(self, seeds, hypers, n_steps):
        """A checkpoint's per-agent seeds, {HYPERS} and n on the host and on the device (PopulationRollout.load_state_dict, after
        the learners' own load_state_dict): the mirrors first, then the handle again from them.  _create() copies seeds,
        hyperparameters, the n-step table and TD3's noise values into the descriptors and launches no update, so destroying the
        handle and making it anew puts all of a checkpoint there at once; graphs captured over the old handle hold its address and
        must be dropped by the caller.  A learn log comes back empty, its cursors at the loaded step counts.  Without a handle
        (no learn() yet) only the host changes: the first eager learn() makes the handle from it.  A TD3 agent's smoothing-noise
        seed becomes its seed, as TD3Learner.set_seed has it: the file holds no noise seeds, so a PopulationTD3Learner built with
        noise_seeds= of its own loses them here (PopulationRollout never passes any)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{type(self).__name__}.restore: not while capturing")
        for a, (seed, h, n) in enumerate(zip(seeds, hypers, n_steps)):
            self._set_seed(a, seed)
            self._set_mirrors(a, {k: float(h[k]) for k in self.HYPERS}, int(n))
        if self._h is not None:
            torch.cuda.synchronize()
            getattr(self.lib, self._DESTROY)(self._h)
            self._h = None
            self._create()
            self._key = self._storage_key()

    def hyper(self, a):
        """Agent a's {HYPERS} as the device descriptors hold them (synchronises)."""
        self._need_handle("hyper")
        out = (C.c_float * len(self.HYPERS))()
        torch.cuda.synchronize()
        L.check(getattr(self.lib, self._HYPER)(self._h, int(a), C.byref(out)))
        return dict(zip(self.HYPERS, (float(x) for x in out)))


class PopulationLearner(_PopulationLearnerBase):
    """learn() of K agents, each with the state of a FusedLearner of its own (Adam moments, step_dev, bias corrections, tail words,
    fc2 images), launched together.  rings / seeds: agent a's TrajectoryRing and the seed of its sampling keys (update u of a vector
    step draws with seed + u * _SEED_STRIDE, the lone loop's sampling key).  The device descriptors are made at the first learn():
    every buffer and parameter storage must stay where it is from then on.
    n_steps: None = the one-step population, launch for launch; one int or one value per agent = n-step returns (include/ttenv.h:
    tt_pop_learn_set_nstep).  Any n > 1, or a list (also of ones), makes the per-agent table, and learn()'s first launch is then the
    n-step kernel for good.  Host mirrors: self.n_steps, and each agent's ring.n_step.
    learn_log: None, or the capacity per agent of the learn log (fused_learn.LearnLog; include/ttenv.h: tt_learn_log_*): learn()
    then ends with one more launch that leaves a record of every agent's update whose step count is a multiple of learn_log_every,
    and drain_learn_log() collects them.  One K-agent handle, made with the descriptors.  Not part of any checkpoint.
    exploit() (include/ttenv.h: tt_pop_exploit): a pair's dict may also hold "n_step" (missing: src's): on an n-step population dst
    then draws with that n and the pair's gamma and discounts with gamma ** n (tt_pop_exploit_nstep); a population without the
    table refuses an n other than 1.
    grad_clips: None = no clip, launch for launch; one grad_clip.GradClip or a list with one GradClip or None per agent = per-agent
    gradient-norm clipping (include/ttenv.h: tt_pop_learn_set_clip).  Any entry makes the clip table, and learn() is then eight
    launches for good.  Host mirrors: self.grad_clips[a] = [max_norm critic, max_norm actor], 0.0 = that network is not clipped.
    exploit(): a pair's dict may hold "clip_critic" / "clip_actor" (missing: src's value -- the clip travels with the weights it was
    tuned on; 0 = not clipped); tt_pop_clip_write follows the exploit launch on the same stream.  clip_stats(a), clip_of(a)."""

    def __init__(self, agents, batch_size, fc2_images=None, rings=None, seeds=None, n_steps=None, learn_log=None, learn_log_every=1,
                 loss_shape=None, demo_loss=None, expert=None, grad_clips=None):
        _refuse_lone_options(loss_shape, demo_loss, expert, agents)
        super().__init__(agents, batch_size, rings, seeds)
        clips = check_population_grad_clip(grad_clips, self.K)
        self.clip_table = clips is not None
        self.grad_clips = [list(clip_values(c)) for c in (clips or [None] * self.K)]      # host mirrors: [max_norm critic, actor], 0 = off
        if any(r._side_struct() is not None for r in rings):
            raise ValueError("expert side buffers are not supported in a population")
        self.n_steps = [check_n_step(n) for n in _per_agent(1 if n_steps is None else n_steps, self.K, "n_steps")]
        self.nstep_table = isinstance(n_steps, (list, tuple)) or any(n > 1 for n in self.n_steps)
        for a, (ring, n) in enumerate(zip(rings, self.n_steps)):
            if ring.slots < slots_needed(n):
                raise ValueError(f"agent {a}: n_step = {n} with a ring of {ring.slots} slots is not supported: the window of base "
                                 f"steps with their n steps intact needs at least {slots_needed(n)} slots")
        self._learn_log_args = check_learn_log(learn_log, learn_log_every) if learn_log is not None else None
        self.learn_log = None
        for ring, n in zip(self.rings, self.n_steps):
            ring.n_step = n                # (load_side refuses tuples an n-step draw cannot use)
        self._adopt(FusedLearner(ag, self.B, fc2_images) for ag in self.agents)

    def _create(self):
        B, keep = self.B, []
        arr = (L.TTPopAgent * self.K)()
        for a, (fl, ring, seed) in enumerate(zip(self.learners, self.rings, self.seeds)):
            sample = ring.sample_args(B, seed=seed, seed_stride=_SEED_STRIDE)
            s, act, r, s2, d = ring._batch_bufs(B)[:5]
            jobs, td = fl.fwd_jobs(s, act, s2), fl.td_input(r, d, n_step=self.n_steps[a])
            arr[a] = L.TTPopAgent(C.pointer(sample), jobs, C.pointer(td), fl.pop_net(fl.critic, fl.ws, fl.hyp_critic),
                                  fl.pop_net(fl.actor, fl.ws_actor, fl.hyp_actor), fl.q_pi.data_ptr(), fl.dq_da.data_ptr(),
                                  fl.tail_words.data_ptr(), fl.tail_gave_up_host.data_ptr())
            keep += [sample, jobs, td]
        h = C.c_void_p()
        L.check(self.lib.tt_pop_learn_create(self.K, B, arr, C.byref(h)))      # (copies everything: `keep` may go now)
        self._h = h
        if self.nstep_table:
            ns = (L.TTPopNstep * self.K)(*[self._nstep_struct(ag.gamma, n) for ag, n in zip(self.agents, self.n_steps)])
            L.check(self.lib.tt_pop_learn_set_nstep(h, ns))
        if self.clip_table:
            L.check(self.lib.tt_pop_learn_set_clip(h, (L.TTPopClip * self.K)(*[L.TTPopClip(c, a) for c, a in self.grad_clips])))
        if self._learn_log_args is not None:       # (rebuilt with the descriptors: a fresh, empty ring)
            self.learn_log = LearnLog(self.learners, *self._learn_log_args)

    @staticmethod
    def _nstep_struct(gamma, n):
        return L.TTPopNstep(int(n), float(gamma), nstep_discount(gamma, n))

    def learn(self, u=0):
        """Update u of the running vector step for every agent, enqueued on the current stream (capturable once created)."""
        self._ready()
        L.check(self.lib.tt_pop_learn(self._h, int(u), L.stream()))
        if self.learn_log is not None:
            self.learn_log.append()

    def drain_learn_log(self):
        """[agent: its learn-log records since the last drain, a dict of numpy columns and "dropped" (fused_learn.LearnLog.drain)].
        Before the first learn() there is no log yet: no records."""
        if self._learn_log_args is None:
            raise ValueError("the learn log is off (PopulationLearner(learn_log=...))")
        if self.learn_log is None:
            return [_no_records() for _ in range(self.K)]
        return [self.learn_log.drain(a) for a in range(self.K)]

    def _pair_n_step(self, i, dst, src, hyp):
        n = check_n_step(hyp.get("n_step", self.n_steps[src]))
        if not self.nstep_table and n != 1:
            raise ValueError(f"exploit: pair {i} sets n_step = {n}, but this population was built without n-step returns "
                             "(PopulationLearner(n_steps=...))")
        if self.rings[dst].slots < slots_needed(n):
            raise ValueError(f"exploit: pair {i}: n_step = {n} needs a ring of {slots_needed(n)} slots, agent {dst}'s has "
                             f"{self.rings[dst].slots}")
        return n

    def _launch_exploit(self, new):
        arr = (L.TTPopExploitPair * len(new))(*[L.TTPopExploitPair(dst, src, *[h[k] for k in self.HYPERS]) for dst, src, h, _ in new])
        if self.nstep_table:
            ns = (L.TTPopNstep * len(new))(*[self._nstep_struct(h["gamma"], n) for _, _, h, n in new])
            L.check(self.lib.tt_pop_exploit_nstep(self._h, len(new), arr, ns, L.stream()))
        else:
            L.check(self.lib.tt_pop_exploit(self._h, len(new), arr, L.stream()))

    def _mirror(self, dst, h, n):
        self.n_steps[dst] = self.rings[dst].n_step = n

    def n_step_of(self, a):
        """Agent a's (n_step, gamma, discount) as the device holds them (include/ttenv.h: tt_pop_nstep; synchronises)."""
        self._need_handle("n_step_of")
        out = L.TTPopNstep()
        torch.cuda.synchronize()
        L.check(self.lib.tt_pop_nstep(self._h, int(a), C.byref(out)))
        return int(out.n_step), float(out.gamma), float(out.discount)

    # ---- the per-agent gradient clip
    def _pair_clips(self, pairs):
        if not self.clip_table:
            return super()._pair_clips(pairs)
        from ddpg_trucktrailer_amd.options import finite_number
        out = []
        for i, (dst, src, hyp) in enumerate(pairs):
            values = []
            for j, key in enumerate(("clip_critic", "clip_actor")):
                x = hyp.get(key, self.grad_clips[int(src)][j])
                finite_number(f"exploit: pair {i}: {key}", x, ">= 0")
                values.append(float(x))
            out.append((int(dst), *values))
        return out

    def _launch_clip_write(self, clips):
        if clips is None:
            return
        agents = (C.c_int32 * len(clips))(*[d for d, _, _ in clips])
        values = (L.TTPopClip * len(clips))(*[L.TTPopClip(c, a) for _, c, a in clips])
        L.check(self.lib.tt_pop_clip_write(self._h, len(clips), agents, values, L.stream()))
        for dst, c, a in clips:
            self.grad_clips[dst] = [c, a]

    def _read_clip(self, a, what):
        if not self.clip_table:
            raise ValueError("grad_clip is off (PopulationLearner(grad_clips=...))")
        self._need_handle(what)
        value, out, counts = L.TTPopClip(), (C.c_float * 4)(), (C.c_int64 * 4)()
        torch.cuda.synchronize()
        L.check(self.lib.tt_pop_clip(self._h, int(a), C.byref(value), C.byref(out), C.byref(counts)))
        return value, out, counts

    def clip_stats(self, a):
        """Agent a's {"critic", "actor": {"norm", "coef", "updates", "clipped"}} of its last update, FusedLearner.clip_stats()'s
        entries -- here for both networks, also one that is not clipped (coef 1.0, clipped 0).  Counted from the handle's creation.
        Synchronises."""
        _, out, counts = self._read_clip(a, "clip_stats")
        return {name: {"norm": float(out[2 * j]), "coef": float(out[2 * j + 1]), "updates": int(counts[2 * j]),
                       "clipped": int(counts[2 * j + 1])} for j, name in enumerate(("critic", "actor"))}

    def clip_of(self, a):
        """Agent a's (max_norm critic, max_norm actor) as the device holds them, 0.0 = not clipped (include/ttenv.h: tt_pop_clip;
        synchronises)."""
        value = self._read_clip(a, "clip_of")[0]
        return float(value.max_norm_critic), float(value.max_norm_actor)


def _no_records():
    import numpy as np
    out = {"step": np.empty(0, np.int64), "nonfinite": np.empty(0, np.int32), "dropped": 0}
    out.update({name: np.empty(0, np.float64) for name in L.LEARN_LOG_VALUES})
    return out


def _listed(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


def _per_agent(x, K, name):
    if isinstance(x, (list, tuple)):
        if len(x) != K:
            raise ValueError(f"{name}: {len(x)} values for {K} agents")
        return list(x)
    return [x] * K


POPULATION_FORMAT = 1          # PopulationRollout.state_dict()["format"]; its agents are DDPGRollout.state_dict()s of format 2


def check_population_state(sd, K, lanes, slots, batch_size, policy_delay=None, n_step_max=1, n_step_table=False, grad_clip_table=False):
    """What PopulationRollout.load_state_dict refuses, each a ValueError that names what differs, before anything is written: sd is a
    PopulationRollout.state_dict(), the other arguments describe the population that would load it (policy_delay: None = DDPG;
    grad_clip_table: it was built with a gradient clip).  Returns the agents' n_steps.  A pure function: no GPU."""
    if sd.get("format") != POPULATION_FORMAT:
        raise ValueError(f"format: the checkpoint has format {sd.get('format')!r}, this code reads format {POPULATION_FORMAT}")
    agents = sd["agents"]
    if int(sd["K"]) != int(K) or len(agents) != int(K):
        raise ValueError(f"K: the checkpoint holds {int(sd['K'])} agents ({len(agents)} agent states), this population has {K}")
    if int(sd["n"]) != int(lanes):
        raise ValueError(f"n_envs_per_agent: the checkpoint was written with {int(sd['n'])} lanes per agent, this population has {lanes}")
    if int(sd["batch_size"]) != int(batch_size):
        raise ValueError(f"batch_size: the checkpoint was written with {int(sd['batch_size'])}, this population has {batch_size}")
    have = sd.get("policy_delay")
    if (have is None) != (policy_delay is None):
        raise ValueError("td3: the checkpoint was written with td3, this population has none" if have is not None else
                         "td3: the checkpoint was written without td3, this population has td3 (no second critics in it)")
    if have is not None and int(have) != int(policy_delay):
        raise ValueError(f"policy_delay: the checkpoint was written with {int(have)}, this population has {policy_delay}")
    if bool(sd.get("grad_clip_table", False)) != bool(grad_clip_table):
        raise ValueError("grad_clip: the checkpoint was written with a gradient clip, this population has none "
                         "(PopulationRollout(grad_clip=...))" if sd.get("grad_clip_table") else
                         "grad_clip: the checkpoint was written without a gradient clip, this population has one")
    ups = int(sd["updates_per_step"])
    if have is not None and ups % int(have) != 0:
        raise ValueError(f"updates_per_step: the checkpoint's {ups} is not a multiple of policy_delay = {int(have)} (the delay is "
                         "counted inside a vector step)")
    n_steps = []
    for a, st in enumerate(agents):
        if st.get("format") != 2:
            raise ValueError(f"format: agent {a}'s state has format {st.get('format')!r}, this code reads format 2")
        ring = st["ring"]
        if int(ring["slots"]) != int(slots):
            raise ValueError(f"replay_slots: agent {a}'s ring was written with {int(ring['slots'])} slots, this population's has {slots}")
        if int(ring["n"]) != int(lanes):
            raise ValueError(f"n_envs_per_agent: agent {a}'s ring was written with {int(ring['n'])} lanes, this population has {lanes}")
        if "obs" not in ring:
            raise ValueError(f"ring: agent {a}'s ring was written without its contents: a population cannot resume from it")
        if int(st["batch_size"]) != int(batch_size):
            raise ValueError(f"batch_size: agent {a}'s state was written with {int(st['batch_size'])}, this population has {batch_size}")
        if ("td3" in st) != (have is not None):
            raise ValueError(f"td3: agent {a}'s state was written {'with' if 'td3' in st else 'without'} td3, the checkpoint "
                             f"{'with' if have is not None else 'without'}")
        if "td3" in st and int(st["td3"][0]) != int(have):
            raise ValueError(f"policy_delay: agent {a}'s state was written with {int(st['td3'][0])}, the checkpoint with {int(have)}")
        need = ("alpha", "beta", "tau", "gamma") + (("target_noise", "noise_clip") if have is not None else ())
        if any(k not in st.get("hyper", {}) for k in need):
            raise ValueError(f"hyper: agent {a}'s state lacks one of {need} (a lone loop's state is no population agent's)")
        if grad_clip_table:
            clip = st.get("clip")
            if not (isinstance(clip, (list, tuple)) and len(clip) == 2 and all(isinstance(x, float) and x >= 0.0 and x != float("inf")
                                                                                for x in clip)):
                raise ValueError(f"grad_clip: agent {a}'s state holds clip = {clip!r}, not [max_norm critic, max_norm actor]")
        n = int(st.get("n_step", 1))
        if n > int(n_step_max):
            raise ValueError(f"n_step: agent {a} was saved with n_step = {n}, above this population's n_step_max = {n_step_max}")
        if n > 1 and not n_step_table:
            raise ValueError(f"n_step: agent {a} was saved with n_step = {n}, but this population was built without n-step returns "
                             "(PopulationRollout(n_step=...))")
        n_steps.append(check_n_step(n))
    return n_steps


class PopulationRollout:
    """K steppers of n_envs_per_agent envs each, one per seed, whose learn() launches are shared.  A vector step, in the serial
    order of a lone loop's step(): every agent's opening pack, policy launch and env step, then updates_per_step population updates.
    run(k) replays captured graphs of whole population steps (graph_steps and 1); step() launches the same step eagerly, with the
    same bits.  alphas / betas / taus / gammas: one value for all agents or one per agent.
    n_step: one value or one per agent (1: the one-step population, launch for launch).  With n_max the largest of them, every
    agent starts learning at vector step 1 + n_max -- an agent with a smaller n later than its lone loop would -- and graph
    replay starts after max(4, 1 + n_max) eager steps.  n_step_max: the largest n an exploit() may give an agent later (PBT over
    n); the ring check and the start use it.
    learn_log / learn_log_every: the learn log's capacity per agent and its stride in updates (PopulationLearner); drain_learn_log().
    grad_clip: None, one grad_clip.GradClip or a list with one GradClip or None per agent (PopulationLearner(grad_clips=)): per-agent
    gradient-norm clipping; exploit() may then set "clip_critic" / "clip_actor"; clip_stats(a), clip_of(a), grad_clips.  Not with td3."""

    def __init__(self, n_envs_per_agent, seeds, alphas=1e-4, betas=1e-3, taus=1e-3, gammas=0.99, batch_size=256, replay_slots=64,
                 updates_per_step=1, graph_steps=4, episode_log=None, fc2_images=None, device="cuda:0", data_parallel=None,
                 pipeline=None, side_buffer=None, episode_log_detail=False, n_step=1, n_step_max=None, learn_log=None,
                 learn_log_every=1, td3=None, loss_shape=None, demo_loss=None, expert=None, grad_clip=None, curriculum=None, randomize=None,
                 task_curriculum=None, success_replay=None):
        from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
        _refuse_lone_options(loss_shape, demo_loss, expert)
        if curriculum is not None:     # (a lone loop's option: curriculum.check_curriculum refuses a population)
            from ddpg_trucktrailer_amd.curriculum import check_curriculum
            check_curriculum(curriculum, population=True)
        if randomize is not None:      # (likewise: randomize.check_randomization refuses a population)
            from ddpg_trucktrailer_amd.randomize import check_randomization
            check_randomization(randomize, population=True)
        if task_curriculum is not None:    # (likewise: task_curriculum.check_task_curriculum; without `randomize` that row comes first)
            from ddpg_trucktrailer_amd.task_curriculum import check_task_curriculum
            check_task_curriculum(task_curriculum, randomize=randomize, population=True)
        if success_replay is not None:     # (likewise: success_replay.check_success_replay)
            from ddpg_trucktrailer_amd.success_replay import check_success_replay
            check_success_replay(success_replay, episode_log=episode_log, population=True)
        grad_clip = check_population_grad_clip(grad_clip, len(seeds), td3=td3, data_parallel=bool(data_parallel), device=device)
        if td3 is not None:            # (before anything else: each refusal names its option)
            from ddpg_trucktrailer_amd.td3 import check_population_td3
            td3 = check_population_td3(td3, len(seeds), updates_per_step, _listed(n_step), 1 if n_step_max is None else n_step_max,
                                       learn_log, device)
        self.td3 = td3                 # None, or the K TD3Configs
        if learn_log is not None:
            check_learn_log(learn_log, learn_log_every)
            if torch.device(device).type != "cuda":
                raise ValueError("learn_log is not supported on a CPU device: the learn log is a launch of the fused learner")
        if data_parallel or pipeline or side_buffer is not None:
            raise ValueError("populations run the serial order on one GPU without expert side buffers (data-parallel populations, "
                             "the pipelined order and side buffers are not supported)")
        self.seeds = [int(s) for s in seeds]
        K = self.K = len(self.seeds)
        if not 1 <= K <= L.POP_MAX_AGENTS:
            raise ValueError(f"a population has 1 to {L.POP_MAX_AGENTS} agents, not {K}")
        n_steps = [check_n_step(n) for n in _per_agent(n_step, K, "n_step")]
        self.n_step_max = max(n_steps) if n_step_max is None else check_n_step(n_step_max)
        if self.n_step_max < max(n_steps):
            raise ValueError(f"n_step_max = {self.n_step_max} is below the largest n_step, {max(n_steps)}")
        nstep = isinstance(n_step, (list, tuple)) or self.n_step_max > 1
        if self.n_step_max > 1 and torch.device(device).type != "cuda":
            raise ValueError(f"n_step = {n_step} is not supported on a CPU device: the population's n-step draw exists only as a HIP "
                             "kernel")
        if replay_slots < slots_needed(self.n_step_max):
            raise ValueError(f"n_step = {self.n_step_max} with replay_slots = {replay_slots} is not supported: the window of base "
                             f"steps with their n steps intact needs at least {slots_needed(self.n_step_max)} slots")
        alphas, betas, taus, gammas = (_per_agent(x, K, nm) for x, nm in ((alphas, "alphas"), (betas, "betas"), (taus, "taus"),
                                                                           (gammas, "gammas")))
        self.device = torch.device(device)
        self.n, self.batch_size, self.updates_per_step = int(n_envs_per_agent), int(batch_size), int(updates_per_step)
        self.loops = []
        for a in range(K):
            env = TruckTrailerVecEnv(self.n, device=self.device)
            env.reset(seed=self.seeds[a])
            lp = VectorStepper(env, batch_size=self.batch_size, replay_slots=replay_slots, seed=self.seeds[a], alpha=alphas[a],
                               beta=betas[a], tau=taus[a], gamma=gammas[a], episode_log=episode_log,
                               episode_log_detail=episode_log_detail, td3=None if td3 is None else td3[a])
            if not lp.ring_mode:
                raise RuntimeError("a population needs the fused policy and ring-addressed steps (reference-shaped actor on a GPU)")
            self.loops.append(lp)
        self.agents = [lp.agent for lp in self.loops]
        if td3 is not None:
            from ddpg_trucktrailer_amd.td3 import PopulationTD3Learner
            self.policy_delay = td3[0].policy_delay
            # (agent a's smoothing noise is keyed by seeds[a], what a lone loop uses)
            self.learner = PopulationTD3Learner(self.agents, self.batch_size, [lp.ring for lp in self.loops], self.seeds,
                                                fc2_images=fc2_images)
        else:
            self.learner = PopulationLearner(self.agents, self.batch_size, fc2_images, rings=[lp.ring for lp in self.loops],
                                             seeds=self.seeds, n_steps=n_steps if nstep else None, learn_log=learn_log,
                                             learn_log_every=learn_log_every, grad_clips=grad_clip)
        self._learn_from, self._warm_steps = learn_start(self.n_step_max)      # (the largest n decides for every agent)
        self.graph_steps = int(graph_steps) if graph_steps else 0
        self.graph1 = self.graphG = self._graph_key = None
        self.vector_steps = 0

    @property
    def k(self):
        return self.loops[0].ring.k

    def _body(self, learn=True):
        """One population vector step's launches (no host work): what the graphs hold."""
        for lp in self.loops:
            lp.open_step()
            lp.act_and_step()
        for u in range(self.updates_per_step if learn else 0):
            if self.td3 is not None:       # (the delay is counted inside the vector step, as in a lone TD3 loop)
                self.learner.learn(u, full=(u + 1) % self.policy_delay == 0)
            else:
                self.learner.learn(u)

    def _advance(self, steps):
        for lp in self.loops:
            lp.advance(steps)
        self.vector_steps += steps

    def _check_handover(self):
        """A launch that gave up waiting in device memory -- a tail weight workgroup for its dQ/da, or a policy launch for its image
        -- went on with stale inputs: that agent's state is garbage.  Raised, never silent."""
        for a, g in enumerate(self.learner.tail_gave_up()):
            if g:
                raise RuntimeError(f"agent {a}, learn step {g}: a weight-gradient workgroup of the population's tail launch gave up "
                                   "waiting (0.25 s) for dQ/da from its agent's row workgroups and went on: that update is garbage")
        for a, lp in enumerate(self.loops):
            mark = lp.ring.gave_up_seen() if lp.ring.gave_up_host is not None else 0
            if mark:
                raise RuntimeError(f"agent {a}: a launch of vector step {mark - 1} gave up waiting for its step's policy image")

    def step(self):
        """One population vector step, launched eagerly."""
        self._body(learn=self.k + 1 >= self._learn_from)      # (as a lone loop's learn(): no update before 1 + n steps are stored)
        self._advance(1)
        self._check_handover()

    def invalidate_graphs(self):
        self.graph1 = self.graphG = None

    def _check_epoch(self):
        key = tuple(lp.graph_key() for lp in self.loops)
        if self._graph_key != key:
            self.invalidate_graphs()
            self._graph_key = key

    def _capture(self, steps):
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with _gc_off(), torch.cuda.graph(g, stream=side, capture_error_mode=_CAPTURE_MODE):
            for _ in range(steps):
                self._body()
        torch.cuda.current_stream().wait_stream(side)
        return g

    def run(self, k):
        """k population vector steps: eager until every agent has stored max(4, 1 + n_step_max) steps, then graph replays of
        graph_steps and 1 steps.  A population that loaded warm rings before its first learn() (load_state_dict) has no handle to
        capture over yet: its first step is an eager one, the same bits, which makes it."""
        self.learner.refresh_images()
        while k > 0:
            if self.graph_steps and self.k >= self._warm_steps and self.learner.has_handle:
                self._check_epoch()
                if self.graph1 is None:
                    self.graph1 = self._capture(1)
                    self.graphG = self._capture(self.graph_steps) if self.graph_steps > 1 else None
                if self.graphG is not None and k >= self.graph_steps:
                    self.graphG.replay()
                    done = self.graph_steps
                else:
                    self.graph1.replay()
                    done = 1
                self._advance(done)
                k -= done
                self._check_handover()
            else:
                self.step()
                k -= 1

    def evaluate(self, ev):
        """A greedy evaluation of the K current actors between two population steps, on this stream: ev is an
        evaluation.Evaluator of K agents (every agent from the same start poses).  Returns its K records (what
        pbt.PBT.step(..., evaluation=) ranks on).  Nothing of the loops is touched -- envs, rings, noise, RNG."""
        return ev.run([ag.actor for ag in self.agents])

    def drain_episodes(self):
        """[agent: its env's episode log since the last drain (VectorStepper.drain_episodes)]."""
        return [lp.drain_episodes() for lp in self.loops]

    def drain_learn_log(self):
        """[agent: its learn-log records since the last drain (PopulationLearner.drain_learn_log)]."""
        if self.td3 is not None:
            raise ValueError("the learn log is off (td3: learn_log is not supported)")
        return self.learner.drain_learn_log()

    def exploit(self, pairs):
        """PBT's exploit/explore step between vector steps, eagerly (PopulationLearner.exploit): pairs = [(dst, src, {"alpha",
        "beta", "tau", "gamma"[, "n_step"][, "clip_critic", "clip_actor"]})].  The captured graphs stay as they are: the descriptors
        and the n-step and clip tables they read change in place, no storage moves, and dst's fc2 images arrive with its weights.
        With td3 a pair's dict may hold six keys -- the four above, "target_noise" and "noise_clip" (a missing key: src's value) --
        and the copy is of six networks and three moment pairs (td3.PopulationTD3Learner.exploit); an "n_step" other than 1 is a
        ValueError there: n-step returns are not supported with td3, so n_step_max has nothing to check."""
        pairs = list(pairs)
        if self.td3 is not None:       # (PopulationTD3Learner.exploit: six networks, and the noise values travel with src's)
            self.learner.exploit(pairs)
            return
        for i, (dst, src, hyp) in enumerate(pairs):
            n = int(hyp.get("n_step", self.learner.n_steps[int(src)]))
            if n > self.n_step_max:
                raise ValueError(f"exploit: pair {i} sets n_step = {n} above this loop's n_step_max = {self.n_step_max}")
        self.learner.exploit(pairs)

    def hyper(self, a):
        return self.learner.hyper(a)

    def n_step_of(self, a):
        return self.learner.n_step_of(a)

    def clip_stats(self, a):
        return self._clipped("clip_stats").clip_stats(a)

    def clip_of(self, a):
        return self._clipped("clip_of").clip_of(a)

    def _clipped(self, what):
        if not self.clip_table:
            raise ValueError(f"{what}: grad_clip is off (PopulationRollout(grad_clip=...))")
        return self.learner

    @property
    def clip_table(self):
        return bool(getattr(self.learner, "clip_table", False))

    @property
    def grad_clips(self):
        """Per agent [max_norm critic, max_norm actor] now, 0.0 = not clipped (the host mirror of the device table); None without
        the option."""
        return [list(c) for c in self.learner.grad_clips] if self.clip_table else None

    # -------------------------------------------------------------- checkpoint / resume of the whole population
    def state_dict(self):
        """Everything the next population step depends on (checkpoint.save_population_checkpoint writes
        it).  "agents"[a] is a lone loop's DDPGRollout.state_dict() of format 2, key for key -- so DDPGRollout.load_state_dict
        takes one agent out of a population -- plus "hyper": agent a's hyperparameters as exploit() left them on the host.  With
        td3 an agent's fused_adam["updates"] is the population's count of learn() calls, what a lone TD3 learner would hold.
        Synchronises; a population with a give-up raises (_check_handover) and returns nothing.  The learn log is not in it."""
        torch.cuda.synchronize(self.device)
        self._check_handover()
        lr, agents = self.learner, []
        for a, lp in enumerate(self.loops):
            st = {"format": 2, "handover_gave_up": [], "batch_size": self.batch_size, "updates_per_step": self.updates_per_step,
                  "n_step": int(self.n_steps[a]), **lp.acting_state(), "fused_adam": lr.state_dict(a), "hyper": lr._hyper_of(a)}
            if self.td3 is not None:
                write_options(st, td3=lp.agent.td3)
                st["fused_adam"]["updates"] = int(lr.updates)
            if self.clip_table:            # (only with the option: a file written without it is what it was)
                st["clip"] = [float(x) for x in lr.grad_clips[a]]
            agents.append(st)
        sd = {"format": POPULATION_FORMAT, "K": self.K, "n": self.n, "batch_size": self.batch_size,
              "updates_per_step": self.updates_per_step, "vector_steps": int(self.vector_steps), "seeds": list(self.seeds),
              "n_step_table": bool(getattr(lr, "nstep_table", False)), "n_step_max": int(self.n_step_max),
              "policy_delay": self.policy_delay if self.td3 is not None else None, "agents": agents}
        if self.clip_table:
            sd["grad_clip_table"] = True
        return sd

    def load_state_dict(self, sd):
        """Restore a state_dict() in place, in a lone loop's order per agent -- networks, learner, ring, OU state, env, counters --
        then the seeds, exploit()'s host mirrors and n, and the device descriptors from them (_PopulationLearnerBase.restore).
        check_population_state names what is refused, before anything is written; updates_per_step follows the file.  That check
        sees the shapes and options listed there, not the contents: an error raised later, inside an agent's own load (an env blob
        of another env variant, a damaged file), leaves the agents before it loaded and the population unusable until a whole
        load succeeds.  An episode log follows the file (capacity and detail mode), as in the lone loop.  Works on a population
        that has never stepped and on one with captured graphs (they are dropped); run() goes on either way."""
        n_steps = check_population_state(sd, self.K, self.n, self.loops[0].ring.slots, self.batch_size,
                                         self.policy_delay if self.td3 is not None else None, self.n_step_max,
                                         bool(getattr(self.learner, "nstep_table", False)), self.clip_table)
        torch.cuda.synchronize(self.device)
        self.invalidate_graphs()           # (they hold the handle's address, and the policy launches their agent's seed)
        lr, agents = self.learner, sd["agents"]
        for lp, fl, st in zip(self.loops, lr.learners, agents):
            lp.load_nets(st["nets"])
            fl.load_state_dict(st["fused_adam"])       # (moments, step counts; tail words reset)
            lp.load_acting_state(st)
            lp.seed, lp.vector_steps = int(st["seed"]), int(st["vector_steps"])
        self.seeds = [int(st["seed"]) for st in agents]
        hypers = [dict(st["hyper"]) for st in agents]
        if self.td3 is not None:
            lr.updates = int(agents[0]["fused_adam"].get("updates", 0))
        if self.clip_table:            # (restore() makes the handle, and with it the clip table, from the mirrors)
            lr.grad_clips = [[float(x) for x in st["clip"]] for st in agents]
        lr.restore(self.seeds, hypers, n_steps)
        self.vector_steps = int(sd["vector_steps"])
        self.updates_per_step = int(sd["updates_per_step"])

    @property
    def n_steps(self):
        """Per agent, the n of its draws now (the host mirror of the device table)."""
        return [1] * self.K if self.td3 is not None else list(self.learner.n_steps)
