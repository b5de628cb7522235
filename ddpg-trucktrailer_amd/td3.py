"""TD3 (Fujimoto, van Hoof, Meger 2018) on the fused learner: twin critics, target-policy smoothing, delayed actor and target updates
(include/ttenv.h: tt_td3_*; csrc/tttd3.hip).

    TD3Config      policy_delay, target_noise, noise_clip -- the noise in the actor's normalised action units (mu in [-1, 1])
    check_td3      every combination the loop refuses with TD3, as one pure function
    TD3Learner     FusedLearner for six networks and two critics: one update is three launches (critic-only) or four (full)
    PopulationTD3Learner   K TD3Learners whose updates share those launches (csrc/ttpop_td3.hip), with PBT's
                   exploit step for six networks

The torch form of the same update is Agent(td3=cfg).learn_batch (agent.py): the CPU path, and the twin the kernels are tested against."""
import ctypes as C

import torch

from ddpg_trucktrailer_amd import _lib as L
from ddpg_trucktrailer_amd.fused_learn import FusedLearner, _NetState
from ddpg_trucktrailer_amd.options import Option, finite_number, refuse
from ddpg_trucktrailer_amd.population import _PopulationLearnerBase


class TD3Config(Option):
    """policy_delay d >= 1: every d-th update is a full one (actor step, soft update of all three targets), the others train the two
    critics only.  target_noise sigma >= 0 and noise_clip c >= 0: a' = clip(mu'(s') + clip(sigma N(0, 1), -c, c), -1, 1).
    Kept as they were: policy_delay may be an integer-valued float, and True / False count as numbers for the two noise values."""
    FIELDS = ("policy_delay", "target_noise", "noise_clip")

    def __init__(self, policy_delay=2, target_noise=0.2, noise_clip=0.5):
        if isinstance(policy_delay, bool) or int(policy_delay) != policy_delay or int(policy_delay) < 1:
            raise ValueError(f"policy_delay = {policy_delay!r} is not an integer >= 1")
        finite_number("target_noise", target_noise, ">= 0", or_bool=True)
        finite_number("noise_clip", noise_clip, ">= 0", or_bool=True)
        self.policy_delay, self.target_noise, self.noise_clip = int(policy_delay), float(target_noise), float(noise_clip)


def check_td3(cfg, updates_per_step=1, n_step=1, data_parallel=False, pipeline=None, learn_log=None):
    """What a loop with TD3 refuses, each a ValueError that names the option.  The delay is counted inside a vector step, so that one
    captured step serves every step: updates_per_step must be a multiple of policy_delay."""
    TD3Config.expect("td3", cfg)
    return refuse("td3", cfg, updates_per_step=updates_per_step, delay=cfg.policy_delay, n_step=n_step, data_parallel=data_parallel,
                  pipeline=pipeline, learn_log=learn_log)


class TD3Learner(FusedLearner):
    """One TD3 update of Agent(td3=cfg) as launches of csrc/tttd3.hip on the draw from `ring`: update u of a vector step draws with the
    key seed + u * the loop's seed stride, as the lone fused learner does.  The descriptor is made at the first learn_batch and rewritten
    in place, at the same device address, when a parameter storage has moved or a seed changed (captured launches stay valid); the
    learner's own buffers stay where they are.  After an update: eps, y (critic 1's
    workgroups) and y2 (critic 2's: the same bits), q and q2 (Q1, Q2 on (s, a)), q1t and q2t (both target heads on a'), and on full
    updates mu, q_pi and dq_da."""

    def __init__(self, agent, batch_size, ring, seed, fc2_images=None, noise_seed=None):
        if getattr(agent, "td3", None) is None:
            raise ValueError("TD3Learner needs an Agent(td3=TD3Config(...))")
        if ring._side_struct() is not None:
            raise ValueError("td3: expert side buffers are not supported")
        super().__init__(agent, batch_size, fc2_images)
        self.cfg, self.ring, self.seed = agent.td3, ring, int(seed)
        self.noise_seed = (int(seed) if noise_seed is None else int(noise_seed)) & (2 ** 64 - 1)
        dev, B = self.dev, self.B
        f = dict(dtype=torch.float32, device=dev)
        self.critic_2 = _NetState(agent.critic_2, agent.target_critic_2, B, dev)
        self.critic_2.images = self._images_of(self.critic_2)
        self.ws_2_t = {k: torch.empty_like(v) for k, v in self.ws_t.items()}
        self.ws_2 = L.TTMlpBwdWs(**{k: v.data_ptr() for k, v in self.ws_2_t.items()})
        self.z_t2 = torch.empty((B, 300), **f)
        self.q2, self.y2, self.q2t, self.eps = (torch.empty(B, **f) for _ in range(4))
        self.q1t = self.q_t
        g2 = agent.critic_2.optimizer.param_groups[0]
        self.hyp_critic_2 = (g2["lr"], g2["betas"][0], g2["betas"][1], g2["eps"], g2["weight_decay"])
        if self.hyp_critic_2[1:3] != self.hyp_critic[1:3]:
            raise ValueError("td3: the two critics share their bias corrections, so their Adam betas must agree")
        self.step_snap = torch.zeros((), dtype=torch.int64, device=dev)         # the critics' step count as an update's first launch saw it
        self.actor_step_dev = torch.zeros((), dtype=torch.int64, device=dev)    # the actor's own Adam step count (full updates)
        self.actor_bias_corr = torch.zeros(8, **f)
        self.fuse_tail = True
        self.updates = 0               # learn_batch calls whose `full` this learner decided or was told (host)
        self._h = self._key = None

    def __del__(self):
        self._destroy()

    def _destroy(self):
        if getattr(self, "_h", None) is not None and L._lib is not None:
            torch.cuda.synchronize()
            L._lib.tt_td3_destroy(self._h)
        self._h = None

    # ---- the six networks ----------------------------------------------------------------------------------------
    def _nets(self):
        ag = self.agent
        return (ag.actor, ag.critic, ag.target_actor, ag.target_critic, ag.critic_2, ag.target_critic_2)

    def _states(self):
        return (self.actor, self.critic) + ((self.critic_2,) if hasattr(self, "critic_2") else ())

    def _images_of(self, st):
        return L.TTFc2Images(net=self._img_ptr(st.net), target=self._img_ptr(st.target)) if self.use_images else None

    def _storage_key(self):
        return tuple(p.data_ptr() for n in self._nets() for p in n.parameters())

    # ---- the descriptor ------------------------------------------------------------------------------------------
    def _describe(self):
        """(the TTTd3Agent description of this learner, the ctypes objects it points into): what tt_td3_create / tt_td3_update and
        a population's tt_pop_td3_create copy.  The second value must live until that call has returned."""
        from ddpg_trucktrailer_amd.rollout import _SEED_STRIDE
        ag, B = self.agent, self.B
        sample = self.ring.sample_args(B, seed=self.seed, seed_stride=_SEED_STRIDE)
        s, a, r, s2, d = self.ring._batch_bufs(B)[:5]
        jobs = (L.TTFwdJob * 6)()
        for j, (net, crit, obs, act, out, saved, zst) in enumerate((
                (ag.target_actor, 0, s2, None, self.mu_t, None, None),
                (ag.target_critic, 1, s2, None, None, None, self.z_t),
                (ag.target_critic_2, 1, s2, None, None, None, self.z_t2),
                (ag.critic, 1, s, a, self.q, self.critic.saved, None),
                (ag.critic_2, 1, s, a, self.q2, self.critic_2.saved, None),
                (ag.actor, 0, s, None, self.mu, self.actor.saved, None))):
            jobs[j].critic, jobs[j].obs, jobs[j].action = crit, L.ptr(obs), L.ptr(act)
            jobs[j].w, jobs[j].out = C.pointer(self.w(net)), L.ptr(out)
            jobs[j].saved = C.pointer(saved) if saved is not None else None
            jobs[j].dq_da, jobs[j].z_state = None, L.ptr(zst)
        td = self.td_input(r, d)
        nets = []
        for st, ws, hyp in ((self.critic, self.ws, self.hyp_critic), (self.critic_2, self.ws_2, self.hyp_critic_2),
                            (self.actor, self.ws_actor, self.hyp_actor)):
            arr = lambda ts: (C.c_void_p * st.count)(*[t.data_ptr() for t in ts])
            st.a_p, st.a_t = arr(st.params), arr(st.targets)          # (a parameter storage may have moved)
            st.images = self._images_of(st)
            nets.append(self.pop_net(st, ws, hyp))
        desc = L.TTTd3Agent(C.pointer(sample), jobs, C.pointer(td), nets[0], nets[1], nets[2], self.z_t2.data_ptr(),
                            C.pointer(self.w(ag.target_critic_2)), self.cfg.target_noise, self.cfg.noise_clip, self.noise_seed,
                            self.eps.data_ptr(), self.y2.data_ptr(), self.q2t.data_ptr(), self.step_snap.data_ptr(),
                            self.actor_step_dev.data_ptr(), self.actor_bias_corr.data_ptr(), self.q_pi.data_ptr(),
                            self.dq_da.data_ptr(), self.tail_words.data_ptr(), self.tail_gave_up_host.data_ptr())
        return desc, (sample, jobs, td, nets)

    def _create(self):
        """Make the descriptor, or -- when there is one -- write the new description over it IN PLACE (tt_td3_update): captured
        launches hold the descriptor's device address by value, so it is never freed while the learner lives."""
        desc, keep = self._describe()
        if self._h is None:
            h = C.c_void_p()
            L.check(self.lib.tt_td3_create(self.B, C.byref(desc), C.byref(h)))      # (copies everything)
            self._h = h
        else:
            L.check(self.lib.tt_td3_update(self._h, C.byref(desc)))            # (waits for the device, then copies)
        del keep
        self._key = self._storage_key()

    def set_noise_seed(self, noise_seed):
        """Another seed of the smoothing noise: the descriptor is rewritten (in place) at the next update."""
        self.noise_seed = int(noise_seed) & (2 ** 64 - 1)
        self._key = None

    def set_seed(self, seed):
        """Another seed of the sampling keys and of the noise (a loop restored from a checkpoint): the descriptor is rewritten in place."""
        if int(seed) != self.seed:
            self.seed = int(seed)
            self.noise_seed = int(seed) & (2 ** 64 - 1)
            self._key = None

    def ensure_descriptor(self):
        """Make the descriptor if there is none, or if a parameter storage moved or a seed changed since it was made.  Not while
        capturing: a loop calls this (through refresh_images) before it captures or replays."""
        if self._h is not None and self._key == self._storage_key():
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("TD3Learner: the descriptor must be made before a capture (refresh_images() or one eager learn_batch)")
        for n in self._nets():
            self.w(n)                      # (a moved storage gets its weight struct and a fresh image first)
        FusedLearner.refresh_images(self)
        self._create()

    def refresh_images(self, force=False):
        super().refresh_images(force)
        if getattr(self, "_key", False) is not False and self.dev.type == "cuda" and not torch.cuda.is_current_stream_capturing():
            self.ensure_descriptor()

    def learn_batch(self, states=None, actions=None, rewards=None, states_=None, done_u8=None, u=0, full=None):
        """Update u of the running vector step on the current stream (capturable once the descriptor exists).  The five tensors, when
        given, must be the ring's batch buffers: the first launch fills them with the draw.  full: None = every policy_delay-th
        update by this learner's own count; else this update is full (True) or critic-only (False)."""
        bufs = self.ring._batch_bufs(self.B)[:5]
        for given, own in zip((states, actions, rewards, states_, done_u8), bufs):
            assert given is None or given.data_ptr() == own.data_ptr(), "TD3Learner draws its batch itself, into the ring's buffers"
        if not torch.cuda.is_current_stream_capturing():
            self.refresh_images()          # (also makes the descriptor when there is none or a storage moved)
        elif self._h is None or self._key != self._storage_key():
            raise RuntimeError("TD3Learner: run one eager learn_batch before capturing it (and after a parameter storage moved)")
        self.updates += 1
        if full is None:
            full = self.updates % self.cfg.policy_delay == 0
        L.check(self.lib.tt_td3_learn(self._h, int(u), 1 if full else 0, self._stream()))

    # ---- checkpoint ----------------------------------------------------------------------------------------------
    def state_dict(self):
        sd = super().state_dict()
        sd["critic_2"] = {"m": self.critic_2.m.cpu(), "v": self.critic_2.v.cpu()}
        sd["actor_step"] = int(self.actor_step_dev.item())
        sd["updates"] = self.updates
        return sd

    def load_state_dict(self, sd):
        if "critic_2" not in sd:
            raise ValueError("this learner state was written without td3 (no critic_2 moments): a TD3 learner cannot load it")
        super().load_state_dict(sd)
        self.critic_2.m.copy_(sd["critic_2"]["m"]); self.critic_2.v.copy_(sd["critic_2"]["v"])
        self.actor_step_dev.fill_(int(sd["actor_step"]))
        self.reset_tail_words(int(sd["actor_step"]))      # (the TD3 tail's epoch is the ACTOR step: FusedLearner.reset_tail_words)
        self.updates = int(sd.get("updates", 0))

    def step_counts(self):
        return {"step": int(self.step_dev.item()), "actor_step": int(self.actor_step_dev.item())}

    def set_step_counts(self, counts):
        super().set_step_counts(counts)
        self.actor_step_dev.fill_(int(counts["actor_step"]))
        self.reset_tail_words(int(counts["actor_step"]))

    def export_to_optimizers(self):
        ag = self.agent
        for st, opt, step_dev in ((self.actor, ag.actor.optimizer, self.actor_step_dev), (self.critic, ag.critic.optimizer, self.step_dev),
                                  (self.critic_2, ag.critic_2.optimizer, self.step_dev)):
            step = step_dev.to(torch.float32)
            for p, m, v in zip(st.params, st.ms, st.vs):
                opt.state[p] = {"step": step.clone(), "exp_avg": m.view_as(p).clone(), "exp_avg_sq": v.view_as(p).clone()}

    def import_from_optimizers(self):
        ag = self.agent
        for st, opt, step_dev in ((self.actor, ag.actor.optimizer, self.actor_step_dev), (self.critic_2, ag.critic_2.optimizer, self.step_dev),
                                  (self.critic, ag.critic.optimizer, self.step_dev)):
            for p, m, v in zip(st.params, st.ms, st.vs):
                s = opt.state.get(p)
                if s:
                    m.copy_(s["exp_avg"].reshape(-1)); v.copy_(s["exp_avg_sq"].reshape(-1))
                    step_dev.fill_(int(float(s["step"])))
        self.reset_tail_words(int(self.actor_step_dev.item()))


HYPERS6 = ("alpha", "beta", "tau", "gamma", "target_noise", "noise_clip")


class PopulationTD3Learner(_PopulationLearnerBase):
    """The TD3 updates of K agents launched together (include/ttenv.h: tt_pop_td3_*): each agent has the state of a TD3Learner of
    its own -- buffers, Adam moments, both step counts, tail words, fc2 images, checkpoint format -- and those learners never make
    lone descriptors; the population's one handle is made at the first eager learn(), from then on every buffer and parameter
    storage must stay where it is.  rings / seeds: agent a's TrajectoryRing and the seed of its sampling keys; noise_seeds: the
    seeds of the smoothing noise (None: the sampling seeds, as in a lone loop).  agents[a].td3 holds agent a's target_noise and
    noise_clip; policy_delay is one value for all, since `full` is an argument of the shared launches.
    exploit() (include/ttenv.h: tt_pop_td3_exploit) copies six networks, three Adam moment pairs and six fc2 images; a pair's dict
    may hold the six HYPERS6, and the mirrors include the second critic's optimizer lr, hyp_critic_2 and the learner's TD3Config."""

    HYPERS = HYPERS6
    _DESTROY, _HYPER = "tt_pop_td3_destroy", "tt_pop_td3_hyper"

    def __init__(self, agents, batch_size, rings, seeds, noise_seeds=None, fc2_images=None, grad_clips=None):
        super().__init__(agents, batch_size, rings, seeds)
        if grad_clips is not None:         # (refused by name: the per-agent clip is the DDPG population's)
            from ddpg_trucktrailer_amd.grad_clip import check_population_grad_clip
            check_population_grad_clip(grad_clips, self.K, td3=[getattr(ag, "td3", True) for ag in agents])
        if noise_seeds is not None and len(noise_seeds) != self.K:
            raise ValueError("one noise seed per agent")
        if any(getattr(ag, "td3", None) is None for ag in agents):
            raise ValueError("PopulationTD3Learner needs agents built with Agent(td3=TD3Config(...))")
        self.policy_delay = same_policy_delay([ag.td3 for ag in agents])
        self._adopt(TD3Learner(ag, self.B, ring, seed, fc2_images, None if noise_seeds is None else noise_seeds[a])
                    for a, (ag, ring, seed) in enumerate(zip(self.agents, self.rings, self.seeds)))
        self.updates = 0                   # learn() calls, for the delay when `full` is left to this learner

    def _create(self):
        arr, keep = (L.TTTd3Agent * self.K)(), []
        for a, fl in enumerate(self.learners):
            desc, objs = fl._describe()
            arr[a] = desc
            keep += [desc, objs]
        h = C.c_void_p()
        L.check(self.lib.tt_pop_td3_create(self.K, self.B, arr, C.byref(h)))      # (copies everything: `keep` may go now)
        self._h = h

    def learn(self, u=0, full=None):
        """Update u of the running vector step for every agent, enqueued on the current stream (capturable once created).  full:
        None = every policy_delay-th learn() by this learner's own count, as TD3Learner counts; else this update is full (True) or
        critic-only (False) for the whole population."""
        self._ready()
        self.updates += 1
        if full is None:
            full = self.updates % self.policy_delay == 0
        L.check(self.lib.tt_pop_td3_learn(self._h, int(u), 1 if full else 0, L.stream()))

    def _hyper_of(self, a):
        cfg = self.learners[a].cfg
        return dict({k: getattr(self.agents[a], k) for k in HYPERS6[:4]}, target_noise=cfg.target_noise, noise_clip=cfg.noise_clip)

    def _pair_n_step(self, i, dst, src, hyp):
        if int(hyp.get("n_step", 1)) != 1:
            raise ValueError(f"exploit: pair {i} sets n_step = {hyp['n_step']}: n-step returns are not supported with td3")
        return 1

    def _launch_exploit(self, new):
        arr = (L.TTPopTd3Pair * len(new))(*[L.TTPopTd3Pair(dst, src, *[h[k] for k in HYPERS6]) for dst, src, h, _ in new])
        L.check(self.lib.tt_pop_td3_exploit(self._h, len(new), arr, L.stream()))

    def _set_seed(self, a, seed):
        """A checkpoint's seed: the sampling keys' and, as TD3Learner.set_seed has it, the smoothing noise's."""
        super()._set_seed(a, seed)
        self.learners[a].seed, self.learners[a].noise_seed = int(seed), int(seed) & (2 ** 64 - 1)

    def _mirror(self, dst, h, n):
        ag, fl = self.agents[dst], self.learners[dst]
        ag.critic_2.optimizer.param_groups[0]["lr"] = h["beta"]
        fl.hyp_critic_2 = (h["beta"],) + tuple(fl.hyp_critic_2[1:])
        fl.cfg = ag.td3 = TD3Config(self.policy_delay, h["target_noise"], h["noise_clip"])


def same_policy_delay(cfgs):
    """The one policy_delay of a population's TD3Configs, or ValueError: `full` is an argument of the shared launches."""
    delays = sorted({c.policy_delay for c in cfgs})
    if len(delays) != 1:
        raise ValueError(f"td3: a population has one policy_delay, not {delays} (target_noise and noise_clip may differ per agent)")
    return delays[0]


def check_population_td3(td3, K, updates_per_step=1, n_steps=(1,), n_step_max=1, learn_log=None, device="cuda:0"):
    """What PopulationRollout(td3=...) refuses, each a ValueError that names the option; returns the K TD3Configs.  td3: one
    TD3Config for every agent, or a list of K with equal policy_delay."""
    if isinstance(td3, (list, tuple)):
        if len(td3) != K:
            raise ValueError(f"td3: {len(td3)} configurations for {K} agents")
        cfgs = list(td3)
    else:
        cfgs = [td3] * K
    for c in cfgs:
        TD3Config.expect("td3", c)
    return refuse("population_td3", cfgs, updates_per_step=updates_per_step, delay=same_policy_delay(cfgs), n_steps=n_steps,
                  n_step_max=n_step_max, learn_log=learn_log, device=device)
