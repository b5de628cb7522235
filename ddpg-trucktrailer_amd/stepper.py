"""The acting half of a vector DDPG loop (rollout.py's docstring has the step): one agent's env of N lanes, four networks, replay
ring and OU noise, and the launches that fill the ring -- the opening pack, the policy launch, the env step.  Nothing here learns or
schedules: DDPGRollout (rollout.py) is a stepper with a learner and a lone loop's orders, PopulationRollout holds K steppers."""
import math
import os

import numpy as np
import torch

from ddpg_trucktrailer_amd import fused
from ddpg_trucktrailer_amd.agent import Agent
from ddpg_trucktrailer_amd.noise import VecOUNoise
from ddpg_trucktrailer_amd.options import compare_options, write_options
from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing


class VectorStepper:
    expert = labels = curriculum = randomize = task_curriculum = success_replay = None         # (what __init__ sets; on the class so that a stepper made without it, as tests make them, has both)

    def __init__(self, env, batch_size=256, replay_slots=64, seed=27, alpha=1e-4, beta=1e-3, tau=1e-3, gamma=0.99, fc1_dims=400,
                 fc2_dims=300, agent=None, capturable=True, policy_workgroups=192, policy_capped_grids=4, episode_log=None,
                 episode_log_detail=False, td3=None, expert=None, labels=None, curriculum=None, randomize=None,
                 task_curriculum=None, success_replay=None):
        """agent: made here from alpha .. batch_size when none is passed (capturable: torch optimizers that a graph may hold);
        td3: its TD3Config (Agent(td3=)), whose torch path draws its smoothing noise from a generator seeded with `seed`.
        episode_log: None, or the capacity of the env's episode log (TruckTrailerVecEnv.enable_episode_log), turned on here,
        before any step or capture: the env step kernel logs every episode that ends in the loop, end_step = the loop's vector
        step, and drain_episodes() collects the records.  episode_log_detail: the detailed log (episode_metrics.py).
        expert: None, or an mpc.ExpertLanes: lanes [0, expert.lanes) are driven by the MPC expert -- one launch
        between the policy launch and the env step writes their decisions over the policy's (ring mode only); the stepper owns
        their plan [lanes, H].
        labels: None, or an mpc.ExpertLabels: the lanes behind the expert's, [M, M + labels.lanes), act on the
        policy's values as every lane does, and the expert's decision on each of them goes to the ring's label array (enabled
        here) -- ONE launch, in the expert lanes' place, plans for both kinds of lane, and the stepper owns the plan [M + L, H].
        curriculum: None, or a curriculum.Curriculum, turned on in the env here, before any step or capture: the
        env step counts every finished episode in the cell it started in and draws the next start pose by the cells' weights; the
        owner of the stepper calls curriculum_tick() after every vector step it has advanced.
        randomize: None, or a randomize.EpisodeRandomization, turned on in the env here, before the first
        observation is taken, and followed by env.reset(seed) with this stepper's seed: every lane then runs a randomised episode 0,
        and slot 0 of the ring holds its observation (columns 12-15: the drawn goal).  A reset the caller made before is replaced.
        task_curriculum: None, or a task_curriculum.TaskCurriculum, which needs `randomize`: turned on in the
        env after randomisation and before that reset, so episode 0's tasks are its draws (uniform over the cells: nothing is counted
        yet); the owner of the stepper calls task_curriculum_tick() after every vector step it has advanced.
        success_replay: None, or a success_replay.SuccessReplay, which needs `episode_log`: the ring's side buffer
        gets a region of its own (TrajectoryRing.enable_success_replay, before anything is captured), and the owner of the stepper
        calls success_replay_tick() after every vector step it has advanced -- the harvest of the successful episodes the log names."""
        self.env, self.n, self.device, self.seed = env, env.n_envs, env.device, seed
        if episode_log:
            env.enable_episode_log(int(episode_log), detail=episode_log_detail)
        self.curriculum = None
        if curriculum is not None:
            from ddpg_trucktrailer_amd.curriculum import check_curriculum
            self.curriculum = check_curriculum(curriculum, expert=expert, labels=labels, device=env.device,
                                               episode_log_detail=bool(episode_log) and episode_log_detail)
            env.enable_curriculum(self.curriculum)
        self.randomize = None
        if randomize is not None:
            from ddpg_trucktrailer_amd.randomize import check_randomization
            self.randomize = check_randomization(randomize, curriculum=self.curriculum, expert=expert, labels=labels, device=env.device,
                                                 episode_log_detail=bool(episode_log) and episode_log_detail)
            env.enable_randomization(self.randomize)
        self.task_curriculum = None
        if task_curriculum is not None:
            from ddpg_trucktrailer_amd.task_curriculum import check_task_curriculum
            self.task_curriculum = check_task_curriculum(task_curriculum, randomize=self.randomize, device=env.device)
            env.enable_task_curriculum(self.task_curriculum)
        if self.randomize is not None:
            env.reset(seed=seed)
        # the order that decides the bits: the seed, the networks, the ring, the noise, the first observation (with randomize: of the
        # reset above -- enable, then reset(seed), then everything else, so that the ring starts on a randomised episode 0)
        torch.manual_seed(seed)
        self.agent = agent if agent is not None else Agent(
            alpha=alpha, beta=beta, input_dims=(env.observation_dim,), tau=tau, n_actions=1, gamma=gamma,
            fc1_dims=fc1_dims, fc2_dims=fc2_dims, batch_size=batch_size, device=self.device,
            capturable=capturable, replay=False, td3=td3)
        if getattr(self.agent, "td3", None) is not None:
            self.agent.seed_td3_noise(seed)
        self.ring = TrajectoryRing(self.n, replay_slots, env.observation_dim, self.device)
        if self.device.type == "cuda":
            self.ring.attach(env)                          # the step kernel advances the ring's device counter
        self.success_replay = None
        if success_replay is not None:
            from ddpg_trucktrailer_amd.success_replay import check_success_replay
            self.success_replay = check_success_replay(success_replay, episode_log=episode_log, td3=td3, expert=expert, labels=labels,
                                                       device=env.device)
            self.ring.enable_success_replay(self.success_replay.capacity)
        self.noise = VecOUNoise(self.n, self.device)
        self.high = float(np.float32(math.pi / 4))       # env.action_space.high (f32 pi/4, simv2.py:86-91)
        self.scaled = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        # the first observation of every env goes into slot 0
        env.observe(out=self.ring.obs[0])
        self.fused_act = fused.supported(self.agent.actor)      # csrc/ttnet.hip: reference-shaped 23-400-300-1 actor
        self.agent.fused_targets = self.fused_act and fused.supported(self.agent.target_critic)
        self.policy_workgroups = int(os.environ.get("TT_POLICY_WG", policy_workgroups))     # (env: A/B measurements)
        # learn() is over after about four of the policy's capped grids (~100 us): the tiles left then (N > 98304 envs) go out
        # in one grid over all CUs
        self.policy_capped_grids = int(os.environ.get("TT_POLICY_CAPPED_GRIDS", policy_capped_grids))
        # the policy reads one of two packed images of the actor, by the step's parity, under a capped grid: set by an owner
        # that runs the pipelined order (rollout.py), where a step's opening launch may run beside the previous step's policy
        self.two_images = False
        self.vector_steps = 0
        # ring addressing: the policy and env launches find the step's ring slots through a device cursor that the step's
        # opening pack launch writes (include/ttenv.h: tt_ring_view), not through per-slot pointers -- so ONE captured
        # graph serves every ring position: a single-step graph and a graph of `graph_steps` steps are all there is
        self.ring_mode = self.fused_act and self.device.type == "cuda" and self.ring._env_counts
        self._view = self.ring.view() if self.ring_mode else None
        self.expert, self.expert_plan = None, None
        if expert is not None:
            from ddpg_trucktrailer_amd.mpc import check_expert_lanes, check_mpc
            self.expert = check_expert_lanes(expert, n_envs=self.n, ring_mode=self.ring_mode)
            check_mpc(expert.mpc, action_scale=env.max_steer)
            with torch.cuda.device(self.device):
                self.expert_plan = torch.zeros((expert.lanes, expert.mpc.horizon), dtype=torch.float32, device=self.device)
        self.labels = None
        if labels is not None:
            from ddpg_trucktrailer_amd.mpc import check_expert_labels, check_mpc
            self.labels = check_expert_labels(labels, expert=self.expert, n_envs=self.n, ring_mode=self.ring_mode)
            check_mpc(labels.mpc, action_scale=env.max_steer)
            self.label_first = self.expert.lanes if self.expert is not None else 0
            self.ring.enable_labels()
            with torch.cuda.device(self.device):       # one plan for the launch's lanes: rows [0, M) the expert lanes'
                self.expert_plan = torch.zeros((self.label_first + labels.lanes, labels.mpc.horizon), dtype=torch.float32,
                                               device=self.device)

    def _image(self):
        """The packed actor under two_images: the image packed at the start of the step, never the live weights learn() updates."""
        return fused.packed_weights_of(self.agent.actor, 0, self.policy_workgroups, self.policy_capped_grids, two_images=True)

    @torch.no_grad()
    def act(self, obs, act_out, done_prev=None):
        if self.fused_act:     # actor forward + OU noise + clip*high in ONE launch (tt_actor_act)
            w = self._image() if self.two_images else None
            dev = self.ring._env_counts    # noise keyed by the DEVICE step counter: the launch is graph-replayable
            return fused.actor_act(self.agent.actor, obs, self.noise.x, act_out, self.scaled, seed=self.seed,
                                   step=0 if dev else self.vector_steps, step_dev=self.ring.k_dev if dev else None,
                                   done_prev=done_prev, high=self.high, weights=w)
        if done_prev is not None:
            self.noise.reset(done_prev)
        mu = self.agent.actor(obs).view(-1)
        torch.add(mu, self.noise.sample(), out=act_out)                   # stored action: unclipped mu + noise
        torch.clamp(act_out, -1.0, 1.0, out=self.scaled).mul_(self.high)  # what the env is driven with
        return self.scaled

    def open_step(self, sample=None, counter=None):
        """The launch that opens a vector step (ring mode): the policy's image from the actor's current weights and the step's ring
        cursor, taken from the device step count `counter` (default: the ring's own); with a tt_sample_args also that draw."""
        cursor = self.ring.cursor(counter)
        if sample is not None:
            fused.pack_and_sample(self.agent.actor, 0, sample, cursor=cursor)
        else:
            fused.pack(self.agent.actor, 0, cursor=cursor)

    def policy_launch(self):
        """The policy launch of the running step alone (ring mode; after open_step): bench.py times it."""
        w = fused.packed_weights_of(self.agent.actor, 0, self.policy_workgroups if self.two_images else 0,
                                    self.policy_capped_grids, two_images=self.two_images)
        return fused.actor_act_ring(self.agent.actor, self._view, w, self.noise.x, self.scaled, seed=self.seed, step=0,
                                    step_dev=self.ring.k_dev, high=self.high)

    def act_and_step(self, k=None):
        """The policy + env launches of the running vector step.  Ring mode: everything that selects the slots is on the
        device (after open_step).  Otherwise (CPU, torch actor) k selects them."""
        if self.ring_mode:
            self.policy_launch()
            if self.labels is not None:       # the labelled lanes' decisions into ring.label[t]; the expert lanes' as below
                self.env.mpc_label_ring(self.labels.mpc, self.expert_plan, self.label_first, self.labels.lanes, self._view,
                                        self.ring.label, self.high, self.scaled, seed=self.labels.seed)
            elif self.expert is not None:     # the expert lanes' decisions over the policy's, in ring.act[t] and self.scaled
                self.env.mpc_act_ring(self.expert.mpc, self.expert_plan, self.expert.lanes, self._view, self.high, self.scaled,
                                      seed=self.expert.seed)
            self.env.step_ring(self.scaled, self._view, auto_reset=True)
            return
        ring = self.ring
        t, t1 = ring.slot(k), ring.slot(k + 1)
        # the noise of an env whose episode ended at the previous step restarts at 0 (trainv2.py:492)
        done_prev = ring.done[ring.slot(k - 1)] if k > 0 else None
        scaled = self.act(ring.obs[t], ring.act[t], done_prev)
        self.env.step(scaled, auto_reset=True, obs_out=ring.obs[t1], reward_out=ring.rew[t], done_out=ring.done[t])

    def advance(self, steps=1):
        """The host mirrors of `steps` launched vector steps."""
        self.ring.advance(steps)
        self.vector_steps += steps

    def curriculum_room(self, k):
        """How many of k further vector steps may run before the curriculum's next update is due (k without a curriculum): graph
        replays are cut there, so that the update sits between replays."""
        for cur in (self.curriculum, self.task_curriculum, self.success_replay):       # (the task curriculum's update likewise, and success replay's harvest)
            if cur is not None:
                k = min(k, cur.every - self.vector_steps % cur.every)
        return k

    def curriculum_tick(self):
        """After advance(): the curriculum's update, on the env's stream, when the vector steps have reached a multiple of `every`."""
        if self.curriculum is not None and self.vector_steps % self.curriculum.every == 0:
            self.env.curriculum_update()

    def task_curriculum_tick(self):
        """After advance(): the task curriculum's update, likewise."""
        if self.task_curriculum is not None and self.vector_steps % self.task_curriculum.every == 0:
            self.env.task_curriculum_update()

    def harvest(self):
        """One harvest (success_replay), on the current stream: the log's records since the harvest's mark, the ring as it stands.
        The log's launch 0 is ring step 0: the stepper enables the log before its first step, and a checkpoint carries both counts."""
        sr = self.success_replay
        self.env.harvest(self.ring.harvest_struct(self.env.episode_log_capacity, tail=sr.tail), self.ring.view(), self.ring.k_dev)

    def success_replay_tick(self):
        """After advance(), between graph replays: the harvest, when the vector steps have reached a multiple of `every`.  No launch
        of the step or the learn chain is in flight there (rollout.py: run)."""
        if self.success_replay is not None and self.vector_steps % self.success_replay.every == 0:
            self.harvest()

    def success_replay_stats(self):
        """{"episodes", "rows", "rows_cut", "expired", "exposed"} of the harvests so far; also moves the side buffer's count up to the
        region's filled rows ("exposed"; captured graphs are captured again while it moves).  Synchronises."""
        if self.success_replay is None:
            raise ValueError("success replay is off (DDPGRollout(success_replay=...))")
        self.ring.harvest_state_async()
        torch.cuda.current_stream(self.device).synchronize()
        return self._exposed()

    def _exposed(self):
        st = self.ring.read_harvest_state()
        return {"episodes": st["episodes"], "rows": st["written_rows"], "rows_cut": st["rows_cut"], "expired": st["expired"],
                "exposed": self.ring.expose_successes(st["written_rows"])}

    def export_successes(self, path):
        """The region's exposed rows as a demonstration file for another run (expert.save_transitions_npz).  Synchronises."""
        from ddpg_trucktrailer_amd.expert import save_transitions_npz
        n, a = self.success_replay_stats()["exposed"], self.ring.harvest["base"]
        sd = self.ring.side
        return save_transitions_npz(path, *(sd[k][a:a + n].cpu().numpy() for k in ("obs", "act", "rew", "obs2", "done")))

    def graph_key(self):
        """What captured launches of this stepper bake in: env.graph_epoch (reset seed, per-env-goal mode, pose pool), the ring's
        side-buffer count, the actor's parameter storages (the policy's packed-image struct is keyed on them, fused.py), the
        expert lanes' and the expert labels' configurations (their numbers are kernel arguments), the episode randomisation
        and the task curriculum (their step kernels are others)."""
        return (getattr(self.env, "graph_epoch", 0), self.ring.side_epoch,
                fused.packed_key_of(self.agent.actor) if self.fused_act else None,
                self.expert.as_tuple() if self.expert is not None else None) + \
               ((self.labels.as_tuple(),) if self.labels is not None else ()) + \
               ((self.randomize.as_tuple(),) if self.randomize is not None else ()) + \
               ((self.task_curriculum.as_tuple(),) if self.task_curriculum is not None else ())

    def drain_episodes(self):
        """The env's episode log since the last drain: records sorted by (end_step, lane), end_step = the vector step it ended in."""
        if self.success_replay is None:
            return self.env.drain_episodes()
        # harvest what the log still holds, drain (which empties the log: the mark goes back to 0), and expose the region's rows --
        # the harvest's words travel to the host behind the harvest and are read after the drain's own synchronize
        self.harvest()
        self.ring.harvest_state_async()
        out = self.env.drain_episodes()
        self.ring.harvest["state"][0] = 0
        self._exposed()
        return out

    # -------------------------------------------------------------- the stepper's part of a checkpoint
    def net_names(self):
        td3 = getattr(self.agent, "td3", None) is not None
        return ("actor", "critic", "target_actor", "target_critic") + (("critic_2", "target_critic_2") if td3 else ())

    def acting_state(self):
        """What DDPGRollout.state_dict and PopulationRollout.state_dict hold of a stepper, under the lone loop's keys: seed,
        vector_steps, nets (four networks, six with TD3), ring, ou and env (with the episode log's state when it is on).  The
        caller has synchronised."""
        ag = self.agent
        ex = write_options({}, expert=self.expert, labels=self.labels, curriculum=self.curriculum, randomize=self.randomize,
                           task_curriculum=self.task_curriculum, success_replay=self.success_replay)
        if self.expert is not None or self.labels is not None:      # (with labels expert_plan is the launch's whole plan [M + L, H])
            ex["expert_plan"] = self.expert_plan.detach().cpu().clone()
        return {**ex, "seed": int(self.seed), "vector_steps": int(self.vector_steps),
                "nets": {n: {k: v.detach().cpu().clone() for k, v in getattr(ag, n).state_dict().items()} for n in self.net_names()},
                "ring": self.ring.state_dict(), "ou": self.noise.x.detach().cpu().clone(),
                "env": self.env.state_dict() if hasattr(self.env, "state_dict") else None}

    def load_nets(self, nets):
        """The networks of a checkpoint, in place: captured graphs and descriptors keep the addresses."""
        with torch.no_grad():
            for n, net_sd in nets.items():
                for k, v in getattr(self.agent, n).state_dict().items():
                    v.copy_(net_sd[k].to(v.device))

    def check_expert_state(self, sd):
        """ValueError when acting_state() `sd` was written with other expert lanes or labels than this stepper's (or with none)."""
        compare_options(sd, expert=self.expert, labels=self.labels, curriculum=self.curriculum, randomize=self.randomize,
                        task_curriculum=self.task_curriculum, success_replay=self.success_replay)

    def load_acting_state(self, sd):
        """Ring, OU state and env of acting_state(), in the lone loop's order (the env's load bumps env.graph_epoch: graphs are
        captured again).  Seed and counters stay with the caller, which knows what bakes the seed in.  A checkpoint written with
        other expert lanes or expert labels (or none) is refused before anything is written: the plan, the lanes' ring rows and the
        label array would not be this loop's."""
        self.check_expert_state(sd)
        if self.expert_plan is not None:
            self.expert_plan.copy_(sd["expert_plan"].to(self.expert_plan.device))
        self.ring.load_state_dict(sd["ring"])
        self.noise.x.copy_(sd["ou"].to(self.noise.x.device))
        if sd.get("env") is not None:
            self.env.load_state_dict(sd["env"])
