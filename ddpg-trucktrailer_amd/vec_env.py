"""TruckTrailerVecEnv: N truck-trailer backing envs stepped by one HIP kernel (libttenv.so).

The vector form of the reference's `Truck_trailer_Env_2` (truck_trailer_sim/simv2.py:20-545):
same reset / step / observe / pose-override surface, but every array is a torch tensor resident
on the GPU and one call advances all N envs.  torch is used for device memory and streams only;
all arithmetic happens in ddpg-trucktrailer_amd/csrc/ttenv.hip and the csrc/ttenv_*.h topic headers
it includes (step_env: csrc/ttenv_step.h), behind the C ABI of include/ttenv.h.
"""
import ctypes as C

import torch

from ddpg_trucktrailer_amd import _lib as L

_ptr = L.ptr      # (the name this module's callers import)


class TruckTrailerVecEnv:
    """N independent envs on one GPU.

    reset(seed, mask)            -> obs [N,23] f32            (simv2.py:459-498)
    step(action, auto_reset)     -> obs, reward, done, info   (simv2.py:499-545)
    set_pose / set_attrs / set_state / set_max_steps          (DDPG/test.py:96-115 pattern)
    observe(steering)            -> obs                       (simv2.py:103-181)
    """
    observation_dim = L.OBS_DIM

    def __init__(self, n_envs, device=None, variant=0, params=None):
        if not torch.cuda.is_available():
            raise RuntimeError("TruckTrailerVecEnv needs a GPU: the env step is a HIP kernel, there is no CPU path")
        self.lib = L.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("device must be a cuda (HIP) device")
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", index)
        self.n_envs = int(n_envs)
        self.params = params if params is not None else L.default_params(variant)
        self.variant = int(self.params.variant)
        h = C.c_void_p()
        L.check(self.lib.tt_env_create(self.n_envs, index, C.byref(self.params), C.byref(h)))
        self._h = h
        n = self.n_envs
        with torch.cuda.device(self.device):
            self.obs = torch.zeros((n, L.OBS_DIM), dtype=torch.float32, device=self.device)
            self.reward = torch.zeros(n, dtype=torch.float32, device=self.device)
            self.done = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self._info_bufs = None
        self.max_steer = float(self.params.max_steer)
        # bumped whenever something a captured step launch bakes in BY VALUE changes (reset seed, per-env-goal mode, pose
        # pool, step counter): holders of hipGraphs of step launches (DDPGRollout) re-capture when it moves
        self.graph_epoch = 0
        self._randomization = None      # the EpisodeRandomization that is on (enable_randomization)

    # ------------------------------------------------------------------ plumbing
    def close(self):
        if getattr(self, "_h", None):
            self.lib.tt_env_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return L.stream(self.device)

    def _check(self, rc):
        L.check(rc, self._h)

    def _as(self, x, dtype, shape=None):
        if x is None:
            return None
        t = torch.as_tensor(x, dtype=dtype, device=self.device).contiguous()
        if shape is not None:
            t = t.reshape(shape)
        return t

    def _info(self):
        if self._info_bufs is None:
            n = self.n_envs
            comp = torch.zeros((L.NINFO, n), dtype=torch.float64, device=self.device)
            viol = torch.zeros(n, dtype=torch.uint8, device=self.device)
            flags = torch.zeros(n, dtype=torch.uint8, device=self.device)
            self._info_bufs = (comp, viol, flags, L.TTInfo(comp.data_ptr(), viol.data_ptr(), flags.data_ptr()))
        return self._info_bufs

    # ------------------------------------------------------------------ reset family
    def reset(self, seed=0, mask=None, out=None):
        """Philox-sampled start poses for all (or masked) envs; returns obs [N,23]."""
        obs = self.obs if out is None else out
        m = self._as(mask, torch.uint8)
        self.graph_epoch += 1
        self._check(self.lib.tt_env_reset(self._h, L.ptr(m), int(seed) & (2 ** 64 - 1), L.ptr(obs), self._stream()))
        return obs

    def set_reset_pool(self, poses):
        """Resets (explicit and in-kernel) draw start poses from this [m,3] pool (x, y, yaw) instead of the box."""
        self.graph_epoch += 1
        if poses is None:
            self._pool = None
            self._check(self.lib.tt_env_set_reset_pool(self._h, None, 0))
            return
        self._pool = self._as(poses, torch.float64).reshape(-1, 3)      # kept alive here: the library only borrows it
        self._check(self.lib.tt_env_set_reset_pool(self._h, L.ptr(self._pool), self._pool.shape[0]))

    def set_pose(self, start, goal=None, L2=None, idx=None, out=None):
        """Pose override: start [k,3] (x, y, yaw), optional goal [k,3], L2 [k], idx [k] (default 0..k-1)."""
        start = self._as(start, torch.float64).reshape(-1, 3)
        k = start.shape[0]
        goal = self._as(goal, torch.float64, (k, 3)) if goal is not None else None
        L2 = self._as(L2, torch.float64, (k,)) if L2 is not None else None
        idx = self._as(idx, torch.int32, (k,)) if idx is not None else None
        obs = self.obs if out is None else out
        if goal is not None or L2 is not None:
            self.graph_epoch += 1          # switches the handle to per-env goals / trailer lengths
        self._check(self.lib.tt_env_set_pose(self._h, L.ptr(idx), k, L.ptr(start), L.ptr(goal), L.ptr(L2), L.ptr(obs),
                                             self._stream()))
        return obs

    def set_attrs(self, start=None, goal=None, L2=None, idx=None):
        k = None
        for x, w in ((start, 3), (goal, 3), (L2, 1)):
            if x is not None:
                k = torch.as_tensor(x).numel() // w
        if k is None:
            return
        start = self._as(start, torch.float64, (k, 3)) if start is not None else None
        goal = self._as(goal, torch.float64, (k, 3)) if goal is not None else None
        L2 = self._as(L2, torch.float64, (k,)) if L2 is not None else None
        idx = self._as(idx, torch.int32, (k,)) if idx is not None else None
        if goal is not None or L2 is not None:
            self.graph_epoch += 1
        self._check(self.lib.tt_env_set_attrs(self._h, L.ptr(idx), k, L.ptr(start), L.ptr(goal), L.ptr(L2), self._stream()))

    def set_state(self, state, idx=None):
        state = self._as(state, torch.float64).reshape(-1, 6)
        k = state.shape[0]
        idx = self._as(idx, torch.int32, (k,)) if idx is not None else None
        self._check(self.lib.tt_env_set_state(self._h, L.ptr(idx), k, L.ptr(state), self._stream()))

    def _counters(self, values, idx, what):
        """values [k] as int32 within the 12-bit packed counters (ValueError otherwise, naming `what`), idx [k] or None, k."""
        m = self._as(values, torch.int32).reshape(-1)
        k = m.shape[0]
        if k and (int(m.min()) < 0 or int(m.max()) > L.MAX_EPISODE_STEPS):
            raise ValueError(f"{what} must lie in [0, {L.MAX_EPISODE_STEPS}] (12-bit packed counters)")
        return m, self._as(idx, torch.int32, (k,)) if idx is not None else None, k

    def set_max_steps(self, max_steps, idx=None):
        m, idx, k = self._counters(max_steps, idx, "max_episode_steps")
        self._check(self.lib.tt_env_set_max_steps(self._h, L.ptr(idx), k, L.ptr(m), self._stream()))

    def set_steps(self, steps, idx=None):
        """`env.episode_steps = ...` for envs idx (default 0..k-1): the step counter alone, the reward carry stays
        (include/ttenv.h: tt_env_set_steps)."""
        m, idx, k = self._counters(steps, idx, "episode_steps")
        self._check(self.lib.tt_env_set_steps(self._h, L.ptr(idx), k, L.ptr(m), self._stream()))

    # ------------------------------------------------------------------ read-back
    @property
    def state(self):
        """[N,6] f64 (psi1, psi2, x1, y1, x2, y2), a fresh copy."""
        buf = torch.empty((6, self.n_envs), dtype=torch.float64, device=self.device)
        self._check(self.lib.tt_env_get_state(self._h, L.ptr(buf), self._stream()))
        return buf.t().contiguous()

    def episode(self):
        n = self.n_envs
        steps = torch.empty(n, dtype=torch.int32, device=self.device)
        maxs = torch.empty(n, dtype=torch.int32, device=self.device)
        start = torch.empty((3, n), dtype=torch.float64, device=self.device)
        goal = torch.empty((3, n), dtype=torch.float64, device=self.device)
        L2 = torch.empty(n, dtype=torch.float64, device=self.device)
        self._check(self.lib.tt_env_get_episode(self._h, L.ptr(steps), L.ptr(maxs), L.ptr(start), L.ptr(goal), L.ptr(L2),
                                                self._stream()))
        return dict(steps=steps, max_episode_steps=maxs, start=start.t().contiguous(), goal=goal.t().contiguous(), L2=L2)

    def observe(self, steering=None, out=None):
        obs = self.obs if out is None else out
        s = self._as(steering, torch.float32, (self.n_envs,)) if steering is not None else None
        self._check(self.lib.tt_env_observe(self._h, L.ptr(s), L.ptr(obs), self._stream()))
        return obs

    # ------------------------------------------------------------------ step
    def _step_outputs(self, obs_out, reward_out, done_out, info):
        """What step() and step_random() write and return: the env's own buffers or the caller's, the info dict (None without
        info) and the tt_info argument of the call."""
        obs = self.obs if obs_out is None else obs_out
        rew = self.reward if reward_out is None else reward_out
        done = self.done if done_out is None else done_out
        if not info:
            return obs, rew, done, None, None
        comp, viol, flags, ti = self._info()
        return obs, rew, done, dict(comp=comp, violation=viol, flags=flags), C.byref(ti)

    def step(self, action, auto_reset=True, info=False, obs_out=None, reward_out=None, done_out=None):
        """action [N] f32 radians (already scaled by action_space.high, trainv2.py:516).

        Returns (obs [N,23] f32, reward [N] f32, done [N] u8, info).  The returned tensors are the
        env's own buffers (or the *_out tensors, e.g. slots of a replay ring) and are overwritten
        by the next step.  info=True adds the per-component f64 SoA of reward_functionv1.py:489-504."""
        a = action if (torch.is_tensor(action) and action.dtype == torch.float32 and action.is_contiguous()
                       and action.device == self.device) else self._as(action, torch.float32)
        if a.numel() != self.n_envs:
            raise ValueError(f"action has {a.numel()} elements, expected {self.n_envs}")
        obs, rew, done, inf, ti = self._step_outputs(obs_out, reward_out, done_out, info)
        self._check(self.lib.tt_env_step(self._h, L.ptr(a), L.ptr(obs), L.ptr(rew), L.ptr(done), ti, 1 if auto_reset else 0,
                                         self._stream()))
        return obs, rew, done, inf

    def step_ring(self, action, ring_view, auto_reset=True):
        """step() with its outputs addressed through a trajectory ring's device cursor (tt_env_step_ring): obs into slot
        t+1, reward and done into slot t -- one captured launch serves every ring position."""
        self._check(self.lib.tt_env_step_ring(self._h, L.ptr(action), C.byref(ring_view), 1 if auto_reset else 0, self._stream()))

    def set_step_counter(self, counter):
        """counter: device int64 scalar tensor that every step launch advances by 1 (None detaches); see
        include/ttenv.h: tt_env_set_step_counter.  The tensor is kept alive by this object."""
        if counter is not None:
            assert counter.dtype == torch.int64 and counter.device == self.device and counter.numel() == 1
        self._step_counter = counter
        self.graph_epoch += 1
        self._check(self.lib.tt_env_set_step_counter(self._h, L.ptr(counter) if counter is not None else None))

    def step_random(self, policy_seed=123, auto_reset=True, info=False, action_out=None, obs_out=None, reward_out=None,
                    done_out=None):
        """step() with the random policy of BASELINE.json config 2 drawn inside the kernel (graph-capturable)."""
        obs, rew, done, inf, ti = self._step_outputs(obs_out, reward_out, done_out, info)
        self._check(self.lib.tt_env_step_random(self._h, int(policy_seed) & (2 ** 64 - 1), L.ptr(action_out), L.ptr(obs),
                                                L.ptr(rew), L.ptr(done), ti, 1 if auto_reset else 0, self._stream()))
        return obs, rew, done, inf

    def rollout_random(self, k_steps, policy_seed=123, obs_out=None, reward_sum=None, episodes_done=None):
        """k_steps random-policy steps in one launch (state stays in registers); returns the last obs buffer."""
        obs = self.obs if obs_out is None else obs_out
        self._check(self.lib.tt_env_rollout_random(self._h, int(k_steps), int(policy_seed) & (2 ** 64 - 1), L.ptr(obs),
                                                   L.ptr(reward_sum), L.ptr(episodes_done), self._stream()))
        return obs

    # ------------------------------------------------------------------ sampling MPC expert
    def mpc_plan(self, cfg, plan, mu_out, live=None, returns_out=None, seed=0):
        """One MPC decision for every lane (include/ttenv.h: tt_env_mpc_plan; mpc.MPCConfig): reads the envs, rolls cfg.samples
        perturbed copies of plan [N, H] f32 through the env step, writes the first action of the weighted mean to mu_out [N] f32
        (normalised units: step with mu_out * max_steer) and the shifted mean back into plan.  live [N] u8: lanes with 0 are skipped;
        returns_out [N, S] f64 receives every sample's return.  The envs do not change.  Capturable.  Returns mu_out."""
        from ddpg_trucktrailer_amd.mpc import check_mpc
        check_mpc(cfg, action_scale=self.max_steer, n_envs=self.n_envs, device=self.device, plan=plan, mu_out=mu_out, live=live,
                  returns_out=returns_out)
        args = L.TTMpcArgs(cfg.horizon, cfg.samples, cfg.sigma, cfg.rho, cfg.temperature, cfg.gamma, cfg.k_lat, cfg.k_yaw,
                           self.max_steer, int(seed) & (2 ** 64 - 1))
        self._check(self.lib.tt_env_mpc_plan(self._h, C.byref(args), L.ptr(plan), L.ptr(mu_out), L.ptr(live), L.ptr(returns_out),
                                             self._stream()))
        return mu_out

    def mpc_act_ring(self, cfg, plan, lanes, ring_view, high, act_scaled, seed=0):
        """One MPC decision for each of lanes [0, lanes), written over what the step's policy launch left for them
        (include/ttenv.h: tt_env_mpc_act_ring): the normalised action into the running step's action row of the ring, times `high`
        into act_scaled [N] f32.  plan [lanes, H] f32 is the lanes' plan, shifted as mpc_plan shifts it.  Between
        fused.actor_act_ring and step_ring, on their stream.  Capturable."""
        from ddpg_trucktrailer_amd.mpc import check_mpc, _check_array
        lanes = int(lanes)
        if not 1 <= lanes <= self.n_envs:
            raise ValueError(f"mpc: lanes = {lanes} is outside [1, {self.n_envs}]")
        check_mpc(cfg, action_scale=self.max_steer)
        _check_array("plan", plan, (lanes, cfg.horizon), "float32", self.device)
        _check_array("act_scaled", act_scaled, (self.n_envs,), "float32", self.device)
        args = L.TTMpcArgs(cfg.horizon, cfg.samples, cfg.sigma, cfg.rho, cfg.temperature, cfg.gamma, cfg.k_lat, cfg.k_yaw,
                           self.max_steer, int(seed) & (2 ** 64 - 1))
        self._check(self.lib.tt_env_mpc_act_ring(self._h, C.byref(args), L.ptr(plan), lanes, C.byref(ring_view), float(high),
                                                 L.ptr(act_scaled), self._stream()))

    def mpc_label_ring(self, cfg, plan, expert_lanes, label_lanes, ring_view, label, high, act_scaled, seed=0):
        """One MPC decision for each of lanes [0, expert_lanes + label_lanes) (include/ttenv.h: tt_env_mpc_label_ring): lanes
        < expert_lanes as mpc_act_ring, bit for bit; a LABELLED lane's decision goes to label [slots, N] f32 at the running step's
        slot and nowhere else -- the ring's action row, act_scaled and the env keep what the policy launch left.  plan
        [expert_lanes + label_lanes, H] f32.  In mpc_act_ring's place: between fused.actor_act_ring and step_ring, on their stream.
        Capturable."""
        from ddpg_trucktrailer_amd.mpc import check_mpc, _check_array
        m, l = int(expert_lanes), int(label_lanes)
        if m < 0 or l < 1 or m + l > self.n_envs:
            raise ValueError(f"mpc: expert_lanes = {m}, label_lanes = {l}: not M >= 0, L >= 1, M + L <= {self.n_envs}")
        check_mpc(cfg, action_scale=self.max_steer)
        _check_array("plan", plan, (m + l, cfg.horizon), "float32", self.device)
        _check_array("label", label, (int(ring_view.slots), self.n_envs), "float32", self.device)
        _check_array("act_scaled", act_scaled, (self.n_envs,), "float32", self.device)
        args = L.TTMpcArgs(cfg.horizon, cfg.samples, cfg.sigma, cfg.rho, cfg.temperature, cfg.gamma, cfg.k_lat, cfg.k_yaw,
                           self.max_steer, int(seed) & (2 ** 64 - 1))
        self._check(self.lib.tt_env_mpc_label_ring(self._h, C.byref(args), L.ptr(plan), m, l, C.byref(ring_view), L.ptr(label),
                                                   float(high), L.ptr(act_scaled), self._stream()))

    # ------------------------------------------------------------------ held lanes (greedy evaluation)
    def enable_hold(self):
        """Allocate the handle's evaluation block (include/ttenv.h: tt_env_set_hold) and the tensors hold_records() fills.
        Outside a graph capture.  step() and the episode log ignore the block."""
        self._check(self.lib.tt_env_set_hold(self._h, 1, self._stream()))
        n = self.n_envs
        with torch.cuda.device(self.device):
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)
            self._hold_out = dict(ret=z(n, torch.float64), len=z(n, torch.int32), flags=z(n, torch.uint8), success=z(n, torch.uint8),
                                  end=z((3, n), torch.float64))
            self.hold_live = z(1, torch.int64)

    def disable_hold(self):
        self._check(self.lib.tt_env_set_hold(self._h, 0, self._stream()))
        self._hold_out = self.hold_live = None

    def hold_begin(self):
        """Every lane live, every record zero: after set_pose / reset, before the first step_hold.  Capturable."""
        self._check(self.lib.tt_env_hold_begin(self._h, self._stream()))

    def step_hold(self, mu, action_scale, obs_out=None):
        """One step of every live lane with the action mu * action_scale (mu [N] f32 on this device); finished lanes hold still
        (include/ttenv.h: tt_env_step_hold).  Returns the observation buffer.  Capturable."""
        if not (torch.is_tensor(mu) and mu.dtype == torch.float32 and mu.is_contiguous() and mu.device == self.device
                and mu.numel() == self.n_envs):
            raise ValueError(f"step_hold: mu must be a contiguous f32 tensor of {self.n_envs} elements on {self.device}")
        obs = self.obs if obs_out is None else obs_out
        self._check(self.lib.tt_env_step_hold(self._h, L.ptr(mu), float(action_scale), L.ptr(obs), self._stream()))
        return obs

    def hold_count_live(self):
        """The number of lanes still live into the device int64 self.hold_live (stream-ordered, capturable); returns the tensor."""
        self._check(self.lib.tt_env_hold_read(self._h, None, None, None, None, None, L.ptr(self.hold_live), self._stream()))
        return self.hold_live

    def hold_records(self):
        """Every lane's record, in lane order, as device tensors (fresh copies): ret f64, len i32, flags u8, success bool,
        end [N,3] f64 (x2, y2, psi2 at the done step); `live`: the number of lanes not finished yet (synchronises)."""
        o = self._hold_out
        self._check(self.lib.tt_env_hold_read(self._h, L.ptr(o["ret"]), L.ptr(o["len"]), L.ptr(o["flags"]), L.ptr(o["success"]),
                                              L.ptr(o["end"]), L.ptr(self.hold_live), self._stream()))
        out = dict(ret=o["ret"].clone(), len=o["len"].clone(), flags=o["flags"].clone(), success=o["success"].bool(),
                   end=o["end"].t().contiguous())
        out["live"] = int(self.hold_live.item())
        return out

    # ------------------------------------------------------------------ episode log
    @property
    def episode_log_capacity(self):
        """Records the episode log holds between drains (0: the log is off)."""
        return getattr(self, "_log_capacity", 0)

    @property
    def episode_log_detail(self):
        """True when the episode log is on with its per-term sums and start poses (enable_episode_log(detail=True))."""
        return bool(self.episode_log_capacity) and getattr(self, "_log_detail", False)

    def enable_episode_log(self, capacity=65536, detail=False):
        """Turn on the episode log (include/ttenv.h: tt_env_set_episode_log): from the next step on, every env that
        finishes an episode appends its f64 return, length, termination flags, success (final_success_bonus > 0, the
        trainv2.py test), lane and end step, and exact counters by outcome are kept; drain_episodes() collects them.
        detail=True (tt_env_set_episode_log2, TT_LOG_DETAIL) adds to every record the episode's sum of each reward term
        (L.LOG_COMPONENTS) and its start pose.  A fresh log each call.  Captured step graphs are re-captured (graph_epoch)."""
        capacity = int(capacity)
        if capacity <= 0:
            raise ValueError("capacity must be positive (disable_episode_log() turns the log off)")
        detail = bool(detail)
        self._check(self.lib.tt_env_set_episode_log2(self._h, capacity, L.LOG_DETAIL if detail else 0, self._stream()))
        self._log_capacity = capacity
        self._log_detail = detail
        self.graph_epoch += 1
        with torch.cuda.device(self.device):
            z = lambda dt: torch.zeros(capacity, dtype=dt, device=self.device)
            self._log_out = dict(ret=z(torch.float64), len=z(torch.int32), flags=z(torch.uint8), success=z(torch.uint8),
                                 lane=z(torch.int32), end_step=z(torch.int64))
            if detail:
                self._log_detail_out = dict(components=torch.zeros((len(L.LOG_COMPONENTS), capacity), dtype=torch.float64,
                                                                   device=self.device),
                                            start=torch.zeros((3, capacity), dtype=torch.float64, device=self.device))
            self._log_n = torch.zeros(1, dtype=torch.int64, device=self.device)
            self._log_counts = torch.zeros(len(L.LOG_COUNTS), dtype=torch.int64, device=self.device)

    def disable_episode_log(self):
        """Free the log; the step launches the kernel without it again (graphs are re-captured)."""
        if self.episode_log_capacity:
            self._check(self.lib.tt_env_set_episode_log(self._h, 0, self._stream()))
        self._log_capacity = 0
        self._log_detail = False
        self._log_out = self._log_detail_out = None
        self.graph_epoch += 1

    def drain_episodes(self):
        """Records appended since the last drain, sorted by (end_step, lane) -- the order inside a launch depends on its
        atomics --, as device tensors: ret f64, len i32, flags u8, success bool, lane i32, end_step i64; plus `counts`
        ({name: int}, cumulative since enable, include/ttenv.h TT_LOG_NCOUNTS order), `written` (records appended since the
        last drain) and `dropped` (those of them past the capacity, not stored).  end_step counts the logging step launches
        since enable_episode_log (in a DDPGRollout that enables it at construction: the vector step).  A detailed log adds
        `components` [m, 9] f64 (the episode's sum of each reward term, columns L.LOG_COMPONENTS) and `start` [m, 3] f64 (its
        start pose x, y, yaw), in the same order."""
        if not self.episode_log_capacity:
            raise RuntimeError("the episode log is off (enable_episode_log)")
        o = self._log_out
        d = self._log_detail_out if self.episode_log_detail else None
        self._check(self.lib.tt_env_drain_episode_log2(self._h, L.ptr(o["ret"]), L.ptr(o["len"]), L.ptr(o["flags"]),
                                                       L.ptr(o["success"]), L.ptr(o["lane"]), L.ptr(o["end_step"]),
                                                       L.ptr(d["components"]) if d else None, L.ptr(d["start"]) if d else None,
                                                       L.ptr(self._log_n), L.ptr(self._log_counts), self._stream()))
        written = int(self._log_n.item())                 # (synchronises this stream)
        m = min(written, self.episode_log_capacity)
        key = o["end_step"][:m] * self.n_envs + o["lane"][:m].long()      # unique: one record per lane per launch
        order = torch.argsort(key)
        out = {k: v[:m][order] for k, v in o.items()}
        if d:
            out.update({k: v[:, :m].t()[order] for k, v in d.items()})
        out["success"] = out["success"].bool()
        out["counts"] = dict(zip(L.LOG_COUNTS, (int(x) for x in self._log_counts.tolist())))
        out["written"], out["dropped"] = written, written - m
        return out

    def harvest(self, h, ring_view, k_dev):
        """The successful episodes the log names since the harvest's mark, copied from the ring into the side buffer's region
        (include/ttenv.h: tt_env_harvest): h a tt_harvest (TrajectoryRing.harvest_struct), k_dev the ring's
        device step count.  Two launches on the current stream, while no step launch is in flight; the log is left untouched."""
        self._check(self.lib.tt_env_harvest(self._h, C.byref(h), C.byref(ring_view), L.ptr(k_dev), self._stream()))

    def _episode_log_state(self):
        nbytes = int(self.lib.tt_env_episode_log_bytes(self._h))
        blob = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        meta = (C.c_uint64 * 2)()
        self._check(self.lib.tt_env_export_episode_log(self._h, L.ptr(blob), C.byref(meta), self._stream()))
        return {"blob": blob.cpu(), "meta": [int(x) for x in meta], "detail": self.episode_log_detail}

    def _load_episode_log_state(self, sd):
        cap = int(sd["meta"][0])
        self.enable_episode_log(cap, detail=sd.get("detail", False))
        blob = sd["blob"].to(self.device)
        meta = (C.c_uint64 * 2)(*sd["meta"])
        self._check(self.lib.tt_env_import_episode_log(self._h, L.ptr(blob), C.byref(meta), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()      # blob is a temporary

    # ------------------------------------------------------------------ start-pose curriculum
    @property
    def curriculum(self):
        """The curriculum.Curriculum that is on, or None."""
        return getattr(self, "_curriculum", None)

    def _curriculum_arrays(self, cells):
        with torch.cuda.device(self.device):
            z = lambda n, dt: torch.zeros(n, dtype=dt, device=self.device)
            # (torch has no unsigned 32 / 64-bit arithmetic: the same bits in int32 / int64 tensors)
            return dict(p=z(cells, torch.float64), seen=z(cells, torch.int64), attempts=z(cells, torch.int32),
                        successes=z(cells, torch.int32), q=z(cells, torch.int32), cum=z(cells, torch.int32),
                        cell=z(self.n_envs, torch.int32))

    def enable_curriculum(self, cur, place=None):
        """Turn on the start-pose curriculum (include/ttenv.h: tt_env_set_curriculum; curriculum.Curriculum): from the next reset
        on, reset() and the step's auto-reset draw start poses by the cells' weights, and every finished episode is counted in the
        cell it started in; curriculum_update() turns the counts into weights.  A fresh curriculum each call.  place: None, or a
        dict of the seven device arrays (L.CURRICULUM_ARRAYS; cell of npad entries) the library is to use instead of its own.
        Outside a graph capture; captured step graphs are re-captured (graph_epoch)."""
        from ddpg_trucktrailer_amd.curriculum import Curriculum
        Curriculum.expect("curriculum", cur)
        if self.episode_log_detail:
            raise ValueError("a curriculum with episode_log_detail is not supported (the curriculum's step kernels carry the plain "
                             "episode log only)")
        cfg = cur.c_struct()
        arrays = None
        if place is not None:
            arrays = L.TTCurriculumArrays(*[place[k].data_ptr() for k in L.CURRICULUM_ARRAYS])
        self._check(self.lib.tt_env_set_curriculum(self._h, C.byref(cfg), C.byref(arrays) if arrays is not None else None,
                                                   self._stream()))
        self._curriculum, self._cur_place = cur, place          # (place is kept alive here: the library only borrows it)
        self._cur_out = self._curriculum_arrays(cur.cells)
        self.graph_epoch += 1

    def disable_curriculum(self):
        """Turn the curriculum off: resets draw from the uniform box again, launch for launch (graphs are re-captured)."""
        if self.curriculum is not None:
            self._check(self.lib.tt_env_set_curriculum(self._h, None, None, self._stream()))
        self._curriculum = self._cur_place = self._cur_out = None
        self.graph_epoch += 1

    def _need_curriculum(self):
        if self.curriculum is None:
            raise RuntimeError("the curriculum is off (enable_curriculum)")

    def curriculum_update(self):
        """The counts since the last update into the cells' success rates and draw weights: one small launch on this stream.
        Capturable."""
        self._need_curriculum()
        self._check(self.lib.tt_env_curriculum_update(self._h, self._stream()))

    def curriculum_state(self):
        """The curriculum's arrays as device tensors (fresh copies): p f64, seen i64, attempts, successes, q and cum (i32 tensors
        holding the u32 bits), each shaped [nyaw, ny, nx], and "cell" [N] i32, the cell every lane's running episode was drawn from
        (-1, the bits of L.CURRICULUM_NO_CELL: none)."""
        self._need_curriculum()
        o = self._cur_out
        arrays = L.TTCurriculumArrays(*[o[k].data_ptr() for k in L.CURRICULUM_ARRAYS])
        self._check(self.lib.tt_env_curriculum_read(self._h, C.byref(arrays), self._stream()))
        nx, ny, nyaw = self.curriculum.bins
        return {k: (v.clone() if k == "cell" else v.clone().view(nyaw, ny, nx)) for k, v in o.items()}

    def load_curriculum_state(self, state):
        """Write the arrays of `state` that are present (curriculum_state()'s names and dtypes; any shape of the right size) into the
        curriculum: a checkpoint's, or counters and weights a test plants.  A writer of q keeps cum its inclusive prefix sum."""
        self._need_curriculum()
        sizes = dict.fromkeys(L.CURRICULUM_ARRAYS, self.curriculum.cells)
        sizes["cell"] = self.n_envs
        held = {}
        for k in L.CURRICULUM_ARRAYS:
            if state.get(k) is None:
                continue
            t = torch.as_tensor(state[k]).to(device=self.device, dtype=self._cur_out[k].dtype).contiguous().reshape(-1)
            if t.numel() != sizes[k]:
                raise ValueError(f"curriculum: {k} has {t.numel()} elements, expected {sizes[k]}")
            held[k] = t
        arrays = L.TTCurriculumArrays(*[held[k].data_ptr() if k in held else None for k in L.CURRICULUM_ARRAYS])
        self._check(self.lib.tt_env_curriculum_write(self._h, C.byref(arrays), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()      # `held` are temporaries

    # ------------------------------------------------------------------ episode randomisation
    @property
    def randomization(self):
        """The randomize.EpisodeRandomization that is on (as given to enable_randomization), or None."""
        return self._randomization

    def enable_randomization(self, rand):
        """Turn on episode randomisation (include/ttenv.h: tt_env_set_randomization; randomize.EpisodeRandomization): from the next
        reset on, reset(), the masked reset and the step's auto-reset draw every new episode's goal and trailer length from the
        option's ranges (a None of the option: this env's parameters' value); the start pose is drawn as without it.  The lanes
        keep what they have until their next reset: reset(seed) after enabling gives a randomised episode 0.  The env becomes a
        per-env env, as set_pose(goal=) makes it.  Outside a graph capture; captured step graphs are re-captured (graph_epoch)."""
        from ddpg_trucktrailer_amd.randomize import EpisodeRandomization
        EpisodeRandomization.expect("randomize", rand)
        if self.curriculum is not None:
            raise ValueError("episode randomisation with a curriculum is not supported (the two have step kernels of their own, and the "
                             "curriculum's cells would be counted under a moving goal)")
        if self.episode_log_detail:
            raise ValueError("episode randomisation with episode_log_detail is not supported (the randomised step kernels carry the "
                             "plain episode log only)")
        cfg = rand.c_struct(self.params)
        self._check(self.lib.tt_env_set_randomization(self._h, C.byref(cfg), self._stream()))
        self._randomization = rand
        self.graph_epoch += 1

    def disable_randomization(self):
        """Turn episode randomisation off: the lanes keep their goals and lengths, and resets are the ones without the option from
        then on -- the parameters' goal, the lane's length (graphs are re-captured)."""
        if self.randomization is not None:
            self._check(self.lib.tt_env_set_randomization(self._h, None, self._stream()))
        self._randomization = None
        self.graph_epoch += 1

    def randomization_ranges(self):
        """The ranges the library draws from, as a resolved EpisodeRandomization (tt_env_randomization), or None when it is off."""
        from ddpg_trucktrailer_amd.randomize import EpisodeRandomization
        out = L.TTRandomization()
        if not self.lib.tt_env_randomization(self._h, C.byref(out)):
            return None
        return EpisodeRandomization(goal=(tuple(out.goal_lo), tuple(out.goal_hi)), L2=(out.L2_lo, out.L2_hi))

    # ------------------------------------------------------------------ task curriculum
    @property
    def task_curriculum(self):
        """The task_curriculum.TaskCurriculum that is on, or None."""
        return getattr(self, "_task_curriculum", None)

    def enable_task_curriculum(self, cur, place=None):
        """Turn on the task curriculum (include/ttenv.h: tt_env_set_task_curriculum; task_curriculum.TaskCurriculum), with episode
        randomisation on: from the next reset on, every reset of a lane draws the episode's goal and trailer length by the weights
        of the cells over randomisation's ranges, and every finished episode is counted in the cell its task was drawn in;
        task_curriculum_update() turns the counts into weights.  A fresh one each call.  place: as enable_curriculum's.  Outside a
        graph capture; captured step graphs are re-captured (graph_epoch)."""
        from ddpg_trucktrailer_amd.task_curriculum import TaskCurriculum, check_task_curriculum
        TaskCurriculum.expect("task_curriculum", cur)
        check_task_curriculum(cur, randomize=self.randomization)
        cur.check_ranges(self.randomization.resolved(self.params))
        cfg = cur.c_struct()
        arrays = None
        if place is not None:
            arrays = L.TTCurriculumArrays(*[place[k].data_ptr() for k in L.CURRICULUM_ARRAYS])
        self._check(self.lib.tt_env_set_task_curriculum(self._h, C.byref(cfg), C.byref(arrays) if arrays is not None else None,
                                                        self._stream()))
        self._task_curriculum, self._task_place = cur, place        # (place is kept alive here: the library only borrows it)
        self._task_out = self._curriculum_arrays(cur.cells)
        self.graph_epoch += 1

    def disable_task_curriculum(self):
        """Turn the task curriculum off: resets draw the task uniformly again, with randomisation's own kernels (graphs are
        re-captured)."""
        if self.task_curriculum is not None:
            self._check(self.lib.tt_env_set_task_curriculum(self._h, None, None, self._stream()))
        self._task_curriculum = self._task_place = self._task_out = None
        self.graph_epoch += 1

    def _need_task_curriculum(self):
        if self.task_curriculum is None:
            raise RuntimeError("the task curriculum is off (enable_task_curriculum)")

    def task_curriculum_update(self):
        """The counts since the last update into the cells' success rates and draw weights: one small launch on this stream.
        Capturable."""
        self._need_task_curriculum()
        self._check(self.lib.tt_env_task_curriculum_update(self._h, self._stream()))

    def task_curriculum_state(self):
        """The task curriculum's arrays as device tensors (fresh copies), as curriculum_state()'s, each shaped
        [nl2, ngyaw, ngy, ngx], and "cell" [N] i32, the cell every lane's running episode's task was drawn in (-1: none)."""
        self._need_task_curriculum()
        o = self._task_out
        arrays = L.TTCurriculumArrays(*[o[k].data_ptr() for k in L.CURRICULUM_ARRAYS])
        self._check(self.lib.tt_env_task_curriculum_read(self._h, C.byref(arrays), self._stream()))
        ngx, ngy, ngyaw, nl2 = self.task_curriculum.bins
        return {k: (v.clone() if k == "cell" else v.clone().view(nl2, ngyaw, ngy, ngx)) for k, v in o.items()}

    def load_task_curriculum_state(self, state):
        """Write the arrays of `state` that are present (task_curriculum_state()'s names and dtypes; any shape of the right size):
        a checkpoint's, or counters and weights a test plants.  A writer of q keeps cum its inclusive prefix sum."""
        self._need_task_curriculum()
        sizes = dict.fromkeys(L.CURRICULUM_ARRAYS, self.task_curriculum.cells)
        sizes["cell"] = self.n_envs
        held = {}
        for k in L.CURRICULUM_ARRAYS:
            if state.get(k) is None:
                continue
            t = torch.as_tensor(state[k]).to(device=self.device, dtype=self._task_out[k].dtype).contiguous().reshape(-1)
            if t.numel() != sizes[k]:
                raise ValueError(f"task_curriculum: {k} has {t.numel()} elements, expected {sizes[k]}")
            held[k] = t
        arrays = L.TTCurriculumArrays(*[held[k].data_ptr() if k in held else None for k in L.CURRICULUM_ARRAYS])
        self._check(self.lib.tt_env_task_curriculum_write(self._h, C.byref(arrays), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()      # `held` are temporaries

    def state_dict(self):
        """Everything needed to resume this env batch (device blob copied to the host + host-side mode); with the episode
        log on, its state as well (running returns, counters, launch count, records not drained yet); with a curriculum on, its
        option and arrays under "curriculum"; with episode randomisation on, its option under "randomize" (the lanes' goals and
        lengths are in the blob); with the task curriculum on, its option and arrays under "task_curriculum"."""
        nbytes = int(self.lib.tt_env_state_bytes(self._h))
        blob = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        meta = (C.c_uint64 * 4)()
        self._check(self.lib.tt_env_export(self._h, L.ptr(blob), C.byref(meta), self._stream()))
        sd = {"blob": blob.cpu(), "meta": [int(x) for x in meta], "variant": self.variant,
              "pool": None if getattr(self, "_pool", None) is None else self._pool.cpu()}
        if self.episode_log_capacity:
            sd["episode_log"] = self._episode_log_state()
        if self.curriculum is not None:
            sd["curriculum"] = {"option": list(self.curriculum.as_tuple()),
                                **{k: v.cpu() for k, v in self.curriculum_state().items()}}
        if self.randomization is not None:
            sd["randomize"] = list(self.randomization.as_tuple())
        if self.task_curriculum is not None:
            sd["task_curriculum"] = {"option": list(self.task_curriculum.as_tuple()),
                                     **{k: v.cpu() for k, v in self.task_curriculum_state().items()}}
        return sd

    def load_state_dict(self, sd):
        if sd.get("randomize") is not None:           # (before the blob: the import hands the blob's seed to the descriptor)
            from ddpg_trucktrailer_amd.options import _tupled
            from ddpg_trucktrailer_amd.randomize import EpisodeRandomization
            rand = EpisodeRandomization.from_tuple(_tupled(sd["randomize"]))
            if self.randomization != rand:
                if self.task_curriculum is not None:  # (its cells lie on the old ranges; the file's comes back below)
                    self.disable_task_curriculum()
                self.enable_randomization(rand)
        if sd.get("task_curriculum") is not None:     # (after randomisation, before the blob, for the same reason)
            from ddpg_trucktrailer_amd.options import _tupled
            from ddpg_trucktrailer_amd.task_curriculum import TaskCurriculum
            task = TaskCurriculum.from_tuple(_tupled(sd["task_curriculum"]["option"]))
            if self.task_curriculum != task:
                self.enable_task_curriculum(task)
            self.load_task_curriculum_state(sd["task_curriculum"])
        blob = sd["blob"].to(self.device)
        meta = (C.c_uint64 * 4)(*sd["meta"])
        self.graph_epoch += 1              # reset seed and per-env-goal mode come back with the blob
        self._check(self.lib.tt_env_import(self._h, L.ptr(blob), C.byref(meta), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()      # blob is a temporary
        if sd.get("pool") is not None:
            self.set_reset_pool(sd["pool"])
        if sd.get("episode_log") is not None:
            self._load_episode_log_state(sd["episode_log"])
        if sd.get("curriculum") is not None:          # (an env without one turns it on as the file has it)
            from ddpg_trucktrailer_amd.curriculum import Curriculum
            from ddpg_trucktrailer_amd.options import _tupled
            cur = Curriculum.from_tuple(_tupled(sd["curriculum"]["option"]))
            if self.curriculum != cur:
                self.enable_curriculum(cur)
            self.load_curriculum_state(sd["curriculum"])

    def profile(self, max_launches):
        """Time the next `max_launches` step-kernel dispatches with per-dispatch HIP events (0 = off)."""
        self._check(self.lib.tt_env_profile(self._h, int(max_launches)))

    def profile_read(self):
        """-> (sum of step-kernel durations in ms, number of launches timed)."""
        ms, cnt = C.c_double(), C.c_int64()
        self._check(self.lib.tt_env_profile_read(self._h, C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def random_actions(self, seed, step, out=None):
        out = torch.empty(self.n_envs, dtype=torch.float32, device=self.device) if out is None else out
        L.check(self.lib.tt_random_actions(self.n_envs, int(seed), int(step), L.ptr(out), self._stream()))
        return out
