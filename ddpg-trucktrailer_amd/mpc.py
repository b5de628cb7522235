"""The sampling MPC expert (MPPI, Williams et al. 2017): demonstrations without a solver (include/ttenv.h: tt_env_mpc_plan;
csrc/ttenv_mpc.h: k_mpc_plan).  The reference makes its demonstrations with a CasADi / IPOPT NMPC
(DDPG/exp_gen.py, npc_solver.py); here every lane rolls S perturbed steering sequences H steps forward through the env's own step,
weights them by their return and executes the first action of the weighted mean.

    MPCConfig                 horizon H, samples S, noise (sigma, rho), temperature lambda, gamma, terminal cost (k_lat, k_yaw)
    check_mpc                 everything a planning call refuses, as one pure function
    MPCExpert                 a TruckTrailerVecEnv's planner: owns the plan buffer, act() -> mu [N] in normalised units
    ExpertLanes               lanes [0, M) of a vector loop's env driven by the expert inside the captured step
    check_expert_lanes        everything a loop refuses with expert lanes, as one pure function; expert_mask: the host's mask rule
    ExpertLabels              lanes [M, M + L) of a vector loop's env labelled by the expert while the policy acts
    check_expert_labels       everything a loop refuses with expert labels, as one pure function; label_mask: the host's mask rule;
                              gather_labels: the labels of a batch's labelled rows from the ring's array
    collect_demonstrations    places lanes, runs plan -> step until every lane is done, returns the five arrays of
                              expert.transitions_to_arrays (what expert.save_transitions_npz and TrajectoryRing.load_side take)

The objective is the env's reward plus, for a rollout that did not terminate inside the horizon, a terminal cost on the trailer's
lateral offset from the goal axis and its yaw error: the reward alone has no term that looks ahead to the final alignment, and
plans that maximise it reach the goal line outside the 0.5 m / 15 degree box.  The exploration noise is AR(1) in time."""
import time

from ddpg_trucktrailer_amd import _lib as L
from ddpg_trucktrailer_amd.options import UNSET, Option, finite_number, is_number, refuse, refuse_value, whole_number

FLAG_NAMES = ("jackknife", "out_of_map", "max_steps", "goal_reached", "goal_passed", "excessive_back", "success")      # TT_F_* bits 0..6
EXP_GEN_START = (0.0, 10.0)                       # DDPG/exp_gen.py:31
EXP_GEN_YAW_DEG = (45.0, 120.0)                   # DDPG/exp_gen.py:32


class MPCConfig(Option):
    """horizon in [1, 64], samples in [1, 1024] (sample 0 is the noise-free nominal), sigma >= 0 and rho in [0, 1) of the AR(1)
    noise in normalised action units, temperature lambda > 0 of the softmax over returns, gamma in (0, 1], k_lat >= 0 [1/m^2] and
    k_yaw >= 0 [1/rad^2] of the terminal cost.  The C struct holds the numbers as f32; the kernel computes with those in f64."""
    FIELDS, A = ("horizon", "samples", "sigma", "rho", "temperature", "gamma", "k_lat", "k_yaw"), "an"

    def __init__(self, horizon=40, samples=256, sigma=0.3, rho=0.8, temperature=10.0, gamma=1.0, k_lat=20.0, k_yaw=300.0):
        self.horizon, self.samples = horizon, samples
        self.sigma, self.rho, self.temperature, self.gamma, self.k_lat, self.k_yaw = sigma, rho, temperature, gamma, k_lat, k_yaw
        check_mpc(self)
        self.horizon, self.samples = int(horizon), int(samples)
        for name in self.FIELDS[2:]:
            setattr(self, name, float(getattr(self, name)))


def _check_array(name, t, shape, dtype, device):
    if not (hasattr(t, "dtype") and hasattr(t, "is_contiguous") and str(t.dtype) == "torch." + dtype and tuple(t.shape) == shape
            and t.is_contiguous() and (device is None or t.device == device)):
        where = "" if device is None else f" on {device}"
        raise ValueError(f"mpc: {name} must be a contiguous {dtype} tensor of shape {list(shape)}{where}")


def check_mpc(cfg, action_scale=None, n_envs=None, device=None, plan=None, mu_out=None, live=None, returns_out=None):
    """What a planning call refuses, each a ValueError that names mpc and the field: the limits of include/ttenv.h
    (tt_env_mpc_plan) on the config and the action scale and, with n_envs, the buffers' dtype, shape, layout and device."""
    MPCConfig.expect("mpc: cfg", cfg)
    whole_number("mpc: horizon", cfg.horizon, 1, L.MPC_MAX_HORIZON)
    whole_number("mpc: samples", cfg.samples, 1, L.MPC_MAX_SAMPLES)
    for name in ("sigma", "k_lat", "k_yaw"):
        finite_number(f"mpc: {name}", getattr(cfg, name), ">= 0")
    if not (is_number(cfg.rho) and 0 <= cfg.rho < 1):
        refuse_value("mpc: rho", cfg.rho, "a number in [0, 1)")
    finite_number("mpc: temperature", cfg.temperature, "> 0")
    if not (is_number(cfg.gamma) and 0 < cfg.gamma <= 1):
        refuse_value("mpc: gamma", cfg.gamma, "a number in (0, 1]")
    if action_scale is not None:
        finite_number("mpc: action_scale", action_scale, "> 0")
    if n_envs is None:
        return cfg
    n = int(n_envs)
    if plan is None or mu_out is None:
        raise ValueError("mpc: plan and mu_out are required")
    _check_array("plan", plan, (n, cfg.horizon), "float32", device)
    _check_array("mu_out", mu_out, (n,), "float32", device)
    if live is not None:
        _check_array("live", live, (n,), "uint8", device)
    if returns_out is not None:
        _check_array("returns_out", returns_out, (n, cfg.samples), "float64", device)
    return cfg


class MPCExpert:
    """The planner of one TruckTrailerVecEnv: plan [N, H] f32 (zeros; a lane at step 0 of an episode reads it as zeros whatever it
    holds, so resets need no call here) and mu [N] f32.  act() makes one decision per live lane and returns mu (normalised units:
    step with mu * env.max_steer).  The noise is keyed by (seed, lane, episode number, step-in-episode) on the device: a captured
    act() replays correctly."""

    def __init__(self, env, cfg, seed=0):
        import torch
        check_mpc(cfg, action_scale=env.max_steer)
        self.env, self.cfg, self.seed = env, cfg, int(seed)
        with torch.cuda.device(env.device):
            self.plan = torch.zeros((env.n_envs, cfg.horizon), dtype=torch.float32, device=env.device)
            self.mu = torch.zeros(env.n_envs, dtype=torch.float32, device=env.device)

    def act(self, live=None, returns_out=None):
        return self.env.mpc_plan(self.cfg, self.plan, self.mu, live=live, returns_out=returns_out, seed=self.seed)


class _Lanes(Option):
    """What ExpertLanes and ExpertLabels share: lanes, an MPCConfig and the seed of the planner's noise, checked by the class's own
    check function under the option's name."""
    FIELDS, NESTED, A = ("lanes", "mpc", "seed"), {"mpc": MPCConfig}, "an"

    def __init__(self, lanes, mpc=None, seed=0):
        self.lanes, self.mpc, self.seed = lanes, MPCConfig() if mpc is None else mpc, seed
        self._well_formed(self.NAME)
        self.lanes, self.seed = int(lanes), int(seed)

    def _well_formed(self, name):
        """The value itself, as the constructor and every later check see it (a field may have been set since)."""
        if not isinstance(self.mpc, MPCConfig):
            refuse_value(f"{name}: mpc", self.mpc, "an MPCConfig")
        check_mpc(self.mpc)
        whole_number(f"{name}: lanes", self.lanes, 1)
        whole_number(f"{name}: seed", self.seed, 0, 2 ** 64 - 1, "in [0, 2^64)")


class ExpertLanes(_Lanes):
    """Expert lanes of a vector loop (include/ttenv.h: tt_env_mpc_act_ring): lanes [0, lanes) of the loop's env
    are driven by the MPC expert in every vector step -- one decision per lane between the policy launch and the env step, inside
    the captured step -- and their transitions land in the ring like any other lane's.  lanes: a whole number >= 1 (at most the
    env's lanes: the loop checks); mpc: an MPCConfig; seed: a whole number in [0, 2^64), the key of the planner's noise."""
    NAME = "expert"


def expert_mask(index, lanes):
    """The demonstration rows of a batch under expert lanes, from the draw's [B, 2] index buffer (a side row is (-1, j), a ring row
    (slot, lane)): a side row, or a ring row of a lane < lanes.  What the kernels test (csrc/ttlearn_bodies.h: DemoIn.lanes)."""
    return (index[:, 0] < 0) | (index[:, 1] < int(lanes))


def check_expert_lanes(expert, n_envs=None, ring_mode=None, population=False, data_parallel=False, force_dp=False):
    """What is refused with expert lanes, each a ValueError that names expert: a malformed ExpertLanes; with n_envs, more lanes than
    the env has; a stepper that is not in ring mode (a CPU device or a torch actor: the launch addresses the ring through its device
    cursor); a population; data-parallel ranks, the p2p exchange or the TT_FORCE_DP launch structure (not testable on one GPU)."""
    ExpertLanes.expect("expert", expert)._well_formed("expert")
    return refuse("expert", expert, n_envs=n_envs, ring_mode=ring_mode, population=population, data_parallel=data_parallel,
                  force_dp=force_dp)


class ExpertLabels(_Lanes):
    """Expert labels of a vector loop (include/ttenv.h: tt_env_mpc_label_ring): the `lanes` lanes behind the
    loop's expert lanes, [M, M + lanes) with M = 0 without ExpertLanes, are driven by the POLICY as every lane is, and in every vector
    step the MPC expert makes one decision on each of them that goes to the ring's label array -- the learner's demonstration term
    clones the label on their ring rows (DAgger: the expert labels the states the policy reaches).  lanes: a whole number >= 1
    (M + lanes at most the env's lanes: the loop checks); mpc: an MPCConfig; seed: a whole number in [0, 2^64), the key of the
    planner's noise.  With ExpertLanes in the same loop mpc and seed must be the expert's: one launch plans for both."""
    NAME = "labels"


def label_mask(index, first, count):
    """The labelled rows of a batch, from the draw's [B, 2] index buffer (a side row is (-1, j), a ring row (slot, lane)): a ring row
    of a lane in [first, first + count).  What the kernels test (csrc/ttlearn_bodies.h: DemoIn.label_first, label_count)."""
    return (index[:, 0] >= 0) & (index[:, 1] >= int(first)) & (index[:, 1] < int(first) + int(count))


def gather_labels(label, index, first, count):
    """([B] bool, [B] f32): label_mask(index, first, count) and, on those rows, label[slot, lane] of the ring's label array [slots, N];
    0 on every other row.  Only labelled rows are gathered: a side row's second index counts side tuples and may be >= N, and a
    labelled row whose slot lies past the array (never left by a draw) is not labelled, as in the kernels."""
    import torch
    mask = label_mask(index, first, count) & (index[:, 0] < label.shape[0])
    out = torch.zeros(index.shape[0], dtype=label.dtype, device=label.device)
    rows = mask.to(label.device)
    idx = index.to(label.device).long()[rows]
    out[rows] = label[idx[:, 0], idx[:, 1]]
    return mask, out


def check_expert_labels(labels, expert=None, n_envs=None, ring_mode=None, population=False, data_parallel=False, force_dp=False,
                        demo_loss=UNSET):
    """What is refused with expert labels, each a ValueError that names labels: a malformed ExpertLabels; with n_envs, more expert
    and labelled lanes together than the env has; with expert (the loop's ExpertLanes), another mpc or seed than the expert's; a
    stepper that is not in ring mode; a population; data-parallel ranks, the p2p exchange or the TT_FORCE_DP launch structure; with
    demo_loss passed, None (labels without a learner that reads them do nothing)."""
    ExpertLabels.expect("labels", labels)._well_formed("labels")
    m = 0
    if expert is not None:
        check_expert_lanes(expert)
        m = expert.lanes
        if labels.mpc.as_tuple() != expert.mpc.as_tuple():
            raise ValueError(f"labels: mpc = {labels.mpc!r} is not the expert lanes' {expert.mpc!r} (one launch plans for both)")
        if labels.seed != expert.seed:
            raise ValueError(f"labels: seed = {labels.seed} is not the expert lanes' {expert.seed} (one launch plans for both)")
    return refuse("labels", labels, first=m, n_envs=n_envs, ring_mode=ring_mode, population=population, data_parallel=data_parallel,
                  force_dp=force_dp, demo_loss=demo_loss)


def exp_gen_poses(lanes, seed=0):
    """[lanes, 3] f64 start poses of the reference's expert generator: (0, 10, U(45, 120) degrees) (DDPG/exp_gen.py:31-32)."""
    import numpy as np
    yaw = np.random.RandomState(seed).uniform(*EXP_GEN_YAW_DEG, size=int(lanes))
    return np.stack([np.full(lanes, EXP_GEN_START[0]), np.full(lanes, EXP_GEN_START[1]), np.radians(yaw)], axis=1)


def collect_demonstrations(lanes, cfg, poses=None, seed=0, goal=None, L2=None, keep="success", max_steps=None, device=None):
    """Run the MPC expert on `lanes` envs, one episode each, and return ((obs, act, rew, obs2, done), stats).

    poses [lanes, 3] (x, y, yaw) places the lanes with set_pose (goal [lanes, 3] / L2 [lanes] optional); poses = None draws the
    env's own start distribution with reset(seed).  `seed` also keys the planner's noise.  Each vector step plans, then steps with
    env.step(mu * max_steer, auto_reset=False, info=True); obs, mu, the f32 reward, the next obs, done and the flags are recorded
    time-major on the device, live &= ~done stays on the device, and the loop ends when no lane is live or after max_steps vector
    steps (None: the longest episode the envs allow).  Every lane is cut at its first done.  keep = "success": only episodes that
    end with TT_F_SUCCESS; "all": every episode, those cut by max_steps included (their last tuple has done = False).
    The arrays are those of expert.transitions_to_arrays -- obs [k, 23] f32, act [k, 1] f32 (the normalised mu, what
    exp_gen.py:80 stores), rew [k] f32, obs2 [k, 23] f32, done [k] bool -- episode after episode in lane order.
    stats: episodes, finished, successes, flags {name: count at the episode's last step}, kept_episodes, transitions, lanes,
    lengths and end_flags (the TT_F_* byte of the last step) of the kept episodes (in order), mean_return (f64 sum of the f32 rewards) and mean_length of the kept episodes,
    vector_steps, seconds."""
    import numpy as np
    import torch
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    if keep not in ("success", "all"):
        raise ValueError(f"collect_demonstrations: keep = {keep!r} is not 'success' or 'all'")
    if poses is None and (goal is not None or L2 is not None):
        raise ValueError("collect_demonstrations: goal / L2 need poses (reset() draws poses for the default goal)")
    n = int(lanes)
    env = TruckTrailerVecEnv(n, device=device)
    check_mpc(cfg, action_scale=env.max_steer)
    dev = env.device
    t_begin = time.perf_counter()
    if poses is None:
        env.reset(seed=seed)
    else:
        env.set_pose(np.asarray(poses, np.float64).reshape(n, 3), goal=goal, L2=L2)
    longest = int(env.episode()["max_episode_steps"].max().item())
    steps_cap = longest if max_steps is None else min(int(max_steps), longest)
    if steps_cap < 1:
        raise ValueError(f"collect_demonstrations: max_steps = {max_steps!r} leaves no step")
    expert = MPCExpert(env, cfg, seed=seed)
    with torch.cuda.device(dev):
        obs = torch.zeros((steps_cap + 1, n, L.OBS_DIM), dtype=torch.float32, device=dev)
        act = torch.zeros((steps_cap, n), dtype=torch.float32, device=dev)
        rew = torch.zeros((steps_cap, n), dtype=torch.float32, device=dev)
        done = torch.zeros((steps_cap, n), dtype=torch.uint8, device=dev)
        flags = torch.zeros((steps_cap, n), dtype=torch.uint8, device=dev)
        live = torch.ones(n, dtype=torch.uint8, device=dev)
        steer = torch.zeros(n, dtype=torch.float32, device=dev)
    obs[0].copy_(env.obs)
    steps = 0
    while steps < steps_cap:
        mu = expert.act(live=live)
        act[steps].copy_(mu)
        torch.mul(mu, env.max_steer, out=steer)
        _, _, _, info = env.step(steer, auto_reset=False, info=True, obs_out=obs[steps + 1], reward_out=rew[steps],
                                 done_out=done[steps])
        flags[steps].copy_(info["flags"])
        live.mul_(done[steps] == 0)
        steps += 1
        if not bool(live.any().item()):
            break
    seconds = time.perf_counter() - t_begin
    env.close()

    done_h = done[:steps].cpu().numpy().astype(bool)
    finished = done_h.any(axis=0)
    length = np.where(finished, done_h.argmax(axis=0) + 1, steps)
    last_flags = flags[:steps].cpu().numpy()[length - 1, np.arange(n)]
    success = finished & ((last_flags & L.F_SUCCESS) != 0)
    kept = np.nonzero(success if keep == "success" else np.ones(n, bool))[0]
    obs_h, act_h, rew_h = obs[:steps + 1].cpu().numpy(), act[:steps].cpu().numpy(), rew[:steps].cpu().numpy()
    cols = [[], [], [], [], []]
    for i in kept:
        k = int(length[i])
        for c, x in zip(cols, (obs_h[:k, i], act_h[:k, i, None], rew_h[:k, i], obs_h[1:k + 1, i], done_h[:k, i])):
            c.append(x)
    if len(kept):
        arrays = tuple(np.concatenate(c) for c in cols)
    else:
        arrays = (np.zeros((0, L.OBS_DIM), np.float32), np.zeros((0, 1), np.float32), np.zeros(0, np.float32),
                  np.zeros((0, L.OBS_DIM), np.float32), np.zeros(0, np.bool_))
    arrays = (arrays[0].astype(np.float32), arrays[1].astype(np.float32), arrays[2].astype(np.float32), arrays[3].astype(np.float32),
              arrays[4].astype(np.bool_))
    returns = [float(rew_h[:int(length[i]), i].astype(np.float64).sum()) for i in kept]
    stats = dict(episodes=n, finished=int(finished.sum()), successes=int(success.sum()),
                 flags={name: int((finished & ((last_flags >> b) & 1 != 0)).sum()) for b, name in enumerate(FLAG_NAMES)},
                 kept_episodes=int(len(kept)), transitions=int(arrays[2].shape[0]), lanes=[int(i) for i in kept],
                 lengths=[int(length[i]) for i in kept], end_flags=[int(last_flags[i]) for i in kept], mean_return=float(np.mean(returns)) if returns else float("nan"),
                 mean_length=float(np.mean(length[kept])) if len(kept) else float("nan"), vector_steps=int(steps),
                 seconds=float(seconds))
    return arrays, stats
