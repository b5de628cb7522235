"""Greedy evaluation on the device: K agents' deterministic policies on the SAME M start poses.

The reference evaluates with evaluate=True from fixed poses (DDPG/test.py:96-115, heatmap.py:79-193).  Here an Evaluator owns one
env of agents * lanes lanes -- agent a's lanes are [a * lanes, (a + 1) * lanes) -- whose step holds finished lanes still
(TruckTrailerVecEnv.step_hold): a step is one policy forward per agent plus one env launch, a chunk of steps is one hipGraph, the
host looks once per chunk (how many lanes are still live), and every lane leaves its episode's record in its own slot, so the
result is bit-reproducible.

    ev = Evaluator(lanes=256, agents=K, seed=0)
    records = ev.run([ag.actor for ag in pop.agents])       # per agent: ret, len, flags, success, end, in lane order
    print(summary(records[0]))
    pbt.step(pop, pop.drain_episodes(), evaluation=records)

The records' keys and dtypes are those PBT.observe and checkpoint.BestModelTracker.update_many take."""
import gc

import numpy as np
import torch

from ddpg_trucktrailer_amd import _lib as L
from ddpg_trucktrailer_amd import fused

FLAG_NAMES = ("jackknife", "out_of_map", "max_steps", "goal_reached", "goal_passed", "excessive_back", "success_flag")


def summary(records):
    """One agent's records -> {"episodes", "mean_return", "success_rate", "mean_len", "flags": {name: count}}."""
    host = lambda x: np.asarray(x.detach().cpu() if hasattr(x, "detach") else x)
    ret, ok, flags, length = host(records["ret"]), host(records["success"]), host(records["flags"]), host(records["len"])
    m = len(ret)
    return {"episodes": m, "mean_return": float(ret.mean()) if m else float("nan"),
            "success_rate": float(ok.astype(bool).mean()) if m else float("nan"),
            "mean_len": float(length.mean()) if m else float("nan"),
            "flags": {name: int(((flags >> b) & 1).sum()) for b, name in enumerate(FLAG_NAMES)}}


def _rows(x, lanes, width, what):
    """x as a host f64 [lanes, width] (one row: the same for every lane), or None."""
    if x is None:
        return None
    a = np.asarray(x.detach().cpu() if hasattr(x, "detach") else x, dtype=np.float64)
    if a.size == width:
        return np.tile(a.reshape(1, width), (lanes, 1))
    if a.size != lanes * width:
        raise ValueError(f"Evaluator: {what} must hold {width} or [{lanes},{width}] values, not {a.shape}")
    return a.reshape(lanes, width)


class Evaluator:
    def __init__(self, lanes, agents=1, poses=None, seed=0, goal=None, L2=None, max_steps=None, chunk=32, device=None,
                 use_graph=True, params=None):
        """lanes start poses per agent (a multiple of 4: every agent's observation slice is then 16-byte aligned), the same for
        every agent: `poses` [lanes,3] (x, y, yaw), or drawn once on the host with np.random.RandomState(seed) from the env
        parameters' reset box.  goal [3] or [lanes,3], L2 scalar or [lanes] (default: the parameters'), max_steps int or [lanes]
        (default: what the pose gives).  chunk: steps per graph replay, and between two looks at the live count.  use_graph=False:
        the same launches, eagerly.  The env is made by the first run()."""
        self.lanes, self.agents, self.chunk = int(lanes), int(agents), int(chunk)
        if self.lanes <= 0 or self.lanes % 4:
            raise ValueError(f"Evaluator: lanes = {lanes} must be a positive multiple of 4 (16-byte aligned observation slices)")
        if self.agents < 1 or self.chunk < 1:
            raise ValueError(f"Evaluator: agents = {agents} and chunk = {chunk} must be >= 1")
        self.params = params if params is not None else L.default_params(0)
        if poses is None:
            rng = np.random.RandomState(seed)
            lo, hi = np.array(self.params.reset_lo[:]), np.array(self.params.reset_hi[:])
            poses = lo + (hi - lo) * rng.uniform(size=(self.lanes, 3))
        else:
            poses = np.asarray(poses.detach().cpu() if hasattr(poses, "detach") else poses, dtype=np.float64)
            if poses.shape != (self.lanes, 3):
                raise ValueError(f"Evaluator: poses must be [{self.lanes},3] (x, y, yaw), not {list(poses.shape)}")
        self.poses = poses
        self.goal = _rows(goal, self.lanes, 3, "goal")
        self.L2 = None if L2 is None else _rows(L2, self.lanes, 1, "L2").reshape(-1)
        self.max_steps = None
        if max_steps is not None:
            m = np.asarray(max_steps, dtype=np.int64).reshape(-1)
            if m.size not in (1, self.lanes) or m.min() < 1 or m.max() > L.MAX_EPISODE_STEPS:
                raise ValueError(f"Evaluator: max_steps must be one or {self.lanes} values in [1, {L.MAX_EPISODE_STEPS}]")
            self.max_steps = np.broadcast_to(m, (self.lanes,)).astype(np.int32)
        self.device, self.use_graph = device, bool(use_graph)
        self.high = float(np.float32(np.pi / 4))           # env.action_space.high (f32 pi/4, simv2.py:86-91)
        self.env = None
        self._graph = self._graph_key = None
        self.steps_run = self.replays = self.captures = 0

    # ------------------------------------------------------------------------------------------------- the env
    def _make_env(self):
        from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
        K = self.agents
        env = self.env = TruckTrailerVecEnv(K * self.lanes, device=self.device, params=self.params)
        env.enable_hold()
        tile = lambda x: None if x is None else torch.as_tensor(np.tile(x, (K,) + (1,) * (x.ndim - 1)), device=env.device)
        self._start, self._goal, self._l2 = tile(self.poses), tile(self.goal), tile(self.L2)
        self._maxs = None if self.max_steps is None else tile(self.max_steps).to(torch.int32)
        self.mu = torch.zeros(K * self.lanes, dtype=torch.float32, device=env.device)
        self._warm = False

    def close(self):
        self._graph = None
        if self.env is not None:
            self.env.close()
            self.env = None

    def _slices(self):
        M = self.lanes
        return [(self.env.obs[a * M:(a + 1) * M], self.mu[a * M:(a + 1) * M]) for a in range(self.agents)]

    def _place(self):
        env = self.env
        env.set_pose(self._start, goal=self._goal, L2=self._l2)
        if self._maxs is not None:
            env.set_max_steps(self._maxs)

    # ------------------------------------------------------------------------------------------------- the fused path
    def _body(self, actors):
        """`chunk` steps' launches and the live count behind them (no host work): what the graph holds."""
        env = self.env
        pairs = self._slices()
        for _ in range(self.chunk):
            for net, (obs, mu) in zip(actors, pairs):
                fused.actor_forward(net, obs, mu)          # (packs the image from the current weights, then the forward)
            env.step_hold(self.mu, self.high)
        env.hold_count_live()

    def _capture(self, actors):
        for net in actors:
            fused.weights_of(net)                          # (its workspace is allocated here, not inside the capture)
        gc.collect()
        was_on = gc.isenabled()
        gc.disable()       # (a collected graph / stream / handle runs HIP calls in its destructor: illegal during capture)
        try:
            cur = torch.cuda.current_stream(self.env.device)
            side = torch.cuda.Stream(device=self.env.device)
            side.wait_stream(cur)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                self._body(actors)
            cur.wait_stream(side)
        finally:
            if was_on:
                gc.enable()
        self.captures += 1
        return g

    def _run_fused(self, actors):
        env = self.env
        if not self._warm:
            # every kernel of the body once before any capture, on an env whose lanes are all held: nothing moves
            for net, (obs, mu) in zip(actors, self._slices()):
                fused.actor_forward(net, obs, mu)
            env.step_hold(self.mu, self.high)
            env.hold_count_live()
            self._warm = True
        self._place()
        env.hold_begin()
        if self.use_graph:
            key = tuple(fused.packed_key_of(net) for net in actors)
            if self._graph is None or self._graph_key != key:
                self._graph, self._graph_key = self._capture(actors), key
        while self.steps_run < L.MAX_EPISODE_STEPS:
            if self.use_graph:
                self._graph.replay()
            else:
                self._body(actors)
            self.steps_run += self.chunk
            self.replays += 1
            if int(env.hold_live.item()) == 0:         # the only synchronize, once per chunk
                break

    # ------------------------------------------------------------------------------------------------- the torch path
    def _run_host(self, actors):
        """grid_eval's host loop (any module through torch; kept for tests): the plain step with info, lanes masked on the host."""
        env, M = self.env, self.lanes
        n = env.n_envs
        dev = env.device
        self._place()
        obs = env.obs
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        rec = dict(ret=z(n, torch.float64), len=z(n, torch.int32), flags=z(n, torch.uint8), success=z(n, torch.bool),
                   end=z((n, 3), torch.float64))
        finished = z(n, torch.bool)
        while self.steps_run < L.MAX_EPISODE_STEPS:
            for a, net in enumerate(actors):
                o = obs[a * M:(a + 1) * M]
                if fused.supported(net):
                    fused.actor_forward(net, o, self.mu[a * M:(a + 1) * M])
                else:
                    self.mu[a * M:(a + 1) * M] = net(o).view(-1)
            obs, _, done, info = env.step(self.mu * self.high, auto_reset=False, info=True)
            self.steps_run += 1
            live = ~finished
            rec["ret"] += torch.where(live, info["comp"][0], torch.zeros_like(rec["ret"]))
            newly = live & done.bool()
            st = env.state
            rec["len"] = torch.where(newly, env.episode()["steps"], rec["len"])
            rec["flags"] = torch.where(newly, info["flags"], rec["flags"])
            rec["success"] = torch.where(newly, info["comp"][L.INFO_ROWS.index("final_success_bonus")] > 0, rec["success"])
            rec["end"] = torch.where(newly.unsqueeze(1), st[:, [4, 5, 1]], rec["end"])
            finished |= done.bool()
            if bool(finished.all()):
                break
        rec["live"] = int((~finished).sum())
        return rec

    # ------------------------------------------------------------------------------------------------- run
    @torch.no_grad()
    def run(self, actors, host_loop=False):
        """One evaluation of `actors` (one module per agent) from the Evaluator's poses, on the current stream.  Returns per agent
        {"ret" f64, "len" i32, "flags" u8, "success" bool, "end" [lanes,3] f64}, device tensors in lane order.  A lane that has
        not finished within TT_MAX_EPISODE_STEPS steps (none can: max_steps ends it) would keep a zero record.
        host_loop=True forces the torch path's host-masked loop."""
        actors = list(actors)
        if len(actors) != self.agents:
            raise ValueError(f"Evaluator.run: {len(actors)} actors for {self.agents} agents")
        if self.env is None:
            self._make_env()
        self.steps_run = self.replays = 0
        dev = self.env.device
        if host_loop or not all(fused.supported(net) and net.fc1.weight.device == dev for net in actors):
            rec = self._run_host(actors)
        else:
            self._run_fused(actors)
            rec = self.env.hold_records()
        self.live_left = rec.pop("live")
        M = self.lanes
        return [{k: v[a * M:(a + 1) * M] for k, v in rec.items()} for a in range(self.agents)]
