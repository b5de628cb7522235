"""What tests/test_mpc_cpu.py (CPU), tests/test_gpu_mpc.py and tests/test_gpu_collect_demos.py (GPU) share: one decision of the
sampling MPC (include/ttenv.h: tt_env_mpc_plan) restated on the host -- the Philox noise with td3_ref.philox4x32 and the recipe of
td3_ref.noise_normal, AR(1), clip and f32 rounding in numpy, every sample rolled on a copy of the C oracle's env (oracle.c_oracle,
tto_step_batch), the return with its terminal term, the f64 softmax and the shift -- a closed loop of such decisions for short
episodes, and the lanes, plans and cases the tests use.  Nothing here touches a GPU."""
import ctypes as C
import functools

import numpy as np

from oracle import c_oracle
from td3_ref import philox4x32

NOISE_TAG = 0x4D50                      # csrc/ttenv_mpc.h: MPC_NOISE_TAG
HIGH = np.float32(np.pi / 4)            # action_scale: the env's max_steer as the C struct holds it
F32 = np.float32


def cfg_f32(cfg):
    """The config's numbers as tt_mpc_args holds them (f32), taken to f64 as the kernel does: a dict."""
    return dict(H=int(cfg.horizon), S=int(cfg.samples), sigma=float(F32(cfg.sigma)), rho=float(F32(cfg.rho)),
                lam=float(F32(cfg.temperature)), gamma=float(F32(cfg.gamma)), k_lat=float(F32(cfg.k_lat)), k_yaw=float(F32(cfg.k_yaw)))


# ---- the noise ------------------------------------------------------------------------------------------------------
def noise_normal(seed, lane, episode, steps, S, H):
    """z [S, H] f64: counter (lane, episode, steps | t << 12 | s << 18, tag), key = seed; td3_ref.noise_normal's recipe."""
    seed = int(seed) & (2 ** 64 - 1)
    s, t = np.arange(S, dtype=np.uint64)[:, None], np.arange(H, dtype=np.uint64)[None, :]
    c2 = np.uint64(int(steps)) | (t << np.uint64(12)) | (s << np.uint64(18))
    r0, r1, _, _ = philox4x32(int(lane), int(episode), c2, NOISE_TAG, seed & 0xFFFFFFFF, seed >> 32)
    u1 = (r0 >> np.uint64(8)).astype(F32) + F32(0.5)
    u2 = (r1 >> np.uint64(8)).astype(F32) + F32(0.5)
    u1, u2 = u1 * F32(1.0 / 16777216.0), u2 * F32(1.0 / 16777216.0)
    angle = (F32(6.28318530717958647692) * u2).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(angle)


def noise_eps(z, sigma, rho):
    """eps [S, H] f64 from z: AR(1) in t, sample 0 the noise-free nominal."""
    eps = np.zeros_like(z)
    c = np.sqrt(1.0 - rho * rho) * sigma
    eps[:, 0] = sigma * z[:, 0]
    for t in range(1, z.shape[1]):
        eps[:, t] = rho * eps[:, t - 1] + c * z[:, t]
    eps[0] = 0.0
    return eps


def samples(cfg, seed, lane, episode, steps, plan):
    """u [S, H] f32 for the plan as READ (the caller zeroes it at step 0)."""
    k = cfg_f32(cfg)
    eps = noise_eps(noise_normal(seed, lane, episode, steps, k["S"], k["H"]), k["sigma"], k["rho"])
    return np.clip(np.asarray(plan, F32).astype(np.float64)[None, :] + eps, -1.0, 1.0).astype(F32)


# ---- rollouts on the oracle ---------------------------------------------------------------------------------------------
def _wrap(a):
    return a - 2.0 * np.pi * np.rint(a / (2.0 * np.pi))


def returns(params, env, u, cfg, nudge=0.0):
    """G [S] f64 of the samples u [S, H] f32 from the oracle env `env` (not changed): each on a copy, the steering u * HIGH as one
    f32 product (+ nudge, in f32), cut at the first done, the terminal term where none came."""
    k = cfg_f32(cfg)
    S, H = u.shape
    envs = (c_oracle.Env * S)()
    for s in range(S):
        C.memmove(C.byref(envs[s]), C.byref(env), C.sizeof(c_oracle.Env))
    G, disc, open_ = np.zeros(S), 1.0, np.ones(S, bool)
    obs, rew, done = np.zeros((S, c_oracle.OBS_DIM), F32), np.zeros(S), np.zeros(S, np.uint8)
    info = np.zeros((S, c_oracle.NINFO))
    P = c_oracle._p
    for t in range(H):
        a = np.ascontiguousarray(u[:, t] * HIGH + F32(nudge), dtype=F32)
        c_oracle.lib().tto_step_batch(C.byref(params), envs, S, P(a, C.c_float), P(obs, C.c_float), P(rew, C.c_double),
                                      P(done, C.c_uint8), P(info, C.c_double), 1)
        G[open_] += disc * rew[open_]           # (a finished sample's copy is stepped on and ignored)
        disc *= k["gamma"]
        open_ &= done == 0
    if open_.any():
        y = np.array([list(e.y) for e in envs])
        gx, gy, gyaw = (float(v) for v in env.goal)
        lat = -(y[:, 4] - gx) * np.sin(gyaw) + (y[:, 5] - gy) * np.cos(gyaw)
        dyaw = _wrap(gyaw - y[:, 1])
        term = disc * -(k["k_lat"] * lat * lat + k["k_yaw"] * dyaw * dyaw)
        G[open_] += term[open_]
    return G


def update(G, u, lam, plan_read):
    """(mu f32, stored plan [H] f32) from the returns G [S] and the samples u [S, H]: f64 softmax, f64 sums, the shift."""
    G, H = np.asarray(G, np.float64), u.shape[1]
    fin = np.isfinite(G)
    if not fin.any():
        new = np.asarray(plan_read, F32)
    else:
        w = np.where(fin, np.exp((np.where(fin, G, 0.0) - G[fin].max()) / lam), 0.0)
        new = ((w[:, None] * u.astype(np.float64)).sum(0) / w.sum()).astype(F32)
    return new[0], np.concatenate([new[1:], new[H - 1:]]).astype(F32)


def decide(params, env, cfg, seed, lane, episode, plan):
    """One decision for the oracle env: (mu, stored plan, G, u).  The step-in-episode is the env's own."""
    steps = int(env.steps)
    plan_read = np.zeros(cfg.horizon, F32) if steps == 0 else np.asarray(plan, F32)
    u = samples(cfg, seed, lane, episode, steps, plan_read)
    G = returns(params, env, u, cfg)
    mu, new = update(G, u, cfg_f32(cfg)["lam"], plan_read)
    return mu, new, G, u


def closed_loop(start, cfg, seed, goal=None, L2=None, max_steps=400):
    """Every lane of start [n, 3] planned and stepped on the oracle until done: per lane a dict with mu [len] f32, flags, success,
    the end pose (x2, y2, psi2), the position and orientation error at the end, and the return."""
    n = len(start)
    ora = c_oracle.COracle(n)
    ora.place(start, goal, L2)
    out = []
    for i in range(n):
        env, plan, mus, ret = ora.envs[i], np.zeros(cfg.horizon, F32), [], 0.0
        obs, rew, done = np.zeros(c_oracle.OBS_DIM, F32), C.c_double(), C.c_uint8()
        info = np.zeros(c_oracle.NINFO)
        for _ in range(max_steps):
            mu, plan, _, _ = decide(ora.params, env, cfg, seed, i, 0, plan)
            c_oracle.lib().tto_step(C.byref(ora.params), C.byref(env), C.c_float(F32(mu) * HIGH), c_oracle._p(obs, C.c_float),
                                    C.byref(rew), C.byref(done), c_oracle._p(info, C.c_double))
            mus.append(mu)
            ret += rew.value
            if done.value:
                break
        y, g = list(env.y), list(env.goal)
        out.append(dict(mu=np.array(mus, F32), flags=int(env.flags), success=bool(env.flags & c_oracle.F_SUCCESS), done=bool(done.value),
                        end=(y[4], y[5], y[1]), pos_err=float(np.hypot(g[0] - y[4], g[1] - y[5])), ori_err=float(abs(_wrap(g[2] - y[1]))),
                        ret=ret))
    return out


# ---- the lanes and cases of the tests ---------------------------------------------------------------------------------------
DEFAULT_GOAL = (0.0, -30.0, np.pi / 2)
# three lanes with goals and trailer lengths of their own (PER_ENV): mid-map; within 5 m of its goal, where the staged bonuses and the
# success test fire inside the horizon; 1 m inside the map's right edge, backing out of it (the truck drives backwards: yaw pi)
START3 = np.array([[5.0, 8.0, np.radians(80.0)], [0.6, -25.8, np.radians(95.0)], [39.0, 5.0, np.pi]])
GOAL3 = np.array([[0.0, -30.0, np.pi / 2], [0.0, -29.0, np.pi / 2], [2.0, -28.0, np.radians(100.0)]])
L2_3 = np.array([7.0, 6.5, 8.0])
START1 = np.array([[-6.0, 12.0, np.radians(70.0)]])
FIRST_STEP_START = np.array([[0.0, -30.2, np.pi / 2]])      # 0.2 m behind the default goal line: the first step flags TT_F_GOAL_PASSED
WARM = 7                              # steps into an episode of the "warm" form of every lane
PLANT_SEED = 4321


def planted_actions(n):
    """[WARM, n] f32 steering in radians that takes a lane WARM steps into its episode (the same on the GPU env and the oracle)."""
    return (np.random.RandomState(PLANT_SEED).uniform(-0.5, 0.5, size=(WARM, n)) * np.pi / 4).astype(F32)


def planted_plan(n, H, seed=77):
    """[n, H] f32 in [-0.9, 0.9]: a plan that is not zero, for lanes past step 0."""
    return np.random.RandomState(seed + H).uniform(-0.9, 0.9, size=(n, H)).astype(F32)


def lanes(which):
    """(start, goal, L2) of the N = 3 PER_ENV set ("three") or the N = 1 default-goal lane ("one")."""
    return (START3, GOAL3, L2_3) if which == "three" else (START1, None, None)


def oracle_lanes(which, warm):
    """A COracle with the lanes placed and, if warm, stepped WARM times with planted_actions."""
    start, goal, L2 = lanes(which)
    ora = c_oracle.COracle(len(start))
    ora.place(start, goal, L2)
    if warm:
        for a in planted_actions(len(start)):
            ora.step(a)
    return ora


RETURN_CASES = [(S, H, rho) for S in (1, 64, 65, 300) for H in (1, 5, 12) for rho in (0.0, 0.8)]
RETURN_SEED = 2024
NEAR_EDGE = 0.5             # a sample is near an edge if a nudge of 1e-6 on every action moves the oracle's return by more
NUDGE = 1e-6
MAX_NEAR_EDGE = 0.01


def return_cfg(S, H, rho):
    from ddpg_trucktrailer_amd.mpc import MPCConfig
    return MPCConfig(horizon=H, samples=S, sigma=0.3, rho=rho, temperature=10.0, gamma=1.0, k_lat=20.0, k_yaw=300.0)


@functools.lru_cache(maxsize=None)
def return_case(S, H, rho, which, warm):
    """Per lane of the set: (u [S, H], G [S], near-edge mask [S]) on the oracle; made once per process: do not write to it."""
    cfg = return_cfg(S, H, rho)
    ora = oracle_lanes(which, warm)
    n = ora.n
    plan = planted_plan(n, H)
    out = []
    for i in range(n):
        env = ora.envs[i]
        u = samples(cfg, RETURN_SEED, i, 0, int(env.steps), plan[i] if warm else np.zeros(H, F32))
        G = returns(ora.params, env, u, cfg)
        edge = np.zeros(S, bool)
        for d in (-NUDGE, NUDGE):
            edge |= ~(np.abs(returns(ora.params, env, u, cfg, nudge=d) - G) <= NEAR_EDGE)
        out.append((u, G, edge))
    return out


# ---- the collection test's poses and config --------------------------------------------------------------------------------
# 8 lanes 8.2 to 11.7 m in front of the default goal (the vehicle reverses down -y towards it), yaw offsets 0, +-2, +-4, +-6 and 3
# degrees, each on the circular arc that meets the goal axis at the goal (bearing 90 + offset / 2 degrees).  The distances are
# tuned, per lane, so that the oracle's closed loop enters the goal box well inside it: success is terminal, so an episode ends on
# the FIRST step inside 0.5 m / 15 degrees, and where that falls depends on the path length modulo the 0.401 m step.  Larger
# offsets were tried on the oracle (5 to 20 degrees, on the axis and on the arc, k_lat to 2000, k_yaw to 20000, lambda 0.5 to 10,
# sigma 0.15 and 0.3): all 8 lanes succeed from k_lat = 500 on, but they enter the box at its orientation edge (12 to 15 degrees)
# -- no margin for a free-running comparison -- so the offsets stay small.
COLLECT_START = np.array([[0.0, -21.811, 1.571], [-0.15, -21.411, 1.606], [0.157, -21.01, 1.536], [-0.339, -20.292, 1.641],
                          [0.352, -19.911, 1.501], [-0.547, -19.572, 1.676], [0.589, -18.753, 1.466], [-0.306, -18.316, 1.623]])
COLLECT_SEED = 5
COLLECT_H, COLLECT_S = 16, 128


def collect_cfg():
    from ddpg_trucktrailer_amd.mpc import MPCConfig
    return MPCConfig(horizon=COLLECT_H, samples=COLLECT_S)


@functools.lru_cache(maxsize=None)
def collect_closed_loop():
    return closed_loop(COLLECT_START, collect_cfg(), COLLECT_SEED)
