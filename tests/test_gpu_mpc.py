"""GPU (-m gpu): one decision of the sampling MPC (csrc/ttenv_mpc.h: k_mpc_plan; include/ttenv.h: tt_env_mpc_plan)
against the env's own step, the C oracle and the host statement of tests/mpc_ref.py.

    prediction   S = 1, sigma = 0, no terminal term: the return is the f64 sum of TT_I_TOTAL over H env.step calls, bit for bit
                 (gamma = 0.9: 1e-12 relative), and the planning launch leaves tt_env_export's blob as it was
    returns      every sample's return against the oracle: H * 1e-5 + 1e-5, samples near a discrete reward edge left out
    update       mu_out and the stored plan from the GPU's own returns and mpc_ref's u: 2^-22 of the f64 host value
    streams      same call, same bits; seed, episode number and step-in-episode key the noise; step 0 ignores the plan; live mask; fences
    capture      six (plan, step) iterations in one hipGraph == the eager loop, bit for bit

The lanes (mpc_ref.lanes): N = 3 with goals and trailer lengths of their own -- mid-map, within 5 m of its goal, 1 m inside the
map's edge heading out -- and N = 1 with the default goal, each fresh (step 0) and WARM = 7 planted steps into its episode.

Measured on MI355X: worst |G - oracle| 8.3e-6 at H = 12 (bound 1.3e-4), no sample near an edge; worst |U' - f64| 3.0e-8 (bound 2.4e-7)."""
import numpy as np
import pytest

import mpc_ref as M

pytestmark = pytest.mark.gpu

FORMS = [(which, warm) for which in ("three", "one") for warm in (False, True)]


def _cfg(**kw):
    from ddpg_trucktrailer_amd.mpc import MPCConfig
    return MPCConfig(**kw)


def _env(dev, which, warm):
    import torch
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    start, goal, L2 = M.lanes(which)
    env = TruckTrailerVecEnv(len(start), device=dev)
    env.set_pose(start, goal=goal, L2=L2)
    if warm:
        for a in M.planted_actions(len(start)):
            env.step(torch.from_numpy(a).to(dev), auto_reset=False)
    return env


def _blob(env):
    sd = env.state_dict()
    return sd["blob"].numpy().copy(), list(sd["meta"])


def _plan(dev, cfg, plan, env, seed=M.RETURN_SEED, live=None, want_returns=True):
    """One planning launch on copies: (mu, stored plan, returns) as numpy."""
    import torch
    p = torch.from_numpy(np.ascontiguousarray(plan, np.float32)).to(dev)
    mu = torch.zeros(env.n_envs, dtype=torch.float32, device=dev)
    ret = torch.zeros((env.n_envs, cfg.samples), dtype=torch.float64, device=dev) if want_returns else None
    env.mpc_plan(cfg, p, mu, live=live, returns_out=ret, seed=seed)
    torch.cuda.synchronize()
    return mu.cpu().numpy(), p.cpu().numpy(), None if ret is None else ret.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])


# ---- 1: prediction is the env ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,warm", FORMS)
@pytest.mark.parametrize("H", [1, 5, 12])
def test_prediction_is_the_env_step(gpu_device, H, which, warm):
    import torch
    n = len(M.lanes(which)[0])
    planted = M.planted_plan(n, H)
    eff = planted if warm else np.zeros_like(planted)            # a lane at step 0 reads its plan as zeros
    for gamma in (1.0, 0.9):
        cfg = _cfg(horizon=H, samples=1, sigma=0.0, rho=0.0, gamma=gamma, k_lat=0.0, k_yaw=0.0)
        env = _env(gpu_device, which, warm)
        before = _blob(env)
        _, _, G = _plan(gpu_device, cfg, planted, env)
        after = _blob(env)
        assert before[1] == after[1] and np.array_equal(before[0], after[0]), "the planning launch changed the env"
        g = float(np.float32(gamma))
        ref, disc, open_ = np.zeros(n), 1.0, np.ones(n, bool)
        high = torch.tensor(float(M.HIGH), dtype=torch.float32, device=gpu_device)
        for t in range(H):
            a = torch.from_numpy(eff[:, t].copy()).to(gpu_device) * high
            _, _, done, info = env.step(a, auto_reset=False, info=True)
            total = info["comp"][0].cpu().numpy()
            ref[open_] += disc * total[open_]
            disc *= g
            open_ &= done.cpu().numpy() == 0
        print(f"H={H} {which} warm={warm} gamma={gamma}: G = {G[:, 0]}, env = {ref}")
        if gamma == 1.0:
            assert np.array_equal(_bits(G[:, 0]), _bits(ref)), (G[:, 0], ref)
        else:
            assert np.all(np.abs(G[:, 0] - ref) <= 1e-12 * np.abs(ref)), (G[:, 0], ref)
        env.close()


# ---- 2: per-sample returns against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("S,H,rho", M.RETURN_CASES)
def test_returns_against_the_oracle(gpu_device, S, H, rho):
    cfg = M.return_cfg(S, H, rho)
    tol = H * 1e-5 + 1e-5
    for which, warm in FORMS:
        ref = M.return_case(S, H, rho, which, warm)
        env = _env(gpu_device, which, warm)
        _, _, G = _plan(gpu_device, cfg, M.planted_plan(env.n_envs, H), env)
        for i, (u, g_ref, edge) in enumerate(ref):
            assert edge.mean() <= M.MAX_NEAR_EDGE
            err = np.abs(G[i] - g_ref)[~edge]
            print(f"S={S} H={H} rho={rho} {which} warm={warm} lane {i}: max |G - oracle| = {err.max():.3e} (tol {tol:.1e}), "
                  f"{int(edge.sum())} near an edge")
            assert np.all(err <= tol), (which, warm, i, float(err.max()), int(np.argmax(np.abs(G[i] - g_ref) * ~edge)))
        env.close()


# ---- 3: the update ------------------------------------------------------------------------------------------------------------
UPDATE_TOL = 2.0 ** -22


def _check_update(dev, cfg, which, warm, env=None, plan=None, seed=M.RETURN_SEED):
    env = env or _env(dev, which, warm)
    n, H = env.n_envs, cfg.horizon
    plan = M.planted_plan(n, H) if plan is None else plan
    steps = env.episode()["steps"].cpu().numpy()
    mu, stored, G = _plan(dev, cfg, plan, env, seed=seed)
    assert np.isfinite(mu).all() and np.isfinite(stored).all() and np.isfinite(G).all()
    for i in range(n):
        read = plan[i] if steps[i] > 0 else np.zeros(H, np.float32)
        u = M.samples(cfg, seed, i, 0, int(steps[i]), read)
        m_ref, p_ref = M.update(G[i], u, M.cfg_f32(cfg)["lam"], read)
        # the host value before its own f32 rounding is within 2^-24 of m_ref; the bound is on the f64 value
        w = np.exp((G[i] - G[i].max()) / M.cfg_f32(cfg)["lam"])
        exact = (w[:, None] * u.astype(np.float64)).sum(0) / w.sum()
        new = np.concatenate([[mu[i]], stored[i][:H - 1]]).astype(np.float64)
        err = np.abs(new - exact).max()
        print(f"{cfg} {which} warm={warm} lane {i}: max |U' - f64| = {err:.3e} (tol {UPDATE_TOL:.3e}), weight of the best {w.max() / w.sum():.3f}")
        assert err <= UPDATE_TOL, (i, err)
        assert abs(float(mu[i]) - float(m_ref)) <= UPDATE_TOL and np.abs(stored[i] - p_ref).max() <= UPDATE_TOL
        if H >= 2:
            assert _bits(stored[i])[H - 1] == _bits(stored[i])[H - 2]
        assert np.all(np.abs(stored[i]) <= 1.0) and abs(mu[i]) <= 1.0
    return mu, stored, G


@pytest.mark.parametrize("which,warm", FORMS)
@pytest.mark.parametrize("S,H", [(1, 1), (65, 12), (300, 5)])
def test_update_against_f64(gpu_device, S, H, which, warm):
    _check_update(gpu_device, M.return_cfg(S, H, 0.8), which, warm)


@pytest.mark.parametrize("lam", [1e-3, 1e6])
def test_update_at_extreme_temperatures(gpu_device, lam):
    """lambda = 1e-3: one sample holds all the weight and nothing is NaN; lambda = 1e6: the plain mean."""
    cfg = _cfg(horizon=12, samples=65, temperature=lam)
    mu, stored, G = _check_update(gpu_device, cfg, "three", True)
    u = [M.samples(cfg, M.RETURN_SEED, i, 0, M.WARM, M.planted_plan(3, 12)[i]) for i in range(3)]
    for i in range(3):
        new = np.concatenate([[mu[i]], stored[i][:11]])
        want = u[i][np.argmax(G[i])] if lam < 1 else u[i].astype(np.float64).mean(0)
        # (the plain mean: every weight is within (max G - min G) / lambda of 1, every u within 2 of the mean)
        tol = UPDATE_TOL if lam < 1 else UPDATE_TOL + 2.0 * (G[i].max() - G[i].min()) / lam
        assert np.abs(new - want).max() <= tol, (i, np.abs(new - want).max(), tol)


def test_update_when_every_sample_ends_on_the_first_step(gpu_device):
    """The lane of mpc_ref.FIRST_STEP_START: tests/test_mpc_cpu.py asserts on the oracle that every sample is done after one step."""
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    cfg = M.return_cfg(65, 5, 0.8)
    env = TruckTrailerVecEnv(1, device=gpu_device)
    env.set_pose(M.FIRST_STEP_START)
    _check_update(gpu_device, cfg, "one", False, env=env)
    # a planted plan two steps into nothing: the same lane with its step counter moved reads the plan
    env.set_steps(np.array([3], np.int32))
    mu, stored, G = _plan(gpu_device, cfg, M.planted_plan(1, 5), env)
    assert np.isfinite(G).all() and np.isfinite(mu).all() and np.isfinite(stored).all()


# ---- 4: streams and masks -----------------------------------------------------------------------------------------------------
def _differ(Ga, Gb):
    """Other noise: in every lane at least 90 % of the noisy samples' returns differ (not all: where the first step ends every
    rollout, as for the lane outside the map, samples clipped to the same bound have the same return under any noise)."""
    return bool(np.all((Ga[:, 1:] != Gb[:, 1:]).mean(axis=1) >= 0.9))


def test_same_call_same_bits_and_what_keys_the_noise(gpu_device):
    import torch
    cfg = M.return_cfg(65, 5, 0.8)
    plan = M.planted_plan(3, 5)
    env = _env(gpu_device, "three", True)
    a = _plan(gpu_device, cfg, plan, env)
    b = _plan(gpu_device, cfg, plan, env)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    c = _plan(gpu_device, cfg, plan, env, seed=M.RETURN_SEED + 1)
    assert np.array_equal(_bits(c[2][:, 0]), _bits(a[2][:, 0])), "sample 0 is the noise-free nominal"
    assert _differ(c[2], a[2]), "another seed, the same noise"
    # another step-in-episode: the counter alone moves (tt_env_set_steps leaves state and reward carry)
    env.set_steps(np.full(3, M.WARM + 1, np.int32))
    d = _plan(gpu_device, cfg, plan, env)
    assert _differ(d[2], a[2]), "another step-in-episode, the same noise"
    env.close()
    # another episode number: a masked reset moves the lanes to episode 1; the same poses and planted steps follow
    env = _env(gpu_device, "three", False)
    env.reset(seed=3, mask=torch.ones(3, dtype=torch.uint8, device=gpu_device))
    start, goal, L2 = M.lanes("three")
    env.set_pose(start, goal=goal, L2=L2)
    for act in M.planted_actions(3):
        env.step(torch.from_numpy(act).to(gpu_device), auto_reset=False)
    e = _plan(gpu_device, cfg, plan, env)
    assert np.array_equal(_bits(e[2][:, 0]), _bits(a[2][:, 0])), "the same state: the nominal's return has the same bits"
    assert _differ(e[2], a[2]), "another episode number, the same noise"
    for i in range(3):          # and it is the noise mpc_ref makes for episode 1
        u = M.samples(cfg, M.RETURN_SEED, i, 1, M.WARM, plan[i])
        m_ref, p_ref = M.update(e[2][i], u, M.cfg_f32(cfg)["lam"], plan[i])
        assert abs(float(e[0][i]) - float(m_ref)) <= UPDATE_TOL and np.abs(e[1][i] - p_ref).max() <= UPDATE_TOL
    env.close()


def test_step_zero_ignores_the_plan(gpu_device):
    cfg = M.return_cfg(65, 5, 0.8)
    env = _env(gpu_device, "three", False)
    a = _plan(gpu_device, cfg, M.planted_plan(3, 5), env)
    b = _plan(gpu_device, cfg, np.zeros((3, 5), np.float32), env)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    env.close()


def test_live_mask_keeps_a_skipped_lane(gpu_device):
    import torch
    import fenced
    cfg = M.return_cfg(65, 5, 0.8)
    env = _env(gpu_device, "three", True)
    full = _plan(gpu_device, cfg, M.planted_plan(3, 5), env)
    plain = fenced.Plain(gpu_device)
    plan = plain.inp("plan", torch.from_numpy(M.planted_plan(3, 5)).to(gpu_device))
    mu, ret = plain.out("mu_out", 3), plain.out("returns_out", (3, 65), torch.float64)
    keep = [t.clone() for t in (plan, mu, ret)]
    live = torch.tensor([1, 0, 1], dtype=torch.uint8, device=gpu_device)
    env.mpc_plan(cfg, plan, mu, live=live, returns_out=ret, seed=M.RETURN_SEED)
    torch.cuda.synchronize()
    for got, was, ref in zip((plan, mu, ret), keep, (full[1], full[0], full[2])):
        got, was = got.cpu().numpy(), was.cpu().numpy()
        assert np.array_equal(_bits(got[1]), _bits(was[1])), "a skipped lane's outputs changed"
        for i in (0, 2):
            assert np.array_equal(_bits(got[i]), _bits(ref[i])), "a live lane depends on the mask"
    env.close()


@pytest.mark.parametrize("H,S", [(1, 1), (1, 65), (12, 1), (12, 65)])
@pytest.mark.parametrize("surround", ["nan", "huge"])
def test_fenced_buffers(gpu_device, H, S, surround):
    """plan [N, H], mu_out [N], returns_out [N, S] and live [N] between fences (tests/fenced.py): nothing
    outside the payloads is written, every output element is, and the result does not depend on what surrounds the inputs."""
    import torch
    import fenced
    cfg = M.return_cfg(S, H, 0.8)
    env = _env(gpu_device, "three", True)
    out = []
    for arena in (fenced.Arena(gpu_device, surround), fenced.Plain(gpu_device)):
        plan = arena.inp("plan", torch.from_numpy(M.planted_plan(3, H)).to(gpu_device))
        live = arena.inp("live", torch.ones(3, dtype=torch.uint8, device=gpu_device))
        mu, ret = arena.out("mu_out", 3), arena.out("returns_out", (3, S), torch.float64)
        env.mpc_plan(cfg, plan, mu, live=live, returns_out=ret, seed=M.RETURN_SEED)
        torch.cuda.synchronize()
        arena.assert_clean(f"H={H} S={S} {surround}")
        out.append([t.cpu().numpy() for t in (plan, mu, ret)])
    for x, y in zip(*out):
        assert np.array_equal(_bits(x), _bits(y))
    env.close()


# ---- 5: capture ---------------------------------------------------------------------------------------------------------------
def test_captured_loop_equals_the_eager_loop(gpu_device):
    """Six (plan, step) iterations in one hipGraph: the noise keys (episode number, step-in-episode) come from the device, so the
    replay plans what the eager loop plans."""
    import torch
    from ddpg_trucktrailer_amd.mpc import MPCExpert
    cfg = M.return_cfg(65, 12, 0.8)
    high = float(M.HIGH)

    def iterate(env, ex, steer):
        for _ in range(6):
            mu = ex.act()
            torch.mul(mu, high, out=steer)
            env.step(steer, auto_reset=False)

    envs = [_env(gpu_device, "three", False) for _ in range(2)]
    experts = [MPCExpert(e, cfg, seed=9) for e in envs]
    steers = [torch.zeros(3, dtype=torch.float32, device=gpu_device) for _ in range(2)]
    iterate(envs[0], experts[0], steers[0])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        iterate(envs[1], experts[1], steers[1])
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    b0, b1 = _blob(envs[0]), _blob(envs[1])
    assert b0[1] == b1[1] and np.array_equal(b0[0], b1[0]), "the envs differ after the replay"
    for x, y in ((experts[0].plan, experts[1].plan), (experts[0].mu, experts[1].mu), (envs[0].obs, envs[1].obs)):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy()))
    assert int(envs[1].episode()["steps"][0]) == 6 and float(experts[1].plan.abs().max()) > 0
    for e in envs:
        e.close()
