"""CPU: the sampling MPC expert without a GPU (ddpg_trucktrailer_amd/mpc.py; include/ttenv.h: tt_env_mpc_plan; tests/mpc_ref.py).

* MPCConfig and check_mpc refuse what the C entry point refuses, and the buffers a planning call cannot take;
* tt_env_mpc_plan refuses bad calls before any HIP call, in its own name (handle and addresses are made up, in the style of
  tests/fake_args.py: a call that read one of them would crash here);
* mpc_ref's noise: mean, variance and lag-1 correlation within sampling error; sample 0 is the nominal;
* the conditions on the oracle that the GPU tests rely on: at most 1 % of a case's samples near a discrete reward edge; the lane
  whose samples all end on the first step; the closed loop of the collection test succeeds in all 8 lanes and ends within half
  of both goal thresholds;
* k_mpc_plan's two variants have no scratch and no vector spill."""
import ctypes as C
import math

import numpy as np
import pytest

import fake_args  # noqa: F401  (the style of the made-up addresses below: one spoiled argument at a time)
import mpc_ref as M


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------- MPCConfig / check_mpc
def test_config_defaults_and_tuple_round_trip():
    from ddpg_trucktrailer_amd.mpc import MPCConfig
    c = MPCConfig()
    assert c.as_tuple() == (40, 256, 0.3, 0.8, 10.0, 1.0, 20.0, 300.0)
    assert MPCConfig.from_tuple(c.as_tuple()) == c and hash(MPCConfig.from_tuple(c.as_tuple())) == hash(c)
    assert c != MPCConfig(horizon=39) and c != c.as_tuple()
    assert repr(c) == "MPCConfig(horizon=40, samples=256, sigma=0.3, rho=0.8, temperature=10.0, gamma=1.0, k_lat=20.0, k_yaw=300.0)"
    assert MPCConfig(horizon=1, samples=1, sigma=0, rho=0, k_lat=0, k_yaw=0).sigma == 0.0
    assert MPCConfig(horizon=64, samples=1024, rho=0.999, gamma=1e-3).samples == 1024


BAD = [("horizon", 0), ("horizon", 65), ("horizon", 4.0), ("horizon", True), ("samples", 0), ("samples", 1025), ("samples", "8"),
       ("sigma", -0.1), ("sigma", math.nan), ("sigma", math.inf), ("k_lat", -1.0), ("k_lat", math.inf), ("k_yaw", -1e-9),
       ("k_yaw", math.nan), ("rho", -0.1), ("rho", 1.0), ("rho", math.nan), ("temperature", 0.0), ("temperature", -1.0),
       ("temperature", math.inf), ("temperature", math.nan), ("gamma", 0.0), ("gamma", 1.0001), ("gamma", math.nan),
       ("sigma", None), ("rho", "0.5")]


@pytest.mark.parametrize("field,value", BAD)
def test_config_refuses(field, value):
    from ddpg_trucktrailer_amd.mpc import MPCConfig
    with pytest.raises(ValueError, match=rf"mpc: {field} = "):
        MPCConfig(**{field: value})


def test_check_mpc_names_every_refused_buffer():
    import torch
    from ddpg_trucktrailer_amd.mpc import MPCConfig, check_mpc
    cfg = MPCConfig(horizon=5, samples=9)
    assert check_mpc(cfg) is cfg and check_mpc(cfg, action_scale=0.78) is cfg
    with pytest.raises(ValueError, match="not an MPCConfig"):
        check_mpc((5, 9))
    for bad in (0.0, -1.0, math.nan, math.inf, "0.5"):
        with pytest.raises(ValueError, match="mpc: action_scale"):
            check_mpc(cfg, action_scale=bad)
    good = dict(plan=torch.zeros(3, 5), mu_out=torch.zeros(3), live=torch.ones(3, dtype=torch.uint8),
                returns_out=torch.zeros(3, 9, dtype=torch.float64))
    assert check_mpc(cfg, n_envs=3, **good) is cfg
    assert check_mpc(cfg, n_envs=3, plan=good["plan"], mu_out=good["mu_out"]) is cfg
    spoiled = [("plan", None), ("mu_out", None), ("plan", torch.zeros(3, 4)), ("plan", torch.zeros(5, 3).t()),
               ("plan", torch.zeros(3, 5, dtype=torch.float64)), ("plan", np.zeros((3, 5), np.float32)), ("mu_out", torch.zeros(4)),
               ("mu_out", torch.zeros(3, 1)), ("live", torch.ones(3, dtype=torch.bool)), ("live", torch.ones(2, dtype=torch.uint8)),
               ("returns_out", torch.zeros(3, 9)), ("returns_out", torch.zeros(3, 8, dtype=torch.float64))]
    for name, value in spoiled:
        with pytest.raises(ValueError, match=f"mpc: .*{name}"):
            check_mpc(cfg, n_envs=3, **dict(good, **{name: value}))
    with pytest.raises(ValueError, match="mpc: plan .* on cuda:0"):
        check_mpc(cfg, n_envs=3, device=torch.device("cuda:0"), **good)


# ------------------------------------------------------------------------------------------------- C ABI
FAKE = 0x10000      # never read: every call below is refused first


def _args(lib, **kw):
    a = dict(horizon=12, samples=65, sigma=0.3, rho=0.8, lambda_=10.0, gamma=1.0, k_lat=20.0, k_yaw=300.0, action_scale=0.785, seed=1)
    a.update(kw)
    return lib.TTMpcArgs(**a)


def _refused(lib, handle, args, plan=FAKE, mu=FAKE):
    dll = lib.load()
    p = lambda x: None if x is None else C.c_void_p(x)
    rc = dll.tt_env_mpc_plan(p(handle), None if args is None else C.byref(args), p(plan), p(mu), None, None, None)
    msg = dll.tt_last_error(None).decode()
    assert rc == lib.TT_EINVAL and msg.startswith("tt_env_mpc_plan:"), (rc, msg)
    return msg


def test_entry_point_is_exported_and_the_version_stays_three(lib):
    assert "tt_env_mpc_plan" in lib.EXPORTS and hasattr(lib.load(), "tt_env_mpc_plan")
    assert lib.load().tt_version() == 3
    assert C.sizeof(lib.TTMpcArgs) == 48 and lib.TTMpcArgs.seed.offset == 40


def test_entry_point_refuses_before_it_reads_the_handle(lib):
    assert "NULL handle" in _refused(lib, None, _args(lib))
    assert "args, plan and mu_out" in _refused(lib, FAKE, None)
    assert "args, plan and mu_out" in _refused(lib, FAKE, _args(lib), plan=None)
    assert "args, plan and mu_out" in _refused(lib, FAKE, _args(lib), mu=None)
    for word, spoil in [("horizon", dict(horizon=0)), ("horizon", dict(horizon=65)), ("horizon", dict(horizon=-3)),
                        ("samples", dict(samples=0)), ("samples", dict(samples=1025)),
                        ("sigma", dict(sigma=-0.1)), ("sigma", dict(sigma=math.nan)), ("sigma", dict(sigma=math.inf)),
                        ("k_lat", dict(k_lat=-1.0)), ("k_lat", dict(k_lat=math.nan)), ("k_yaw", dict(k_yaw=-1.0)),
                        ("k_yaw", dict(k_yaw=math.inf)), ("rho", dict(rho=-0.01)), ("rho", dict(rho=1.0)), ("rho", dict(rho=math.nan)),
                        ("lambda", dict(lambda_=0.0)), ("lambda", dict(lambda_=-2.0)), ("lambda", dict(lambda_=math.inf)),
                        ("lambda", dict(lambda_=math.nan)), ("gamma", dict(gamma=0.0)), ("gamma", dict(gamma=1.5)),
                        ("gamma", dict(gamma=math.nan)), ("action_scale", dict(action_scale=0.0)),
                        ("action_scale", dict(action_scale=-0.5)), ("action_scale", dict(action_scale=math.nan)),
                        ("action_scale", dict(action_scale=math.inf))]:
        assert word in _refused(lib, FAKE, _args(lib, **spoil)), (word, spoil)


# ------------------------------------------------------------------------------------------------- the noise
def test_noise_statistics():
    """S * H = 65536 normals: |mean| <= 4 / sqrt(n), |var - 1| <= 4 sqrt(2 / n); the AR(1) eps has variance sigma^2 at every t and
    lag-1 correlation rho within 4 / sqrt(S H); sample 0 is zero."""
    S, H, sigma, rho = 1024, 64, 0.3, 0.8
    z = M.noise_normal(11, 2, 3, 17, S, H)
    n = z.size
    assert np.isfinite(z).all() and abs(z.mean()) <= 4 / np.sqrt(n) and abs(z.var() - 1) <= 4 * np.sqrt(2 / n)
    assert abs(np.corrcoef(z[:, :-1].ravel(), z[:, 1:].ravel())[0, 1]) <= 4 / np.sqrt(n)
    eps = M.noise_eps(z, sigma, rho)
    assert np.all(eps[0] == 0)
    e = eps[1:]
    for t in (0, 1, H - 1):
        assert abs(e[:, t].var() / sigma ** 2 - 1) <= 4 * np.sqrt(2 / (S - 1)), t
    r = np.corrcoef(e[:, :-1].ravel(), e[:, 1:].ravel())[0, 1]
    assert abs(r - rho) <= 4 / np.sqrt(e[:, 1:].size), r
    assert abs(np.corrcoef(M.noise_eps(z, sigma, 0.0)[1:, :-1].ravel(), M.noise_eps(z, sigma, 0.0)[1:, 1:].ravel())[0, 1]) <= 4 / np.sqrt(n)


def test_noise_keys():
    base = M.noise_normal(11, 2, 3, 17, 8, 4)
    assert np.array_equal(base, M.noise_normal(11, 2, 3, 17, 8, 4))
    assert np.array_equal(base[:5, :3], M.noise_normal(11, 2, 3, 17, 5, 3)), "z[s, t] does not depend on S or H"
    for other in ((12, 2, 3, 17), (11, 1, 3, 17), (11, 2, 4, 17), (11, 2, 3, 18), (11 + 2 ** 32, 2, 3, 17)):
        assert np.all(base != M.noise_normal(*other, 8, 4)), other


def test_samples_clip_and_round():
    from ddpg_trucktrailer_amd.mpc import MPCConfig
    cfg = MPCConfig(horizon=6, samples=200, sigma=0.6)
    plan = np.array([0.9, -0.9, 0.0, 0.5, -1.0, 1.0], np.float32)
    u = M.samples(cfg, 1, 0, 0, 5, plan)
    assert u.dtype == np.float32 and u.shape == (200, 6) and np.array_equal(u[0], plan)
    assert u.min() == -1.0 and u.max() == 1.0 and (np.abs(u) == 1.0).mean() > 0.1


def test_update_definition():
    u = np.array([[0.0, 0.5, 1.0], [1.0, -1.0, 0.25], [-1.0, 0.0, 0.0]], np.float32)
    mu, plan = M.update(np.array([0.0, 0.0, -np.inf]), u, 10.0, np.zeros(3, np.float32))
    assert mu == np.float32(0.5) and np.array_equal(plan, np.array([-0.25, 0.625, 0.625], np.float32))
    mu, plan = M.update(np.array([np.nan, np.inf, -np.inf]), u, 10.0, np.array([0.1, 0.2, 0.3], np.float32))
    assert mu == np.float32(0.1) and np.array_equal(plan, np.array([0.2, 0.3, 0.3], np.float32))
    mu, plan = M.update(np.array([5.0, 1000.0, 7.0]), u, 1e-3, np.zeros(3, np.float32))
    assert mu == 1.0 and np.array_equal(plan, np.array([-1.0, 0.25, 0.25], np.float32))


# ------------------------------------------------------------------------------------------------- conditions on the oracle
@pytest.mark.parametrize("S,H,rho", M.RETURN_CASES)
def test_return_cases_stay_clear_of_reward_edges(S, H, rho):
    """A sample is near an edge if the oracle's return moves by more than 0.5 (the smallest discrete reward event is 2) when every
    action is nudged by +-1e-6; at most 1 % of a case's samples may be, and tests/test_gpu_mpc.py leaves those out."""
    events = 0
    for which in ("three", "one"):
        for warm in (False, True):
            for u, G, edge in M.return_case(S, H, rho, which, warm):
                assert np.isfinite(G).all() and edge.mean() <= M.MAX_NEAR_EDGE, (which, warm, edge.sum())
                events += 1
    assert events == 8


def test_the_lanes_are_what_the_gpu_tests_say():
    """Within 5 m of the goal: the staged bonus is paid inside the horizon; the edge lane leaves the map inside it; the warm
    lanes are WARM steps into their episodes; every sample of the first-step lane is done after one step."""
    from oracle import c_oracle
    ora = M.oracle_lanes("three", False)
    _, _, done, info = ora.step(np.zeros(3, np.float32))
    assert info[1, c_oracle.INFO_KEYS.index("staged_success")] >= 10.0 and not done.any()
    for _ in range(4):
        _, _, done, _ = ora.step(np.zeros(3, np.float32))
    assert ora.flags()[2] & c_oracle.F_OUT_OF_MAP and done[2]
    assert [e.steps for e in M.oracle_lanes("three", True).envs] == [M.WARM] * 3
    one = c_oracle.COracle(1)
    one.place(M.FIRST_STEP_START)
    cfg = M.return_cfg(65, 5, 0.8)
    u = M.samples(cfg, M.RETURN_SEED, 0, 0, 0, np.zeros(5, np.float32))
    for s in range(65):
        probe = c_oracle.COracle(1)
        probe.place(M.FIRST_STEP_START)
        _, _, done, _ = probe.step(u[s, :1] * M.HIGH)
        assert done[0], s


def test_collection_closed_loop_on_the_oracle():
    """H = 16, S = 128, the other defaults: all 8 lanes of mpc_ref.COLLECT_START succeed on the oracle and end within half of both
    goal thresholds (0.25 m, 7.5 degrees)."""
    from oracle import c_oracle
    p = c_oracle.COracle(1).params
    out = M.collect_closed_loop()
    assert len(out) == 8
    d = np.hypot(M.COLLECT_START[:, 0] - M.DEFAULT_GOAL[0], M.COLLECT_START[:, 1] - M.DEFAULT_GOAL[1])
    assert d.min() >= 8.0 and d.max() <= 12.0 and np.abs(np.degrees(M.COLLECT_START[:, 2]) - 90.0).max() <= 20.0
    for i, r in enumerate(out):
        print(i, r["success"], r["flags"], len(r["mu"]), round(r["pos_err"], 3), round(float(np.degrees(r["ori_err"])), 2))
        assert r["success"] and r["done"], (i, r["flags"])
        assert r["pos_err"] <= 0.5 * p.position_threshold and r["ori_err"] <= 0.5 * p.orientation_threshold, (i, r["pos_err"], r["ori_err"])
        assert np.all(np.abs(r["mu"]) <= 1.0)


# ------------------------------------------------------------------------------------------------- resources
def test_planning_kernels_have_no_scratch_and_no_vector_spill(lib):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    plan = kr.find(kr.kernels(), "10k_mpc_planILb")
    assert len(plan) == 2, sorted(plan)
    for n, v in plan.items():
        assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["max_threads"] == 256, (n, v)
        assert kr.waves_per_simd(v["vgpr"]) >= 2, (n, v)
