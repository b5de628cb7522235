"""CPU: expert lanes of the vector loop without a GPU (ddpg_trucktrailer_amd/mpc.py: ExpertLanes, check_expert_lanes; include/ttenv.h:
tt_env_mpc_act_ring, tt_mlp_forward_save_demo_lanes, tt_mlp_actor_tail_demo_lanes).

* ExpertLanes and check_expert_lanes refuse every malformed option and every combination a loop cannot run, naming `expert`;
* DDPGRollout, VectorStepper, PopulationRollout, PopulationLearner and FusedLearner refuse what the issue lists;
* the three new entry points refuse bad calls in their own names before any HIP call (made-up addresses: tests/fake_args.py);
* tt_demo_loss keeps its 48 bytes, tt_version stays 3;
* the host's mask rule; the new kernels' resources (no scratch, no vector spill, two waves per SIMD) and the planner's two
  existing instantiations beside them."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import fake_args as F
from cpu_env import CpuEnv as _CpuEnv


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------- ExpertLanes / check_expert_lanes
def test_expert_lanes_holds_its_numbers_and_compares_by_value():
    from ddpg_trucktrailer_amd.mpc import ExpertLanes, MPCConfig, check_expert_lanes
    e = ExpertLanes(3, mpc=MPCConfig(horizon=5, samples=65), seed=7)
    assert (e.lanes, e.mpc.horizon, e.mpc.samples, e.seed) == (3, 5, 65, 7)
    assert e == ExpertLanes(3, MPCConfig(horizon=5, samples=65), 7) and hash(e) == hash(ExpertLanes.from_tuple(e.as_tuple()))
    assert e != ExpertLanes(4, MPCConfig(horizon=5, samples=65), 7) and e != ExpertLanes(3, MPCConfig(horizon=6, samples=65), 7)
    assert e != ExpertLanes(3, MPCConfig(horizon=5, samples=65), 8)
    assert ExpertLanes(1).mpc == MPCConfig() and ExpertLanes(1).seed == 0
    assert check_expert_lanes(e) is e and check_expert_lanes(e, n_envs=3, ring_mode=True) is e
    assert "lanes=3" in repr(e)


@pytest.mark.parametrize("kw", [dict(lanes=0), dict(lanes=-2), dict(lanes=2.0), dict(lanes=True), dict(lanes="3"), dict(lanes=None),
                                dict(mpc=(5, 65)), dict(mpc="mpc"), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5)])
def test_expert_lanes_refuses(kw):
    from ddpg_trucktrailer_amd.mpc import ExpertLanes
    with pytest.raises(ValueError, match="expert"):
        ExpertLanes(**dict(dict(lanes=2), **kw))


def test_a_spoiled_mpc_config_is_refused_by_its_own_check():
    from ddpg_trucktrailer_amd.mpc import ExpertLanes, MPCConfig, check_expert_lanes
    e = ExpertLanes(2, MPCConfig(horizon=5))
    e.mpc.horizon = 65                      # (spoiled after construction: the pure function looks again)
    with pytest.raises(ValueError, match="mpc: horizon"):
        check_expert_lanes(e)


@pytest.mark.parametrize("kw, word", [(dict(n_envs=2), "lanes = 3 is outside"), (dict(ring_mode=False), "ring mode"),
                                      (dict(population=True), "population"), (dict(data_parallel=True), "data-parallel"),
                                      (dict(force_dp=True), "TT_FORCE_DP")])
def test_check_expert_lanes_names_every_refused_combination(kw, word):
    from ddpg_trucktrailer_amd.mpc import ExpertLanes, check_expert_lanes
    with pytest.raises(ValueError, match="expert") as exc:
        check_expert_lanes(ExpertLanes(3), **kw)
    assert word in str(exc.value)


def test_check_expert_lanes_refuses_what_is_not_an_expert_lanes():
    from ddpg_trucktrailer_amd.mpc import check_expert_lanes
    for bad in (3, (3, None, 0), "lanes"):
        with pytest.raises(ValueError, match="expert = .* is not an ExpertLanes"):
            check_expert_lanes(bad)


# ------------------------------------------------------------------------------------------------- the loops
def test_steppers_and_populations_refuse_expert_lanes(monkeypatch):
    from ddpg_trucktrailer_amd.mpc import ExpertLanes
    from ddpg_trucktrailer_amd.population import PopulationLearner, PopulationRollout
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.stepper import VectorStepper
    e = ExpertLanes(2)
    with pytest.raises(ValueError, match="expert.*ring mode"):
        VectorStepper(_CpuEnv(), batch_size=4, replay_slots=8, expert=e)            # a CPU device: not in ring mode
    with pytest.raises(ValueError, match="expert.*ring mode"):
        DDPGRollout(_CpuEnv(), batch_size=4, replay_slots=8, expert=e, use_graph=False)
    with pytest.raises(ValueError, match="expert.*lanes = 5"):
        DDPGRollout(_CpuEnv(), batch_size=4, replay_slots=8, expert=ExpertLanes(5))
    with pytest.raises(ValueError, match="expert = "):
        DDPGRollout(_CpuEnv(), batch_size=4, replay_slots=8, expert=2)
    with pytest.raises(ValueError, match="expert.*data-parallel"):
        DDPGRollout(_CpuEnv(), batch_size=4, replay_slots=8, expert=e, data_parallel=True)
    with pytest.raises(ValueError, match="expert.*data-parallel"):
        DDPGRollout(_CpuEnv(), batch_size=4, replay_slots=8, expert=e, world_size=2)
    with pytest.raises(ValueError, match="expert.*data-parallel"):
        DDPGRollout(_CpuEnv(), batch_size=4, replay_slots=8, expert=e, dp_exchange="p2p")
    monkeypatch.setenv("TT_FORCE_DP", "1")
    with pytest.raises(ValueError, match="expert.*TT_FORCE_DP"):
        DDPGRollout(_CpuEnv(), batch_size=4, replay_slots=8, expert=e)
    monkeypatch.delenv("TT_FORCE_DP")
    with pytest.raises(ValueError, match="expert.*population"):
        PopulationRollout(64, [1, 2], expert=e)
    with pytest.raises(ValueError, match="expert.*population"):
        PopulationLearner([], 4, expert=e)


def test_demo_loss_with_n_step_stays_refused_with_expert_lanes():
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    from ddpg_trucktrailer_amd.mpc import ExpertLanes
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    with pytest.raises(ValueError, match="demo_loss with n_step = 3"):
        DDPGRollout(_CpuEnv(), batch_size=4, replay_slots=16, expert=ExpertLanes(2), demo_loss=DemoLoss(1.0), n_step=3)


def test_a_stepper_without_expert_lanes_refuses_a_checkpoint_with_them():
    from ddpg_trucktrailer_amd.mpc import ExpertLanes
    from ddpg_trucktrailer_amd.stepper import VectorStepper
    st = VectorStepper(_CpuEnv(), batch_size=4, replay_slots=8)
    assert st.expert is None and st.graph_key()[-1] is None and "expert" not in st.acting_state()
    st.check_expert_state({})
    with pytest.raises(ValueError, match="expert = \\(2, "):
        st.check_expert_state({"expert": list(ExpertLanes(2).as_tuple())})


# ------------------------------------------------------------------------------------------------- the mask rule
def test_the_host_mask_rule():
    from ddpg_trucktrailer_amd.mpc import expert_mask
    idx = torch.tensor([[-1, 0], [-1, 9], [0, 0], [5, 3], [5, 4], [7, 100]], dtype=torch.int32)
    for M in (0, 1, 4, 5, 101):
        want = (idx[:, 0] < 0) | (idx[:, 1] < M)
        assert torch.equal(expert_mask(idx, M), want)
    assert expert_mask(idx, 0).tolist() == [True, True, False, False, False, False]
    assert expert_mask(idx, 4).tolist() == [True, True, True, True, False, False]


def test_the_loops_torch_path_uses_the_mask_rule():
    """DDPGRollout._demo_rows: what Agent.learn_batch(demo_rows=) gets of a draw's index buffer."""
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    from ddpg_trucktrailer_amd.mpc import ExpertLanes
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    idx = torch.tensor([[-1, 2], [3, 0], [3, 1], [3, 2]], dtype=torch.int64)
    loop = DDPGRollout.__new__(DDPGRollout)
    loop.demo_loss, loop.expert = DemoLoss(1.0), ExpertLanes(2)
    assert loop._demo_rows(idx)["demo_rows"].tolist() == [True, True, True, False]
    loop.expert = None
    assert loop._demo_rows(idx)["demo_rows"].tolist() == [True, False, False, False]
    loop.demo_loss = None
    assert loop._demo_rows(idx) == {}


# ------------------------------------------------------------------------------------------------- C ABI: tt_env_mpc_act_ring
FAKE = 0x10000      # never read: every call below is refused first


def _mpc_args(L, **kw):
    a = dict(horizon=12, samples=65, sigma=0.3, rho=0.8, lambda_=10.0, gamma=1.0, k_lat=20.0, k_yaw=300.0, action_scale=0.785, seed=1)
    a.update(kw)
    return L.TTMpcArgs(**a)


def _act_ring_refused(L, handle=FAKE, args="good", plan=FAKE, lanes=3, ring="good", high=0.785, act_scaled=FAKE, **view):
    dll = L.load()
    p = lambda x: None if x is None else C.c_void_p(x)
    if args == "good":
        args = _mpc_args(L)
    if ring == "good":
        v = dict(cursor=FAKE, obs=FAKE, act=FAKE, rew=FAKE, done=FAKE, n_envs=8, slots=8)
        v.update(view)
        ring = L.TTRingView(**v)
    rc = dll.tt_env_mpc_act_ring(p(handle), None if args is None else C.byref(args), p(plan), lanes,
                                 None if ring is None else C.byref(ring), high, p(act_scaled), None)
    msg = dll.tt_last_error(None).decode()
    assert rc == L.TT_EINVAL and msg.startswith("tt_env_mpc_act_ring:"), (rc, msg)
    return msg


def test_act_ring_is_exported_and_the_abi_keeps_its_sizes(lib):
    L = lib
    for name in ("tt_env_mpc_act_ring", "tt_mlp_forward_save_demo_lanes", "tt_mlp_actor_tail_demo_lanes"):
        assert name in L.EXPORTS and hasattr(L.load(), name)
    assert L.load().tt_version() == 3
    assert C.sizeof(L.TTDemoLoss) == 48 and C.sizeof(L.TTMpcArgs) == 48


def test_act_ring_refuses_before_it_reads_the_handle(lib):
    L = lib
    assert "NULL handle" in _act_ring_refused(L, handle=None)
    for kw in (dict(args=None), dict(plan=None), dict(ring=None), dict(act_scaled=None)):
        assert "args, plan, ring and act_scaled" in _act_ring_refused(L, **kw), kw
    assert "ring->cursor" in _act_ring_refused(L, cursor=None)
    assert "ring->cursor and ring->act" in _act_ring_refused(L, act=None)
    assert "slots" in _act_ring_refused(L, slots=0)
    for lanes in (0, -1, 9, 2 ** 31 - 1):
        assert "lanes" in _act_ring_refused(L, lanes=lanes), lanes
    assert "lanes" not in _act_ring_refused(L, lanes=8, high=0.0)          # lanes = n_envs is allowed
    for high in (0.0, -0.5, math.nan, math.inf):
        assert "high" in _act_ring_refused(L, high=high), high
    for word, spoil in [("horizon", dict(horizon=0)), ("horizon", dict(horizon=65)), ("samples", dict(samples=0)),
                        ("samples", dict(samples=1025)), ("sigma", dict(sigma=-0.1)), ("sigma", dict(sigma=math.nan)),
                        ("k_lat", dict(k_lat=-1.0)), ("k_yaw", dict(k_yaw=math.inf)), ("rho", dict(rho=1.0)),
                        ("rho", dict(rho=math.nan)), ("lambda", dict(lambda_=0.0)), ("lambda", dict(lambda_=math.nan)),
                        ("gamma", dict(gamma=0.0)), ("gamma", dict(gamma=1.5)), ("action_scale", dict(action_scale=0.0)),
                        ("action_scale", dict(action_scale=math.inf))]:
        assert word in _act_ring_refused(L, args=_mpc_args(L, **spoil)), (word, spoil)


# ------------------------------------------------------------------------------------------------- C ABI: the _lanes entry points
_LANES = dict(fwd="tt_mlp_forward_save_demo_lanes", tail_="tt_mlp_actor_tail_demo_lanes")


class FakeLanes(F.Fake):
    """fake_args.Fake's demonstration form through the _lanes entry points: the same arguments, then expert_lanes, then the stream."""

    def __init__(self, L, B, expert_lanes=4):
        super().__init__(L, B, "demo")
        self.expert_lanes = expert_lanes

    def _call(self, entry, args):
        if entry == "tail_":
            args.append(C.byref(self.shape) if self.with_shape else None)
        args.append(C.byref(self.demo) if self.with_demo else None)
        return getattr(self.L.load(), _LANES[entry])(*args, self.expert_lanes, None)


_set = F.set_field
_COMMON = [("demo is NULL", None, False), ("expert_lanes = -1", lambda f: setattr(f, "expert_lanes", -1), True),
           ("expert_lanes = -2147483648", lambda f: setattr(f, "expert_lanes", -2 ** 31), True),
           ("demo->k", _set("demo", "k", -0.5), True), ("demo->k", _set("demo", "k", float("nan")), True),
           ("NULL", _set("demo", "a", None), True), ("NULL", _set("demo", "idx", None), True), ("NULL", _set("demo", "dq_eff", None), True),
           ("NULL", _set("demo", "code", None), True), ("demo->q is NULL", _set("demo", "q", None), True),
           ("dq_eff is dq_da", lambda f: setattr(f.demo, "dq_eff", f.dq_da), True),
           ("dq_da is NULL", lambda f: setattr(f, "dq_da", None), True)]
_FWD = [("actor", lambda f: setattr(f, "fwd_critic", 0), True), ("n = -1", lambda f: setattr(f, "B", -1), True),
        ("obs", lambda f: setattr(f, "obs", None), True), ("action", lambda f: setattr(f, "mu", None), True),
        ("out", lambda f: setattr(f, "q_pi", None), True), ("weights", _set("critic", "wa", None), True)]
_TAIL = [("n = 0", lambda f: setattr(f, "B", 0), True), ("n = 1025", lambda f: setattr(f, "B", 1025), True),
         ("obs", lambda f: setattr(f, "obs", None), True), ("mu", lambda f: setattr(f, "mu", None), True),
         ("q_out", lambda f: setattr(f, "q_pi", None), True), ("critic", _set("critic", "wa", None), True),
         ("saved", _set("saved_a", "h1", None), True), ("workspace", _set("ws_a", "dy1", None), True),
         ("grads", _set("grads", "w1", None), True), ("count = 0", lambda f: setattr(f, "count", 0), True),
         ("tail_words", lambda f: setattr(f, "tail", None), True), ("huber_delta", _set("shape", "huber_delta", -1.0), True)]
_REFUSALS = [(e, *r) for e, rs in (("fwd", _COMMON + _FWD), ("tail_", _COMMON + _TAIL)) for r in rs]


@pytest.mark.parametrize("entry, word, spoil, with_demo", _REFUSALS,
                         ids=[f"{e}-{i}-{w.replace(' ', '_').replace('>', '')}" for i, (e, w, _, _) in enumerate(_REFUSALS)])
def test_lanes_entry_points_check_their_arguments_before_any_hip_call(lib, entry, word, spoil, with_demo):
    L = lib
    f = FakeLanes(L, 256)
    if spoil is not None:
        spoil(f)
    f.with_demo = with_demo
    rc, msg = getattr(f, entry)(), f.last_error()
    assert rc == L.TT_EINVAL, (rc, msg)
    assert msg.startswith(_LANES[entry] + ":") and word in msg, msg


def test_fused_learner_checks_expert_lanes_before_it_touches_anything():
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    for bad in (-1, 2.0, True, "4"):
        with pytest.raises(ValueError, match="expert_lanes"):
            FusedLearner(None, 4, demo_loss=DemoLoss(1.0), expert_lanes=bad)
    with pytest.raises(ValueError, match="expert_lanes = 3 without demo_loss"):
        FusedLearner(None, 4, expert_lanes=3)


# ------------------------------------------------------------------------------------------------- resources
def test_the_ring_form_of_the_planner_has_no_scratch_no_vector_spill_and_two_waves(lib):
    """k_mpc_act_ring (the planner's body with the ring epilogue), per-env goals or not: the budget of k_mpc_plan's own two
    instantiations, which stay two."""
    from ddpg_trucktrailer_amd import kernel_resources as kr
    ks = kr.kernels()
    ring, plan = kr.find(ks, "14k_mpc_act_ringILb"), kr.find(ks, "10k_mpc_planILb")
    assert len(ring) == 2 and len(plan) == 2, (sorted(ring), sorted(plan))
    for n, v in {**ring, **plan}.items():
        assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["max_threads"] == 256 and v["lds"] == 0, (n, v)
        assert kr.waves_per_simd(v["vgpr"]) >= 2, (n, v)
