"""CPU: expert labels of the vector loop without a GPU (ddpg_trucktrailer_amd/mpc.py: ExpertLabels, check_expert_labels, label_mask;
include/ttenv.h: tt_env_mpc_label_ring, tt_demo_labels, tt_mlp_forward_save_demo_labels, tt_mlp_actor_tail_demo_labels; DESIGN.md
section 30).

* ExpertLabels and check_expert_labels refuse every malformed option and every combination a loop cannot run, naming `labels`;
* DDPGRollout, VectorStepper, FusedLearner and the ring refuse what the issue lists; the unchanged refusals stay;
* the three new entry points refuse bad calls in their own names before any HIP call (made-up addresses: tests/fake_args.py);
* tt_demo_loss keeps its 48 bytes, tt_demo_labels has 24, tt_version stays 3;
* label_mask against a hand-written table; tests/label_ref.py against learn_ref / demo_ref where they must agree;
* Agent.learn_batch(label_rows=, labels=) in f32 against tests/label_ref.py at B = 33;
* k_mpc_label_ring's resources (no scratch, no vector spill, 256 threads, two waves per SIMD) beside the planner's two k_mpc_plan and
  two k_mpc_act_ring instantiations, which stay two each."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import demo_ref as D
import fake_args as F
import label_ref as LR
import learn_ref as R
from cpu_env import CpuEnv as _CpuEnv

_CASE = D.F64_CASES[1]          # B = 33, fresh state


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------- ExpertLabels / check_expert_labels
def test_expert_labels_holds_its_numbers_and_compares_by_value():
    from ddpg_trucktrailer_amd.mpc import ExpertLabels, ExpertLanes, MPCConfig, check_expert_labels
    cfg = MPCConfig(horizon=5, samples=65)
    e = ExpertLabels(3, mpc=cfg, seed=7)
    assert (e.lanes, e.mpc.horizon, e.mpc.samples, e.seed) == (3, 5, 65, 7)
    assert e.as_tuple() == (3, cfg.as_tuple(), 7)
    assert e == ExpertLabels(3, MPCConfig(horizon=5, samples=65), 7) and hash(e) == hash(ExpertLabels.from_tuple(e.as_tuple()))
    assert e != ExpertLabels(4, cfg, 7) and e != ExpertLabels(3, MPCConfig(horizon=6, samples=65), 7) and e != ExpertLabels(3, cfg, 8)
    assert e != ExpertLanes(3, cfg, 7)
    assert ExpertLabels(1).mpc == MPCConfig() and ExpertLabels(1).seed == 0
    assert check_expert_labels(e) is e
    assert check_expert_labels(e, expert=ExpertLanes(2, cfg, 7), n_envs=5, ring_mode=True, demo_loss=object()) is e
    assert "lanes=3" in repr(e)


@pytest.mark.parametrize("kw", [dict(lanes=0), dict(lanes=-2), dict(lanes=2.0), dict(lanes=True), dict(lanes="3"), dict(lanes=None),
                                dict(mpc=(5, 65)), dict(mpc="mpc"), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5)])
def test_expert_labels_refuses(kw):
    from ddpg_trucktrailer_amd.mpc import ExpertLabels
    with pytest.raises(ValueError, match="labels"):
        ExpertLabels(**dict(dict(lanes=2), **kw))


def test_a_spoiled_mpc_config_is_refused_by_its_own_check():
    from ddpg_trucktrailer_amd.mpc import ExpertLabels, MPCConfig, check_expert_labels
    e = ExpertLabels(2, MPCConfig(horizon=5))
    e.mpc.horizon = 65                      # (spoiled after construction: the pure function looks again)
    with pytest.raises(ValueError, match="mpc: horizon"):
        check_expert_labels(e)


def _expert(**kw):
    from ddpg_trucktrailer_amd.mpc import ExpertLanes, MPCConfig
    return ExpertLanes(kw.pop("lanes", 2), MPCConfig(**kw.pop("cfg", {})), seed=kw.pop("seed", 0))


@pytest.mark.parametrize("kw, word", [(dict(n_envs=2), "3 labelled lanes are more than the env's 2"),
                                      (dict(n_envs=4, expert="two"), "2 expert lanes + 3 labelled lanes"),
                                      (dict(expert="other-mpc"), "one launch plans for both"),
                                      (dict(expert="other-seed"), "seed = 0 is not the expert lanes' 4"),
                                      (dict(ring_mode=False), "ring mode"), (dict(population=True), "population"),
                                      (dict(data_parallel=True), "data-parallel"), (dict(force_dp=True), "TT_FORCE_DP"),
                                      (dict(demo_loss=None), "without demo_loss")])
def test_check_expert_labels_names_every_refused_combination(kw, word):
    from ddpg_trucktrailer_amd.mpc import ExpertLabels, check_expert_labels
    experts = {"two": _expert(), "other-mpc": _expert(cfg=dict(horizon=7)), "other-seed": _expert(seed=4)}
    if "expert" in kw:
        kw = dict(kw, expert=experts[kw["expert"]])
    with pytest.raises(ValueError, match="labels") as exc:
        check_expert_labels(ExpertLabels(3), **kw)
    assert word in str(exc.value)


def test_check_expert_labels_allows_what_fits_and_refuses_what_is_not_an_expert_labels():
    from ddpg_trucktrailer_amd.mpc import ExpertLabels, check_expert_labels
    check_expert_labels(ExpertLabels(3), expert=_expert(), n_envs=5)            # M + L = N
    check_expert_labels(ExpertLabels(8), n_envs=8)
    for bad in (3, (3, None, 0), "lanes", _expert()):
        with pytest.raises(ValueError, match="labels = .* is not an ExpertLabels"):
            check_expert_labels(bad)
    with pytest.raises(ValueError, match="expert = 2 is not an ExpertLanes"):
        check_expert_labels(ExpertLabels(3), expert=2)


# ------------------------------------------------------------------------------------------------- the loop, the stepper, the learner
def test_the_loop_and_the_stepper_refuse_expert_labels(monkeypatch):
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    from ddpg_trucktrailer_amd.mpc import ExpertLabels
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.stepper import VectorStepper
    e, bc = ExpertLabels(2), DemoLoss(1.0)
    kw = dict(batch_size=4, replay_slots=8)
    with pytest.raises(ValueError, match="labels.*ring mode"):
        VectorStepper(_CpuEnv(), labels=e, **kw)                               # a CPU device: not in ring mode
    with pytest.raises(ValueError, match="labels.*ring mode"):
        DDPGRollout(_CpuEnv(), labels=e, demo_loss=bc, use_graph=False, **kw)
    with pytest.raises(ValueError, match="labels.*without demo_loss"):
        DDPGRollout(_CpuEnv(), labels=e, **kw)
    with pytest.raises(ValueError, match="labels.*5 labelled lanes are more than the env's 4"):
        DDPGRollout(_CpuEnv(), labels=ExpertLabels(5), demo_loss=bc, **kw)
    with pytest.raises(ValueError, match="labels.*2 expert lanes \\+ 3 labelled lanes"):
        DDPGRollout(_CpuEnv(), labels=ExpertLabels(3), expert=_expert(), demo_loss=bc, **kw)
    with pytest.raises(ValueError, match="labels.*one launch plans for both"):
        DDPGRollout(_CpuEnv(), labels=e, expert=_expert(seed=3), demo_loss=bc, **kw)
    with pytest.raises(ValueError, match="labels = "):
        DDPGRollout(_CpuEnv(), labels=2, demo_loss=bc, **kw)
    with pytest.raises(ValueError, match="labels.*data-parallel"):
        DDPGRollout(_CpuEnv(), labels=e, demo_loss=bc, data_parallel=True, **kw)
    with pytest.raises(ValueError, match="labels.*data-parallel"):
        DDPGRollout(_CpuEnv(), labels=e, demo_loss=bc, world_size=2, **kw)
    with pytest.raises(ValueError, match="labels.*data-parallel"):
        DDPGRollout(_CpuEnv(), labels=e, demo_loss=bc, dp_exchange="p2p", **kw)
    monkeypatch.setenv("TT_FORCE_DP", "1")
    with pytest.raises(ValueError, match="labels.*TT_FORCE_DP"):
        DDPGRollout(_CpuEnv(), labels=e, demo_loss=bc, **kw)
    monkeypatch.delenv("TT_FORCE_DP")


def test_the_unchanged_refusals_stay_with_expert_labels():
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    from ddpg_trucktrailer_amd.mpc import ExpertLabels
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.td3 import TD3Config
    with pytest.raises(ValueError, match="demo_loss with n_step = 3"):
        DDPGRollout(_CpuEnv(), batch_size=4, replay_slots=16, labels=ExpertLabels(2), demo_loss=DemoLoss(1.0), n_step=3)
    with pytest.raises(ValueError, match="demo_loss"):
        DDPGRollout(_CpuEnv(), batch_size=4, replay_slots=16, labels=ExpertLabels(2), demo_loss=DemoLoss(1.0), td3=TD3Config())


def test_a_stepper_without_labels_keeps_its_key_and_state_and_refuses_a_checkpoint_with_them():
    from ddpg_trucktrailer_amd.mpc import ExpertLabels
    from ddpg_trucktrailer_amd.stepper import VectorStepper
    st = VectorStepper(_CpuEnv(), batch_size=4, replay_slots=8)
    assert st.labels is None and len(st.graph_key()) == 4 and st.ring.label is None
    sd = st.acting_state()
    assert "labels" not in sd and "expert_plan" not in sd and "label" not in sd["ring"]
    st.check_expert_state({})
    with pytest.raises(ValueError, match="labels = \\(2, "):
        st.check_expert_state({"labels": list(ExpertLabels(2).as_tuple())})


def test_the_ring_carries_the_label_array_only_when_it_is_enabled():
    from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing
    plain, lab = TrajectoryRing(4, 8, 23, "cpu"), TrajectoryRing(4, 8, 23, "cpu")
    label = lab.enable_labels()
    assert lab.enable_labels() is label and tuple(label.shape) == (8, 4) and label.dtype == torch.float32 and not label.any()
    assert set(lab.state_dict()) - set(plain.state_dict()) == {"label"} and "label" not in lab.state_dict(with_replay=False)
    label.copy_(torch.arange(32.0).view(8, 4))
    other = TrajectoryRing(4, 8, 23, "cpu")
    other.enable_labels()
    other.load_state_dict(lab.state_dict())
    assert torch.equal(other.label, label)
    before = plain.act.clone()
    with pytest.raises(ValueError, match="label array"):
        plain.load_state_dict(lab.state_dict())
    with pytest.raises(ValueError, match="label array"):
        other.load_state_dict(plain.state_dict())
    assert torch.equal(plain.act, before) and torch.equal(other.label, label)


def test_fused_learner_checks_labels_before_it_touches_anything():
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    for bad in ((2,), (-1, 3), (2, 0), (2.0, 3), (2, True), "23", 5, (1, 2, 3, 4)):
        with pytest.raises(ValueError, match="labels = "):
            FusedLearner(None, 4, demo_loss=DemoLoss(1.0), labels=bad)
    with pytest.raises(ValueError, match="labels = \\(2, 3\\) without demo_loss"):
        FusedLearner(None, 4, labels=(2, 3))
    with pytest.raises(ValueError, match="labels.*first = 1 overlaps the 2 expert lanes"):
        FusedLearner(None, 4, demo_loss=DemoLoss(1.0), expert_lanes=2, labels=(1, 3))


# ------------------------------------------------------------------------------------------------- the mask rule
def test_label_mask_against_a_table():
    from ddpg_trucktrailer_amd.mpc import label_mask
    idx = torch.tensor([[-1, 0], [-1, 3], [0, 0], [5, 1], [5, 2], [5, 3], [2, 4], [7, 5], [7, 100]], dtype=torch.int32)
    assert label_mask(idx, 2, 3).tolist() == [False, False, False, False, True, True, True, False, False]
    assert label_mask(idx, 0, 1).tolist() == [False, False, True, False, False, False, False, False, False]
    assert label_mask(idx, 0, 101).tolist() == [False, False, True, True, True, True, True, True, True]
    assert label_mask(idx, 5, 1).tolist() == [False] * 7 + [True, False]
    assert torch.equal(label_mask(idx, 2, 3), LR.label_rows(idx, 2, 3))


def test_the_loops_torch_path_hands_label_rows_and_labels_on():
    """DDPGRollout._demo_rows: what Agent.learn_batch gets of a draw's index buffer and the ring's label array."""
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    from ddpg_trucktrailer_amd.mpc import ExpertLabels, ExpertLanes
    from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    idx = torch.tensor([[-1, 2], [3, 0], [3, 1], [3, 2], [1, 3], [0, 0]], dtype=torch.int64)
    loop = DDPGRollout.__new__(DDPGRollout)
    loop.demo_loss, loop.expert, loop.labels, loop.label_first = DemoLoss(1.0), ExpertLanes(1), ExpertLabels(2), 1
    loop.ring = TrajectoryRing(4, 8, 23, "cpu")
    loop.ring.enable_labels().copy_(torch.arange(32.0).view(8, 4))
    rows = loop._demo_rows(idx)
    assert rows["demo_rows"].tolist() == [True, True, False, False, False, True]
    assert rows["label_rows"].tolist() == [False, False, True, True, False, False]
    assert rows["labels"][2].item() == 13.0 and rows["labels"][3].item() == 14.0
    loop.labels = None
    assert set(loop._demo_rows(idx)) == {"demo_rows"}


def test_a_side_row_whose_index_is_past_the_lanes_is_not_gathered():
    """A side row's pair is (-1, j), j counting SIDE TUPLES: with more tuples than lanes j >= N, and neither the loop's torch path nor
    demo_stats() may index the label array [slots, N] with it."""
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    from ddpg_trucktrailer_amd.mpc import ExpertLabels, ExpertLanes, gather_labels
    from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    idx = torch.tensor([[-1, 9], [-1, 4], [3, 0], [3, 1], [7, 2], [-1, 1000], [2, 3]], dtype=torch.int32)
    ring = TrajectoryRing(4, 8, 23, "cpu")
    ring.enable_labels().copy_(torch.arange(32.0).view(8, 4))
    mask, values = gather_labels(ring.label, idx, 1, 2)
    assert mask.tolist() == [False, False, False, True, True, False, False]
    assert values.tolist() == [0.0, 0.0, 0.0, 13.0, 30.0, 0.0, 0.0]
    # a slot past the array is not labelled (the kernels' rule), and nothing is read for it
    assert gather_labels(ring.label, torch.tensor([[8, 1], [100, 2]], dtype=torch.int32), 1, 2)[0].tolist() == [False, False]
    # the loop's torch path
    loop = DDPGRollout.__new__(DDPGRollout)
    loop.demo_loss, loop.expert, loop.labels, loop.label_first, loop.ring = DemoLoss(1.0), ExpertLanes(1), ExpertLabels(2), 1, ring
    rows = loop._demo_rows(idx.long())
    assert rows["demo_rows"].tolist() == [True, True, True, False, False, True, False]
    assert rows["label_rows"].tolist() == mask.tolist() and rows["labels"].tolist() == values.tolist()
    # demo_stats() of a learner whose last batch held such side rows (the state learn_batch leaves, on the CPU)
    fl = FusedLearner.__new__(FusedLearner)
    fl.demo_loss, fl.labels, fl.label_array, fl.B, fl.dev = DemoLoss(2.0, False), (1, 2), ring.label, 7, torch.device("cpu")
    fl._demo_index, fl._demo_actions = idx, torch.full((7, 1), 0.5)
    fl.code = torch.tensor([2, 2, 2, 3, 3, 1, 0], dtype=torch.int32)
    fl.mu = torch.tensor([1.0, 0.5, 0.0, 12.0, 31.0, 0.25, 0.75])
    st = fl.demo_stats()
    want = 2.0 * (0.5 ** 2 + 0.0 + 0.5 ** 2 + 1.0 + 1.0) / 7
    assert st["demo_rows"] == 4 and st["labelled"] == 2 and st["applied"] == 5 and abs(st["bc_loss"] - want) <= 1e-12


# ------------------------------------------------------------------------------------------------- label_ref and the torch form
def test_planted_index_mixes_the_four_kinds_of_row():
    from ddpg_trucktrailer_amd.mpc import expert_mask, label_mask
    for B in (33, 257):
        idx = LR.planted_index(B)
        demo, lab = expert_mask(idx, LR.EXPERT), label_mask(idx, LR.FIRST, LR.COUNT)
        assert torch.equal(demo | lab, D.demo_mask(B)) and not bool((demo & lab).any())
        side, ring_demo = idx[:, 0] < 0, (idx[:, 0] >= 0) & (idx[:, 1] < LR.EXPERT)
        assert min(int(side.sum()), int(ring_demo.sum()), int(lab.sum()), int((~(demo | lab)).sum())) >= B // 9
        assert int(idx[:, 0].max()) < LR.SLOTS and int(idx[:, 1].max()) < LR.LANES
        assert set(idx[lab, 1].tolist()) == {2, 3, 4} and set(idx[ring_demo, 1].tolist()) == {0, 1}
    assert LR.planted_labels().unique().numel() == LR.ARRAY_SLOTS * LR.LANES


def test_label_ref_without_labelled_rows_is_demo_ref_and_its_gradient_is_the_stated_one():
    state, hyper, batch, _, _ = R.case(*_CASE)
    B, lam = _CASE[0], 0.7
    none = torch.zeros(B, dtype=torch.bool)
    out, want = LR.ref_step(state, batch, hyper, torch.zeros(B), none, lam=lam, mask=D.demo_mask(B)), D.ref_step(state, batch, hyper, lam=lam)
    for k in ("y", "q", "q_pi", "dq_da", "dq_eff", "code", "applied"):
        assert torch.equal(out[k], want[k]), k
    for name in R.NETS:
        for k, v in want["nets"][name].items():
            assert torch.equal(out["nets"][name][k], v), (name, k)
    # with labelled rows: the head's bias gradient is the sum of the row terms, the labelled ones with their label and unfiltered
    idx = LR.planted_index(B)
    lab, labels = LR.label_rows(idx), LR.labels_of(idx, LR.planted_labels()).double()
    out = LR.ref_step(state, batch, hyper, labels, lab, lam=lam, q_filter=True, mask=D.demo_mask(B) & ~lab)
    mu, a = out["mu"], batch[1].double().view(-1)
    assert bool(out["applied"][lab].all()) and bool((out["code"][lab] == 3).all()) and not bool((out["code"][~lab] == 3).any())
    assert int((out["code"] == 1).sum()) >= 1, "the filter left no demonstration row out: the case shows nothing about labelled rows"
    target = torch.where(lab, labels, a)
    total = (-(1.0 / B) * (out["dq_da"] - 2 * lam * out["applied"].double() * (mu - target)) * (1 - mu * mu)).sum()
    assert abs(out["grads"]["actor"]["mu.bias"].item() - total.item()) <= 1e-12 * max(1.0, abs(total.item()))
    assert float((labels - a)[lab].abs().min()) > 1e-3


@pytest.mark.parametrize("lam, q_filter", D.DEMOS, ids=[f"lam{l:g}-{'filter' if q else 'all'}" for l, q in D.DEMOS])
def test_agent_learn_batch_with_label_rows_in_f32_against_label_ref(lam, q_filter):
    """One Agent(demo_loss=).learn_batch(demo_rows=, label_rows=, labels=) in f32 on the CPU against label_ref.ref_step at B = 33 with
    test_demo_loss_cpu.py's bounds: gradients at both optimizer sites within 3e-5 max |g64| + 1e-7 per tensor, both losses within 1e-5
    relative.  The applied rows are the reference's: the labelled rows all, the others by the filter (no undecided row in this case)."""
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    state, hyper, batch, _, _ = R.case(*_CASE)
    B = _CASE[0]
    idx = LR.planted_index(B)
    lab, labels = LR.label_rows(idx), LR.labels_of(idx, LR.planted_labels())
    mask = D.demo_mask(B) & ~lab
    ref = LR.ref_step(state, batch, hyper, labels, lab, lam=lam, q_filter=q_filter, mask=mask)
    assert int(D.filter_of(ref["q"], ref["q_pi"], mask)["undecided"].sum()) == 0
    agent = R.load_agent(state, hyper, torch.device("cpu"), torch.float32)
    agent.demo_loss = DemoLoss(lam, q_filter)
    seen = {}
    for key in ("critic", "actor"):
        net = getattr(agent, key)

        def step(*a, _net=net, _key=key, _orig=net.optimizer.step, **kw):
            seen[_key] = {k: p.grad.clone() for k, p in _net.named_parameters()}
            return _orig(*a, **kw)
        net.optimizer.step = step
    s, a, r, s2, d = batch
    agent.learn_batch(s, a, r, s2, d.bool(), demo_rows=mask, label_rows=lab, labels=labels)
    assert torch.equal(agent.last_demo_mask, ref["applied"]) and bool(agent.last_demo_mask[lab].all())
    for key in ("critic", "actor"):
        for k, want in ref["grads"][key].items():
            tol = 3e-5 * want.abs().max().item() + 1e-7
            err = (seen[key][k].double() - want).abs().max().item()
            assert err <= tol, (key, k, err, tol)
    for name, got, want in (("critic_loss", agent.last_critic_loss.item(), ref["critic_loss"]),
                            ("actor_loss", agent.last_actor_loss.item(), ref["actor_loss"])):
        assert abs(got - want) <= 1e-5 * max(1e-1, abs(want)), (name, got, want)
    # the label is what is cloned: the same call with the stored actions for labels gives another actor gradient
    other = R.load_agent(state, hyper, torch.device("cpu"), torch.float32)
    other.demo_loss = DemoLoss(lam, q_filter)
    other.learn_batch(s, a, r, s2, d.bool(), demo_rows=mask, label_rows=lab, labels=a.view(-1))
    assert not torch.equal(other.actor.mu.bias.grad, agent.actor.mu.bias.grad)      # (the gradient: one Adam step from zero moments hides it)


def test_agent_learn_batch_refuses_half_a_label():
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    state, hyper, batch, _, _ = R.case(*_CASE)
    s, a, r, s2, d = batch
    rows = torch.zeros(_CASE[0], dtype=torch.bool)
    agent = R.load_agent(state, hyper, torch.device("cpu"), torch.float32)
    with pytest.raises(ValueError, match="label_rows without demo_loss"):
        agent.learn_batch(s, a, r, s2, d.bool(), label_rows=rows, labels=a.view(-1))
    agent.demo_loss = DemoLoss(1.0)
    for kw in (dict(label_rows=rows), dict(labels=a.view(-1))):
        with pytest.raises(ValueError, match="label_rows and labels go together"):
            agent.learn_batch(s, a, r, s2, d.bool(), **kw)


# ------------------------------------------------------------------------------------------------- C ABI: tt_env_mpc_label_ring
FAKE = 0x10000      # never read: every call below is refused first


def _mpc_args(L, **kw):
    a = dict(horizon=12, samples=65, sigma=0.3, rho=0.8, lambda_=10.0, gamma=1.0, k_lat=20.0, k_yaw=300.0, action_scale=0.785, seed=1)
    a.update(kw)
    return L.TTMpcArgs(**a)


def _label_ring_refused(L, handle=FAKE, args="good", plan=FAKE, expert=2, lanes=3, ring="good", label=FAKE, high=0.785,
                        act_scaled=FAKE, **view):
    dll = L.load()
    p = lambda x: None if x is None else C.c_void_p(x)
    if args == "good":
        args = _mpc_args(L)
    if ring == "good":
        v = dict(cursor=FAKE, obs=FAKE, act=FAKE, rew=FAKE, done=FAKE, n_envs=8, slots=8)
        v.update(view)
        ring = L.TTRingView(**v)
    rc = dll.tt_env_mpc_label_ring(p(handle), None if args is None else C.byref(args), p(plan), expert, lanes,
                                   None if ring is None else C.byref(ring), p(label), high, p(act_scaled), None)
    msg = dll.tt_last_error(None).decode()
    assert rc == L.TT_EINVAL and msg.startswith("tt_env_mpc_label_ring:"), (rc, msg)
    return msg


def test_the_entry_points_are_exported_and_the_abi_keeps_its_sizes(lib):
    L = lib
    for name in ("tt_env_mpc_label_ring", "tt_mlp_forward_save_demo_labels", "tt_mlp_actor_tail_demo_labels"):
        assert name in L.EXPORTS and hasattr(L.load(), name)
    assert L.load().tt_version() == 3
    assert C.sizeof(L.TTDemoLoss) == 48 and C.sizeof(L.TTDemoLabels) == 24 and C.sizeof(L.TTMpcArgs) == 48


def test_label_ring_refuses_before_it_reads_the_handle(lib):
    L = lib
    assert "NULL handle" in _label_ring_refused(L, handle=None)
    for kw in (dict(args=None), dict(plan=None), dict(ring=None), dict(label=None)):
        assert "args, plan, ring and label" in _label_ring_refused(L, **kw), kw
    for m in (-1, -2 ** 31):
        assert "expert_lanes" in _label_ring_refused(L, expert=m)
    for n in (0, -1, -2 ** 31):
        assert "label_lanes" in _label_ring_refused(L, lanes=n)
    assert "ring->cursor" in _label_ring_refused(L, cursor=None)
    assert "ring->act and act_scaled" in _label_ring_refused(L, act=None)
    assert "ring->act and act_scaled" in _label_ring_refused(L, act_scaled=None)
    # with no expert lane the two are not needed: the call gets as far as the next refusal
    assert "high" in _label_ring_refused(L, expert=0, act=None, act_scaled=None, high=0.0)
    assert "slots" in _label_ring_refused(L, slots=0)
    for m, n in ((2, 7), (0, 9), (8, 1), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert "more than n_envs = 8" in _label_ring_refused(L, expert=m, lanes=n), (m, n)
    assert "n_envs" not in _label_ring_refused(L, expert=2, lanes=6, high=0.0)          # M + L = n_envs is allowed
    for high in (0.0, -0.5, math.nan, math.inf):
        assert "high" in _label_ring_refused(L, high=high), high
    for word, spoil in [("horizon", dict(horizon=0)), ("horizon", dict(horizon=65)), ("samples", dict(samples=0)),
                        ("samples", dict(samples=1025)), ("sigma", dict(sigma=-0.1)), ("sigma", dict(sigma=math.nan)),
                        ("k_lat", dict(k_lat=-1.0)), ("k_yaw", dict(k_yaw=math.inf)), ("rho", dict(rho=1.0)),
                        ("rho", dict(rho=math.nan)), ("lambda", dict(lambda_=0.0)), ("lambda", dict(lambda_=math.nan)),
                        ("gamma", dict(gamma=0.0)), ("gamma", dict(gamma=1.5)), ("action_scale", dict(action_scale=0.0)),
                        ("action_scale", dict(action_scale=math.inf))]:
        assert word in _label_ring_refused(L, args=_mpc_args(L, **spoil)), (word, spoil)


# ------------------------------------------------------------------------------------------------- C ABI: the _labels entry points
_LABELS = dict(fwd="tt_mlp_forward_save_demo_labels", tail_="tt_mlp_actor_tail_demo_labels")


class FakeLabels(F.Fake):
    """fake_args.Fake's demonstration form through the _labels entry points: the same arguments, then expert_lanes, the tt_demo_labels
    (NULL with with_labels false), then the stream."""

    def __init__(self, L, B, expert_lanes=2):
        super().__init__(L, B, "demo")
        self.expert_lanes, self.with_labels = expert_lanes, True
        self.labels = L.TTDemoLabels(label=self.nxt(), n_envs=8, slots=8, first=2, count=3)

    def _call(self, entry, args):
        if entry == "tail_":
            args.append(C.byref(self.shape) if self.with_shape else None)
        args.append(C.byref(self.demo) if self.with_demo else None)
        return getattr(self.L.load(), _LABELS[entry])(*args, self.expert_lanes, C.byref(self.labels) if self.with_labels else None, None)


_set = F.set_field
_NO_LABELS = lambda f: setattr(f, "with_labels", False)
_COMMON = [("demo is NULL", None, False), ("expert_lanes = -1", lambda f: setattr(f, "expert_lanes", -1), True),
           ("demo->k", _set("demo", "k", -0.5), True), ("demo->k", _set("demo", "k", float("nan")), True),
           ("NULL", _set("demo", "a", None), True), ("NULL", _set("demo", "idx", None), True), ("NULL", _set("demo", "dq_eff", None), True),
           ("NULL", _set("demo", "code", None), True), ("demo->q is NULL", _set("demo", "q", None), True),
           ("dq_eff is dq_da", lambda f: setattr(f.demo, "dq_eff", f.dq_da), True),
           ("dq_da is NULL", lambda f: setattr(f, "dq_da", None), True),
           ("labels->label is NULL", _set("labels", "label", None), True),
           ("0 envs", _set("labels", "n_envs", 0), True), ("-3 slots", _set("labels", "slots", -3), True),
           ("labels->first = -1", _set("labels", "first", -1), True), ("labels->count = 0", _set("labels", "count", 0), True),
           ("labels->count = -2", _set("labels", "count", -2), True),
           ("leave the 8 envs", _set("labels", "count", 7), True), ("leave the 8 envs", _set("labels", "first", 2 ** 31 - 1), True),
           ("overlaps the 3 expert lanes", lambda f: setattr(f, "expert_lanes", 3), True),
           # labels == NULL is the _lanes form: its refusals, in this entry point's name
           ("expert_lanes = -1", lambda f: (_NO_LABELS(f), setattr(f, "expert_lanes", -1)), True),
           ("demo->k", lambda f: (_NO_LABELS(f), setattr(f.demo, "k", -0.5)), True)]
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
def test_labels_entry_points_check_their_arguments_before_any_hip_call(lib, entry, word, spoil, with_demo):
    L = lib
    f = FakeLabels(L, 256)
    if spoil is not None:
        spoil(f)
    f.with_demo = with_demo
    rc, msg = getattr(f, entry)(), f.last_error()
    assert rc == L.TT_EINVAL, (rc, msg)
    assert msg.startswith(_LABELS[entry] + ":") and word in msg, msg


# ------------------------------------------------------------------------------------------------- resources
def test_the_label_form_of_the_planner_has_no_scratch_no_vector_spill_and_two_waves(lib):
    """k_mpc_label_ring (the planner's body with the third epilogue), per-env goals or not: the budget of the planner's other two
    launches, whose instantiations stay two each."""
    from ddpg_trucktrailer_amd import kernel_resources as kr
    ks = kr.kernels()
    label, ring, plan = kr.find(ks, "16k_mpc_label_ringILb"), kr.find(ks, "14k_mpc_act_ringILb"), kr.find(ks, "10k_mpc_planILb")
    assert len(label) == 2 and len(ring) == 2 and len(plan) == 2, (sorted(label), sorted(ring), sorted(plan))
    for n, v in {**label, **ring, **plan}.items():
        assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["max_threads"] == 256 and v["lds"] == 0, (n, v)
        assert kr.waves_per_simd(v["vgpr"]) >= 2, (n, v)


def test_the_demonstration_kernels_keep_their_class_and_lds(lib):
    """The three kernels that read DemoIn: no scratch, no vector spill, the waves-per-SIMD class of the 200 / 194 / 194 registers they
    had before the label fields, and at most 83648 B of LDS."""
    from ddpg_trucktrailer_amd import kernel_resources as kr
    ks = kr.kernels()
    demo = {**kr.find(ks, "16k_fwd_small_demo"), **kr.find(ks, "17k_actor_tail_demoILb")}
    assert len(demo) == 3, sorted(demo)
    for n, v in demo.items():
        was = 200 if "fwd_small" in n else 194
        assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["lds"] <= 83648, (n, v)
        assert kr.waves_per_simd(v["vgpr"]) >= kr.waves_per_simd(was), (n, v)
