"""GPU (-m gpu): expert lanes of the vector loop (include/ttenv.h: tt_env_mpc_act_ring, tt_mlp_*_demo_lanes; csrc/ttenv_mpc.h:
k_mpc_act_ring; ddpg_trucktrailer_amd/mpc.py: ExpertLanes).

    entry     tt_env_mpc_act_ring after tt_actor_act_ring against tt_env_mpc_plan on an identical env: ring.act[t][:M], act_scaled[:M]
              and the plan bit for bit; lanes >= M, every other slot, the env and the fences untouched; both cursor parities
    lockstep  two VectorSteppers, one with expert lanes: the other lanes agree bit for bit; the expert rows are MPCExpert.act's on a
              twin env; the decision after an auto-reset is the one from an all-zero plan
    learner   FusedLearner(expert_lanes=4) on demo_ref's batch with ring rows of lanes < 4 among the demonstration rows: the f64 check of
              tests/learn_checks.py with its bounds; expert_lanes = 0 == the entry points without the count; rows of other lanes do not
              reach the actor gradient
    loop      DDPGRollout(expert=, demo_loss=): graphs == eager in both orders, resume, demo_stats against code; without demo_loss and
              with n_step = 3; a checkpoint with another option is refused

Every test here fails without the feature (the entry points and the options do not exist).

Measured on MI355X: 33 tests in 7.8 s.  The learner's worst error / bound per check equals test_gpu_demo_loss.py's rows for the same
batches (the mask is the same): at B = 257 with the filter dq_eff 0.016, grad actor 0.021, Adam's v 0.63 of their bounds; 86 demonstration
rows, 24 applied, none undecided; the fused tail leaves the two launches' ratios."""
import ctypes as C

import numpy as np
import pytest

import demo_ref as D
import learn_checks as K
import mpc_ref as M

pytestmark = pytest.mark.gpu

N, LANES = 8, 3
HIGH = float(M.HIGH)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])


def _same(x, y):
    return np.array_equal(_bits(x.detach().cpu().numpy()), _bits(y.detach().cpu().numpy()))


def _cfg(H, S):
    return M.return_cfg(S, H, 0.8)


def _eight_lanes():
    """test_gpu_mpc.py's three lanes (goals and trailer lengths of their own), repeated to N = 8."""
    start, goal, L2 = M.lanes("three")
    pick = np.arange(N) % len(start)
    return start[pick], goal[pick], np.asarray(L2)[pick]


def _placed_env(dev, warm):
    import torch
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    start, goal, L2 = _eight_lanes()
    env = TruckTrailerVecEnv(N, device=dev)
    env.set_pose(start, goal=goal, L2=L2)
    if warm:
        for a in M.planted_actions(N):
            env.step(torch.from_numpy(a).to(dev), auto_reset=False)
    return env


def _blob(env):
    sd = env.state_dict()
    return sd["blob"].numpy().copy(), list(sd["meta"])


# ---- 1: the entry point against tt_env_mpc_plan -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K_STEP", [4, 5], ids=["even-step", "odd-step"])
@pytest.mark.parametrize("warm", [False, True], ids=["fresh", "warm"])
@pytest.mark.parametrize("H,S", [(5, 1), (5, 65), (12, 1), (12, 65)])
def test_entry_point_against_mpc_plan(gpu_device, H, S, warm, K_STEP):
    import torch
    import fenced
    from ddpg_trucktrailer_amd import _lib as L, fused
    from ddpg_trucktrailer_amd.networks import ActorNetwork
    dev, SLOTS, SEED = gpu_device, 4, 31
    cfg = _cfg(H, S)
    t = K_STEP % SLOTS
    torch.manual_seed(3)
    actor = ActorNetwork(1e-4, (23,), 400, 300, 1, name="actor", device=torch.device(dev))
    env, twin = _placed_env(dev, warm), _placed_env(dev, warm)
    lib, h, p = env.lib, env._h, L.ptr
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    arena = fenced.Arena(dev, "nan")
    R = dict(full=False, tile_bytes=256 * 23 * 4, also_input=True)
    ring = dict(obs=arena.out("~ring.obs", (SLOTS, N, 23), **R), act=arena.out("~ring.act", (SLOTS, N), **R),
                rew=arena.out("~ring.rew", (SLOTS, N), **R), done=arena.out("~ring.done", (SLOTS, N), torch.uint8, **R))
    env.observe(out=ring["obs"][t])
    ring["done"][(K_STEP - 1) % SLOTS].zero_()
    cursor = arena.inp("cursor", torch.zeros(32, dtype=torch.int32, device=dev))
    k_dev = arena.inp("k_dev", torch.tensor(K_STEP, dtype=torch.int64, device=dev))
    ou = arena.inp("ou_state", torch.full((N,), 0.05, device=dev), tile_rows=128)
    scaled = arena.out("act_scaled", (N,), tile_rows=128, also_input=True)
    planted = torch.from_numpy(M.planted_plan(N, H)).to(dev)
    plan = arena.inp("plan", planted[:LANES].clone())
    w = fused._fill_weights(actor, L.TTMlpWeights())
    img = arena.out("~split_ws", (int(lib.tt_mlp_split_ws_bytes()),), torch.uint8, full=False, tile_bytes=1 << 16, also_input=True)
    w.split_ws, w.ws_packed = img.data_ptr(), 1
    cur = L.TTRingCursor(k_dev.data_ptr(), SLOTS, 0, cursor.data_ptr())
    view = L.TTRingView(cursor.data_ptr(), ring["obs"].data_ptr(), ring["act"].data_ptr(), ring["rew"].data_ptr(),
                        ring["done"].data_ptr(), N, SLOTS)
    L.check(lib.tt_mlp_split_pack(C.byref(w), 0, p(img), None, C.byref(cur), st))
    L.check(lib.tt_actor_act_ring(N, C.byref(view), C.byref(w), p(ou), 27, 0, p(k_dev), 0.2 * 1e-2, 0.15 * 0.1, HIGH, p(scaled), st))
    torch.cuda.synchronize()
    assert cursor[:4].tolist()[0] == t
    policy = {k: v.clone() for k, v in ring.items()}
    policy_scaled, policy_ou, before = scaled.clone(), ou.clone(), _blob(env)
    assert torch.isfinite(policy["act"][t]).all() and torch.isfinite(policy_scaled).all()

    env.mpc_act_ring(cfg, plan, LANES, view, HIGH, scaled, seed=SEED)
    torch.cuda.synchronize()
    arena.assert_clean(f"H={H} S={S} warm={warm} k={K_STEP}")

    # the same decision through tt_env_mpc_plan on the identical env, the full plan and the same seed
    plan2, mu2 = planted.clone(), torch.zeros(N, dtype=torch.float32, device=dev)
    twin.mpc_plan(cfg, plan2, mu2, seed=SEED)
    torch.cuda.synchronize()
    assert _same(ring["act"][t][:LANES], mu2[:LANES]), (ring["act"][t][:LANES], mu2[:LANES])
    assert _same(scaled[:LANES], mu2[:LANES] * torch.tensor(HIGH, dtype=torch.float32, device=dev))
    assert _same(plan, plan2[:LANES])
    assert not _same(ring["act"][t][:LANES], policy["act"][t][:LANES]), "the expert's rows are the policy's"
    # the other lanes, every other slot and array, the OU state, the env
    assert _same(ring["act"][t][LANES:], policy["act"][t][LANES:]) and _same(scaled[LANES:], policy_scaled[LANES:])
    for k in ring:
        for slot in range(SLOTS):
            if not (k == "act" and slot == t):
                assert _same(ring[k][slot], policy[k][slot]), (k, slot)
    assert _same(ou, policy_ou) and int(k_dev.item()) == K_STEP
    after = _blob(env)
    assert before[1] == after[1] and np.array_equal(before[0], after[0]), "the launch changed the env"
    env.close()
    twin.close()


# ---- 2: the stepper in lock-step ----------------------------------------------------------------------------------------------------
def _loop_poses():
    """Lane 0 (an expert lane) 0.2 m behind the default goal line: its first step ends the episode; the others mid-approach."""
    return np.concatenate([M.FIRST_STEP_START, M.COLLECT_START[1:N]])


def _loop_env(dev, seed=5):
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    env = TruckTrailerVecEnv(N, device=dev)
    env.reset(seed=seed)
    env.set_pose(_loop_poses())
    return env


def test_stepper_in_lock_step(gpu_device):
    import torch
    from ddpg_trucktrailer_amd.mpc import ExpertLanes, MPCExpert
    from ddpg_trucktrailer_amd.stepper import VectorStepper
    dev, STEPS = gpu_device, 12
    cfg = _cfg(5, 65)
    expert = ExpertLanes(LANES, cfg, seed=9)
    with_, without = (VectorStepper(_loop_env(dev), batch_size=33, replay_slots=8, seed=6, expert=e) for e in (expert, None))
    assert with_.ring_mode and tuple(with_.expert_plan.shape) == (LANES, 5) and without.expert_plan is None
    assert with_.graph_key()[-1] == expert.as_tuple()
    twin = _loop_env(dev)
    ref = MPCExpert(twin, cfg, seed=9)
    high = torch.tensor(HIGH, dtype=torch.float32, device=dev)
    zero_plan_checked = 0
    for k in range(STEPS):
        t, t1 = with_.ring.slot(k), with_.ring.slot(k + 1)
        steps_in_episode = twin.episode()["steps"].cpu().numpy()
        plan_before = ref.plan.clone()
        mu = ref.act().clone()
        for stp in (with_, without):
            stp.open_step()
            stp.act_and_step()
            stp.advance()
        torch.cuda.synchronize()
        a, b = with_.ring, without.ring
        for x, y in ((a.obs[t1], b.obs[t1]), (a.act[t], b.act[t]), (a.rew[t], b.rew[t]), (a.done[t], b.done[t])):
            assert _same(x[LANES:], y[LANES:]), k
        assert _same(with_.noise.x, without.noise.x), "an expert lane's OU state keeps evolving as the policy's"
        assert _same(a.act[t][:LANES], mu[:LANES]) and _same(with_.scaled[:LANES], mu[:LANES] * high), k
        assert _same(with_.expert_plan, ref.plan[:LANES]), k
        assert float(a.act[t][:LANES].abs().max()) <= 1.0
        for i in range(LANES):
            if k > 0 and steps_in_episode[i] == 0:          # the step after an auto-reset: the stored plan is not read
                assert float(plan_before[i].abs().max()) > 0
                # (zero_mu: made at the end of the previous iteration, from the state this step started in and an all-zero plan)
                assert _same(zero_mu[i], a.act[t][i]), (k, i)
                zero_plan_checked += 1
        # the twin follows with the loop's own scaled actions; first the decision the NEXT step would make from an all-zero plan
        twin.step(with_.scaled.clone(), auto_reset=True)
        zero_mu = torch.zeros(N, dtype=torch.float32, device=dev)
        twin.mpc_plan(cfg, torch.zeros((N, 5), dtype=torch.float32, device=dev), zero_mu, seed=9)
        assert _same(twin.obs, a.obs[t1]), k
        if k == 0:
            assert int(a.done[t][0]) == 1, "lane 0 was placed to finish on its first step"
    assert zero_plan_checked >= 1
    for e in (with_.env, without.env, twin):
        e.close()


# ---- 3: the learner's flag -----------------------------------------------------------------------------------------------------------
EXPERT = 4


def _planted_index(B, dev):
    """demo_ref's mask b % 3 == 0 from two kinds of row: b % 6 == 0 a side row (-1, j); b % 6 == 3 a ring row (slot, lane < 4); every
    other row a ring row of a lane >= 4."""
    import torch
    b = torch.arange(B, dtype=torch.int32)
    idx = torch.stack((b % 5, EXPERT + b), 1)
    side, ring = b % 6 == 0, b % 6 == 3
    idx[side, 0], idx[side, 1] = -1, torch.arange(int(side.sum()), dtype=torch.int32)
    idx[ring, 1] = (b[ring] // 6) % EXPERT
    return idx.to(dev).contiguous()


def test_planted_index_is_demo_refs_mask():
    import torch
    from ddpg_trucktrailer_amd.mpc import expert_mask
    for B in (33, 257):
        idx = _planted_index(B, "cpu")
        assert torch.equal(expert_mask(idx, EXPERT), D.demo_mask(B)) and not torch.equal(idx[:, 0] < 0, D.demo_mask(B))
        assert int(((idx[:, 0] >= 0) & (idx[:, 1] < EXPERT)).sum()) >= B // 6


def _lanes_learner(expert_lanes, index_of):
    """learn_checks.learner whose FusedLearner goes through the _lanes entry points with `expert_lanes` and takes index_of(B, dev) for
    the draw's index buffer whatever the caller passes (learn_checks.against_f64 passes demo_ref.demo_index, the side-row form of the
    same mask): every check and bound of against_f64 then applies unchanged."""
    plain = K.learner

    def make(dev, state, hyper, batch, step, images=True, shape=None, tail=False, demo=None):
        agent, fl, dbatch = plain(dev, state, hyper, batch, step, images, shape, tail, demo)
        fl.expert_lanes = expert_lanes
        learn = fl.learn_batch

        def learn_batch(*args, demo_index=None, **kw):
            return learn(*args, demo_index=index_of(fl.B, dev), **kw)
        fl.learn_batch = learn_batch
        return agent, fl, dbatch
    return make


@pytest.mark.parametrize("tail", [False, True], ids=["two-launches", "tail"])
@pytest.mark.parametrize("q_filter", [True, False], ids=["filter", "all"])
@pytest.mark.parametrize("case", [D.F64_CASES[1], D.F64_CASES[2]], ids=K.case_id)
def test_one_learn_step_with_expert_lane_rows_against_f64(gpu_device, monkeypatch, case, q_filter, tail):
    """B = 33 and 257 (demo_ref.F64_CASES; their CPU-asserted input conditions carry over: the mask and the batch are the same), lambda =
    1: learn_checks.against_f64 with test_gpu_demo_loss.py's bounds as they stand, code per row included (undecided rows by its rule)."""
    import torch
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    assert case[0] in (33, 257)
    state, hyper, batch, delta, ref = D.demo_case(case, 1.0, q_filter)
    make = _lanes_learner(EXPERT, _planted_index)
    if tail:
        inner = make

        def make(*a, **kw):
            agent, fl, dbatch = inner(*a, **kw)
            fl.fuse_tail = True
            return agent, fl, dbatch
    monkeypatch.setattr(K, "learner", make)
    tag = f"expert-lanes B{case[0]} {'filter' if q_filter else 'all'} {'tail' if tail else 'two launches'}"
    _, fl, _, _ = K.against_f64(gpu_device, state, hyper, batch, ref, delta=delta, demo=DemoLoss(1.0, q_filter), images=True, tag=tag)
    assert fl.expert_lanes == EXPERT and fl.fuse_tail == tail and fl.tail_gave_up() == 0
    code, idx = fl.code.cpu(), _planted_index(case[0], "cpu")
    ring_demo = (idx[:, 0] >= 0) & (idx[:, 1] < EXPERT)
    assert bool((code[ring_demo] > 0).all()) and bool((code[~D.demo_mask(case[0])] == 0).all())
    assert int((code[ring_demo] == 2).sum()) >= 1, "no ring row of an expert lane was applied"


@pytest.mark.parametrize("tail", [False, True], ids=["two-launches", "tail"])
def test_zero_expert_lanes_is_the_entry_points_without_the_count(gpu_device, tail):
    import torch
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    case = D.F64_CASES[2]
    state, hyper, batch, _, _ = D.demo_case(case, 1.0, True)
    idx = D.demo_index(case[0], gpu_device)
    runs = []
    for lanes in (None, 0):
        _, fl, dbatch = K.learner(gpu_device, state, hyper, batch, case[3], True, None, tail, DemoLoss(1.0))
        fl.expert_lanes = lanes
        for _ in range(2):
            fl.learn_batch(*dbatch, demo_index=idx)
        torch.cuda.synchronize()
        assert fl.tail_gave_up() == 0
        runs.append(K.results(fl) + [fl.dq_eff.clone(), fl.code.clone()])
    K.same(runs[1], runs[0], "expert_lanes = 0")
    assert int((runs[0][-1] == 2).sum()) >= 1


def test_rows_of_other_lanes_do_not_reach_the_actor_gradient(gpu_device):
    """After one update: the critic's pass on (s, mu(s)) and the actor's weight launch again (count = 0) with the stored action of every
    row of a lane >= 4 set to 1e6 leave the actor gradient's bits; moving an applied ring row's action does not."""
    import torch
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    dev, case = gpu_device, D.F64_CASES[2]
    B = case[0]
    state, hyper, batch, _, _ = D.demo_case(case, 1.0, True)
    _, fl, (s, a, r, s2, d8) = K.learner(dev, state, hyper, batch, case[3], True, None, False, DemoLoss(1.0))
    fl.expert_lanes = EXPERT
    idx = _planted_index(B, dev)
    fl.learn_batch(s, a, r, s2, d8, demo_index=idx)
    torch.cuda.synchronize()
    g, code = fl.actor.flat_grad.clone(), fl.code.clone()

    def again(actions):
        fl._fwd(fl.agent.critic, s, fl.mu, fl.q_pi, dq_da=fl.dq_da, demo=fl._demo_struct(actions, idx))
        fl._weights(fl.actor, fl.hyp_actor, fl.agent.tau, s, None, fl.ws_actor, adam=False, row=(fl.dq_eff, fl.mu, -1.0 / B))
        torch.cuda.synchronize()
        return fl.actor.flat_grad.clone(), fl.code.clone()

    g1, c1 = again(a)
    assert torch.equal(g1, g) and torch.equal(c1, code)
    other = (idx[:, 0] >= 0) & (idx[:, 1] >= EXPERT)
    assert int(other.sum()) == B - int(D.demo_mask(B).sum()) and bool((code[other] == 0).all())
    g2, c2 = again(torch.where(other.view(-1, 1), torch.full_like(a, 1e6), a).contiguous())
    assert torch.equal(g2, g) and torch.equal(c2, code), "a row of a lane >= 4 contributed to the actor gradient"
    applied_ring = (idx[:, 0] >= 0) & (code == 2)
    assert int(applied_ring.sum()) >= 1
    g3, _ = again(torch.where(applied_ring.view(-1, 1), a + 0.5, a).contiguous())
    assert not torch.equal(g3, g)


# ---- 4: the loop ---------------------------------------------------------------------------------------------------------------------
def _expert(lanes=LANES, H=5, S=65, seed=9):
    from ddpg_trucktrailer_amd.mpc import ExpertLanes
    return ExpertLanes(lanes, _cfg(H, S), seed=seed)


def _loop(dev, seed=6, graph_steps=4, pipeline=False, expert="default", demo="default", **kw):
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    env = _loop_env(dev, seed=seed)
    return DDPGRollout(env, batch_size=33, replay_slots=8, seed=seed, graph_steps=graph_steps, pipeline=pipeline,
                       expert=_expert() if expert == "default" else expert, demo_loss=DemoLoss(1.0) if demo == "default" else demo, **kw)


def _acting(loop):
    return [K.flat(loop).clone(), loop.ring.act.clone(), loop.ring.obs.clone(), loop.ring.rew.clone(), loop.ring.done.clone(),
            loop.expert_plan.clone(), loop.noise.x.clone()]


def _stats_agree(loop):
    import torch
    from ddpg_trucktrailer_amd.mpc import expert_mask
    fl = loop.learner
    st = loop.demo_stats()
    code, index, a = fl.code.cpu(), loop.ring._bufs[5].cpu(), loop.ring._bufs[1].cpu().view(-1)
    assert tuple(index.shape) == (33, 2) and bool((index[:, 0] >= 0).all())
    assert torch.equal(code > 0, expert_mask(index, LANES))
    assert st["demo_rows"] == int((code > 0).sum()) and st["applied"] == int((code == 2).sum())
    d = (fl.mu.double().cpu() - a.double())[code == 2]
    want = fl.demo_loss.bc_weight * float((d * d).sum()) / 33
    assert abs(st["bc_loss"] - want) <= 1e-12 * max(1.0, want)
    assert torch.equal(fl.dq_eff[(code != 2).to(fl.dev)], fl.dq_da[(code != 2).to(fl.dev)])
    return st


@pytest.mark.parametrize("pipeline", [False, True], ids=["serial", "pipelined"])
def test_loop_with_expert_lanes_and_demo_loss_graphs_equal_eager(gpu_device, pipeline):
    import torch
    runs, rows = [], []
    for graph_steps in (4, 0):
        loop = _loop(gpu_device, graph_steps=graph_steps, pipeline=pipeline)
        assert loop.pipeline == pipeline and loop.graph_steps == graph_steps and loop.learner.expert_lanes == LANES
        assert loop.ring.side_count == 0
        loop.run(5)
        loop.run(7)
        torch.cuda.synchronize()
        assert loop.handover_gave_up == [] and loop.ring.policy_gave_up() == 0 and loop.learner.tail_gave_up() == 0
        assert int(loop.ring.k_dev.item()) == 12 and int(loop.learner.step_dev.item()) >= 5
        runs.append(_acting(loop))
        rows.append(_stats_agree(loop))
        loop.env.close()
    K.same(runs[1], runs[0], "graphs == eager")
    assert all(torch.isfinite(x.float()).all() for x in runs[0]) and rows[0] == rows[1]
    assert float(runs[0][1][:, :LANES].abs().max()) <= 1.0 and float(runs[0][5].abs().max()) > 0


def test_loop_with_expert_lanes_resumes_bitwise_and_refuses_another_option(gpu_device, tmp_path):
    import torch
    from ddpg_trucktrailer_amd import checkpoint
    a = _loop(gpu_device, seed=21)
    a.run(6)
    path = checkpoint.save_loop_checkpoint(str(tmp_path / "loop.pt"), a)
    sd = a.state_dict()
    assert sd["expert"] == list(_expert().as_tuple()) and tuple(sd["expert_plan"].shape) == (LANES, 5)
    a.run(6)
    b = _loop(gpu_device, seed=99)
    b.run(5)                           # its graphs are already captured when the file is loaded
    checkpoint.load_loop_checkpoint(path, b)
    assert b.ring.k == 6
    b.run(6)
    torch.cuda.synchronize()
    K.same(_acting(b), _acting(a), "resume")
    for st_a, st_b in ((a.learner.actor, b.learner.actor), (a.learner.critic, b.learner.critic)):
        assert torch.equal(st_a.m, st_b.m) and torch.equal(st_a.v, st_b.v)
    assert _stats_agree(a) == _stats_agree(b)
    for other in (_expert(lanes=2), _expert(H=6), _expert(seed=10), None):
        c = _loop(gpu_device, seed=3, expert=other)
        before = K.flat(c).clone()
        with pytest.raises(ValueError, match="expert"):
            checkpoint.load_loop_checkpoint(path, c)
        assert torch.equal(K.flat(c), before), "a refused checkpoint wrote the networks"
        c.env.close()
    for lp in (a, b):
        lp.env.close()


def test_loop_where_expert_lanes_only_act_with_n_step(gpu_device):
    """Without demo_loss the expert only acts: with n_step = 3, graphs == eager; the learner goes through the plain entry points."""
    import torch
    runs = []
    for graph_steps in (4, 0):
        loop = _loop(gpu_device, graph_steps=graph_steps, demo=None, n_step=3)
        assert loop.learner.demo_loss is None and loop.learner.expert_lanes is None and loop.n_step == 3
        loop.run(12)
        torch.cuda.synchronize()
        assert int(loop.ring.k_dev.item()) == 12 and int(loop.learner.step_dev.item()) >= 1
        runs.append(_acting(loop))
        loop.env.close()
    K.same(runs[1], runs[0], "n_step = 3")
    assert torch.isfinite(runs[0][0]).all()
