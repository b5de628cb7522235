"""GPU (-m gpu): expert labels of the vector loop (include/ttenv.h: tt_env_mpc_label_ring, tt_demo_labels, tt_mlp_*_demo_labels;
csrc/ttenv_mpc.h: k_mpc_label_ring; ddpg_trucktrailer_amd/mpc.py: ExpertLabels).

    launch    tt_env_mpc_label_ring after tt_actor_act_ring on fenced buffers against tt_env_mpc_plan on an identical env: the labels
              of lanes [M, M + L) and the plan bit for bit; lanes < M as tt_env_mpc_act_ring leaves them on a third identical setup;
              ring.act and act_scaled of lanes >= M, every other label, the OU state, the counter and the env untouched; both cursor
              parities; a cursor of -1 stores no label
    lockstep  two VectorSteppers, one with labels: EVERY lane agrees bit for bit (labels do not act); each step's labels are
              MPCExpert.act's on a twin env; the label after an auto-reset is the one from an all-zero plan
    learner   FusedLearner(expert_lanes=2, labels=(2, 3)) on demo_ref's batches with the four kinds of row mixed (label_ref.planted_index):
              tests/learn_checks.py's f64 check with its bounds as they stand; NULL labels == the _lanes entry points; the filter does not
              touch labelled rows; labels of other lanes and slots do not reach the actor gradient; the term follows the label
    loop      DDPGRollout(expert=, labels=, demo_loss=): graphs == eager in both orders, resume, demo_stats against code and the two
              mask rules; a checkpoint with another option is refused before a network is written

Every test here fails without the feature (the entry points and the options do not exist).

Measured on MI355X: 50 tests in 7.7 s.  The learner's worst error / bound per check at B = 257 with the filter: dq_eff 0.017, grad actor
0.014, Adam's v 0.63 (critic), p 0.50 of their bounds; 86 rows of demo_ref's mask of which 28 are labelled, 41 applied, none undecided; the
fused tail leaves the two launches' ratios."""
import ctypes as C

import numpy as np
import pytest

import demo_ref as D
import label_ref as LR
import learn_checks as K
import learn_ref as R
import mpc_ref as M

pytestmark = pytest.mark.gpu

N = 8
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


# ---- 1: the launch against tt_env_mpc_plan and tt_env_mpc_act_ring ---------------------------------------------------------------
SLOTS, SEED = 4, 31


class _Setup:
    """An env, a fenced ring with a label array, and the state tt_mlp_split_pack and tt_actor_act_ring leave for step K_STEP: what
    the planner's launch of that step finds.  plan_rows: the rows of the planted plan the launch owns."""

    def __init__(self, dev, H, warm, K_STEP, plan_rows):
        import torch
        import fenced
        from ddpg_trucktrailer_amd import _lib as L, fused
        from ddpg_trucktrailer_amd.networks import ActorNetwork
        self.t = t = K_STEP % SLOTS
        torch.manual_seed(3)
        actor = ActorNetwork(1e-4, (23,), 400, 300, 1, name="actor", device=torch.device(dev))
        self.env = env = _placed_env(dev, warm)
        lib, p = env.lib, L.ptr
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.arena = arena = fenced.Arena(dev, "nan")
        R_ = dict(full=False, tile_bytes=256 * 23 * 4, also_input=True)
        self.ring = ring = dict(obs=arena.out("~ring.obs", (SLOTS, N, 23), **R_), act=arena.out("~ring.act", (SLOTS, N), **R_),
                                rew=arena.out("~ring.rew", (SLOTS, N), **R_), done=arena.out("~ring.done", (SLOTS, N), torch.uint8, **R_))
        env.observe(out=ring["obs"][t])
        ring["done"][(K_STEP - 1) % SLOTS].zero_()
        self.cursor = arena.inp("cursor", torch.zeros(32, dtype=torch.int32, device=dev))
        self.k_dev = arena.inp("k_dev", torch.tensor(K_STEP, dtype=torch.int64, device=dev))
        self.ou = arena.inp("ou_state", torch.full((N,), 0.05, device=dev), tile_rows=128)
        self.scaled = arena.out("act_scaled", (N,), tile_rows=128, also_input=True)
        self.planted = torch.from_numpy(M.planted_plan(N, H)).to(dev)
        self.plan = arena.inp("plan", self.planted[:plan_rows].clone())
        # a pattern in every label: 100 + slot * N + lane (no decision is outside [-1, 1])
        self.pattern = 100.0 + torch.arange(SLOTS * N, dtype=torch.float32, device=dev).view(SLOTS, N)
        self.label = arena.inp("label", self.pattern.clone(), tile_rows=128)
        w = fused._fill_weights(actor, L.TTMlpWeights())
        img = arena.out("~split_ws", (int(lib.tt_mlp_split_ws_bytes()),), torch.uint8, full=False, tile_bytes=1 << 16, also_input=True)
        w.split_ws, w.ws_packed = img.data_ptr(), 1
        cur = L.TTRingCursor(self.k_dev.data_ptr(), SLOTS, 0, self.cursor.data_ptr())
        self.view = L.TTRingView(self.cursor.data_ptr(), ring["obs"].data_ptr(), ring["act"].data_ptr(), ring["rew"].data_ptr(),
                                 ring["done"].data_ptr(), N, SLOTS)
        L.check(lib.tt_mlp_split_pack(C.byref(w), 0, p(img), None, C.byref(cur), st))
        L.check(lib.tt_actor_act_ring(N, C.byref(self.view), C.byref(w), p(self.ou), 27, 0, p(self.k_dev), 0.2 * 1e-2, 0.15 * 0.1, HIGH,
                                      p(self.scaled), st))
        torch.cuda.synchronize()
        assert self.cursor[:4].tolist()[0] == t
        self.policy = {k: v.clone() for k, v in ring.items()}
        self.policy_scaled, self.policy_ou, self.before = self.scaled.clone(), self.ou.clone(), _blob(env)
        assert torch.isfinite(self.policy["act"][t]).all() and torch.isfinite(self.policy_scaled).all()
        self._keep = (actor, w, img)


@pytest.mark.parametrize("K_STEP", [4, 5], ids=["even-step", "odd-step"])
@pytest.mark.parametrize("warm", [False, True], ids=["fresh", "warm"])
@pytest.mark.parametrize("H,S", [(5, 1), (5, 65), (12, 1), (12, 65)])
@pytest.mark.parametrize("M_,L_", [(2, 3), (0, 8)], ids=["M2-L3", "M0-L8"])
def test_launch_against_mpc_plan_and_act_ring(gpu_device, M_, L_, H, S, warm, K_STEP):
    import torch
    dev = gpu_device
    cfg = _cfg(H, S)
    a = _Setup(dev, H, warm, K_STEP, M_ + L_)
    t, ring, live_n = a.t, a.ring, M_ + L_
    a.env.mpc_label_ring(cfg, a.plan, M_, L_, a.view, a.label, HIGH, a.scaled, seed=SEED)
    torch.cuda.synchronize()
    a.arena.assert_clean(f"M={M_} L={L_} H={H} S={S} warm={warm} k={K_STEP}")

    # the same decisions through tt_env_mpc_plan on an identical env, the full plan, the same seed, live = the launch's lanes
    twin = _placed_env(dev, warm)
    plan2, mu2 = a.planted.clone(), torch.full((N,), 7.0, dtype=torch.float32, device=dev)
    live = (torch.arange(N, device=dev) < live_n).to(torch.uint8)
    twin.mpc_plan(cfg, plan2, mu2, live=live, seed=SEED)
    torch.cuda.synchronize()
    assert _same(a.label[t][M_:live_n], mu2[M_:live_n]), (a.label[t], mu2)
    assert _same(a.plan, plan2[:live_n])
    assert float(a.label[t][M_:live_n].abs().max()) <= 1.0
    # every other label: the planted pattern (other slots, lanes < M and lanes >= M + L of slot t)
    keep = torch.ones((SLOTS, N), dtype=torch.bool, device=dev)
    keep[t, M_:live_n] = False
    assert _same(a.label[keep], a.pattern[keep])
    # lanes >= M: the policy's bits in ring.act[t] and act_scaled
    assert _same(ring["act"][t][M_:], a.policy["act"][t][M_:]) and _same(a.scaled[M_:], a.policy_scaled[M_:])
    if M_:
        # lanes < M: what tt_env_mpc_act_ring leaves on a third identical setup
        b = _Setup(dev, H, warm, K_STEP, M_)
        b.env.mpc_act_ring(cfg, b.plan, M_, b.view, HIGH, b.scaled, seed=SEED)
        torch.cuda.synchronize()
        assert _same(ring["act"][t][:M_], b.ring["act"][t][:M_]) and _same(a.scaled[:M_], b.scaled[:M_])
        assert _same(a.plan[:M_], b.plan) and _same(ring["act"][t][:M_], mu2[:M_])
        assert not _same(ring["act"][t][:M_], a.policy["act"][t][:M_]), "the expert's rows are the policy's"
        b.env.close()
    for k in ring:
        for slot in range(SLOTS):
            if not (k == "act" and slot == t):
                assert _same(ring[k][slot], a.policy[k][slot]), (k, slot)
    assert _same(a.ou, a.policy_ou) and int(a.k_dev.item()) == K_STEP
    after = _blob(a.env)
    assert a.before[1] == after[1] and np.array_equal(a.before[0], after[0]), "the launch changed the env"
    a.env.close()
    twin.close()


@pytest.mark.parametrize("M_,L_", [(2, 3), (0, 8)], ids=["M2-L3", "M0-L8"])
def test_a_cursor_outside_the_ring_stores_no_label(gpu_device, M_, L_):
    import torch
    dev, H = gpu_device, 5
    cfg = _cfg(H, 65)
    a = _Setup(dev, H, True, 5, M_ + L_)
    a.cursor[0] = -1
    act = a.ring["act"].clone()
    a.env.mpc_label_ring(cfg, a.plan, M_, L_, a.view, a.label, HIGH, a.scaled, seed=SEED)
    torch.cuda.synchronize()
    a.arena.assert_clean("cursor -1")
    assert _same(a.label, a.pattern) and _same(a.ring["act"], act)
    assert not _same(a.plan, a.planted[:M_ + L_]), "the decision itself is made: the plan moved on"
    assert _same(a.scaled[M_:], a.policy_scaled[M_:])
    a.env.close()


# ---- 2: the stepper in lock-step ----------------------------------------------------------------------------------------------------
LABELS = 3


def _loop_poses():
    """Lane 0 (a labelled lane) 0.2 m behind the default goal line: its first step ends the episode; the others mid-approach."""
    return np.concatenate([M.FIRST_STEP_START, M.COLLECT_START[1:N]])


def _loop_env(dev, seed=5):
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    env = TruckTrailerVecEnv(N, device=dev)
    env.reset(seed=seed)
    env.set_pose(_loop_poses())
    return env


def test_stepper_in_lock_step(gpu_device):
    import torch
    from ddpg_trucktrailer_amd.mpc import ExpertLabels, MPCExpert
    from ddpg_trucktrailer_amd.stepper import VectorStepper
    dev, STEPS = gpu_device, 12
    cfg = _cfg(5, 65)
    labels = ExpertLabels(LABELS, cfg, seed=9)
    with_, without = (VectorStepper(_loop_env(dev), batch_size=33, replay_slots=8, seed=6, labels=e) for e in (labels, None))
    assert with_.ring_mode and with_.expert is None and tuple(with_.expert_plan.shape) == (LABELS, 5) and without.expert_plan is None
    assert with_.graph_key()[-1] == labels.as_tuple() and len(without.graph_key()) == 4
    assert tuple(with_.ring.label.shape) == (8, N) and without.ring.label is None
    twin = _loop_env(dev)
    ref = MPCExpert(twin, cfg, seed=9)
    zero_plan_checked = 0
    for k in range(STEPS):
        t, t1 = with_.ring.slot(k), with_.ring.slot(k + 1)
        steps_in_episode = twin.episode()["steps"].cpu().numpy()
        plan_before = ref.plan.clone()
        mu = ref.act().clone()
        label_before = with_.ring.label.clone()
        for stp in (with_, without):
            stp.open_step()
            stp.act_and_step()
            stp.advance()
        torch.cuda.synchronize()
        a, b = with_.ring, without.ring
        for x, y in ((a.obs[t1], b.obs[t1]), (a.act[t], b.act[t]), (a.rew[t], b.rew[t]), (a.done[t], b.done[t])):
            assert _same(x, y), k                                   # EVERY lane: labels do not act
        assert _same(with_.noise.x, without.noise.x) and _same(with_.scaled, without.scaled)
        assert _same(a.label[t][:LABELS], mu[:LABELS]), (k, a.label[t], mu)
        assert _same(with_.expert_plan, ref.plan[:LABELS]), k
        other = torch.ones_like(a.label, dtype=torch.bool)
        other[t, :LABELS] = False
        assert _same(a.label[other], label_before[other]), k
        for i in range(LABELS):
            if k > 0 and steps_in_episode[i] == 0:          # the step after an auto-reset: the stored plan is not read
                assert float(plan_before[i].abs().max()) > 0
                # (zero_mu: made at the end of the previous iteration, from the state this step started in and an all-zero plan)
                assert _same(zero_mu[i], a.label[t][i]), (k, i)
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


# ---- 3: the learner ------------------------------------------------------------------------------------------------------------------
def _with_labels(fl, dev, array=None):
    fl.expert_lanes, fl.labels = LR.EXPERT, (LR.FIRST, LR.COUNT)
    fl.set_label_array((LR.planted_labels() if array is None else array).to(dev).contiguous())
    return fl


def _labels_learner(dev_index):
    """learn_checks.learner whose FusedLearner goes through the _labels entry points with label_ref's lanes and label array and takes
    label_ref.planted_index for the draw's index buffer whatever the caller passes (learn_checks.against_f64 passes demo_ref.demo_index,
    the side-row form of the same rows).  against_f64 knows codes 0 / 1 / 2 and the stored action for a target; so that every check
    and bound of it applies unchanged, a labelled row is SHOWN to it as what it is arithmetically -- an applied demonstration row
    whose target is the label: after the update fl.code holds 2 where the kernels wrote 3 (fl.code_true keeps what they wrote),
    demo_stats() counts the labelled rows among the demonstration rows, and the test puts label_ref.actor_half in learn_ref.actor_half's
    place and the always-applied rule in demo_ref.codes'.

    What of learn_checks.against_f64 the three patches and the shown code rely on (look here first if against_f64 changes):
      * it makes its learner through K.learner(...) and calls fl.learn_batch(s, a, r, s2, d8, demo_index=...) exactly once;
      * it reads fl.code once after the update (`code = fl.code.cpu()`) and derives `applied = code == 2`, which it uses for the
        dq_eff check, the bit test on rows without the term and both actor_half calls with `applied=`;
      * it forms the wanted codes with D.codes(mask, above or mask) -- looked up in demo_ref at call time;
      * every f64 / f32 actor half is R.actor_half(critic, actor, s, a, ..., applied=...) -- looked up in learn_ref at call time --
        with the batch's stored actions for `a`;
      * it calls fl.demo_stats() once and compares demo_rows with the mask's count, applied with `applied`, bc_loss with bc_part.
    The test asserts afterwards that the patches were used (each counts its calls), so a change of that pattern fails loudly."""
    import torch
    plain = K.learner

    def make(dev, state, hyper, batch, step, images=True, shape=None, tail=False, demo=None):
        agent, fl, dbatch = plain(dev, state, hyper, batch, step, images, shape, tail, demo)
        _with_labels(fl, dev)
        learn, stats = fl.learn_batch, fl.demo_stats

        def learn_batch(*args, demo_index=None, **kw):
            out = learn(*args, demo_index=dev_index(fl.B, dev), **kw)
            torch.cuda.synchronize()
            fl.code_true, fl.code_shown = fl.code, torch.where(fl.code == 3, torch.full_like(fl.code, 2), fl.code)
            fl.code = fl.code_shown
            return out

        def demo_stats():
            fl.code = fl.code_true
            st = stats()
            fl.code = fl.code_shown
            fl.stats_true = st
            return dict(st, demo_rows=st["demo_rows"] + st["labelled"])
        fl.learn_batch, fl.demo_stats = learn_batch, demo_stats
        return agent, fl, dbatch
    return make


@pytest.mark.parametrize("tail", [False, True], ids=["two-launches", "tail"])
@pytest.mark.parametrize("q_filter", [True, False], ids=["filter", "all"])
@pytest.mark.parametrize("case", [D.F64_CASES[1], D.F64_CASES[2]], ids=K.case_id)
def test_one_learn_step_with_labelled_rows_against_f64(gpu_device, monkeypatch, case, q_filter, tail):
    """B = 33 and 257, lambda = 1: learn_checks.against_f64 with test_gpu_demo_loss.py's bounds as they stand (outputs, dq_eff, the
    gradients at both optimizer sites, Adam's m, v, p and the targets of every element) against label_ref: weights, dq_eff and code."""
    import torch
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    B = case[0]
    assert B in (33, 257)
    state, hyper, batch, _, _ = R.case(*case)
    idx = LR.planted_index(B)
    lab, labels = LR.label_rows(idx), LR.labels_of(idx, LR.planted_labels())
    mask = D.demo_mask(B) & ~lab
    ref = LR.ref_step(state, batch, hyper, labels, lab, lam=1.0, q_filter=q_filter, mask=mask)
    assert float((labels.double() - batch[1].double().view(-1))[lab].abs().min()) > 1e-3      # label and stored action differ
    make = _labels_learner(LR.planted_index)
    if tail:
        inner = make

        def make(*a, **kw):
            agent, fl, dbatch = inner(*a, **kw)
            fl.fuse_tail = True
            return agent, fl, dbatch
    monkeypatch.setattr(K, "learner", make)
    codes, used = D.codes, dict(codes=0, actor_half=0)

    def codes_with_labels(m, applied):                      # (a labelled row is never left out)
        used["codes"] += 1
        return codes(m, applied | lab)

    def actor_half_with_labels(critic, actor, s, a=None, dq_da=None, c=0.0, lam=0.0, applied=None):
        used["actor_half"] += 1
        return LR.actor_half(critic, actor, s, a, labels, lab, dq_da=dq_da, c=c, lam=lam, applied=applied)
    monkeypatch.setattr(D, "codes", codes_with_labels)
    monkeypatch.setattr(R, "actor_half", actor_half_with_labels)
    tag = f"expert-labels B{B} {'filter' if q_filter else 'all'} {'tail' if tail else 'two launches'}"
    shown = dict(ref, demo=ref["demo"] | ref["labelled"])
    _, fl, half, _ = K.against_f64(gpu_device, state, hyper, batch, shown, delta=None, demo=DemoLoss(1.0, q_filter), images=True, tag=tag)
    assert fl.labels == (LR.FIRST, LR.COUNT) and fl.fuse_tail == tail and fl.tail_gave_up() == 0
    assert used["codes"] >= 1 and used["actor_half"] >= 3 and hasattr(fl, "code_true") and hasattr(fl, "stats_true"), used
    # the codes the kernels wrote: 3 on exactly the labelled rows, label_ref's elsewhere (undecided rows by demo_ref's rule)
    code = fl.code_true.cpu()
    assert torch.equal(code == 3, lab)
    und = D.filter_of(ref["q"], half["q_pi"], mask)["undecided"] if q_filter else torch.zeros_like(mask)
    assert torch.equal(code[~und], ref["code"][~und])
    assert bool((code[mask] > 0).all()) and bool((code[mask] < 3).all()) and bool((code[~(mask | lab)] == 0).all())
    st = fl.stats_true
    assert st["labelled"] == int(lab.sum()) and st["demo_rows"] == int(mask.sum()) and st["applied"] == int((code >= 2).sum())
    # the term follows the label: dq_eff - dQ/da on a labelled row is -2 lambda (mu - label), far from the stored action's
    d = (fl.dq_eff.double() - fl.dq_da.double()).cpu()[lab]
    mu, a = fl.mu.double().cpu()[lab], batch[1].double().view(-1)[lab]
    assert float((d + 2.0 * (mu - labels.double()[lab])).abs().max()) <= 2e-5 * max(1.0, float(half["dq_eff"].abs().max()))
    assert float((d + 2.0 * (mu - a)).abs().min()) > 1e-3


@pytest.mark.parametrize("tail", [False, True], ids=["two-launches", "tail"])
def test_null_labels_is_the_lanes_entry_points(gpu_device, tail):
    """The _labels entry points with labels = NULL against the _lanes entry points: two updates, every result bit for bit."""
    import torch
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    case = D.F64_CASES[2]
    state, hyper, batch, _, _ = D.demo_case(case, 1.0, True)
    idx = LR.planted_index(case[0], gpu_device)
    runs = []
    for null_labels in (False, True):
        _, fl, dbatch = K.learner(gpu_device, state, hyper, batch, case[3], True, None, tail, DemoLoss(1.0))
        fl.expert_lanes = LR.EXPERT
        if null_labels:
            fl.labels, fl._labels_ref = (LR.FIRST, LR.COUNT), lambda: None
        for _ in range(2):
            fl.learn_batch(*dbatch, demo_index=idx)
        torch.cuda.synchronize()
        assert fl.tail_gave_up() == 0
        runs.append(K.results(fl) + [fl.dq_eff.clone(), fl.code.clone()])
    K.same(runs[1], runs[0], "labels = NULL")
    assert int((runs[0][-1] == 2).sum()) >= 1 and int((runs[0][-1] == 3).sum()) == 0


def test_filter_isolation_and_target(gpu_device):
    """After one update, the critic's pass on (s, mu(s)) and the actor's weight launch again (count = 0):
    filter     q planted below q_pi on every row: side rows and rows of lanes 0-1 get code 1, labelled rows still code 3, term applied
    isolation  labels of lanes outside [2, 5) and of undrawn slots set to 1e6: the actor gradient keeps its bits
    target     a labelled row's stored action moved: nothing changes; its label moved: the gradient does"""
    import torch
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    dev, case = gpu_device, D.F64_CASES[2]
    B = case[0]
    state, hyper, batch, _, _ = D.demo_case(case, 1.0, True)
    _, fl, (s, a, r, s2, d8) = K.learner(dev, state, hyper, batch, case[3], True, None, False, DemoLoss(1.0))
    array = LR.planted_labels().to(dev)
    _with_labels(fl, dev, array)
    idx = LR.planted_index(B, dev)
    lab = LR.label_rows(idx).to(dev)
    demo = ((idx[:, 0] < 0) | (idx[:, 1] < LR.EXPERT))
    fl.learn_batch(s, a, r, s2, d8, demo_index=idx)
    torch.cuda.synchronize()
    g, code, dq_eff = fl.actor.flat_grad.clone(), fl.code.clone(), fl.dq_eff.clone()
    assert torch.equal(code == 3, lab) and int((code == 1).sum()) >= 1 and int((code == 2).sum()) >= 1

    def again(actions=a, labels=array, q=None):
        fl.set_label_array(labels.contiguous())
        struct = fl._demo_struct(actions, idx)
        if q is not None:
            struct.q = q.data_ptr()
        fl._fwd(fl.agent.critic, s, fl.mu, fl.q_pi, dq_da=fl.dq_da, demo=struct)
        fl._weights(fl.actor, fl.hyp_actor, fl.agent.tau, s, None, fl.ws_actor, adam=False, row=(fl.dq_eff, fl.mu, -1.0 / B))
        torch.cuda.synchronize()
        return fl.actor.flat_grad.clone(), fl.code.clone(), fl.dq_eff.clone()

    g1, c1, e1 = again()
    assert torch.equal(g1, g) and torch.equal(c1, code) and torch.equal(e1, dq_eff)
    # filter
    low = (fl.q_pi - 1.0).contiguous()
    _, c2, e2 = again(q=low)
    assert bool((c2[demo] == 1).all()) and bool((c2[lab] == 3).all()) and bool((c2[~(demo | lab)] == 0).all())
    assert torch.equal(e2[lab], dq_eff[lab]) and torch.equal(e2[~lab], fl.dq_da[~lab]) and not torch.equal(e2[lab], fl.dq_da[lab])
    # isolation
    drawn = torch.zeros_like(array, dtype=torch.bool)
    drawn[idx[lab, 0].long(), idx[lab, 1].long()] = True
    assert bool(drawn[:, LR.FIRST:LR.FIRST + LR.COUNT].any()) and not bool(drawn[LR.SLOTS:].any())      # (undrawn slots of labelled lanes too)
    g3, c3, e3 = again(labels=torch.where(drawn, array, torch.full_like(array, 1e6)))
    assert torch.equal(g3, g) and torch.equal(c3, code) and torch.equal(e3, dq_eff), "a label that no row drew reached the gradient"
    # target
    g4, c4, e4 = again(actions=torch.where(lab.view(-1, 1), a + 0.5, a).contiguous())
    assert torch.equal(g4, g) and torch.equal(e4, dq_eff), "a labelled row's stored action reached the gradient"
    g5, _, e5 = again(labels=torch.where(drawn, array + 0.5, array))
    assert not torch.equal(g5, g) and not torch.equal(e5[lab], dq_eff[lab]) and torch.equal(e5[~lab], dq_eff[~lab])


def test_side_rows_whose_index_is_past_the_lanes(gpu_device):
    """A side row's pair is (-1, j) with j counting side tuples: j >= the label array's lanes (and far past it) changes no bit of an
    update, and demo_stats() gathers no label for such a row."""
    import torch
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    dev, case = gpu_device, D.F64_CASES[2]
    state, hyper, batch, _, _ = D.demo_case(case, 1.0, True)
    runs, stats = [], []
    for shift in (0, 10 ** 6):
        _, fl, dbatch = K.learner(dev, state, hyper, batch, case[3], True, None, False, DemoLoss(1.0))
        _with_labels(fl, dev)
        idx = LR.planted_index(case[0], dev)
        idx[idx[:, 0] < 0, 1] += shift
        assert shift == 0 or int(idx[idx[:, 0] < 0, 1].min()) >= LR.LANES
        fl.learn_batch(*dbatch, demo_index=idx.contiguous())
        torch.cuda.synchronize()
        runs.append(K.results(fl) + [fl.dq_eff.clone(), fl.code.clone()])
        stats.append(fl.demo_stats())
    K.same(runs[1], runs[0], "side rows past the lanes")
    assert stats[0] == stats[1] and stats[0]["labelled"] == int(LR.label_rows(LR.planted_index(case[0])).sum()) >= 1


# ---- 4: the loop ---------------------------------------------------------------------------------------------------------------------
EXPERT = 2


def _options(lanes=LABELS, expert=EXPERT, H=5, S=65, seed=9):
    from ddpg_trucktrailer_amd.mpc import ExpertLabels, ExpertLanes
    return dict(expert=ExpertLanes(expert, _cfg(H, S), seed=seed) if expert else None,
                labels=ExpertLabels(lanes, _cfg(H, S), seed=seed) if lanes else None)


def _loop(dev, seed=6, graph_steps=4, pipeline=False, options=None, **kw):
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    env = _loop_env(dev, seed=seed)
    return DDPGRollout(env, batch_size=33, replay_slots=8, seed=seed, graph_steps=graph_steps, pipeline=pipeline,
                       demo_loss=DemoLoss(1.0), **(_options() if options is None else options), **kw)


def _acting(loop):
    return [K.flat(loop).clone(), loop.ring.act.clone(), loop.ring.obs.clone(), loop.ring.rew.clone(), loop.ring.done.clone(),
            loop.ring.label.clone(), loop.expert_plan.clone(), loop.noise.x.clone()]


def _stats_agree(loop):
    import torch
    from ddpg_trucktrailer_amd.mpc import expert_mask, label_mask
    fl = loop.learner
    st = loop.demo_stats()
    code, index, a = fl.code.cpu(), loop.ring._bufs[5].cpu(), loop.ring._bufs[1].cpu().view(-1)
    assert tuple(index.shape) == (33, 2) and bool((index[:, 0] >= 0).all())
    lab = label_mask(index, EXPERT, LABELS)
    assert torch.equal(code == 3, lab) and torch.equal((code == 1) | (code == 2), expert_mask(index, EXPERT))
    assert st["labelled"] == int(lab.sum()) and st["demo_rows"] == int(((code == 1) | (code == 2)).sum())
    assert st["applied"] == int((code >= 2).sum())
    target = torch.where(lab, loop.ring.label.cpu()[index[:, 0].long(), index[:, 1].long()], a)
    d = (fl.mu.double().cpu() - target.double())[code >= 2]
    want = fl.demo_loss.bc_weight * float((d * d).sum()) / 33
    assert abs(st["bc_loss"] - want) <= 1e-12 * max(1.0, want)
    assert torch.equal(fl.dq_eff[(code < 2).to(fl.dev)], fl.dq_da[(code < 2).to(fl.dev)])
    return st


@pytest.mark.parametrize("pipeline", [False, True], ids=["serial", "pipelined"])
def test_loop_with_expert_lanes_labels_and_demo_loss_graphs_equal_eager(gpu_device, pipeline):
    import torch
    runs, rows = [], []
    for graph_steps in (4, 0):
        loop = _loop(gpu_device, graph_steps=graph_steps, pipeline=pipeline)
        assert loop.pipeline == pipeline and loop.graph_steps == graph_steps
        assert loop.learner.expert_lanes == EXPERT and loop.learner.labels == (EXPERT, LABELS)
        assert loop.learner.label_array.data_ptr() == loop.ring.label.data_ptr() and tuple(loop.expert_plan.shape) == (EXPERT + LABELS, 5)
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
    label = runs[0][5]
    assert float(label.abs().max()) <= 1.0 and float(label[:, EXPERT:EXPERT + LABELS].abs().max()) > 0
    assert not bool(label[:, :EXPERT].any()) and not bool(label[:, EXPERT + LABELS:].any()), "a lane that is not labelled got a label"
    assert float(runs[0][6].abs().max()) > 0


def test_loop_resumes_bitwise_and_refuses_another_option(gpu_device, tmp_path):
    import torch
    from ddpg_trucktrailer_amd import checkpoint
    a = _loop(gpu_device, seed=21)
    a.run(6)
    path = checkpoint.save_loop_checkpoint(str(tmp_path / "loop.pt"), a)
    sd = a.state_dict()
    assert sd["labels"] == list(_options()["labels"].as_tuple()) and sd["expert"] == list(_options()["expert"].as_tuple())
    assert tuple(sd["expert_plan"].shape) == (EXPERT + LABELS, 5) and tuple(sd["ring"]["label"].shape) == (8, N)
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
    # other label lanes, another horizon, another seed, no labels at all
    for other in (_options(lanes=2), _options(H=6), _options(seed=10), _options(lanes=0)):
        c = _loop(gpu_device, seed=3, options=other)
        before = K.flat(c).clone()
        with pytest.raises(ValueError, match="the checkpoint was written with (labels|expert) = "):
            checkpoint.load_loop_checkpoint(path, c)
        assert torch.equal(K.flat(c), before), "a refused checkpoint wrote the networks"
        c.env.close()
    for lp in (a, b):
        lp.env.close()
