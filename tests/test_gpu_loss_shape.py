"""GPU (-m gpu): the loss shape of learn() (csrc/ttshape.hip; ddpg_trucktrailer_amd/loss_shape.py) -- a Huber
critic loss and the actor's pre-activation penalty inside the launches learn() makes anyway.

    off      the shaped entry points with delta = 0 and k = 0 against the plain FusedLearner, bit for bit
    f64      one update against tests/shape_ref.py with every check and bound of test_gpu_learn_shapes.py's f64 test, plus pre
    sat      rows whose mu is exactly +-1.0f: no gradient without the penalty, shape_ref's gradient with it
    paths    tail in one grid, sampled first launch, n-step draw: the same bits
    loop     DDPGRollout(loss_shape=): graphs == eager in both orders, resume, refusals

Worst error / bound per check of the f64 test, measured on MI355X ("huber" = delta on, the case's median |q - y|; "images" / "f32" =
fc2 images on / off; m, v, p, target: the worse of the two nets; the last row is the saturated state of the test after it):

    case                         pre-ReLU            y            q         q_pi        dq_da          pre  grad critic   grad actor            m            v            p       target
    B1 huber c=0 images              0.11        0.016        0.022        0.005      5.1e-05       0.0089        0.068       0.0072         0.43         0.61          0.5         0.32
    B1 mse c=0.01 images             0.11        0.016        0.022      2.4e-05      5.4e-06       0.0089        0.069        0.018         0.43         0.61         0.48          0.3
    B1 mse c=1 images                0.11        0.016        0.022      2.4e-05      5.4e-06       0.0089        0.069        0.023         0.43         0.61         0.48          0.3
    B1 huber c=0.01 images           0.11        0.016        0.022        0.005      5.1e-05       0.0089        0.068         0.02         0.43         0.61         0.49         0.32
    B1 huber c=1 images              0.11        0.016        0.022        0.005      5.1e-05       0.0089        0.068        0.023         0.43         0.61         0.49         0.32
    B33 huber c=0 images             0.19        0.012        0.015       0.0088      0.00051        0.015        0.017        0.016         0.42         0.63          0.5         0.25
    B33 mse c=0.01 images            0.19        0.012        0.015         0.01       0.0005        0.015        0.018         0.01         0.43         0.61          0.5         0.51
    B33 mse c=1 images               0.19        0.012        0.015         0.01       0.0005        0.015        0.018       0.0098         0.43         0.61         0.49         0.51
    B33 huber c=0.01 images          0.19        0.012        0.015       0.0088      0.00051        0.015        0.017       0.0098         0.42         0.63          0.5         0.25
    B33 huber c=1 images             0.19        0.012        0.015       0.0088      0.00051        0.015        0.017        0.011         0.42         0.63         0.49         0.25
    B257 huber c=0 images            0.26        0.012        0.017        0.011      0.00058        0.025        0.012        0.006         0.42         0.61          0.5         0.43
    B257 mse c=0.01 images           0.26        0.012        0.017        0.017      0.00058        0.025        0.022       0.0066         0.43         0.63          0.5         0.27
    B257 mse c=1 images              0.26        0.012        0.017        0.017      0.00058        0.025        0.022       0.0083         0.43         0.63         0.49         0.27
    B257 huber c=0.01 images         0.26        0.012        0.017        0.011      0.00058        0.025        0.012       0.0063         0.42         0.61          0.5         0.43
    B257 huber c=1 images            0.26        0.012        0.017        0.011      0.00058        0.025        0.012       0.0067         0.42         0.61         0.48         0.43
    B1 huber c=1 f32                 0.17         0.01      0.00052       0.0043      3.5e-05       0.0032        0.021        0.026         0.43         0.63         0.49         0.32
    B33 huber c=1 f32                0.33        0.011         0.02        0.015      0.00048        0.019        0.017        0.013         0.43         0.64         0.49         0.26
    B257 huber c=1 f32               0.34        0.017        0.019        0.016      0.00046        0.019        0.014       0.0084         0.43          0.6         0.48         0.38
    saturated c=0.01 images          0.19       0.0081        0.015        0.009      0.00036        0.023        0.013        0.015         0.43         0.64         0.49         0.39

The largest share of any bound is Adam's v (0.64, as without a shape); pre is at most 0.025 of its bound, the actor's gradient at most
0.026 -- also at c = 1, where the penalty's term is the larger part of it.  No row of Q(s, mu(s)) fell on the other side of a ReLU
boundary than in f64.  In the saturated state the kernel's mu is exactly +-1.0f on 12 of the 33 rows (+1: 4, -1: 8).
"""
import functools
import math

import pytest

import learn_checks as K
import learn_ref as R
import shape_ref as S

pytestmark = pytest.mark.gpu

_id = K.case_id
_ACTOR_NAMES, _learner, _results, _same, _flat, _ring_with_batch = K.ACTOR_NAMES, K.learner, K.results, K.same, K.flat, K.ring_with_batch
_shape = K.loss_shape


# ---- off equals today ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [False, True], ids=["two-launches", "tail"])
@pytest.mark.parametrize("images", [True, False], ids=["images", "f32"])
@pytest.mark.parametrize("case", S.OFF_CASES, ids=_id)
def test_shaped_entry_points_with_both_options_off_leave_todays_bits(gpu_device, case, images, tail):
    """Three updates from the trained-scale state through tt_mlp_backward_rows_pair_shaped, tt_mlp_backward_weights_shaped /
    tt_mlp_actor_tail_shaped with delta = 0 and k = 0 (LossShape()) against three through the plain FusedLearner: the four nets, all
    moments, both flat gradients, y, q, q_pi, dq_da and the step count, bit for bit."""
    import torch
    state, hyper, batch, _, _ = R.case(*case)
    runs = []
    for shape in (None, _shape(None, 0.0)):
        _, fl, dbatch = _learner(gpu_device, state, hyper, batch, case[3], images, shape, tail)
        assert (fl._shape is None) == (shape is None)
        if shape is not None:
            assert fl._shape.huber_delta == 0.0 and fl._shape.pre_scale == 0.0 and shape.critic_scale(case[0]) == 2.0 / case[0]
        for _ in range(3):
            fl.learn_batch(*dbatch)
        torch.cuda.synchronize()
        assert fl.tail_gave_up() == 0 and int(fl.step_dev.item()) == case[3] + 3
        runs.append(_results(fl))
    assert all(torch.isfinite(x).all() for x in runs[0])
    _same(runs[1], runs[0], "off")


# ---- one update against f64 ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _shaped(case, huber, c):
    return S.shaped(case, huber, c)


_F64 = [(case, huber, c, True) for case in S.F64_CASES for huber, c in S.SHAPES] + [(case, True, 1.0, False) for case in S.F64_CASES]


@pytest.mark.parametrize("case, huber, c, images", _F64,
                         ids=[f"B{k[0]}-{'huber' if h else 'mse'}-c{c:g}-{'images' if im else 'f32'}" for k, h, c, im in _F64])
def test_one_shaped_learn_step_against_f64(gpu_device, case, huber, c, images):
    """One learn_batch with LossShape(delta, c) from shape_ref.shaped(case): B = 1, 33, 257; delta on (the median |q - y| of the f64
    reference: half the rows on each side of the clamp), c on (0.01, and 1.0, where the penalty dominates the actor's gradient), both
    together.  Every check of test_one_learn_step_against_f64 with its bounds, and pre within 2e-5 max(1, max |pre64|)."""
    state, hyper, batch, delta, ref = _shaped(case, huber, c)
    K.against_f64(gpu_device, state, hyper, batch, ref, delta=delta, c=c, images=images, tag=f"B{case[0]} {'huber ' if huber else 'mse '}c={c:g}")


# ---- a saturated row ------------------------------------------------------------------------------------------------------
def test_a_saturated_row_learns_only_with_the_penalty(gpu_device):
    """B = 33 from a state whose actor head bias is set to -18.5 and its weights scaled by 13 (shape_ref.saturated_state: both signs
    saturate, two thirds of the rows do not), so that mu is exactly +-1.0f on some rows.
    Without c those rows' factors are exactly 0: the plain learner's actor gradient does not move by a bit when dQ/da of those rows is
    replaced by 1e6 (the weight launch alone, count = 0, on the buffers learn() left).
    With c = 0.01 the whole f64 check passes -- the actor's gradient is shape_ref's under test_one_learn_step_against_f64's bound --
    and the plain learner's actor gradient misses that reference by more than the bound.  (This test fails without the feature.)"""
    import torch
    dev = gpu_device
    case, c = S.F64_CASES[1], 0.01
    state0, hyper, batch, _, _ = R.case(*case)
    state = S.saturated_state(state0, batch)
    B = case[0]
    # the plain learner
    _, plain, (s, a, r, s2, d8) = _learner(dev, state, hyper, batch, case[3])
    plain.learn_batch(s, a, r, s2, d8)
    torch.cuda.synchronize()
    sat = plain.mu.abs() == 1.0
    n_sat = int(sat.sum().item())
    print(f"saturated rows: {n_sat} of {B} (+1: {int((plain.mu == 1.0).sum().item())}, -1: {int((plain.mu == -1.0).sum().item())})")
    assert 2 <= n_sat <= B - 2 and (plain.mu == 1.0).any() and (plain.mu == -1.0).any()
    g_plain = plain.actor.flat_grad.clone()
    plain._weights(plain.actor, plain.hyp_actor, plain.agent.tau, s, None, plain.ws_actor, adam=False, row=(plain.dq_da, plain.mu, -1.0 / B))
    torch.cuda.synchronize()
    assert torch.equal(plain.actor.flat_grad, g_plain)                  # (the launch alone repeats learn()'s gradient)
    dq = torch.where(sat, torch.full_like(plain.dq_da, 1e6), plain.dq_da)
    plain._weights(plain.actor, plain.hyp_actor, plain.agent.tau, s, None, plain.ws_actor, adam=False, row=(dq, plain.mu, -1.0 / B))
    torch.cuda.synchronize()
    assert torch.equal(plain.actor.flat_grad, g_plain), "a saturated row contributed to the plain actor gradient"
    dq = torch.where(~sat, plain.dq_da * 2, plain.dq_da)                   # (and the others do count)
    plain._weights(plain.actor, plain.hyp_actor, plain.agent.tau, s, None, plain.ws_actor, adam=False, row=(dq, plain.mu, -1.0 / B))
    torch.cuda.synchronize()
    assert not torch.equal(plain.actor.flat_grad, g_plain)
    # with the penalty: the whole f64 check on the same state
    ref = R.ref_step(state, batch, hyper, delta=None, c=c)
    _, fl, half_dq, _ = K.against_f64(dev, state, hyper, batch, ref, c=c, images=True, tag="saturated c=0.01")
    assert torch.equal(fl.mu, plain.mu)
    far = 0
    off = 0
    for name, g in zip(_ACTOR_NAMES, plain.actor.grads):
        want = half_dq["grads"][name]
        n = want.numel()
        got = g_plain[off:off + n].view_as(g).double().cpu()
        off += n
        far += (got - want).abs().max().item() > 100 * (3e-5 * want.abs().max().item() + 1e-7)
    assert far >= 8, f"the plain gradient is within 100 bounds of the penalised reference in {10 - far} of 10 tensors"
    # the penalty's share on the saturated rows: d(loss)/d(pre) = 2 c pre / B there, nothing else
    pre = fl.pre.double().cpu()
    assert (pre[sat.cpu()].abs() > 9.0).all()


# ---- paths ----------------------------------------------------------------------------------------------------------------
def _path_shape():
    _, _, _, ref, _ = R.case(*S.PATH_CASE)
    return _shape(S.delta_of(ref), 0.01)


def test_shaped_tail_in_one_grid_equals_the_two_launches(gpu_device):
    import torch
    state, hyper, batch, _, _ = R.case(*S.PATH_CASE)
    B, step0 = S.PATH_CASE[0], S.PATH_CASE[3]
    runs = []
    for tail in (False, True):
        _, fl, dbatch = _learner(gpu_device, state, hyper, batch, step0, True, _path_shape(), tail)
        for _ in range(2):
            fl.learn_batch(*dbatch)
        torch.cuda.synchronize()
        assert fl.tail_gave_up() == 0 and int(fl.step_dev.item()) == step0 + 2
        if tail:
            producers = math.ceil(B / 16)
            hints = fl.tail_words[:64].cpu()
            assert hints[:producers].tolist() == [step0 + 2] * producers and hints[producers:].eq(-1).all()
        runs.append(_results(fl) + [fl.pre.clone()])
    assert all(torch.isfinite(x).all() for x in runs[0])
    _same(runs[1], runs[0], "tail")
    # and the shape is on: the plain learner leaves other bits
    _, fl, dbatch = _learner(gpu_device, state, hyper, batch, step0, True, None, False)
    for _ in range(2):
        fl.learn_batch(*dbatch)
    torch.cuda.synchronize()
    assert not torch.equal(_results(fl)[0], runs[0][0])


def test_shaped_learn_with_the_draw_made_by_its_first_launch(gpu_device):
    """The sampled first launch (tt_mlp_forward_multi_sampled) against a batch drawn before, with a shape: the same bits."""
    import torch
    dev = gpu_device
    state, hyper, batch, _, _ = R.case(*S.PATH_CASE)
    B, step0 = S.PATH_CASE[0], S.PATH_CASE[3]
    runs = []
    for sampled in (False, True):
        _, fl, dbatch = _learner(dev, state, hyper, batch, step0, True, _path_shape(), True)
        ring, seed = _ring_with_batch(dev, B, dbatch)
        for _ in range(2):
            if sampled:
                for t in ring._batch_bufs(B)[:5]:
                    t.zero_()
                args = ring.sample_args(B, seed=seed)
                s, a, r, s2, d = ring._batch_bufs(B)[:5]
                fl.learn_batch(s, a, r, s2, d, sample=args)
            else:
                fl.learn_batch(*dbatch)
        torch.cuda.synchronize()
        if sampled:
            for got, want in zip(ring._batch_bufs(B)[:5], dbatch):
                assert torch.equal(got.view(-1), want.view(-1))
        runs.append(_results(fl) + [fl.pre.clone()])
    _same(runs[1], runs[0], "sampled")


def test_shaped_learn_with_an_n_step_draw(gpu_device):
    """n_step = 3: tt_mlp_forward_multi_sampled_nstep's draw against tt_ring_sample_nstep followed by the same shaped learn()."""
    import torch
    import nstep_ref
    dev, n_step = gpu_device, 3
    state, hyper, batch, _, _ = R.case(*S.PATH_CASE)
    B, step0 = S.PATH_CASE[0], S.PATH_CASE[3]
    ring = nstep_ref.synthetic_ring(dev)
    learners = [_learner(dev, state, hyper, batch, step0, True, _path_shape(), True)[1] for _ in range(2)]
    gamma = float(learners[0].agent.gamma)
    for step in range(2):
        kw = dict(seed=1234 + step)
        s, a, r, s2, d = ring.sample_fused(B, done_as_bool=False, n_step=n_step, gamma=gamma, **kw)
        drawn = [t.clone() for t in (s, a, r, s2, d)]
        learners[0].learn_batch(s, a, r, s2, d, n_step=n_step)
        for t in ring._batch_bufs(B)[:5]:
            t.zero_()
        args = ring.sample_args(B, **kw)
        s, a, r, s2, d = ring._batch_bufs(B)[:5]
        learners[1].learn_batch(s, a, r, s2, d, sample=args, n_step=n_step)
        torch.cuda.synchronize()
        for x, y in zip(drawn, (s, a, r, s2, d)):
            assert torch.equal(x, y), step
        _same(_results(learners[1]) + [learners[1].pre.clone()], _results(learners[0]) + [learners[0].pre.clone()], f"n-step {step}")
    assert all(torch.isfinite(x).all() for x in _results(learners[0]))


# ---- the loop ---------------------------------------------------------------------------------------------------------------
def _loop(seed=6, graph_steps=4, pipeline=False, shape="default", **kw):
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    env = TruckTrailerVecEnv(64)
    env.reset(seed=seed)
    if shape == "default":
        shape = _shape(1.0, 0.01)
    return DDPGRollout(env, batch_size=33, replay_slots=16, seed=seed, graph_steps=graph_steps, pipeline=pipeline, loss_shape=shape, **kw)


@pytest.mark.parametrize("pipeline", [False, True], ids=["serial", "pipelined"])
def test_vector_loop_with_a_loss_shape_graphs_equal_eager(gpu_device, pipeline):
    """DDPGRollout(loss_shape=LossShape(1.0, 0.01)) at N = 64, B = 33, 12 steps: whole-step graphs == eager steps over the flat weights,
    bit for bit; finite; other bits than the loop without a shape.  The learn log beside it is unchanged: its critic loss is the TD
    mean square and its actor loss -mean q_pi of the last update."""
    import torch
    flats = []
    for graph_steps in (4, 0):
        loop = _loop(graph_steps=graph_steps, pipeline=pipeline, learn_log=16)
        assert loop.pipeline == pipeline and loop.graph_steps == graph_steps and loop.learner.loss_shape == _shape(1.0, 0.01)
        loop.run(5)
        loop.run(7)
        torch.cuda.synchronize()
        assert loop.handover_gave_up == [] and loop.ring.policy_gave_up() == 0 and loop.learner.tail_gave_up() == 0
        assert int(loop.ring.k_dev.item()) == 12 and int(loop.learner.step_dev.item()) >= 9
        flats.append(_flat(loop).clone())
        fl = loop.learner
        rec = loop.drain_learn_log()
        td2 = ((fl.q.double() - fl.y.double()) ** 2).mean().item()
        assert int(rec["step"][-1]) == int(fl.step_dev.item()) and int(rec["nonfinite"].sum()) == 0
        assert abs(rec["critic_loss"][-1] - td2) <= 1e-5 * max(1e-3, td2)
        assert abs(rec["actor_loss"][-1] + fl.q_pi.double().mean().item()) <= 1e-5 * max(1e-3, abs(fl.q_pi.double().mean().item()))
        loop.env.close()
    assert torch.equal(flats[0], flats[1]) and torch.isfinite(flats[0]).all()
    plain = _loop(graph_steps=4, pipeline=pipeline, shape=None)
    plain.run(12)
    torch.cuda.synchronize()
    assert not torch.equal(_flat(plain), flats[0])
    plain.env.close()


def test_vector_loop_with_a_loss_shape_resumes_bitwise(gpu_device, tmp_path):
    """A checkpoint taken at step 6 and resumed in another loop ends step 12 with the same bits; the checkpoint carries the shape, and
    a loop with another shape (or none) refuses it."""
    import torch
    from ddpg_trucktrailer_amd import checkpoint
    a = _loop(seed=21)
    a.run(6)
    path = checkpoint.save_loop_checkpoint(str(tmp_path / "loop.pt"), a)
    assert a.state_dict()["loss_shape"] == [1.0, 0.01] and a.state_dict()["fused_adam"]["loss_shape"] == [1.0, 0.01]
    a.run(6)
    b = _loop(seed=99)
    b.run(5)                           # its graphs are already captured when the file is loaded
    checkpoint.load_loop_checkpoint(path, b)
    assert b.ring.k == 6
    b.run(6)
    torch.cuda.synchronize()
    assert torch.equal(_flat(a), _flat(b))
    for st_a, st_b in ((a.learner.actor, b.learner.actor), (a.learner.critic, b.learner.critic)):
        assert torch.equal(st_a.m, st_b.m) and torch.equal(st_a.v, st_b.v)
    assert int(a.learner.step_dev.item()) == int(b.learner.step_dev.item())
    for other in (_shape(2.0, 0.01), _shape(1.0, 0.0), None):
        c = _loop(seed=3, shape=other)
        with pytest.raises(ValueError, match="loss_shape"):
            checkpoint.load_loop_checkpoint(path, c)
        c.env.close()
    for lp in (a, b):
        lp.env.close()


def test_refused_combinations_raise(gpu_device, monkeypatch):
    from ddpg_trucktrailer_amd.agent import Agent
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    from ddpg_trucktrailer_amd.population import PopulationRollout
    from ddpg_trucktrailer_amd.td3 import TD3Config
    with pytest.raises(ValueError, match="loss_shape"):
        _loop(td3=TD3Config(), updates_per_step=2)
    with pytest.raises(ValueError, match="loss_shape"):
        _loop(data_parallel=True, dp_exchange="p2p")
    with pytest.raises(ValueError, match="loss_shape"):
        _loop(dp_exchange="p2p")
    with pytest.raises(ValueError, match="loss_shape"):
        _loop(shape=(1.0, 0.01))
    monkeypatch.setenv("TT_FORCE_DP", "1")
    with pytest.raises(ValueError, match="loss_shape"):
        _loop()
    monkeypatch.delenv("TT_FORCE_DP")
    with pytest.raises(ValueError, match="loss_shape"):
        PopulationRollout(64, [1, 2], loss_shape=_shape(1.0, 0.0))
    # an agent built with another shape than the loop's, and a learner whose ranks exchange gradients
    kw = dict(alpha=1e-4, beta=1e-3, input_dims=(23,), tau=1e-3, n_actions=1, batch_size=33, device=gpu_device, replay=False)
    with pytest.raises(ValueError, match="loss_shape"):
        _loop(agent=Agent(loss_shape=_shape(2.0, 0.0), capturable=True, **kw))
    with pytest.raises(ValueError, match="loss_shape"):
        _loop(shape=None, agent=Agent(loss_shape=_shape(2.0, 0.0), capturable=True, **kw))
    fl = FusedLearner(Agent(**kw), 33, loss_shape=_shape(1.0, 0.5))
    with pytest.raises(ValueError, match="loss_shape"):
        fl.enable_p2p()
    fl.grad_sync_critic = fl.grad_sync_actor = lambda: None
    import torch
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=gpu_device)
    with pytest.raises(ValueError, match="loss_shape"):
        fl.learn_batch(z(33, 23), z(33, 1), z(33), z(33, 23), z(33, dtype=torch.uint8))
