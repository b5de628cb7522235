"""GPU (-m gpu): the demonstration loss of learn() (csrc/ttdemo.hip; ddpg_trucktrailer_amd/demo_loss.py) -- a
behaviour-cloning term on the batch rows that came from the side buffer, gated by a Q-filter, inside the launches learn() makes anyway.

    off      demo_loss set and no demonstration row in the batch against the plain (or the shaped) FusedLearner, bit for bit
    f64      one update against tests/demo_ref.py with every check and bound of test_gpu_learn_shapes.py's f64 test, plus code, dq_eff
    zero     a critic with dQ/da exactly 0: the plain learner's actor gradient is all zeros, the demonstration learner's is demo_ref's
    paths    tail in one grid, sampled first launch: the same bits
    loop     DDPGRollout(demo_loss=): graphs == eager in both orders, resume, demo_stats, refusals

Worst error / bound per check of the f64 test, measured on MI355X ("filter" / "all" = the Q-filter on / off; "x1" the fresh states,
"x20" the trained-scale one; "images" / "f32" = fc2 images on / off; m, v, p, target: the worse of the two nets; the last column:
demonstration rows / rows the learner applied / rows within FILTER_MARGIN of the filter; the last row is the test after the f64 one):

    case                                            pre-ReLU           y           q        q_pi       dq_da      dq_eff grad critic  grad actor           m           v           p      target  demo/applied/undecided
    B1 x1 lam=0.1 filter images                         0.11       0.016       0.022     2.4e-05     5.4e-06     0.00029       0.069       0.011        0.43        0.61         0.5         0.3  1/1/0
    B1 x1 lam=10 filter images                          0.11       0.016       0.022     2.4e-05     5.4e-06     0.00013       0.069       0.015        0.43        0.61        0.48         0.3  1/1/0
    B1 x1 lam=0.1 all images                            0.11       0.016       0.022     2.4e-05     5.4e-06     0.00029       0.069       0.011        0.43        0.61         0.5         0.3  1/1/0
    B1 x1 lam=10 all images                             0.11       0.016       0.022     2.4e-05     5.4e-06     0.00013       0.069       0.015        0.43        0.61        0.48         0.3  1/1/0
    B33 x1 lam=0.1 filter images                        0.19       0.012       0.015        0.01      0.0005      0.0032       0.018       0.032        0.43        0.61         0.5        0.51  11/2/0
    B33 x1 lam=10 filter images                         0.19       0.012       0.015        0.01      0.0005       0.017       0.018       0.051        0.43        0.61        0.49        0.51  11/2/0
    B33 x1 lam=0.1 all images                           0.19       0.012       0.015        0.01      0.0005      0.0043       0.018       0.024        0.43        0.61         0.5        0.51  11/11/0
    B33 x1 lam=10 all images                            0.19       0.012       0.015        0.01      0.0005       0.015       0.018       0.025        0.43        0.61        0.49        0.51  11/11/0
    B257 x1 lam=0.1 filter images                       0.26       0.012       0.017       0.017     0.00058      0.0065       0.022       0.012        0.43        0.63         0.5        0.27  86/24/0
    B257 x1 lam=10 filter images                        0.26       0.012       0.017       0.017     0.00058       0.016       0.022       0.021        0.43        0.63        0.49        0.27  86/24/0
    B257 x1 lam=0.1 all images                          0.26       0.012       0.017       0.017     0.00058      0.0065       0.022       0.011        0.43        0.63         0.5        0.27  86/86/0
    B257 x1 lam=10 all images                           0.26       0.012       0.017       0.017     0.00058       0.015       0.022       0.026        0.43        0.63        0.49        0.27  86/86/0
    B257 x20 lam=0.1 filter huber c=0.01 images          0.3       0.012       0.015       0.022     0.00063      0.0051       0.012      0.0053        0.67        0.64        0.49        0.63  86/29/0
    B257 x1 lam=10 filter f32                           0.34       0.017       0.019        0.02     0.00057       0.018       0.013       0.035        0.43        0.62        0.49        0.35  86/24/0
    zero dQ/da lam=0.1 images                           0.26        0.01       0.019       0.013           0      0.0067       0.012       0.013        0.43        0.61         0.5        0.27  86/17/0

The largest share of any bound is Adam's m at the trained scale (0.67) and v (0.64), as without the option; dq_eff is at most 0.018 of its bound, the actor's gradient
at most 0.051 -- also at lambda = 10, where the cloning term is the larger part of it.  No demonstration row was undecided, and every
code equals the f64 reference's.
"""
import functools
import math

import pytest

import demo_ref as D
import learn_checks as K
import learn_ref as R
import shape_ref as S

pytestmark = pytest.mark.gpu

_id = K.case_id
_learner, _results, _same, _flat, _shape = K.learner, K.results, K.same, K.flat, K.loss_shape


def _demo(lam, q_filter=True):
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    return DemoLoss(lam, q_filter)


def _ring_index(B, dev):
    """An index buffer without a demonstration row: (0, b)."""
    import torch
    return torch.stack((torch.zeros(B, dtype=torch.int32), torch.arange(B, dtype=torch.int32)), 1).to(dev).contiguous()


def _extras(fl):
    return [fl.dq_eff.clone(), fl.code.clone()] + ([fl.pre.clone()] if fl.pre is not None else [])


# ---- off equals today ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shaped", [False, True], ids=["plain", "shaped"])
@pytest.mark.parametrize("tail", [False, True], ids=["two-launches", "tail"])
@pytest.mark.parametrize("images", [True, False], ids=["images", "f32"])
@pytest.mark.parametrize("case", D.OFF_CASES, ids=_id)
def test_no_demonstration_row_leaves_todays_bits(gpu_device, case, images, tail, shaped):
    """Three updates from the trained-scale state through tt_mlp_forward_save_demo + tt_mlp_backward_weights[_shaped] / tt_mlp_actor_tail_demo
    with DemoLoss(10.0) and an index buffer without a demonstration row, against three through the plain FusedLearner (shaped: both with
    LossShape(delta, 0.01), against the shaped learner): the four nets, all moments, both flat gradients, y, q, q_pi, dq_da and the step
    count, bit for bit; dq_eff holds the bits of dq_da and every code is 0."""
    import torch
    state, hyper, batch, ref, _ = R.case(*case)
    B = case[0]
    shape = _shape(S.delta_of(ref), 0.01) if shaped else None
    idx = _ring_index(B, gpu_device)
    runs = []
    for demo in (None, _demo(10.0)):
        _, fl, dbatch = _learner(gpu_device, state, hyper, batch, case[3], images, shape, tail, demo)
        for _ in range(3):
            fl.learn_batch(*dbatch, **({} if demo is None else dict(demo_index=idx)))
        torch.cuda.synchronize()
        assert fl.tail_gave_up() == 0 and int(fl.step_dev.item()) == case[3] + 3
        runs.append(_results(fl))
        if demo is not None:
            assert torch.equal(fl.dq_eff, fl.dq_da) and int(fl.code.abs().sum().item()) == 0
            assert fl.demo_stats() == {"demo_rows": 0, "applied": 0, "bc_loss": 0.0}
    assert all(torch.isfinite(x).all() for x in runs[0])
    _same(runs[1], runs[0], "off")


# ---- one update against f64 ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(case, lam, q_filter, huber, c):
    return D.demo_case(case, lam, q_filter, huber, c)


_F64 = [(case, lam, qf, False, 0.0, True) for case in D.F64_CASES for lam, qf in D.DEMOS] + \
       [(D.OFF_CASES[1], 0.1, True, True, 0.01, True), (D.F64_CASES[2], 10.0, True, False, 0.0, False)]


@pytest.mark.parametrize("case, lam, q_filter, huber, c, images", _F64,
                         ids=[f"B{k[0]}-x{k[1]:g}-lam{l:g}-{'filter' if q else 'all'}{'-huber-c0.01' if h else ''}-{'images' if im else 'f32'}"
                              for k, l, q, h, c, im in _F64])
def test_one_demo_learn_step_against_f64(gpu_device, case, lam, q_filter, huber, c, images):
    """One learn_batch with DemoLoss(lam, q_filter) from demo_ref.demo_case(case): B = 1, 33, 257, every third row a demonstration row;
    the filter on and off, lambda = 0.1 and 10 (where the cloning term dominates the actor's gradient), once with LossShape(delta,
    0.01) -- from the trained-scale B = 257 state, where the Huber step leaves 29 of 86 rows above the filter (the fresh states leave 1
    of 11 and 3 of 86: below the inputs' condition) -- and once with the fc2 images off.  Every check of test_one_learn_step_against_f64 with its bounds; code equals the reference's
    except on undecided rows; dq_da stays the true derivative; dq_eff within 2e-5 max(1, max |ref|)."""
    state, hyper, batch, delta, ref = _case(case, lam, q_filter, huber, c)
    tag = f"B{case[0]} x{case[1]:g} lam={lam:g} {'filter' if q_filter else 'all'}{' huber c=%g' % c if huber else ''}"
    _, fl, _, _ = K.against_f64(gpu_device, state, hyper, batch, ref, delta=delta, c=c, demo=_demo(lam, q_filter), images=images, tag=tag)
    if case[0] >= 33:
        assert int((fl.code == 2).sum().item()) >= 1 and (not q_filter or int((fl.code == 1).sum().item()) >= 1)


# ---- the term alone -------------------------------------------------------------------------------------------------------
def test_a_critic_without_dq_da_learns_the_actor_only_from_demonstrations(gpu_device):
    """B = 257 from demo_ref.zero_action_case: the critics' action_value weights and every stored action are zero, so dQ/da through
    the updated critic is exactly 0 on every row.
    The plain learner's actor gradient is then all zeros.  The demonstration learner's (lambda = 0.1, the filter on) passes the whole
    f64 check -- its actor gradient is demo_ref's, the applied rows' contribution, under test_one_learn_step_against_f64's bound -- and is
    not zero.  Replacing the stored action of every row with code 0 or 1 by 1e6 does not move that gradient by a bit (the critic's pass
    on (s, mu(s)) and the weight launch alone, count = 0, on the buffers learn() left); replacing an applied row's does.
    (This test fails without the feature.)"""
    import torch
    dev = gpu_device
    case, lam = D.F64_CASES[2], 0.1
    B = case[0]
    state, hyper, batch = D.zero_action_case(case)
    _, plain, (s, a, r, s2, d8) = _learner(dev, state, hyper, batch, case[3])
    plain.learn_batch(s, a, r, s2, d8)
    torch.cuda.synchronize()
    assert bool((plain.dq_da == 0).all()) and bool((plain.actor.flat_grad == 0).all())
    assert not bool((plain.critic.flat_grad == 0).all())
    ref = D.ref_step(state, batch, hyper, lam=lam)
    _, fl, half_dq, _ = K.against_f64(dev, state, hyper, batch, ref, demo=_demo(lam), images=True, tag="zero dQ/da lam=0.1",
                                      frozen=("action_value.weight",))
    assert bool((fl.dq_da == 0).all()) and torch.equal(fl.mu, plain.mu)
    code = fl.code.clone()
    n0, n1, n2 = (int((code == k).sum().item()) for k in (0, 1, 2))
    print(f"codes: {n0} ring rows, {n1} demonstration rows left out, {n2} applied")
    assert n0 == B - (B + 2) // 3 and n1 >= 8 and n2 >= 8
    g = fl.actor.flat_grad.clone()
    assert float(g.abs().max().item()) > 1e-4
    assert bool((fl.dq_eff[code < 2] == 0).all()) and bool((fl.dq_eff[code == 2] != 0).any())
    idx = D.demo_index(B, dev)

    def again(actions):
        fl._fwd(fl.agent.critic, s, fl.mu, fl.q_pi, dq_da=fl.dq_da, demo=fl._demo_struct(actions, idx))
        fl._weights(fl.actor, fl.hyp_actor, fl.agent.tau, s, None, fl.ws_actor, adam=False, row=(fl.dq_eff, fl.mu, -1.0 / B))
        torch.cuda.synchronize()
        return fl.actor.flat_grad.clone(), fl.code.clone()

    g1, c1 = again(a)
    assert torch.equal(g1, g) and torch.equal(c1, code)                  # (the two launches alone repeat learn()'s gradient)
    big = torch.where((code < 2).view(-1, 1), torch.full_like(a, 1e6), a).contiguous()
    g2, c2 = again(big)
    assert torch.equal(g2, g) and torch.equal(c2, code), "a row without the term contributed to the actor gradient"
    other = torch.where((code == 2).view(-1, 1), a + 0.5, a).contiguous()
    g3, _ = again(other)
    assert not torch.equal(g3, g)


# ---- paths ----------------------------------------------------------------------------------------------------------------
def _path_options():
    _, _, _, ref, _ = R.case(*D.PATH_CASE)
    return _shape(S.delta_of(ref), 0.01), _demo(1.0)


@pytest.mark.parametrize("shaped", [False, True], ids=["plain", "shaped"])
def test_demo_tail_in_one_grid_equals_the_two_launches(gpu_device, shaped):
    import torch
    state, hyper, batch, _, _ = R.case(*D.PATH_CASE)
    B, step0 = D.PATH_CASE[0], D.PATH_CASE[3]
    shape, demo = _path_options()
    shape = shape if shaped else None
    idx = D.demo_index(B, gpu_device)
    runs = []
    for tail in (False, True):
        _, fl, dbatch = _learner(gpu_device, state, hyper, batch, step0, True, shape, tail, demo)
        for _ in range(2):
            fl.learn_batch(*dbatch, demo_index=idx)
        torch.cuda.synchronize()
        assert fl.tail_gave_up() == 0 and int(fl.step_dev.item()) == step0 + 2
        if tail:
            producers = math.ceil(B / 16)
            hints = fl.tail_words[:64].cpu()
            assert hints[:producers].tolist() == [step0 + 2] * producers and hints[producers:].eq(-1).all()
            # the rows' words carry dq_eff, not dQ/da
            words = fl.tail_words[64:64 + 2 * B].view(B, 2).cpu()
            assert torch.equal(words[:, 0].contiguous().view(torch.float32), fl.dq_eff.cpu()) and words[:, 1].eq(step0 + 2).all()
        runs.append(_results(fl) + _extras(fl))
    assert all(torch.isfinite(x).all() for x in runs[0])
    _same(runs[1], runs[0], "tail")
    assert int((runs[0][-2 if shaped else -1] == 2).sum().item()) >= 1 and not torch.equal(fl.dq_eff, fl.dq_da)
    # and the term is on: the learner without it leaves other bits
    _, fl, dbatch = _learner(gpu_device, state, hyper, batch, step0, True, shape, False)
    for _ in range(2):
        fl.learn_batch(*dbatch)
    torch.cuda.synchronize()
    assert not torch.equal(_results(fl)[0], runs[0][0])


def _ring_with_demos(dev, B, batch, side=1 << 18):
    """A ring of one stored step over 2^20 envs and a side buffer of `side` tuples (a fifth of every draw) whose draw with `seed` IS the
    batch, in order: the first seed of a short list whose ring rows pick distinct envs and whose side rows pick distinct tuples, with at
    least three of each.  Returns (ring, seed, the draw's index)."""
    import torch
    from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing
    s, a, r, s2, d8 = batch
    ring = TrajectoryRing(1 << 20, 3, 23, dev)
    ring.k = 1
    ring.k_dev.fill_(1)
    z = lambda *shape: torch.zeros(shape, device=dev)
    ring.load_side(z(side, 23), z(side), z(side), z(side, 23), torch.zeros(side, dtype=torch.uint8, device=dev))
    for seed in range(4242, 4242 + 64):
        idx = ring.sample_fused(B, seed=seed, return_index=True)[-1].clone()
        demo = idx[:, 0] < 0
        env, j = idx[~demo, 1].long(), idx[demo, 1].long()
        if env.unique().numel() == env.numel() >= 3 and j.unique().numel() == j.numel() >= 3:
            break
    else:
        raise AssertionError("no seed of the list draws distinct rows")
    assert idx[~demo, 0].eq(0).all() and idx[demo, 0].eq(-1).all()
    ring.obs[0, env], ring.obs[1, env] = s[~demo], s2[~demo]
    ring.act[0, env], ring.rew[0, env], ring.done[0, env] = a.view(-1)[~demo], r[~demo], d8[~demo]
    sd = ring.side
    sd["obs"][j], sd["obs2"][j], sd["act"][j], sd["rew"][j], sd["done"][j] = s[demo], s2[demo], a.view(-1)[demo], r[demo], d8[demo]
    return ring, seed, idx


def test_demo_learn_with_the_draw_made_by_its_first_launch(gpu_device):
    """The sampled first launch (tt_mlp_forward_multi_sampled) against a batch drawn before, with a demonstration loss and a shape, from
    a ring with a side buffer: the same batch, the same index buffer, the same bits."""
    import torch
    dev = gpu_device
    state, hyper, batch, _, _ = R.case(*D.PATH_CASE)
    B, step0 = D.PATH_CASE[0], D.PATH_CASE[3]
    shape, demo = _path_options()
    runs = []
    for sampled in (False, True):
        _, fl, dbatch = _learner(dev, state, hyper, batch, step0, True, shape, True, demo)
        ring, seed, idx = _ring_with_demos(dev, B, dbatch)
        for _ in range(2):
            if sampled:
                for t in ring._batch_bufs(B):
                    t.zero_()
                args = ring.sample_args(B, seed=seed)
                s, a, r, s2, d, index = ring._batch_bufs(B)
                fl.learn_batch(s, a, r, s2, d, sample=args, demo_index=index)
            else:
                fl.learn_batch(*dbatch, demo_index=idx)
        torch.cuda.synchronize()
        if sampled:
            for got, want in zip(ring._batch_bufs(B), dbatch + [idx]):
                assert torch.equal(got.view(-1), want.view(-1))
        assert fl.demo_stats()["demo_rows"] == int((idx[:, 0] < 0).sum().item()) >= 3
        runs.append(_results(fl) + _extras(fl))
    _same(runs[1], runs[0], "sampled")


# ---- the loop ---------------------------------------------------------------------------------------------------------------
_SIDE = 150


def _side_tuples(seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((_SIDE, 23), generator=g) * 2 - 1, torch.rand(_SIDE, generator=g) * 2 - 1, torch.randn(_SIDE, generator=g),
            torch.rand((_SIDE, 23), generator=g) * 2 - 1, (torch.rand(_SIDE, generator=g) < 0.1).to(torch.uint8))


def _loop(seed=6, graph_steps=4, pipeline=False, demo="default", side_seed=11, **kw):
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    env = TruckTrailerVecEnv(64)
    env.reset(seed=seed)
    if demo == "default":
        demo = _demo(1.0)
    loop = DDPGRollout(env, batch_size=33, replay_slots=8, seed=seed, graph_steps=graph_steps, pipeline=pipeline, demo_loss=demo, **kw)
    if side_seed is not None:
        loop.ring.load_side(*_side_tuples(side_seed))      # about a quarter of every batch
    return loop


def _stats_agree(loop):
    import torch
    fl = loop.learner
    st = loop.demo_stats()
    code, index, a = fl.code.cpu(), loop.ring._bufs[5].cpu(), loop.ring._bufs[1].cpu().view(-1)
    assert tuple(index.shape) == (33, 2) and torch.equal(code > 0, index[:, 0] < 0)
    assert st["demo_rows"] == int((code > 0).sum()) and st["applied"] == int((code == 2).sum())
    d = (fl.mu.double().cpu() - a.double())[code == 2]
    want = fl.demo_loss.bc_weight * float((d * d).sum()) / 33
    assert abs(st["bc_loss"] - want) <= 1e-12 * max(1.0, want)
    assert torch.equal(fl.dq_eff[(code != 2).to(fl.dev)], fl.dq_da[(code != 2).to(fl.dev)])
    return st


@pytest.mark.parametrize("pipeline", [False, True], ids=["serial", "pipelined"])
def test_vector_loop_with_a_demo_loss_graphs_equal_eager(gpu_device, pipeline):
    """DDPGRollout(demo_loss=DemoLoss(1.0)) at N = 64, B = 33, 8 ring slots, 150 side tuples, 12 steps: whole-step graphs == eager steps
    over the flat weights, bit for bit; finite; demo_stats() agrees with code, the draw's index buffer and the batch's actions; other
    bits than the loop without the option on the same ring."""
    import torch
    flats, rows = [], []
    for graph_steps in (4, 0):
        loop = _loop(graph_steps=graph_steps, pipeline=pipeline)
        assert loop.pipeline == pipeline and loop.graph_steps == graph_steps and loop.learner.demo_loss == _demo(1.0)
        loop.run(5)
        loop.run(7)
        torch.cuda.synchronize()
        assert loop.handover_gave_up == [] and loop.ring.policy_gave_up() == 0 and loop.learner.tail_gave_up() == 0
        assert int(loop.ring.k_dev.item()) == 12 and int(loop.learner.step_dev.item()) >= 9
        flats.append(_flat(loop).clone())
        rows.append(_stats_agree(loop))
        loop.env.close()
    assert torch.equal(flats[0], flats[1]) and torch.isfinite(flats[0]).all()
    assert rows[0] == rows[1] and rows[0]["demo_rows"] >= 1
    plain = _loop(graph_steps=4, pipeline=pipeline, demo=None)
    plain.run(12)
    torch.cuda.synchronize()
    assert not torch.equal(_flat(plain), flats[0])
    plain.env.close()


def test_vector_loop_without_side_tuples_equals_the_plain_loop(gpu_device):
    """A ring with no side tuples is allowed: no row is a demonstration, and 12 steps end with the plain loop's bits."""
    import torch
    flats = []
    for demo in (_demo(5.0), None):
        loop = _loop(demo=demo, side_seed=None)
        loop.run(12)
        torch.cuda.synchronize()
        flats.append(_flat(loop).clone())
        if demo is not None:
            assert loop.demo_stats() == {"demo_rows": 0, "applied": 0, "bc_loss": 0.0}
        loop.env.close()
    assert torch.equal(flats[0], flats[1])


def test_vector_loop_with_a_demo_loss_resumes_bitwise(gpu_device, tmp_path):
    """A checkpoint taken at step 6 and resumed in another loop ends step 12 with the same bits; the checkpoint carries the option for
    the loop and the learner, and a loop with another one (or none) refuses it."""
    import torch
    from ddpg_trucktrailer_amd import checkpoint
    a = _loop(seed=21)
    a.run(6)
    path = checkpoint.save_loop_checkpoint(str(tmp_path / "loop.pt"), a)
    assert a.state_dict()["demo_loss"] == [1.0, True] and a.state_dict()["fused_adam"]["demo_loss"] == [1.0, True]
    a.run(6)
    b = _loop(seed=99, side_seed=12)
    b.run(5)                           # its graphs are already captured when the file is loaded
    checkpoint.load_loop_checkpoint(path, b)
    assert b.ring.k == 6 and b.ring.side_count == _SIDE
    b.run(6)
    torch.cuda.synchronize()
    assert torch.equal(_flat(a), _flat(b))
    for st_a, st_b in ((a.learner.actor, b.learner.actor), (a.learner.critic, b.learner.critic)):
        assert torch.equal(st_a.m, st_b.m) and torch.equal(st_a.v, st_b.v)
    assert int(a.learner.step_dev.item()) == int(b.learner.step_dev.item())
    assert _stats_agree(a) == _stats_agree(b)
    for other in (_demo(2.0), _demo(1.0, False), None):
        c = _loop(seed=3, demo=other)
        with pytest.raises(ValueError, match="demo_loss"):
            checkpoint.load_loop_checkpoint(path, c)
        c.env.close()
    for lp in (a, b):
        lp.env.close()


def test_refused_combinations_raise(gpu_device, monkeypatch):
    import torch
    from ddpg_trucktrailer_amd.agent import Agent
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    from ddpg_trucktrailer_amd.population import PopulationRollout
    from ddpg_trucktrailer_amd.td3 import TD3Config
    with pytest.raises(ValueError, match="demo_loss"):
        _loop(td3=TD3Config(), updates_per_step=2)
    with pytest.raises(ValueError, match="demo_loss"):
        _loop(data_parallel=True, dp_exchange="p2p")
    with pytest.raises(ValueError, match="demo_loss"):
        _loop(dp_exchange="p2p")
    with pytest.raises(ValueError, match="demo_loss"):
        _loop(n_step=3)
    with pytest.raises(ValueError, match="demo_loss"):
        _loop(demo=(1.0, True))
    monkeypatch.setenv("TT_FORCE_DP", "1")
    with pytest.raises(ValueError, match="demo_loss"):
        _loop()
    monkeypatch.delenv("TT_FORCE_DP")
    with pytest.raises(ValueError, match="demo_loss"):
        PopulationRollout(64, [1, 2], demo_loss=_demo(1.0))
    # an agent built with another option than the loop's, a learner whose ranks exchange gradients, a learner without its index
    kw = dict(alpha=1e-4, beta=1e-3, input_dims=(23,), tau=1e-3, n_actions=1, batch_size=33, device=gpu_device, replay=False)
    with pytest.raises(ValueError, match="demo_loss"):
        _loop(agent=Agent(demo_loss=_demo(2.0), capturable=True, **kw))
    with pytest.raises(ValueError, match="demo_loss"):
        _loop(demo=None, agent=Agent(demo_loss=_demo(2.0), capturable=True, **kw))
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=gpu_device)
    batch = (z(33, 23), z(33, 1), z(33), z(33, 23), z(33, dtype=torch.uint8))
    fl = FusedLearner(Agent(**kw), 33, demo_loss=_demo(1.0))
    with pytest.raises(ValueError, match="demo_index"):
        fl.learn_batch(*batch)
    with pytest.raises(ValueError, match="demo_loss"):
        fl.learn_batch(*batch, demo_index=z(33, 2, dtype=torch.int32), n_step=2)
    with pytest.raises(ValueError, match="demo_loss"):
        fl.enable_p2p()
    fl.grad_sync_critic = fl.grad_sync_actor = lambda: None
    with pytest.raises(ValueError, match="demo_loss"):
        fl.learn_batch(*batch, demo_index=z(33, 2, dtype=torch.int32))
    plain = FusedLearner(Agent(**kw), 33)
    with pytest.raises(ValueError, match="demo_loss"):
        plain.learn_batch(*batch, demo_index=z(33, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="demo_loss"):
        plain.demo_stats()
