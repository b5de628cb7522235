"""GPU (-m gpu): one learn() of the hand-written kernels (csrc/ttlearn.hip, csrc/ttpop.hip, bodies in csrc/ttlearn_bodies.h) against
learn() in f64 (tests/learn_ref.py) at the batch sizes where the kernels take other paths than at 256 rows, and the four ways of
launching learn() against each other at those sizes.

    B = 1      one row: three of a workgroup's four waves have an empty row range; loss scale 2 / B
    B = 250    rows_w = 64: the last wave's in-flight chunk is ragged, every clamped load min(b, n - 1) is used
    B = 257    rows_w = 80: waves 0..2 run one step of the beyond-256 loops, the sums a third load_rows round of one row, 17 row
               workgroups of which the last holds one row
    B = 1000   four chunks per wave, a ragged last k16 step inside the beyond-256 loops, 63 producers of the actor tail
    B = 1024   MAXB: the whole row-factor table, 64 producers (all one polling wave can watch)

The batches hold no row with a ReLU unit of critic(s, a) or actor(s) within 3e-5 of zero (learn_ref.make_batch), so no bound here
gives way near a boundary; the units of Q(s, mu(s)) through the updated critic cannot be kept away from zero by construction
(learn_ref's docstring) and are enumerated instead: dQ/da of a row with such a unit must be one of the values it takes with the
unit on either side.

Worst error / bound per check, measured on MI355X (fc2 images on | off; "x20" = the trained-scale state at step 999 -> 1000 with
learn_ref.TRAINED_HYPER; m, v, p, target: the worse of the two nets; "near": rows of Q(s, mu(s)) with a unit within 3e-5 of zero --
every one of them came out on f64's side):

    case         pre-ReLU          y           q        q_pi          dq_da  grad critic    grad actor          m          v          p     target  near
    B1          0.11|0.17  0.016|0.01  0.022|5e-4  2e-5|0.003    5e-6|0.0002   0.069|0.12   0.007|0.013  0.43|0.43  0.61|0.61  0.50|0.50  0.30|0.30     0
    B250        0.36|0.30 0.015|0.017 0.021|0.021 0.019|0.021  0.0008|0.0008   0.095|0.14  0.011|0.0086  0.42|0.43  0.61|0.62  0.50|0.50  0.61|0.65     3
    B257        0.26|0.34 0.012|0.017 0.017|0.019 0.017|0.020  0.0006|0.0006  0.022|0.013 0.0076|0.0057  0.43|0.43  0.63|0.62  0.50|0.50  0.27|0.35     1
    B1000       0.30|0.33 0.012|0.015 0.021|0.022 0.018|0.022  0.0006|0.0006  0.018|0.019 0.0055|0.0059  0.43|0.42  0.62|0.63  0.50|0.50  0.35|0.35     2
    B1024       0.33|0.37 0.015|0.015 0.028|0.025 0.017|0.017  0.0006|0.0006  0.021|0.015 0.0052|0.0074  0.42|0.42  0.61|0.62  0.50|0.50  0.34|0.35     7
    B257 x20    0.30|0.31 0.012|0.013 0.015|0.025 0.022|0.024  0.0006|0.0006  0.014|0.016 0.0076|0.0056  0.65|0.65  0.65|0.64  0.50|0.49  0.46|0.53     3
    B1024 x20   0.28|0.41 0.014|0.015 0.022|0.026 0.023|0.029  0.0006|0.0007  0.020|0.024 0.0088|0.0067  0.63|0.67  0.64|0.65  0.49|0.49  0.39|0.47     9

In the gradient bound 3 e32 never exceeded the first term (at most 0.90 of it, critic at B = 1).  kappa (see the test) reached 4.2e4 in
the critic and 1.7e4 in the actor of the x20 cases and is 1 from zero moments; with 2^-19 alone in p's bound (no kappa) the worst
element is at 0.46 to 0.58 of it everywhere except the actor at B1024 x20: 1.45 | 2.81 times.  The path test found the row factor of the actor's
weight gradient rounded differently per launch path from 257 rows on (csrc/ttlearn_bodies.h: row_factor_of); with the beyond-256 loop
of dW2 cut to one iteration the f64 test fails at B = 1000 and 1024 (critic gradient 18000 to 26000 times its bound) and passes
at B <= 257.
"""
import math

import pytest

import learn_checks as K
import learn_ref as R

pytestmark = pytest.mark.gpu

_id = K.case_id


def _learner(dev, case, images):
    """(agent, FusedLearner, batch on the device) holding the case's state: f32 nets, Adam moments and step count."""
    state, hyper, batch, _, _ = R.case(*case)
    return K.learner(dev, state, hyper, batch, case[3], images)


@pytest.mark.parametrize("images", [True, False], ids=["images", "f32"])
@pytest.mark.parametrize("case", R.FRESH_CASES + R.TRAINED_CASES, ids=_id)
def test_one_learn_step_against_f64(gpu_device, case, images):
    """One learn_batch from learn_ref.case(*case), every result against f64.

    No unit changes side: the pre-ReLU values of critic(s, a) and actor(s), formed from the saved x-hat and the incoming affine, are
    within margin / 3 = 1e-5 of the f64 ones (the batch keeps them 3e-5 from zero).
    Outputs: y, q, q_pi, dq_da within 2e-5 max(1, max |ref|) (tests/test_gpu_fused_net.py's forward bound); y[done] == r[done].  q_pi
    and dq_da are Q(s, mu(s)) in f64 on the critic this learn() left -- tied to f64 by the two checks below -- and dq_da of a row
    with a unit within 3e-5 of zero there is compared with the nearest of learn_ref.dq_da_choices.
    Gradients at both optimizer sites, every tensor: tol = max(3e-5 max |g64| + 1e-7, 3 e32), the first term test_learner's
    _check_grads bound, e32 the error of plain f32 torch on the same state against the same g64 (critic: Agent.learn_batch on an f32
    twin; actor: f32 autograd of the same sum_b c_b mu_b).  A row dropped or counted twice moves a tensor by ~1 / B of its scale.
    Optimizer arithmetic, every element of both nets: adam64 at the kernel's OWN gradient, the incoming p, m, v, target and step,
    and the hyperparameters as f32 (what the launches are given):
        |m - m64| <= 4 2^-24 (|beta1 m0| + |(1 - beta1) g'|)
        |v - v64| <= 6 2^-24 v64 + 2^-149
        |p - p64| <= ulp32(p64) + max(2^-19, (18 + 6 kappa) 2^-24) |p64 - p0|,  kappa = (|beta1 m0| + |(1 - beta1) g'|) / |m64|
        |target - soft64(target0, p)| <= 2 ulp32, with the kernel's own p
    Rounding count of the update term (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps)): three roundings that end in m (the fma of g',
    (1 - beta1) g', the fma of m) -- each relative to the LARGER of m's two terms, hence kappa times as large relative to m where
    beta1 m0 and (1 - beta1) g' cancel, which warmed moments do in a few percent of the elements -- and nine that do not: (1 -
    beta2) g', its product with g', the fma of v (together 1.5 after the root), sqrtf, bc2 and sqrtf(bc2), the division, + eps, m /
    denom, bc1, lr / bc1, the product.  The bound is twice the count, (18 + 6 kappa) 2^-24, and never below 2^-19 = 32 2^-24, which
    it is for kappa <= 2.3 (always, from zero moments); the last subtraction rounds p once more.
    Step count + 1; with images, each of the four fc2 images equals one packed from scratch, bit for bit (a target's over its forward
    planes only)."""
    state, hyper, batch, ref, _ = R.case(*case)
    K.against_f64(gpu_device, state, hyper, batch, ref, images=images, tag=_id(case))


def _results(fl):
    ag = fl.agent
    out = [p.detach().clone() for n in (ag.actor, ag.critic, ag.target_actor, ag.target_critic) for p in n.parameters()]
    return out + [t.clone() for t in (fl.actor.m, fl.actor.v, fl.critic.m, fl.critic.v, fl.actor.flat_grad, fl.critic.flat_grad,
                                      fl.q_pi, fl.dq_da, fl.step_dev)]


@pytest.mark.parametrize("case", R.PATH_CASES, ids=_id)
def test_learn_paths_agree_bitwise_at_every_batch(gpu_device, case):
    """Two learn() steps from the trained-scale state (step 999, learn_ref.TRAINED_HYPER), images on, four ways: learn_batch as it is;
    the actor tail in one launch; the optimizer in launches of its own (as after a gradient all-reduce); a PopulationLearner of two
    agents that both hold this state and draw this batch.  All four nets, both m and v, both flat gradients, q_pi, dq_da and the step
    count agree bit for bit.  With the tail no consumer gave up, the first ceil(B / 16) hint words hold the step and the rest -1."""
    import torch
    from ddpg_trucktrailer_amd.population import PopulationLearner
    dev = gpu_device
    B, step0 = case[0], case[3]
    state, hyper, _, _, _ = R.case(*case)
    runs = {}
    for how in ("plain", "tail", "separate"):
        _, fl, batch = _learner(dev, case, True)
        if how == "tail":
            fl.fuse_tail = True
        if how == "separate":
            fl.grad_sync_critic = fl.grad_sync_actor = lambda: None
        for _ in range(2):
            fl.learn_batch(*batch)
        torch.cuda.synchronize()
        assert fl.tail_gave_up() == 0 and int(fl.step_dev.item()) == step0 + 2
        if how == "tail":
            producers = math.ceil(B / 16)
            hints = fl.tail_words[:64].cpu()
            assert hints[:producers].tolist() == [step0 + 2] * producers and hints[producers:].eq(-1).all()
            rows = fl.tail_words[64:64 + 2 * B].cpu().view(B, 2)
            assert rows[:, 1].eq(step0 + 2).all() and torch.equal(rows[:, 0].contiguous().view(torch.float32), fl.dq_da.cpu())
            assert fl.tail_words[64 + 2 * B:].eq(-1).all()
        runs[how] = _results(fl)
    rings = [K.ring_with_batch(dev, B, batch) for _ in range(2)]
    agents = [R.load_agent(state, hyper, dev, torch.float32) for _ in range(2)]
    pop = PopulationLearner(agents, B, fc2_images=True, rings=[ring for ring, _ in rings], seeds=[seed for _, seed in rings])
    for fl in pop.learners:
        fl.import_from_optimizers()
    for _ in range(2):
        pop.learn(0)                 # (update 0 both times: the same key, the same draw)
    torch.cuda.synchronize()
    assert pop.tail_gave_up() == [0, 0]
    for ring, _ in rings:
        for got, want in zip(ring._batch_bufs(B)[:5], batch):
            assert torch.equal(got.view(-1), want.view(-1))
    runs["population 0"], runs["population 1"] = (_results(fl) for fl in pop.learners)
    assert all(torch.isfinite(x).all() for x in runs["plain"])
    for how, got in runs.items():
        assert len(got) == len(runs["plain"])
        for i, (x, y) in enumerate(zip(got, runs["plain"])):
            assert torch.equal(x, y), (how, B, i)
