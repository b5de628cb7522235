"""CPU: the loss shape (ddpg_trucktrailer_amd/loss_shape.py; include/ttenv.h: tt_loss_shape) without a GPU -- the f64 reference's own
inputs (tests/shape_ref.py), Agent(loss_shape=).learn_batch in f32 against it, the off case against a plain Agent bit for bit, every
refusal in Python and every refusal of the three shaped entry points on made-up addresses."""
import ctypes as C
import hashlib

import pytest
import torch

import fake_args as F
import learn_ref as R
import shape_ref as S

_CASE = S.F64_CASES[1]          # B = 33, fresh state


def _id(case):
    return "B{}-x{:g}".format(case[0], case[1])


# ---- the inputs: delta splits the batch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.F64_CASES + S.OFF_CASES + [S.PATH_CASE], ids=_id)
def test_delta_is_the_median_td_error_and_splits_the_batch(case):
    """delta = median |q - y| of the f64 reference; at least a quarter of the rows lie strictly on each side, so both branches of the
    clamp carry rows.  (A one-row batch has its row ON delta, where the clamp is continuous: nothing to split.)"""
    B = case[0]
    _, _, _, ref, share = R.case(*case)
    delta = S.delta_of(ref)
    below, above = S.sides(ref, delta)
    print(f"B {B}: delta {delta:.6g}, {below} rows below, {above} above, discarded {share:.4f}")
    assert delta > 0 and share <= R.MAX_DISCARD
    if B >= 4:
        assert below >= B / 4 and above >= B / 4, (below, above)


def test_the_saturated_state_saturates_some_rows_on_both_sides_and_keeps_the_batch_clean():
    """shape_ref.saturated_state on the B = 33 case, in f64: at least two rows beyond +9.3 and two beyond -9.3 (tanh is exactly +-1.0f
    in f32 from 9.02 on), at least two within 8.7, none between; every pre-ReLU value of actor(s) and critic(s, a) is the case's own."""
    state, hyper, batch, ref, _ = R.case(*_CASE)
    out = R.ref_step(S.saturated_state(state, batch), batch, hyper, c=0.01)
    pre = out["pre"]
    counts = (int((pre > 9.3).sum()), int((pre < -9.3).sum()), int((pre.abs() < 8.7).sum()))
    print("rows beyond +9.3, beyond -9.3, within 8.7:", counts)
    assert min(counts) >= 2 and sum(counts) == _CASE[0]
    for key in ("critic", "actor"):
        for x, y in zip(out["z"][key], ref["z"][key]):
            assert torch.equal(x, y)
    assert out["margin"].min().item() >= R.MARGIN


def test_shape_ref_without_a_shape_is_learn_refs_step_exactly():
    state, hyper, batch, ref, _ = R.case(*_CASE)
    out = R.ref_step(state, batch, hyper)
    for k in ("y", "q", "q_pi", "dq_da", "mu"):
        assert torch.equal(out[k], ref[k]), k
    for name in R.NETS:
        for k, v in ref["nets"][name].items():
            assert torch.equal(out["nets"][name][k], v), (name, k)
    assert torch.equal(torch.tanh(out["pre"]), out["mu"])          # (pre is the value in front of tanh)


def test_shape_ref_gradients_are_the_stated_ones():
    """d(huber)/dq = clamp(q - y, -delta, delta) / B -- half the MSE gradient inside the zone -- and the penalty adds 2 c pre / B at
    the head's pre-activation: checked on the head's bias gradients, which are the sums of exactly those row terms."""
    state, hyper, batch, ref, _ = R.case(*_CASE)
    B = _CASE[0]
    delta = S.delta_of(ref)
    out = R.ref_step(state, batch, hyper, delta=delta, c=0.5)
    e = ref["q"] - ref["y"]
    want = e.clamp(-delta, delta).sum() / B
    assert abs(out["grads"]["critic"]["q.bias"].item() - want.item()) <= 1e-12 * max(1.0, abs(want.item()))
    inside = e.abs() < delta
    assert torch.allclose(e.clamp(-delta, delta)[inside] / B, 0.5 * (2.0 / B) * e[inside], rtol=1e-15, atol=0)
    plain = R.ref_step(state, batch, hyper, delta=delta, c=0.0)
    extra = out["grads"]["actor"]["mu.bias"] - plain["grads"]["actor"]["mu.bias"]
    pen = (2 * 0.5 * out["pre"] / B).sum()
    assert abs(extra.item() - pen.item()) <= 1e-12 * max(1.0, abs(pen.item()))
    assert out["actor_loss"] > plain["actor_loss"] and out["critic_loss"] == plain["critic_loss"]


# ---- Agent(loss_shape=) in f32 on the CPU against f64 ---------------------------------------------------------------------
@pytest.mark.parametrize("huber, c", S.SHAPES, ids=lambda x: str(x))
def test_agent_learn_batch_in_f32_against_shape_ref(huber, c):
    """One Agent(loss_shape=).learn_batch in f32 on the CPU against shape_ref.ref_step, with the bounds tests/test_learn_ref.py holds
    learn_ref to against the reference's fixture: gradients at both optimizer sites within 3e-5 max |g64| + 1e-7 per tensor
    (test_learner._check_grads), both losses within 1e-5 relative.  The optimizers behind those gradients are torch's own, which no
    option touches: from zero moments Adam's step is lr g / (|g| + eps), which turns a gradient error of 3e-9 into 3e-6 of a parameter
    where |g| is near eps, so the nets afterwards are not held to the f64 nets here."""
    from ddpg_trucktrailer_amd.loss_shape import LossShape
    state, hyper, batch, delta, ref = S.shaped(_CASE, huber, c)
    agent = R.load_agent(state, hyper, torch.device("cpu"), torch.float32)
    agent.loss_shape = LossShape(delta, c)
    seen = {}
    for key in ("critic", "actor"):
        net = getattr(agent, key)

        def step(*a, _net=net, _key=key, _orig=net.optimizer.step, **kw):
            seen[_key] = {k: p.grad.clone() for k, p in _net.named_parameters()}
            return _orig(*a, **kw)
        net.optimizer.step = step
    s, a, r, s2, d = batch
    agent.learn_batch(s, a, r, s2, d.bool())
    worst = {}
    for key in ("critic", "actor"):
        for k, want in ref["grads"][key].items():
            tol = 3e-5 * want.abs().max().item() + 1e-7
            err = (seen[key][k].double() - want).abs().max().item()
            worst["grad " + key] = max(worst.get("grad " + key, 0.0), err / tol)
            assert err <= tol, (key, k, err, tol)
    for name, got, want in (("critic_loss", agent.last_critic_loss.item(), ref["critic_loss"]),
                            ("actor_loss", agent.last_actor_loss.item(), ref["actor_loss"])):
        worst[name] = abs(got - want) / (1e-5 * max(1e-1, abs(want)))
        assert worst[name] <= 1.0, (name, got, want)
    for key in ("critic", "actor"):                        # both optimizers stepped, once
        for k, pp in getattr(agent, key).named_parameters():
            assert not torch.equal(pp.detach(), state["nets"][key][k]), (key, k)
            assert float(getattr(agent, key).optimizer.state[pp]["step"]) == state["step"] + 1
    print(f"RATIOS huber {huber} c {c}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def _digest(agent):
    h = hashlib.sha256()
    for name in R.NETS:
        for v in getattr(agent, name).state_dict().values():
            h.update(v.detach().contiguous().numpy().tobytes())
    for name in ("actor", "critic"):
        net = getattr(agent, name)
        for p in net.parameters():
            st = net.optimizer.state[p]
            h.update(st["exp_avg"].contiguous().numpy().tobytes())
            h.update(st["exp_avg_sq"].contiguous().numpy().tobytes())
    return h.hexdigest()


def test_an_empty_shape_leaves_the_plain_agents_bits():
    """Agent(loss_shape=LossShape()) -- both options off -- after three learn_batch calls: the SHA-256 over the four nets and both
    optimizers' moments is the plain Agent's."""
    from ddpg_trucktrailer_amd.loss_shape import LossShape
    state, hyper, batch, _, _ = R.case(*_CASE)
    s, a, r, s2, d = batch
    digests = []
    for shape in (None, LossShape()):
        agent = R.load_agent(state, hyper, torch.device("cpu"), torch.float32)
        agent.loss_shape = shape
        for _ in range(3):
            agent.learn_batch(s, a, r, s2, d.bool())
        digests.append(_digest(agent))
    assert digests[0] == digests[1]
    agent = R.load_agent(state, hyper, torch.device("cpu"), torch.float32)
    agent.loss_shape = LossShape(None, 0.5)
    for _ in range(3):
        agent.learn_batch(s, a, r, s2, d.bool())
    assert _digest(agent) != digests[0]


# ---- refusals in Python -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, word", [(dict(huber_delta=0.0), "huber_delta"), (dict(huber_delta=-1.0), "huber_delta"),
                                      (dict(huber_delta=float("nan")), "huber_delta"), (dict(huber_delta=float("inf")), "huber_delta"),
                                      (dict(huber_delta=True), "huber_delta"), (dict(huber_delta="1"), "huber_delta"),
                                      (dict(pre_penalty=-0.1), "pre_penalty"), (dict(pre_penalty=float("nan")), "pre_penalty"),
                                      (dict(pre_penalty=float("inf")), "pre_penalty"), (dict(pre_penalty=None), "pre_penalty"),
                                      (dict(pre_penalty=True), "pre_penalty")])
def test_loss_shape_refuses(kw, word):
    from ddpg_trucktrailer_amd.loss_shape import LossShape
    with pytest.raises(ValueError, match=word):
        LossShape(**kw)


def test_loss_shape_defaults_equality_and_launch_constants():
    from ddpg_trucktrailer_amd.loss_shape import LossShape
    assert LossShape().as_tuple() == (None, 0.0) and LossShape() == LossShape(None, 0) and LossShape(2, 0.5) != LossShape(2, 0.25)
    assert repr(LossShape(2, 0.5)) == "LossShape(huber_delta=2.0, pre_penalty=0.5)"
    assert LossShape.from_tuple(LossShape(2, 0.5).as_tuple()) == LossShape(2, 0.5)
    assert LossShape().critic_scale(256) == 2.0 / 256 and LossShape(3.0).critic_scale(256) == 1.0 / 256
    assert LossShape().delta_arg() == 0.0 and LossShape(3.0).delta_arg() == 3.0
    assert LossShape(None, 0.01).pre_scale(33) == 2 * 0.01 / 33


@pytest.mark.parametrize("kw", [dict(td3="cfg"), dict(population=True), dict(data_parallel=True), dict(force_dp=True)],
                         ids=lambda kw: next(iter(kw)))
def test_check_loss_shape_refuses(kw):
    from ddpg_trucktrailer_amd.loss_shape import LossShape, check_loss_shape
    with pytest.raises(ValueError, match="loss_shape"):
        check_loss_shape(LossShape(1.0, 0.1), **kw)


def test_check_loss_shape_accepts_the_supported_loop_and_refuses_a_non_shape():
    from ddpg_trucktrailer_amd.loss_shape import LossShape, check_loss_shape
    shape = LossShape(1.0, 0.1)
    assert check_loss_shape(shape) is shape and check_loss_shape(shape, td3=None, population=False, data_parallel=False) is shape
    with pytest.raises(ValueError, match="loss_shape"):
        check_loss_shape((1.0, 0.1))


def test_agent_and_population_refuse_a_loss_shape_where_it_has_no_kernels():
    from ddpg_trucktrailer_amd.agent import Agent
    from ddpg_trucktrailer_amd.loss_shape import LossShape
    from ddpg_trucktrailer_amd.population import PopulationLearner, PopulationRollout
    from ddpg_trucktrailer_amd.td3 import TD3Config
    kw = dict(alpha=1e-4, beta=1e-3, input_dims=(23,), tau=1e-3, n_actions=1, batch_size=4, device="cpu", replay=False)
    with pytest.raises(ValueError, match="loss_shape"):
        Agent(td3=TD3Config(), loss_shape=LossShape(1.0), **kw)
    with pytest.raises(ValueError, match="loss_shape"):
        Agent(loss_shape=(1.0, 0.0), **kw)
    agent = Agent(loss_shape=LossShape(1.0, 0.1), **kw)
    assert agent.loss_shape == LossShape(1.0, 0.1)
    with pytest.raises(ValueError, match="loss_shape"):
        PopulationRollout(64, [1, 2], loss_shape=LossShape(1.0))
    with pytest.raises(ValueError, match="loss_shape"):
        PopulationLearner([agent], 4, rings=[None], seeds=[1])
    with pytest.raises(ValueError, match="loss_shape"):
        PopulationLearner([], 4, loss_shape=LossShape(None, 0.1))


# ---- refusals of the three entry points, before any HIP call ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib as L
    return L


_ENTRY = dict(rows="tt_mlp_backward_rows_pair_shaped", weights="tt_mlp_backward_weights_shaped", tail_="tt_mlp_actor_tail_shaped")


_set = F.set_field


_COMMON = [("shape is NULL", None, False),
           ("huber_delta", _set("shape", "huber_delta", -1.0), True), ("huber_delta", _set("shape", "huber_delta", float("nan")), True),
           ("huber_delta", _set("shape", "huber_delta", float("inf")), True),
           ("pre_scale", _set("shape", "pre_scale", -0.5), True), ("pre_scale", _set("shape", "pre_scale", float("nan")), True),
           ("pre_scale", _set("shape", "pre_scale", float("inf")), True),
           ("pre is NULL", _set("shape", "pre", None), True)]
_ROWS, _WEIGHTS, _TAIL = ([(w, spoil, True) for w, spoil in rs] for rs in (F.ROWS, F.WEIGHTS, F.TAIL))
_REFUSALS = [(e, *r) for e, rs in (("rows", _COMMON + _ROWS), ("weights", _COMMON + _WEIGHTS), ("tail_", _COMMON + _TAIL)) for r in rs]


@pytest.mark.parametrize("entry, word, spoil, with_shape", _REFUSALS,
                         ids=[f"{e}-{i}-{w.replace(' ', '_')}" for i, (e, w, _, _) in enumerate(_REFUSALS)])
def test_shaped_entry_points_check_their_arguments_before_any_hip_call(lib, entry, word, spoil, with_shape):
    """TT_EINVAL and a message that starts with the entry point's name and names the argument, for one spoiled argument at a time."""
    L = lib
    f = F.Fake(L, 256, "shaped")
    if spoil is not None:
        spoil(f)
    f.with_shape = with_shape
    rc, msg = getattr(f, entry)(), f.last_error()
    assert rc == L.TT_EINVAL, (rc, msg)
    assert msg.startswith(_ENTRY[entry] + ":") and word in msg, msg


def test_the_library_exports_the_shaped_entry_points_and_stays_at_version_3(lib):
    L = lib
    assert L.load().tt_version() == 3
    for name in _ENTRY.values():
        assert name in L.EXPORTS and hasattr(L.load(), name)
    assert C.sizeof(L.TTLossShape) == 16


def test_the_new_kernels_are_in_the_library_within_the_budgets_of_the_launches_they_stand_in_for(lib):
    """The three kernels exist (a missing kernel is an error, not a fall-back); tests/test_kernel_resources.py's budgets hold for them
    by their names, restated here for the three alone."""
    from ddpg_trucktrailer_amd import kernel_resources as kr
    ks = kr.kernels()
    for part, waves in (("k_bwd_rows_pair_shaped", 2), ("k_bwd_weights_shaped", 3), ("k_actor_tail_shaped", 2)):
        found = kr.find(ks, part)
        assert len(found) == 1, part
        (n, v), = found.items()
        assert kr.waves_per_simd(v["vgpr"]) >= waves and v["scratch"] == 0 and v["vgpr_spills"] == 0, (n, v)
        if waves == 3:
            assert v["vgpr"] <= 168 and 3 * v["lds"] <= 160 * 1024, (n, v)
