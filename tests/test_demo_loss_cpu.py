"""CPU: the demonstration loss (ddpg_trucktrailer_amd/demo_loss.py; include/ttenv.h: tt_demo_loss) without a GPU -- the f64 reference's
own inputs (tests/demo_ref.py), Agent(demo_loss=).learn_batch in f32 against it, the off case against a plain Agent bit for bit, every
refusal in Python, every refusal of the two entry points on made-up addresses, and the demonstration file's round trip."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

import demo_ref as D
import fake_args as F
import learn_ref as R
import shape_ref as S

_CASE = D.F64_CASES[1]          # B = 33, fresh state
_SHAPED_CASES = [D.PATH_CASE, D.OFF_CASES[1]]      # the cases the tests run with a LossShape: B = 33 and 257, trained scale


def _id(case):
    return "B{}-x{:g}".format(case[0], case[1])


# ---- the inputs: the filter splits the demonstration rows ---------------------------------------------------------------------
@pytest.mark.parametrize("case", D.F64_CASES + D.OFF_CASES + [D.PATH_CASE], ids=_id)
def test_the_filter_splits_the_demonstration_rows_and_few_are_undecided(case):
    """demo_ref.demo_mask names every third row.  In the f64 reference -- q from the critic before its step, q_pi through the updated
    one -- at most MAX_DISCARD of those rows lie within FILTER_MARGIN of the filter's boundary, and from 33 rows on each side of the
    filter holds at least one eighth of them (demo_ref.check_inputs)."""
    B = case[0]
    state, hyper, batch, _, _ = R.case(*case)
    out = D.ref_step(state, batch, hyper, lam=0.1, q_filter=True)
    mask = D.demo_mask(B)
    assert torch.equal(out["demo"], mask) and bool(mask[0]) and int(mask.sum()) == (B + 2) // 3
    above, below, und, n = D.check_inputs(out["q"], out["q_pi"], mask)
    print(f"B {B}: {n} demonstration rows, {above} with q > q_pi, {below} without, {und} undecided; all rows: "
          f"{int((out['q'] > out['q_pi']).sum())} of {B} with q > q_pi")
    assert torch.equal(out["applied"], mask & (out["q"] > out["q_pi"])) and torch.equal(out["code"], D.codes(mask, out["applied"]))
    assert set(out["code"][~mask].tolist()) <= {0} and set(out["code"][mask].tolist()) <= {1, 2}


@pytest.mark.parametrize("case", _SHAPED_CASES, ids=_id)
def test_the_filter_splits_the_demonstration_rows_with_a_loss_shape_too(case):
    """The same conditions for the cases the tests run with LossShape(delta, 0.01), whose critic step is another one."""
    _, _, _, _, out = D.demo_case(case, 0.1, True, True, 0.01)
    above, below, und, n = D.check_inputs(out["q"], out["q_pi"], out["demo"])
    print(f"B {case[0]} with LossShape(delta, 0.01): {n} demonstration rows, {above} with q > q_pi, {und} undecided")


def test_the_zero_action_case_has_no_dq_da_and_rows_on_both_sides():
    """demo_ref.zero_action_case at B = 257, in f64: dQ/da through the UPDATED critic is exactly 0 on every row, the actor's gradient
    without the option is exactly zero, and the filter leaves demonstration rows on both sides, none undecided."""
    state, hyper, batch = D.zero_action_case(D.F64_CASES[2])
    plain = D.ref_step(state, batch, hyper, lam=0.0)
    assert float(plain["dq_da"].abs().max()) == 0.0
    assert all(float(g.abs().max()) == 0.0 for g in plain["grads"]["actor"].values())
    out = D.ref_step(state, batch, hyper, lam=0.1)
    above, below, und, n = D.check_inputs(out["q"], out["q_pi"], out["demo"])
    assert und == 0 and above >= 8 and below >= 8
    assert max(float(g.abs().max()) for g in out["grads"]["actor"].values()) > 1e-4


def test_demo_ref_without_the_term_is_shape_refs_step_exactly():
    state, hyper, batch, ref, _ = R.case(*_CASE)
    delta = S.delta_of(ref)
    for lam, mask in ((0.0, None), (0.5, torch.zeros(_CASE[0], dtype=torch.bool))):
        out, want = D.ref_step(state, batch, hyper, delta=delta, c=0.01, lam=lam, mask=mask), R.ref_step(state, batch, hyper, delta=delta, c=0.01)
        for k in ("y", "q", "q_pi", "dq_da", "mu", "pre"):
            assert torch.equal(out[k], want[k]), k
        for name in R.NETS:
            for k, v in want["nets"][name].items():
                assert torch.equal(out["nets"][name][k], v), (name, k)


def test_demo_ref_gradient_is_the_stated_one():
    """The term adds (2 lambda / B) m_b (mu_b - a_b)(1 - mu_b^2) at the head's pre-activation of row b: checked on the head's bias
    gradient, the sum of exactly those row terms; and it is the row factor of dq_eff = dQ/da - 2 lambda m (mu - a)."""
    state, hyper, batch, _, _ = R.case(*_CASE)
    B, lam = _CASE[0], 0.7
    out, plain = D.ref_step(state, batch, hyper, lam=lam), D.ref_step(state, batch, hyper, lam=0.0)
    mu, a, m = out["mu"], batch[1].double().view(-1), out["applied"].double()
    extra = out["grads"]["actor"]["mu.bias"] - plain["grads"]["actor"]["mu.bias"]
    want = (2 * lam / B * m * (mu - a) * (1 - mu * mu)).sum()
    assert abs(extra.item() - want.item()) <= 1e-12 * max(1.0, abs(want.item()))
    total = (-(1.0 / B) * out["dq_eff"] * (1 - mu * mu)).sum()
    assert abs(out["grads"]["actor"]["mu.bias"].item() - total.item()) <= 1e-12 * max(1.0, abs(total.item()))
    assert out["bc_loss"] > 0 and abs(out["actor_loss"] - plain["actor_loss"] - out["bc_loss"]) <= 1e-12
    assert torch.equal(out["dq_eff"][~out["applied"]], out["dq_da"][~out["applied"]])


# ---- Agent(demo_loss=) in f32 on the CPU against f64 ---------------------------------------------------------------------------
_AGENT = [(lam, qf, False, 0.0) for lam, qf in D.DEMOS] + [(0.1, True, True, 0.01)]


@pytest.mark.parametrize("lam, q_filter, huber, c", _AGENT, ids=[f"lam{l:g}-{'filter' if q else 'all'}{'-shape' if h else ''}" for l, q, h, c in _AGENT])
def test_agent_learn_batch_in_f32_against_demo_ref(lam, q_filter, huber, c):
    """One Agent(demo_loss=).learn_batch(demo_rows=) in f32 on the CPU against demo_ref.ref_step with test_loss_shape_cpu.py's bounds:
    gradients at both optimizer sites within 3e-5 max |g64| + 1e-7 per tensor, both losses within 1e-5 relative; with and without the
    filter, and with a LossShape (there from the trained-scale state: with the Huber step the fresh B = 33 state leaves one demonstration
    row above the filter, fewer than the inputs' condition asks for).  The applied rows are the reference's except on undecided rows
    (none in these cases)."""
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    from ddpg_trucktrailer_amd.loss_shape import LossShape
    state, hyper, batch, delta, ref = D.demo_case(_SHAPED_CASES[0] if huber else _CASE, lam, q_filter, huber, c)
    D.check_inputs(ref["q"], ref["q_pi"], ref["demo"])
    agent = R.load_agent(state, hyper, torch.device("cpu"), torch.float32)
    agent.demo_loss = DemoLoss(lam, q_filter)
    if huber or c:
        agent.loss_shape = LossShape(delta, c)
    seen = {}
    for key in ("critic", "actor"):
        net = getattr(agent, key)

        def step(*a, _net=net, _key=key, _orig=net.optimizer.step, **kw):
            seen[_key] = {k: p.grad.clone() for k, p in _net.named_parameters()}
            return _orig(*a, **kw)
        net.optimizer.step = step
    s, a, r, s2, d = batch
    agent.learn_batch(s, a, r, s2, d.bool(), demo_rows=ref["demo"])
    und = D.filter_of(ref["q"], ref["q_pi"], ref["demo"])["undecided"]
    assert int(und.sum()) == 0 and torch.equal(agent.last_demo_mask, ref["applied"])
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
    print(f"RATIOS lam {lam} filter {q_filter} huber {huber} c {c}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


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


def test_no_demonstration_row_leaves_the_plain_agents_bits():
    """Agent(demo_loss=) with an all-false demo_rows (and with demo_rows=None) after three learn_batch calls: the SHA-256 over the
    four nets and both optimizers' moments is the plain Agent's; with demonstration rows it is another."""
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    state, hyper, batch, _, _ = R.case(*_CASE)
    s, a, r, s2, d = batch
    B = _CASE[0]
    digests = []
    for demo, rows in ((None, None), (DemoLoss(10.0), torch.zeros(B, dtype=torch.bool)), (DemoLoss(10.0), None),
                       (DemoLoss(10.0, False), D.demo_mask(B))):
        agent = R.load_agent(state, hyper, torch.device("cpu"), torch.float32)
        agent.demo_loss = demo
        for _ in range(3):
            agent.learn_batch(s, a, r, s2, d.bool(), **({} if demo is None else dict(demo_rows=rows)))
        digests.append(_digest(agent))
    assert digests[0] == digests[1] == digests[2] and digests[3] != digests[0]
    plain = R.load_agent(state, hyper, torch.device("cpu"), torch.float32)
    with pytest.raises(ValueError, match="demo_loss"):
        plain.learn_batch(s, a, r, s2, d.bool(), demo_rows=D.demo_mask(B))


# ---- refusals in Python ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [(0.0,), (-1.0,), (float("nan"),), (float("inf"),), (True,), ("1",), (None,), (1.0, None), (1.0, "yes"),
                                  (1.0, 2)], ids=str)
def test_demo_loss_refuses(args):
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    with pytest.raises(ValueError, match="demo_loss"):
        DemoLoss(*args)


def test_demo_loss_defaults_equality_and_launch_constant():
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    assert DemoLoss(1).as_tuple() == (1.0, True) and DemoLoss(1) == DemoLoss(1.0, True) and DemoLoss(1) != DemoLoss(1, False)
    assert DemoLoss(0.5) != DemoLoss(0.25) and hash(DemoLoss(2)) == hash(DemoLoss(2.0))
    assert repr(DemoLoss(0.5, False)) == "DemoLoss(bc_weight=0.5, q_filter=False)"
    assert DemoLoss.from_tuple(DemoLoss(0.5, False).as_tuple()) == DemoLoss(0.5, False)
    assert DemoLoss.from_tuple([0.5, True]) == DemoLoss(0.5)
    assert DemoLoss(0.1).k() == 2.0 * 0.1 and isinstance(DemoLoss(0.1).k(), float)


@pytest.mark.parametrize("kw", [dict(td3="cfg"), dict(population=True), dict(data_parallel=True), dict(force_dp=True), dict(n_step=3)],
                         ids=lambda kw: next(iter(kw)))
def test_check_demo_loss_refuses(kw):
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss, check_demo_loss
    with pytest.raises(ValueError, match="demo_loss"):
        check_demo_loss(DemoLoss(1.0), **kw)


def test_check_demo_loss_accepts_the_supported_loop_and_refuses_a_non_demo_loss():
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss, check_demo_loss
    demo = DemoLoss(1.0)
    assert check_demo_loss(demo) is demo
    assert check_demo_loss(demo, td3=None, population=False, data_parallel=False, force_dp=False, n_step=1) is demo
    with pytest.raises(ValueError, match="demo_loss"):
        check_demo_loss((1.0, True))


def test_agent_and_population_refuse_a_demo_loss_where_it_has_no_kernels():
    from ddpg_trucktrailer_amd.agent import Agent
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    from ddpg_trucktrailer_amd.population import PopulationLearner, PopulationRollout
    from ddpg_trucktrailer_amd.td3 import TD3Config
    kw = dict(alpha=1e-4, beta=1e-3, input_dims=(23,), tau=1e-3, n_actions=1, batch_size=4, device="cpu", replay=False)
    with pytest.raises(ValueError, match="demo_loss"):
        Agent(td3=TD3Config(), demo_loss=DemoLoss(1.0), **kw)
    with pytest.raises(ValueError, match="demo_loss"):
        Agent(demo_loss=(1.0, True), **kw)
    agent = Agent(demo_loss=DemoLoss(1.0, False), **kw)
    assert agent.demo_loss == DemoLoss(1.0, False)
    with pytest.raises(ValueError, match="demo_loss"):
        PopulationRollout(64, [1, 2], demo_loss=DemoLoss(1.0))
    with pytest.raises(ValueError, match="demo_loss"):
        PopulationLearner([agent], 4, rings=[None], seeds=[1])
    with pytest.raises(ValueError, match="demo_loss"):
        PopulationLearner([], 4, demo_loss=DemoLoss(0.1))


# ---- refusals of the two entry points, before any HIP call ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib as L
    return L


_ENTRY = dict(fwd="tt_mlp_forward_save_demo", tail_="tt_mlp_actor_tail_demo")


_set = F.set_field


_COMMON = [("demo is NULL", None, False),
           ("demo->k", _set("demo", "k", -0.5), True), ("demo->k", _set("demo", "k", float("nan")), True),
           ("demo->k", _set("demo", "k", float("inf")), True),
           ("NULL", _set("demo", "a", None), True), ("NULL", _set("demo", "idx", None), True), ("NULL", _set("demo", "dq_eff", None), True),
           ("NULL", _set("demo", "code", None), True), ("demo->q is NULL", _set("demo", "q", None), True),
           ("dq_eff is dq_da", lambda f: setattr(f.demo, "dq_eff", f.dq_da), True),
           ("dq_da is NULL", lambda f: setattr(f, "dq_da", None), True)]
_FWD = [("actor", lambda f: setattr(f, "fwd_critic", 0), True), ("n = -1", lambda f: setattr(f, "B", -1), True),
        ("obs", lambda f: setattr(f, "obs", None), True), ("action", lambda f: setattr(f, "mu", None), True),
        ("out", lambda f: setattr(f, "q_pi", None), True), ("weights", _set("critic", "wa", None), True),
        ("weights", _set("critic", "fc2_dims", 301), True)]
_TAIL = [("n = 0", lambda f: setattr(f, "B", 0), True), ("n = 1025", lambda f: setattr(f, "B", 1025), True),
         ("obs", lambda f: setattr(f, "obs", None), True), ("mu", lambda f: setattr(f, "mu", None), True),
         ("q_out", lambda f: setattr(f, "q_pi", None), True),
         ("critic", _set("critic", "wa", None), True), ("saved", _set("saved_a", "h1", None), True),
         ("workspace", _set("ws_a", "dy1", None), True), ("grads", _set("grads", "w1", None), True),
         ("count = 0", lambda f: setattr(f, "count", 0), True), ("optimizer step", lambda f: f.tables[0].__setitem__(9, None), True),
         ("tail_words", lambda f: setattr(f, "tail", None), True),
         ("huber_delta", _set("shape", "huber_delta", -1.0), True), ("pre_scale", _set("shape", "pre_scale", float("nan")), True),
         ("pre is NULL", _set("shape", "pre", None), True)]
_REFUSALS = [(e, *r) for e, rs in (("fwd", _COMMON + _FWD), ("tail_", _COMMON + _TAIL)) for r in rs]


@pytest.mark.parametrize("entry, word, spoil, with_demo", _REFUSALS,
                         ids=[f"{e}-{i}-{w.replace(' ', '_').replace('>', '')}" for i, (e, w, _, _) in enumerate(_REFUSALS)])
def test_demo_entry_points_check_their_arguments_before_any_hip_call(lib, entry, word, spoil, with_demo):
    """TT_EINVAL and a message that starts with the entry point's name and names the argument, for one spoiled argument at a time."""
    L = lib
    f = F.Fake(L, 256, "demo")
    if spoil is not None:
        spoil(f)
    f.with_demo = with_demo
    rc, msg = getattr(f, entry)(), f.last_error()
    assert rc == L.TT_EINVAL, (rc, msg)
    assert msg.startswith(_ENTRY[entry] + ":") and word in msg, msg


def test_q_may_be_null_without_the_filter_and_the_shape_may_be_null(lib):
    """q NULL is refused only with q_filter; a NULL shape is allowed in the tail (the refusal then met is the next spoiled argument's)."""
    L = lib
    for entry in ("fwd", "tail_"):
        f = F.Fake(L, 256, "demo")
        f.demo.q, f.demo.q_filter, f.with_shape = None, 0, False
        f.obs = None
        rc, msg = getattr(f, entry)(), f.last_error()
        assert rc == L.TT_EINVAL and msg.startswith(_ENTRY[entry] + ":") and "obs" in msg and "demo->q" not in msg, msg


def test_the_library_exports_the_demo_entry_points_and_stays_at_version_3(lib):
    L = lib
    assert L.load().tt_version() == 3
    for name in _ENTRY.values():
        assert name in L.EXPORTS and hasattr(L.load(), name)
    assert C.sizeof(L.TTDemoLoss) == 48


def test_the_new_kernels_are_in_the_library_within_the_budgets_of_the_launches_they_stand_in_for(lib):
    """The kernels exist (a missing kernel is an error, not a fall-back): k_fwd_small_demo and k_actor_tail_demo for a learner with and
    without a LossShape; the row-kernel budget -- two waves per SIMD, no scratch, no spills -- and no more registers or LDS than the
    kernels they stand in for."""
    from ddpg_trucktrailer_amd import kernel_resources as kr
    ks = kr.kernels()
    for part, count, old in (("k_fwd_small_demo", 1, "k_fwd_smallILb1"), ("k_actor_tail_demo", 2, "k_actor_tail_shaped")):
        found = kr.find(ks, part)
        assert len(found) == count, (part, list(found))
        (_, was), = kr.find(ks, old).items()
        for n, v in found.items():
            assert kr.waves_per_simd(v["vgpr"]) >= 2 and v["scratch"] == 0 and v["vgpr_spills"] == 0, (n, v)
            assert v["vgpr"] <= was["vgpr"] and v["lds"] == was["lds"], (n, v, was)


# ---- the demonstration file --------------------------------------------------------------------------------------------------------
def test_transitions_round_trip_through_an_npz_file(tmp_path):
    from ddpg_trucktrailer_amd import expert
    rng = np.random.RandomState(3)
    episodes = [[(rng.randn(23), rng.uniform(-1, 1, 1), float(rng.randn()), rng.randn(23), bool(t == 4)) for t in range(5)] for _ in range(3)]
    arrays = expert.transitions_to_arrays(episodes)
    path = str(tmp_path / "demos.npz")
    assert expert.save_transitions_npz(path, *arrays) == 15
    back = expert.load_transitions_npz(path)
    assert len(back) == 5
    for x, y in zip(arrays, back):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
    assert back[1].shape == (15, 1) and back[4].dtype == np.bool_
    # an action given as [k] is stored as [k, 1]; a file without one of the five arrays, or with ragged shapes, is refused
    expert.save_transitions_npz(path, arrays[0], arrays[1][:, 0], *arrays[2:])
    assert np.array_equal(expert.load_transitions_npz(path)[1], arrays[1])
    np.savez(str(tmp_path / "short.npz"), obs=arrays[0], act=arrays[1], rew=arrays[2], obs2=arrays[3])
    with pytest.raises(ValueError, match="done"):
        expert.load_transitions_npz(str(tmp_path / "short.npz"))
    with pytest.raises(ValueError, match="shapes"):
        expert.save_transitions_npz(path, arrays[0], arrays[1], arrays[2], arrays[3][:, :5], arrays[4])
    np.savez(str(tmp_path / "ragged.npz"), obs=arrays[0], act=arrays[1], rew=arrays[2][:4], obs2=arrays[3], done=arrays[4])
    with pytest.raises(ValueError, match="shapes"):
        expert.load_transitions_npz(str(tmp_path / "ragged.npz"))
