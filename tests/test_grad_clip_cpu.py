"""CPU: gradient-norm clipping (ddpg_trucktrailer_amd/grad_clip.py; include/ttenv.h: tt_grad_clip) without a GPU -- the f64
reference's own inputs (tests/clip_ref.py), Agent(grad_clip=).learn_batch in f32 against it, an inactive clip against a plain Agent
bit for bit, every refusal in Python, every refusal of the entry point on made-up addresses, the struct's layout and the two new
kernels' resource rows."""
import ctypes as C
import hashlib
import math

import pytest
import torch

import clip_ref as K
import fake_args as F
import learn_ref as R

_CASE = K.FRESH_CASES[1]          # B = 33, fresh state
_ENTRY = "tt_adam_soft_update_clipped"


def _id(case):
    return "B{}-x{:g}".format(case[0], case[1])


# ---- the inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.CASES, ids=_id)
def test_the_cases_norms_are_not_zero_and_the_factors_decide_the_side(case):
    """The f64 norms of every case (3.5 to 40 for the critic, 0.035 to 0.28 for the actor behind the clipped critic, at the time of writing; printed) are far
    from zero, so 0.5 x norm gives coef = 0.5 / (1 + 1e-6 / norm) in (0.49998, 0.5) and 2 x norm gives exactly 1; the unclipped
    gradients of a clipped step are learn_ref's (the critic's) and the batch stays clean."""
    state, hyper, batch, ref, share = R.case(*case)
    _, _, _, (max_c, max_a), out = K.clipped(case, K.BOTH)
    print(f"B {case[0]} x{case[1]:g}: |g| critic {out['norm']['critic']:.6g} actor {out['norm']['actor']:.6g}, coef {out['coef']}")
    assert out["norm"]["critic"] > 1e-2 and out["norm"]["actor"] > 1e-3 and share <= R.MAX_DISCARD
    for key in ("critic", "actor"):
        assert 0.4999 < out["coef"][key] < 0.5
    for k, g in ref["grads"]["critic"].items():
        assert torch.equal(out["grads"]["critic"][k], g)
    assert out["margin"].min().item() >= R.MARGIN
    _, _, _, _, off = K.clipped(case, (K.INACTIVE, K.INACTIVE))
    assert off["coef"] == dict(critic=1.0, actor=1.0)
    for name in R.NETS:                      # an inactive clip in f64 is the plain step
        for k, v in ref["nets"][name].items():
            assert torch.equal(off["nets"][name][k], v), (name, k)


# ---- Agent(grad_clip=) in f32 on the CPU against f64 ------------------------------------------------------------------------------
def _agent(state, hyper, clip):
    agent = R.load_agent(state, hyper, torch.device("cpu"), torch.float32)
    agent.grad_clip = clip
    return agent


@pytest.mark.parametrize("factors", [K.BOTH, K.CRITIC_ONLY, K.ACTOR_ONLY, (K.ACTIVE, None), (None, K.ACTIVE)], ids=str)
def test_agent_learn_batch_in_f32_against_clip_ref(factors):
    """One Agent(grad_clip=).learn_batch in f32 on the CPU against clip_ref.clip_step with tests/test_loss_shape_cpu.py's bounds: the
    gradients the optimizers saw -- the CLIPPED ones -- within 3e-5 max |g64| + 1e-7 per tensor, both losses within 1e-5 relative.
    And exp_avg after the step: from the incoming moment m0 it is b1 m0 + (1 - b1)(coef g + wd p0), coef and g the reference's, within
    (1 - b1) times the gradient bound; where the clip is active, tensors are NOT within ten times that of what the unclipped gradient gives."""
    from ddpg_trucktrailer_amd.grad_clip import GradClip
    state, hyper, batch, (max_c, max_a), ref = K.clipped(_CASE, factors)
    agent = _agent(state, hyper, GradClip(max_c, max_a))
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
        h = hyper[key]
        b1, wd, coef = h["betas"][0], h["weight_decay"], ref["coef"][key]
        active = coef < 1.0
        assert active == (factors[0 if key == "critic" else 1] == K.ACTIVE)
        far = 0
        for k, pp in getattr(agent, key).named_parameters():
            want = ref["clipped"][key][k]
            tol = 3e-5 * want.abs().max().item() + 1e-7
            err = (seen[key][k].double() - want).abs().max().item()
            worst["grad " + key] = max(worst.get("grad " + key, 0.0), err / tol)
            assert err <= tol, (key, k, err, tol)
            m0, p0, g = state["m"][key][k].double(), state["nets"][key][k].double(), ref["grads"][key][k]
            m = getattr(agent, key).optimizer.state[pp]["exp_avg"].double()
            with_clip, without = (b1 * m0 + (1 - b1) * (cf * g + wd * p0) for cf in (coef, 1.0))
            mtol = (1 - b1) * tol + 2.0 ** -22 * with_clip.abs().max().item()
            merr = (m - with_clip).abs().max().item()
            worst["exp_avg " + key] = max(worst.get("exp_avg " + key, 0.0), merr / mtol)
            assert merr <= mtol, (key, k, merr, mtol)
            far += int((m - without).abs().max().item() > 10 * mtol)
        assert (far > 0) == active, (key, far)
    for name, got, want in (("critic_loss", agent.last_critic_loss.item(), ref["critic_loss"]),
                            ("actor_loss", agent.last_actor_loss.item(), ref["actor_loss"])):
        worst[name] = abs(got - want) / (1e-5 * max(1e-1, abs(want)))
        assert worst[name] <= 1.0, (name, got, want)
    print(f"RATIOS factors {factors}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


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


def test_an_inactive_clip_leaves_the_plain_agents_bits():
    """Agent(grad_clip=GradClip(1e30, 1e30)) after three learn_batch calls: the SHA-256 over the four nets and both optimizers'
    moments is the plain Agent's (coef = 1: the product is exact); an active clip's is another."""
    from ddpg_trucktrailer_amd.grad_clip import GradClip
    state, hyper, batch, _, _ = R.case(*_CASE)
    s, a, r, s2, d = batch
    digests = []
    for clip in (None, GradClip(1e30, 1e30), GradClip(1e-3, None)):
        agent = _agent(state, hyper, clip)
        for _ in range(3):
            agent.learn_batch(s, a, r, s2, d.bool())
        digests.append(_digest(agent))
    assert digests[0] == digests[1] and digests[2] != digests[0]


# ---- refusals in Python -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, word", [(dict(critic=0.0), "critic"), (dict(critic=-1.0), "critic"), (dict(critic=float("nan")), "critic"),
                                      (dict(critic=float("inf")), "critic"), (dict(critic=True), "critic"), (dict(critic="1"), "critic"),
                                      (dict(actor=0.0), "actor"), (dict(actor=-0.5), "actor"), (dict(actor=float("nan")), "actor"),
                                      (dict(actor=float("inf")), "actor"), (dict(actor=False), "actor"), (dict(), "grad_clip"),
                                      (dict(critic=None, actor=None), "grad_clip")])
def test_grad_clip_refuses(kw, word):
    from ddpg_trucktrailer_amd.grad_clip import GradClip
    with pytest.raises(ValueError, match=word):
        GradClip(**kw)


def test_grad_clip_equality_repr_and_tuple():
    from ddpg_trucktrailer_amd.grad_clip import GradClip
    from ddpg_trucktrailer_amd.options import CHECKPOINT_KEYS, compare_options, write_options
    assert GradClip(10).as_tuple() == (10.0, None) and GradClip(10) == GradClip(10.0, None) and GradClip(10, 1) != GradClip(10, 2)
    assert repr(GradClip(10, 0.5)) == "GradClip(critic=10.0, actor=0.5)"
    assert GradClip.from_tuple(GradClip(None, 0.5).as_tuple()) == GradClip(actor=0.5)
    assert "grad_clip" in CHECKPOINT_KEYS
    sd = write_options({}, grad_clip=GradClip(10, 0.5))
    assert sd == {"grad_clip": [10.0, 0.5]}
    compare_options(sd, grad_clip=GradClip(10, 0.5))
    for other in (None, GradClip(10, 0.25)):
        with pytest.raises(ValueError, match="grad_clip"):
            compare_options(sd, grad_clip=other)
    with pytest.raises(ValueError, match="grad_clip"):
        compare_options({}, grad_clip=GradClip(10))


@pytest.mark.parametrize("kw", [dict(td3="cfg"), dict(population=True), dict(data_parallel=True), dict(force_dp=True),
                                dict(demo_loss="demo"), dict(expert="lanes"), dict(labels="labels")], ids=lambda kw: next(iter(kw)))
def test_check_grad_clip_refuses(kw):
    from ddpg_trucktrailer_amd.grad_clip import GradClip, check_grad_clip
    with pytest.raises(ValueError, match="grad_clip"):
        check_grad_clip(GradClip(1.0, 0.1), **kw)


def test_check_grad_clip_accepts_the_supported_loop_and_refuses_a_non_clip():
    from ddpg_trucktrailer_amd.grad_clip import GradClip, check_grad_clip
    clip = GradClip(1.0)
    assert check_grad_clip(clip) is clip and check_grad_clip(clip, td3=None, population=False, demo_loss=None, expert=None) is clip
    with pytest.raises(ValueError, match="grad_clip"):
        check_grad_clip((1.0, None))


def test_agent_population_and_loop_refuse_a_clip_where_it_has_no_kernels():
    from ddpg_trucktrailer_amd.agent import Agent
    from ddpg_trucktrailer_amd.grad_clip import GradClip
    from ddpg_trucktrailer_amd.population import PopulationLearner
    from ddpg_trucktrailer_amd.td3 import TD3Config
    kw = dict(alpha=1e-4, beta=1e-3, input_dims=(23,), tau=1e-3, n_actions=1, batch_size=4, device="cpu", replay=False)
    with pytest.raises(ValueError, match="grad_clip"):
        Agent(td3=TD3Config(), grad_clip=GradClip(1.0), **kw)
    with pytest.raises(ValueError, match="grad_clip"):
        Agent(grad_clip=(1.0, None), **kw)
    agent = Agent(grad_clip=GradClip(1.0, 0.1), **kw)
    assert agent.grad_clip == GradClip(1.0, 0.1)
    with pytest.raises(ValueError, match="grad_clip.*population"):
        PopulationLearner([agent], 4, rings=[None], seeds=[1])


# ---- the entry point's refusals, before any HIP call -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib as L
    return L


class _Fake(F.Fake):
    """fake_args.Fake with the arguments of tt_adam_soft_update_clipped: five tables of twelve made-up addresses, numel, a clip."""

    def __init__(self, L):
        super().__init__(L, 256, "plain")
        self.count = 12
        self.g_table = (C.c_void_p * 12)(*[self.nxt() for _ in range(12)])
        self.numel = (C.c_int32 * 12)(9200, 400, 400, 400, 120000, 300, 300, 300, 300, 1, 300, 300)
        self.clip = L.TTGradClip(max_norm=1.0, partials=self.nxt(), out=self.nxt(), counts=self.nxt())
        self.with_clip = True
        self.arrays = dict(params=self.tables[0], grads=self.g_table, exp_avg=self.tables[1], exp_avg_sq=self.tables[2],
                           targets=self.tables[3], numel=self.numel)

    def call(self):
        a = self.arrays
        return getattr(self.L.load(), _ENTRY)(self.count, a["params"], a["grads"], a["exp_avg"], a["exp_avg_sq"], a["targets"], a["numel"],
                                              self.step, 1e-4, 0.9, 0.999, 1e-8, 0.0, 1e-3, None, self.bias_corr,
                                              C.byref(self.clip) if self.with_clip else None, None)


_set = F.set_field
_REFUSALS = [("clip is NULL", lambda f: setattr(f, "with_clip", False)),
             ("partials", _set("clip", "partials", None)), ("out", _set("clip", "out", None)),
             ("max_norm", _set("clip", "max_norm", 0.0)), ("max_norm", _set("clip", "max_norm", -1.0)),
             ("max_norm", _set("clip", "max_norm", float("nan"))), ("max_norm", _set("clip", "max_norm", float("inf"))),
             ("count = 0", lambda f: setattr(f, "count", 0)), ("count = 13", lambda f: setattr(f, "count", 13)),
             ("count = -1", lambda f: setattr(f, "count", -1))] + \
            [("NULL", lambda f, k=k: f.arrays.__setitem__(k, None)) for k in ("params", "grads", "exp_avg", "exp_avg_sq", "numel")] + \
            [("step_dev", lambda f: setattr(f, "step", None)),
             ("numel[4] = -1", lambda f: f.numel.__setitem__(4, -1)), ("numel[11] = -300", lambda f: f.numel.__setitem__(11, -300)),
             ("tensor", lambda f: f.g_table.__setitem__(3, None)), ("tensor", lambda f: f.tables[0].__setitem__(0, None)),
             ("tensor", lambda f: f.tables[2].__setitem__(11, None))]


@pytest.mark.parametrize("word, spoil", _REFUSALS, ids=[f"{i}-{w.replace(' ', '_')}" for i, (w, _) in enumerate(_REFUSALS)])
def test_the_entry_point_checks_its_arguments_before_any_hip_call(lib, word, spoil):
    """TT_EINVAL and a message that starts with the entry point's name and names the argument, for one spoiled argument at a time
    (the addresses are made up: with one bad argument nothing reaches the GPU)."""
    f = _Fake(lib)
    spoil(f)
    rc, msg = f.call(), f.last_error()
    assert rc == lib.TT_EINVAL, (rc, msg)
    assert msg.startswith(_ENTRY + ":") and word in msg, msg


def test_the_library_exports_the_entry_point_and_the_struct_has_the_headers_layout(lib):
    L = lib
    assert L.load().tt_version() == 3
    assert _ENTRY in L.EXPORTS and hasattr(L.load(), _ENTRY)
    G = L.TTGradClip            # { float max_norm; double *partials; float *out; int64_t *counts; } on LP64
    assert C.sizeof(G) == 32
    assert [getattr(G, n).offset for n in ("max_norm", "partials", "out", "counts")] == [0, 8, 16, 24]
    assert G.max_norm.size == 4
    header = open(L.HERE + "/../include/ttenv.h").read()
    assert f"#define TT_GRAD_CLIP_PARTIALS {L.GRAD_CLIP_PARTIALS}\n" in header


def test_the_new_kernels_use_no_scratch_and_the_library_has_one_more_code_object(lib):
    """k_grad_sqnorm and k_adam_soft_clip exist (a missing kernel is an error, not a fall-back), spill nothing and use no scratch;
    k_grad_sqnorm's LDS is its tree's 256 doubles; k_adam_soft_clip keeps k_adam_soft's occupancy.  csrc/ttclip.hip is a code object
    of its own: kernel_resources.text_sections() lists thirteen, one per source that defines a kernel."""
    from ddpg_trucktrailer_amd import build
    from ddpg_trucktrailer_amd import kernel_resources as kr
    ks = kr.kernels()
    rows = {}
    for part in ("k_grad_sqnorm", "k_adam_soft_clip", "k_adam_softENS"):
        found = kr.find(ks, part)
        assert len(found) == 1, part
        (n, v), = found.items()
        assert v["scratch"] == 0 and v["vgpr_spills"] == 0, (n, v)
        rows[part] = v
    assert rows["k_grad_sqnorm"]["lds"] == 256 * 8 and rows["k_adam_soft_clip"]["lds"] == 0
    assert kr.waves_per_simd(rows["k_adam_soft_clip"]["vgpr"]) == kr.waves_per_simd(rows["k_adam_softENS"]["vgpr"]) == 8
    assert build.SRC[-1].endswith("ttclip.hip")
    with_kernels = [p for p in build.SRC if "__global__" in open(p).read()]
    assert len(kr.text_sections()) == len(with_kernels) == 13


def test_the_fused_learners_state_dict_carries_the_clip_and_refuses_another():
    """FusedLearner.state_dict / load_state_dict through the options' entries alone (a bare learner: no GPU)."""
    import types
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    from ddpg_trucktrailer_amd.grad_clip import GradClip
    fl = FusedLearner.__new__(FusedLearner)
    fl.loss_shape = fl.demo_loss = fl.p2p = fl.learn_log = None
    for name in ("actor", "critic"):
        setattr(fl, name, types.SimpleNamespace(m=torch.zeros(3), v=torch.zeros(3)))
    fl.step_dev = torch.zeros((), dtype=torch.int64)
    fl.tail_words = torch.full((64 + 2 * 1024,), -1, dtype=torch.int32)
    assert "grad_clip" not in fl.state_dict()
    fl.grad_clip = GradClip(10.0, None)
    sd = fl.state_dict()
    assert sd["grad_clip"] == [10.0, None]
    fl.load_state_dict(sd)
    fl.grad_clip = GradClip(5.0, None)
    with pytest.raises(ValueError, match="grad_clip"):
        fl.load_state_dict(sd)
    assert math.isfinite(fl.grad_clip.critic)
