"""CPU: per-agent gradient-norm clipping in a population (csrc/ttclip.hip, include/ttenv.h: tt_pop_learn_set_clip and its neighbours;
DESIGN.md section 36) as far as no GPU is needed: the option's forms and every Python refusal, the two refusals that stay pinned, the
refusals of the three entry points that come before any HIP call, the struct's layout, the controller's moves of the clip, what a
checkpoint carries and refuses, and the new kernels' resource rows.

Where the C-side refusals are tested: a handle is made by tt_pop_learn_create, which allocates device memory, so here a NULL handle
(all three entry points, with good and with NULL arrays) is reachable, and -- because each entry point looks at its arrays before it
reads the handle -- NULL arrays behind a handle that is never dereferenced.  Every refusal that needs a live handle is in
tests/test_gpu_population_clip.py."""
import ctypes as C
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib
    return _lib


# ---- the option ----------------------------------------------------------------------------------------------------------------
def test_the_options_forms():
    from ddpg_trucktrailer_amd.grad_clip import GradClip, check_population_grad_clip, clip_of_values, clip_values
    one = GradClip(10.0, 0.5)
    assert check_population_grad_clip(None, 3) is None
    assert check_population_grad_clip([None, None, None], 3) is None              # no entry: no table
    assert check_population_grad_clip(one, 3) == [one, one, one]
    assert check_population_grad_clip([one, None, GradClip(actor=1.0)], 3) == [one, None, GradClip(None, 1.0)]
    assert check_population_grad_clip((one, None), 2) == [one, None]
    assert clip_values(None) == (0.0, 0.0) and clip_values(one) == (10.0, 0.5) and clip_values(GradClip(actor=2)) == (0.0, 2.0)
    assert clip_of_values(0.0, 0.0) is None and clip_of_values(10.0, 0.5) == one and clip_of_values(0.0, 2.0) == GradClip(None, 2.0)


def test_the_options_refusals():
    from ddpg_trucktrailer_amd.grad_clip import GradClip, check_population_grad_clip
    from ddpg_trucktrailer_amd.td3 import TD3Config
    one = GradClip(1.0)
    with pytest.raises(ValueError, match=r"grad_clip: 2 values for 3 agents"):
        check_population_grad_clip([one, None], 3)
    for bad in ((1.0, None), 1.0, "1"):
        with pytest.raises(ValueError, match="grad_clip"):
            check_population_grad_clip([one, bad], 2)
        with pytest.raises(ValueError, match="grad_clip"):
            check_population_grad_clip(bad, 2)
    with pytest.raises(ValueError, match="grad_clip in a TD3 population.*PopulationTD3Learner"):
        check_population_grad_clip(one, 2, td3=TD3Config())
    with pytest.raises(ValueError, match="grad_clip in a data-parallel population"):
        check_population_grad_clip(one, 2, data_parallel=True)
    with pytest.raises(ValueError, match="grad_clip in a population on device = 'cpu'"):
        check_population_grad_clip(one, 2, device="cpu")
    assert check_population_grad_clip(None, 2, td3=TD3Config(), device="cpu") is None        # no clip: nothing to refuse
    assert check_population_grad_clip(one, 2, device="cuda:0") == [one, one]


def test_the_loop_and_the_learners_refuse_where_the_clip_has_no_kernels():
    from ddpg_trucktrailer_amd.agent import Agent
    from ddpg_trucktrailer_amd.grad_clip import GradClip
    from ddpg_trucktrailer_amd.population import PopulationLearner, PopulationRollout
    from ddpg_trucktrailer_amd.td3 import PopulationTD3Learner, TD3Config
    one = GradClip(1.0, 0.1)
    with pytest.raises(ValueError, match="grad_clip in a TD3 population"):
        PopulationRollout(64, [1, 2], td3=TD3Config(), updates_per_step=2, grad_clip=one)
    with pytest.raises(ValueError, match="grad_clip in a TD3 population"):
        PopulationRollout(64, [1, 2], td3=[TD3Config(), TD3Config()], updates_per_step=2, grad_clip=[None, one])
    with pytest.raises(ValueError, match="grad_clip in a data-parallel population"):
        PopulationRollout(64, [1, 2], data_parallel=True, grad_clip=one)
    with pytest.raises(ValueError, match="grad_clip in a population on device = 'cpu'"):
        PopulationRollout(64, [1, 2], device="cpu", grad_clip=one)
    with pytest.raises(ValueError, match="grad_clip: 3 values for 2 agents"):
        PopulationRollout(64, [1, 2], grad_clip=[one, one, one])
    with pytest.raises(ValueError, match="grad_clip"):
        PopulationRollout(64, [1, 2], grad_clip=(1.0, 0.1))
    kw = dict(alpha=1e-4, beta=1e-3, input_dims=(23,), tau=1e-3, n_actions=1, batch_size=4, device="cpu", replay=False)
    agents = [Agent(td3=TD3Config(), **kw) for _ in range(2)]
    with pytest.raises(ValueError, match="grad_clip in a TD3 population.*PopulationTD3Learner"):
        PopulationTD3Learner(agents, 4, [None, None], [1, 2], grad_clips=one)
    with pytest.raises(ValueError, match="grad_clip: 1 values for 2 agents"):
        PopulationLearner([Agent(**kw), Agent(**kw)], 4, rings=[None, None], seeds=[1, 2], grad_clips=[one])


def test_the_two_pinned_refusals_still_hold():
    """An Agent that itself carries grad_clip stays refused with the message it had, and check_grad_clip(population=True) keeps
    refusing: the population's own option is another check."""
    from ddpg_trucktrailer_amd.agent import Agent
    from ddpg_trucktrailer_amd.grad_clip import GradClip, check_grad_clip
    from ddpg_trucktrailer_amd.population import PopulationLearner
    kw = dict(alpha=1e-4, beta=1e-3, input_dims=(23,), tau=1e-3, n_actions=1, batch_size=4, device="cpu", replay=False)
    message = r"grad_clip in a population is not supported \(the population's launches have no clipped optimizer step\)"
    with pytest.raises(ValueError, match=message):
        PopulationLearner([Agent(grad_clip=GradClip(1.0, 0.1), **kw)], 4, rings=[None], seeds=[1])
    with pytest.raises(ValueError, match=message):
        PopulationLearner([Agent(grad_clip=GradClip(1.0, 0.1), **kw)], 4, rings=[None], seeds=[1], grad_clips=GradClip(1.0))
    with pytest.raises(ValueError, match=message):
        check_grad_clip(GradClip(1.0), population=True)


# ---- the entry points ------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_null_arguments_before_any_hip_call(L):
    lib = L.load()

    def refused(rc, *words):
        msg = lib.tt_last_error(None).decode()
        assert rc == L.TT_EINVAL, rc
        assert all(w in msg for w in words), msg
    values = (L.TTPopClip * 2)(L.TTPopClip(1.0, 0.5), L.TTPopClip(0.0, 2.0))
    agents = (C.c_int32 * 2)(0, 1)
    value, out, counts = L.TTPopClip(-7.0, -7.0), (C.c_float * 4)(), (C.c_int64 * 4)()
    never_read = C.c_void_p(0x1000)          # a handle the entry points must not look into before they have seen the arrays
    refused(lib.tt_pop_learn_set_clip(None, values), "tt_pop_learn_set_clip", "handle is NULL")
    refused(lib.tt_pop_learn_set_clip(None, None), "tt_pop_learn_set_clip", "NULL")
    refused(lib.tt_pop_learn_set_clip(never_read, None), "tt_pop_learn_set_clip", "per_agent is NULL")
    refused(lib.tt_pop_clip_write(None, 2, agents, values, None), "tt_pop_clip_write", "handle is NULL")
    refused(lib.tt_pop_clip_write(never_read, 2, None, values, None), "tt_pop_clip_write", "agents is NULL")
    refused(lib.tt_pop_clip_write(never_read, 2, agents, None, None), "tt_pop_clip_write", "values is NULL")
    refused(lib.tt_pop_clip(None, 0, C.byref(value), C.byref(out), C.byref(counts)), "tt_pop_clip", "handle is NULL")
    refused(lib.tt_pop_clip(never_read, 0, None, C.byref(out), C.byref(counts)), "tt_pop_clip", "value, out or counts is NULL")
    refused(lib.tt_pop_clip(never_read, 0, C.byref(value), None, C.byref(counts)), "tt_pop_clip", "value, out or counts is NULL")
    refused(lib.tt_pop_clip(never_read, 0, C.byref(value), C.byref(out), None), "tt_pop_clip", "value, out or counts is NULL")
    assert (value.max_norm_critic, value.max_norm_actor) == (-7.0, -7.0)


def test_the_library_exports_the_entry_points_and_the_struct_has_the_headers_layout(L):
    for name in ("tt_pop_learn_set_clip", "tt_pop_clip_write", "tt_pop_clip"):
        assert name in L.EXPORTS and hasattr(L.load(), name)
    G = L.TTPopClip                 # struct tt_pop_clip { float max_norm_critic, max_norm_actor; }
    assert C.sizeof(G) == 8 and [getattr(G, n).offset for n in ("max_norm_critic", "max_norm_actor")] == [0, 4]
    header = open(L.HERE + "/../include/ttenv.h").read()
    assert "struct tt_pop_clip {" in header and "float max_norm_critic, max_norm_actor;" in header
    # the structs the new entry points sit beside keep their layout
    assert C.sizeof(L.TTPopExploitPair) == 24 and C.sizeof(L.TTPopNstep) == 12 and L.load().tt_version() == 3


def test_kernel_resources(L):
    """k_pop_grad_sqnorm and k_pop_adam_soft_clip exist (a missing kernel is an error, not a fall-back), spill nothing and use no
    scratch; the norm kernel's LDS is its tree's 256 doubles; the clipped step keeps at least k_adam_soft_clip's waves per SIMD; the
    two lone kernels' rows are what they were before the population's kernels joined their code object (the numbers of the parent
    build); the library still has thirteen code objects."""
    from ddpg_trucktrailer_amd import build
    from ddpg_trucktrailer_amd import kernel_resources as kr
    ks = kr.kernels()
    rows = {}
    for part in ("13k_grad_sqnorm", "16k_adam_soft_clip", "17k_pop_grad_sqnorm", "20k_pop_adam_soft_clip", "16k_pop_clip_write"):
        found = kr.find(ks, part)
        assert len(found) == 1, (part, sorted(found))
        (n, v), = found.items()
        assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (n, v)
        rows[part[2:]] = v
    assert rows["k_pop_grad_sqnorm"]["lds"] == 2048 and rows["k_pop_adam_soft_clip"]["lds"] == 0
    assert kr.waves_per_simd(rows["k_pop_adam_soft_clip"]["vgpr"]) >= kr.waves_per_simd(rows["k_adam_soft_clip"]["vgpr"]) == 8
    parent = {"k_grad_sqnorm": dict(vgpr=18, agpr=0, sgpr=42, lds=2048, scratch=0, vgpr_spills=0, sgpr_spills=0, max_threads=256),
              "k_adam_soft_clip": dict(vgpr=36, agpr=0, sgpr=84, lds=0, scratch=0, vgpr_spills=0, sgpr_spills=0, max_threads=256)}
    for name, want in parent.items():
        assert {k: rows[name][k] for k in want} == want, (name, rows[name])
    assert build.SRC[-1].endswith("ttclip.hip")
    assert len(kr.text_sections()) == len([p for p in build.SRC if "__global__" in open(p).read()]) == 13


# ---- PBT ---------------------------------------------------------------------------------------------------------------------------
def test_pbt_without_clip_factors_decides_as_the_golden_rounds():
    from ddpg_trucktrailer_amd.pbt import PBT
    spec = importlib.util.spec_from_file_location("make_golden_pbt_rounds", os.path.join(GOLDEN, "make_golden_pbt_rounds.py"))
    rounds = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rounds)
    want = json.load(open(os.path.join(GOLDEN, "pbt_rounds.json")))
    assert rounds.play(PBT, lambda p, pop, d: p.step(pop, d)) == want
    assert rounds.play(lambda K, **kw: PBT(K, clip_factors=None, **kw), lambda p, pop, d: p.step(pop, d)) == want
    assert "clip_factors" not in PBT(4, 10).state_dict()


def _records(K, means):
    return [{"ret": [m] * 4, "success": [m > 0] * 4} for m in means[:K]]


def _hypers(K, clips):
    out = [dict(alpha=1e-4 * (a + 1), beta=1e-3, tau=1e-3, gamma=0.99 - 0.01 * a) for a in range(K)]
    for h, (c, a) in zip(out, clips):
        h["clip_critic"], h["clip_actor"] = c, a
    return out


MEANS = [3.0, -1.0, 5.0, 0.5, -4.0, 2.0, 9.0, -2.0]


def _play(seed, rounds=40, bounds=None, state_at=None):
    """(decisions, the clips at the end[, the controller's state and clips after round state_at])."""
    from ddpg_trucktrailer_amd.pbt import PBT
    K = 8
    clips = [[10.0, 0.5], [0.0, 0.25], [40.0, 0.0], [0.0, 0.0], [5.0, 1.0], [20.0, 2.0], [80.0, 0.125], [2.5, 0.0]]
    pbt = PBT(K, 10, seed=seed, window=4, quantile=0.25, clip_factors=(0.8, 1.2), bounds=bounds)
    out, saved = [], None
    for rnd in range(1, rounds + 1):
        pbt.observe(_records(K, MEANS))
        for d in pbt.decide(10 * rnd, _hypers(K, clips)):
            out.append(d)
            clips[d["dst"]] = [d["new"]["clip_critic"], d["new"]["clip_actor"]]
        if rnd == state_at:
            saved = (pbt.state_dict(), [list(c) for c in clips], len(out))
    return out, clips, saved


def test_pbt_explores_the_clip_inside_its_bounds_and_keeps_zero_at_zero():
    from ddpg_trucktrailer_amd.pbt import BOUNDS, HYPERS, PBT
    plain = PBT(8, 10, seed=5, window=4, quantile=0.25)
    plain.observe(_records(8, MEANS))
    first = plain.decide(10, _hypers(8, [[0.0, 0.0]] * 8))[0]
    bounds = {"clip": (0.2, 50.0)}
    out, clips, _ = _play(5, bounds=bounds)
    assert len(out) == 80
    assert (out[0]["dst"], out[0]["src"]) == (first["dst"], first["src"])          # the clip's draws come after the pair's others
    assert {k: out[0]["new"][k] for k in HYPERS} == first["new"]
    factors, now = set(), [[10.0, 0.5], [0.0, 0.25], [40.0, 0.0], [0.0, 0.0], [5.0, 1.0], [20.0, 2.0], [80.0, 0.125], [2.5, 0.0]]
    for d in out:
        assert set(d["new"]) == set(HYPERS) | {"clip_critic", "clip_actor"}
        for j, k in enumerate(("clip_critic", "clip_actor")):
            src, new = now[d["src"]][j], d["new"][k]
            assert d["old"][k] == now[d["dst"]][j]
            if src == 0.0:
                assert new == 0.0, d                                # not clipped stays not clipped
            else:
                assert 0.2 <= new <= 50.0, d
                want = [min(max(src * f, 0.2), 50.0) for f in (0.8, 1.2)]
                assert new in want, (d, want)
                factors.add(want.index(new))
        now[d["dst"]] = [d["new"]["clip_critic"], d["new"]["clip_actor"]]
    assert factors == {0, 1} and now == clips
    assert BOUNDS["clip"][0] > 0
    for bad in ((), (0.0, 1.2), (-1.0,), (float("inf"),)):
        with pytest.raises(ValueError, match="clip_factors"):
            PBT(8, 10, clip_factors=bad)


def test_pbt_with_clip_factors_is_a_function_of_the_seed_and_round_trips_its_state():
    from ddpg_trucktrailer_amd.pbt import PBT
    a, b, c = _play(5), _play(5), _play(6)
    assert a[0] == b[0] and a[1] == b[1] and a[0] != c[0]
    whole, clips, (sd, clips_at, n_at) = _play(5, state_at=17)
    assert sd["clip_factors"] == [0.8, 1.2]
    pbt = PBT(8, 10, seed=99, window=4, quantile=0.25, clip_factors=(0.8, 1.2))
    pbt.load_state_dict(sd)
    assert pbt.state_dict()["clip_factors"] == [0.8, 1.2] and pbt.last_round == 170
    rest = []
    for rnd in range(18, 41):
        pbt.observe(_records(8, MEANS))
        for d in pbt.decide(10 * rnd, _hypers(8, clips_at)):
            rest.append(d)
            clips_at[d["dst"]] = [d["new"]["clip_critic"], d["new"]["clip_actor"]]
    assert rest == whole[n_at:] and clips_at == clips
    for other in (PBT(8, 10, window=4), PBT(8, 10, window=4, clip_factors=(0.5, 2.0))):
        with pytest.raises(ValueError, match="clip_factors"):
            other.load_state_dict(sd)
    with pytest.raises(ValueError, match="clip_factors"):
        pbt.load_state_dict(PBT(8, 10, window=4).state_dict())


class _Pop:
    """What PBT.step asks of a population."""

    def __init__(self, K, clips):
        import types
        self.agents = [types.SimpleNamespace(**{k: v for k, v in h.items() if not k.startswith("clip")}) for h in _hypers(K, clips or [[0.0, 0.0]] * K)]
        self.vector_steps, self.pairs = 10, None
        self.clip_table, self.grad_clips = clips is not None, clips

    def exploit(self, pairs):
        self.pairs = pairs


def test_pbt_step_passes_the_clip_through_to_exploit_and_the_file_state_carries_the_option():
    from ddpg_trucktrailer_amd import checkpoint
    from ddpg_trucktrailer_amd.pbt import PBT
    pop = _Pop(4, [[10.0, 0.5], [0.0, 0.25], [40.0, 0.0], [5.0, 1.0]])
    pbt = PBT(4, 10, seed=2, window=4, clip_factors=(0.8, 1.2))
    out = pbt.step(pop, _records(4, [3.0, -1.0, 5.0, 0.5]))
    assert len(out) == 1 and pop.pairs == [(out[0]["dst"], out[0]["src"], out[0]["new"])] and out[0]["src"] == 2
    assert pop.pairs[0][2]["clip_critic"] in (32.0, 48.0) and pop.pairs[0][2]["clip_actor"] == 0.0
    with pytest.raises(ValueError, match="clip_factors"):
        PBT(4, 10, seed=2, window=4, clip_factors=(0.8, 1.2)).step(_Pop(4, None), _records(4, [3.0, -1.0, 5.0, 0.5]))
    fs = checkpoint.pbt_file_state(pbt)
    assert fs["clip_factors"] == [0.8, 1.2] and "clip_factors" not in checkpoint.pbt_file_state(PBT(4, 10))
    fresh = PBT(4, 10, seed=7, window=4, clip_factors=(0.8, 1.2))
    checkpoint.load_pbt_file_state(fresh, fs)
    assert fresh.history == pbt.history and fresh.rng.get_state()[1].tolist() == pbt.rng.get_state()[1].tolist()


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------
def _state(K=2, clips=None):
    """A PopulationRollout.state_dict() as far as check_population_state reads it."""
    agents = []
    for a in range(K):
        st = {"format": 2, "batch_size": 33, "ring": {"slots": 16, "n": 64, "obs": None}, "n_step": 1,
              "hyper": dict(alpha=1e-4, beta=1e-3, tau=1e-3, gamma=0.99)}
        if clips is not None:
            st["clip"] = list(clips[a])
        agents.append(st)
    sd = {"format": 1, "K": K, "n": 64, "batch_size": 33, "updates_per_step": 1, "vector_steps": 5, "seeds": [1, 2],
          "n_step_table": False, "n_step_max": 1, "policy_delay": None, "agents": agents}
    if clips is not None:
        sd["grad_clip_table"] = True
    return sd


def test_check_population_state_accepts_and_refuses_the_clip_table():
    from ddpg_trucktrailer_amd.population import check_population_state
    args = (2, 64, 16, 33)
    plain, clipped = _state(), _state(clips=[[0.5, 0.01], [0.0, 2.0]])
    assert "grad_clip_table" not in plain and all("clip" not in st for st in plain["agents"])
    assert check_population_state(plain, *args) == [1, 1]
    assert check_population_state(clipped, *args, grad_clip_table=True) == [1, 1]
    with pytest.raises(ValueError, match="grad_clip: the checkpoint was written with a gradient clip, this population has none"):
        check_population_state(clipped, *args)
    with pytest.raises(ValueError, match="grad_clip: the checkpoint was written without a gradient clip, this population has one"):
        check_population_state(plain, *args, grad_clip_table=True)
    for bad in (None, [0.5], [0.5, -1.0], [0.5, float("nan")], [float("inf"), 0.0], ["a", 0.0]):
        sd = _state(clips=[[0.5, 0.01], [0.0, 2.0]])
        sd["agents"][1]["clip"] = bad
        with pytest.raises(ValueError, match="grad_clip: agent 1"):
            check_population_state(sd, *args, grad_clip_table=True)
