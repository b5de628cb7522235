"""CPU: per-agent n-step returns in a population (csrc/ttpop_nstep.hip, include/ttenv.h: tt_pop_learn_set_nstep and its neighbours)
as far as no GPU is needed: the new kernel's budget, the refusals of the three entry points that come before any HIP call, what the
Python classes refuse, and the controller's moves of n.

Where the C-side refusals are tested: a handle is made by tt_pop_learn_create, which allocates device memory, so here only a NULL
handle (all three entry points, with good and with NULL arrays) and tt_pop_nstep's NULL `out` are reachable.  Every refusal that
needs a live handle -- NULL arrays behind a good handle, n_step, gamma, discount, the ring's window, ns.gamma != the pair's gamma,
plain tt_pop_exploit on a population with a table -- is in tests/test_gpu_population_nstep.py."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib
    return _lib


def test_population_nstep_kernel_keeps_two_waves_per_simd(L):
    """k_fwd_multi_nstep sits at 204 VGPRs with 83,648 B of LDS; two waves per SIMD allow 256 VGPRs."""
    from ddpg_trucktrailer_amd import kernel_resources as kr
    ks = kr.kernels()
    found = kr.find(ks, "21k_pop_fwd_multi_nstep")
    assert len(found) == 1, sorted(found)
    (n, v), = found.items()
    assert v["max_threads"] == 512 and kr.waves_per_simd(v["vgpr"]) >= 2, (n, v)
    assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["lds"] <= 160 * 1024, (n, v)
    assert len(kr.find(ks, "15k_pop_fwd_multi")) == 1          # the new name does not shadow the one-step kernel's pattern


def test_entry_points_refuse_null_arguments_before_any_hip_call(L):
    lib = L.load()

    def refused(rc, *words):
        msg = lib.tt_last_error(None).decode()
        assert rc == L.TT_EINVAL, rc
        assert all(w in msg for w in words), msg
    ns = (L.TTPopNstep * 2)(L.TTPopNstep(5, 0.99, 0.99 ** 5), L.TTPopNstep(1, 0.98, 0.98))
    pairs = (L.TTPopExploitPair * 2)(L.TTPopExploitPair(1, 0, 1e-4, 1e-3, 1e-3, 0.99), L.TTPopExploitPair(2, 0, 1e-4, 1e-3, 1e-3, 0.98))
    out = L.TTPopNstep(-7, -7.0, -7.0)
    refused(lib.tt_pop_learn_set_nstep(None, ns), "tt_pop_learn_set_nstep", "handle is NULL")
    refused(lib.tt_pop_learn_set_nstep(None, None), "tt_pop_learn_set_nstep", "NULL")
    refused(lib.tt_pop_exploit_nstep(None, 2, pairs, ns, None), "tt_pop_exploit_nstep", "handle is NULL")
    refused(lib.tt_pop_exploit_nstep(None, 2, None, None, None), "tt_pop_exploit_nstep", "NULL")
    refused(lib.tt_pop_nstep(None, 0, C.byref(out)), "tt_pop_nstep", "handle is NULL")
    refused(lib.tt_pop_nstep(None, 0, None), "tt_pop_nstep", "NULL")
    assert (out.n_step, out.gamma, out.discount) == (-7, -7.0, -7.0)
    refused(lib.tt_pop_exploit(None, 2, pairs, None), "tt_pop_exploit:", "handle is NULL")        # (as before)
    assert lib.tt_version() == 3
    assert C.sizeof(L.TTPopNstep) == 12


def test_python_side_refusals():
    from ddpg_trucktrailer_amd.population import PopulationRollout
    with pytest.raises(ValueError, match=r"n_step.*\b3\b.*\b2\b"):
        PopulationRollout(64, [1, 2], device="cpu", n_step=[5, 3, 1])
    for n in (17, 0, [1, 17], [0, 1]):
        with pytest.raises(ValueError, match="n_step"):
            PopulationRollout(64, [1, 2], device="cpu", n_step=n)
    with pytest.raises(ValueError, match="not supported on a CPU device"):
        PopulationRollout(64, [1, 2], device="cpu", n_step=[1, 5])
    with pytest.raises(ValueError, match="not supported on a CPU device"):        # n = 1 now, but PBT may raise it
        PopulationRollout(64, [1, 2], device="cpu", n_step=1, n_step_max=3)
    with pytest.raises(ValueError, match="n_step_max"):
        PopulationRollout(64, [1, 2], device="cuda:0", n_step=[5, 3], n_step_max=4)
    with pytest.raises(ValueError, match="replay_slots"):                         # 3 + (8 - 1) = 10 slots
        PopulationRollout(64, [1, 2], device="cuda:0", n_step=[5, 3], n_step_max=8, replay_slots=9)
    with pytest.raises(ValueError, match="not supported"):                        # side buffers stay refused
        PopulationRollout(64, [1, 2], device="cuda:0", n_step=5, side_buffer=object())


def test_discount_helper_is_the_lone_learners_expression():
    from ddpg_trucktrailer_amd.fused_learn import nstep_discount
    for gamma in (0.99, 0.985, 0.9):
        assert nstep_discount(gamma, 1) == float(gamma)
        for n in (2, 5, 16):
            assert nstep_discount(gamma, n) == float(gamma) ** int(n)


def _records(K, means):
    return [{"ret": [m] * 4, "success": [m > 0] * 4} for m in means[:K]]


def _hypers(K, n_steps=None):
    out = [dict(alpha=1e-4 * (a + 1), beta=1e-3, tau=1e-3, gamma=0.99 - 0.01 * a) for a in range(K)]
    if n_steps is not None:
        for h, n in zip(out, n_steps):
            h["n_step"] = n
    return out


def test_pbt_without_n_step_choices_is_the_controller_as_it_was():
    from ddpg_trucktrailer_amd.pbt import HYPERS, PBT
    K, means = 8, [3.0, -1.0, 5.0, 0.5, -4.0, 2.0, 9.0, -2.0]
    runs = []
    for kw in ({}, dict(n_step_choices=None)):
        pbt = PBT(K, 10, seed=5, window=4, quantile=0.25, **kw)
        out = []
        for rnd in range(1, 4):
            pbt.observe(_records(K, means))
            out += pbt.decide(10 * rnd, _hypers(K))
        runs.append((out, pbt.rng.get_state()[1].tolist()))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1] and len(runs[0][0]) == 6
    for d in runs[0][0]:
        assert set(d["old"]) == set(HYPERS) and set(d["new"]) == set(HYPERS)


def test_pbt_moves_n_to_a_neighbour_inside_the_choices():
    from ddpg_trucktrailer_amd.pbt import HYPERS, PBT
    K, means, choices = 8, [3.0, -1.0, 5.0, 0.5, -4.0, 2.0, 9.0, -2.0], (1, 3, 5, 8)
    n_now = [1, 3, 5, 8, 1, 3, 5, 8]
    plain = PBT(K, 10, seed=5, window=4, quantile=0.25)
    plain.observe(_records(K, means))
    first = plain.decide(10, _hypers(K))[0]
    pbt = PBT(K, 10, seed=5, window=4, quantile=0.25, n_step_choices=(5, 1, 8, 3))
    assert pbt.n_step_choices == choices
    moves = set()
    for rnd in range(1, 41):
        pbt.observe(_records(K, means))
        out = pbt.decide(10 * rnd, _hypers(K, n_now))
        assert len(out) == 2
        if rnd == 1:      # the first pair's src and its four factor draws come before the new draw
            assert (out[0]["dst"], out[0]["src"]) == (first["dst"], first["src"])
            assert {k: out[0]["new"][k] for k in HYPERS} == first["new"]
        for d in out:
            assert d["old"]["n_step"] == n_now[d["dst"]] and set(d["new"]) == set(HYPERS) | {"n_step"}
            i, j = choices.index(n_now[d["src"]]), choices.index(d["new"]["n_step"])
            assert abs(i - j) <= 1, d
            moves.add(j - i)
            n_now[d["dst"]] = d["new"]["n_step"]
    assert moves == {-1, 0, 1}
    with pytest.raises(ValueError, match="n_step_choices"):
        PBT(K, 10, n_step_choices=(0, 3))


class _Pop:
    """What PBT.step asks of a population."""

    def __init__(self, K, n_steps):
        import types
        self.agents = [types.SimpleNamespace(**h) for h in _hypers(K)]
        self.n_steps, self.vector_steps, self.pairs = list(n_steps), 10, None

    def exploit(self, pairs):
        self.pairs = pairs


def test_pbt_step_passes_n_step_through_to_exploit():
    from ddpg_trucktrailer_amd.pbt import PBT
    pop = _Pop(4, [1, 3, 5, 8])
    pbt = PBT(4, 10, seed=2, window=4, n_step_choices=(1, 3, 5, 8))
    out = pbt.step(pop, _records(4, [3.0, -1.0, 5.0, 0.5]))
    assert len(out) == 1 and pop.pairs == [(out[0]["dst"], out[0]["src"], out[0]["new"])]
    assert pop.pairs[0][2]["n_step"] in (3, 5, 8) and out[0]["src"] == 2 and out[0]["old"]["n_step"] == 3
