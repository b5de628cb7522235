"""CPU: population-based training -- the controller (ddpg_trucktrailer_amd/pbt.py) on synthetic drained episode records, and the
exploit launch of the library (csrc/ttpop.hip: k_pop_exploit, include/ttenv.h: tt_pop_exploit / tt_pop_hyper) as far as no GPU is
needed: its code object's budget and its argument checks before any HIP call."""
import ctypes as C
import math

import pytest
import torch

HYP = {"alpha": 1e-4, "beta": 1e-3, "tau": 1e-3, "gamma": 0.99}


def _rec(rets, succ=None):
    rets = torch.tensor(rets, dtype=torch.float64)
    succ = torch.zeros(len(rets), dtype=torch.bool) if succ is None else torch.tensor(succ, dtype=torch.bool)
    return {"ret": rets, "success": succ}


def _hypers(K):
    return [dict(HYP) for _ in range(K)]


def _pbt(K, **kw):
    from ddpg_trucktrailer_amd.pbt import PBT
    kw.setdefault("window", 4)
    return PBT(K, 10, **kw)


def test_selection_is_bottom_m_from_top_m_and_reproducible():
    K = 8
    recs = [_rec([10.0 * a] * 4) for a in range(K)]           # agent a's mean return is 10 a: 7 is the best, 0 the worst
    runs = []
    for _ in range(2):
        p = _pbt(K, seed=5, quantile=0.25)
        p.observe(recs)
        runs.append(p.decide(10, _hypers(K)))
    d = runs[0]
    assert runs[0] == runs[1]
    m = 2                                                     # floor(0.25 * 8)
    assert [x["dst"] for x in d] == [0, 1]                    # worst first
    assert all(x["src"] in (6, 7) for x in d)
    assert {x["dst"] for x in d}.isdisjoint({x["src"] for x in d}) and len(d) == m
    # another seed, many rounds: every src of the top m is drawn
    p = _pbt(K, seed=1)
    seen = set()
    for r in range(1, 30):
        p.observe(recs)
        seen |= {x["src"] for x in p.decide(10 * r, _hypers(K))}
    assert seen == {6, 7}


def test_m_is_at_most_half_of_the_eligible():
    p = _pbt(3, quantile=0.5)
    p.observe([_rec([1.0] * 4), _rec([2.0] * 4), _rec([3.0] * 4)])
    d = p.decide(10, _hypers(3))
    assert [(x["dst"], x["src"]) for x in d] == [(0, 2)]      # m = min(max(1, 1), 1)


def test_no_decision_for_one_agent_or_fewer_than_two_eligible():
    p = _pbt(1, min_episodes=1)
    p.observe([_rec([1.0] * 10)])
    assert p.decide(100, _hypers(1)) == []
    p = _pbt(4)
    p.observe([_rec([1.0] * 4), _rec([5.0] * 3), _rec([]), _rec([9.0])])
    assert p.decide(10, _hypers(4)) == []                     # only agent 0 has window = 4 episodes
    p.observe([_rec([]), _rec([5.0]), _rec([]), _rec([])])
    d = p.decide(11, _hypers(4))                              # retried at the next call: now agents 0 and 1
    assert [(x["dst"], x["src"]) for x in d] == [(0, 1)] and d[0]["step"] == 11


def test_rounds_wait_for_ready_steps():
    p = _pbt(2, min_episodes=1)
    p.observe([_rec([1.0]), _rec([2.0])])
    assert p.decide(9, _hypers(2)) == []
    assert len(p.decide(10, _hypers(2))) == 1
    p.observe([_rec([1.0]), _rec([2.0])])
    assert p.decide(19, _hypers(2)) == [] and len(p.decide(20, _hypers(2))) == 1


def test_ties_go_to_the_lower_index():
    p = _pbt(4, quantile=0.25)
    p.observe([_rec([3.0] * 4) for _ in range(4)])
    d = p.decide(10, _hypers(4))
    assert [(x["dst"], x["src"]) for x in d] == [(3, 0)]


def test_metrics_return_and_success():
    # agent 0: high return, no successes; agent 1: lower return, one success; agent 2: same success rate as 1, higher return
    recs = [_rec([100.0] * 4, [0, 0, 0, 0]), _rec([10.0] * 4, [1, 0, 0, 0]), _rec([20.0] * 4, [0, 0, 1, 0])]
    p = _pbt(3, metric="return", quantile=0.5)
    p.observe(recs)
    d = p.decide(10, _hypers(3))
    assert [(x["dst"], x["src"]) for x in d] == [(1, 0)] and d[0]["src_score"] == (100.0,)
    p = _pbt(3, metric="success", quantile=0.5)
    p.observe(recs)
    d = p.decide(10, _hypers(3))
    assert [(x["dst"], x["src"]) for x in d] == [(0, 2)] and d[0]["src_score"] == (0.25, 20.0)


def test_explore_factors_bounds_and_gamma_in_one_minus_gamma():
    from ddpg_trucktrailer_amd.pbt import BOUNDS
    p = _pbt(2, factors=(2.0,), bounds={"beta": (1e-6, 1.5e-3)})
    p.observe([_rec([1.0] * 4), _rec([2.0] * 4)])
    src = {"alpha": 3e-4, "beta": 1e-3, "tau": 5e-3, "gamma": 0.98}
    d = p.decide(10, [dict(HYP), src])[0]
    assert (d["dst"], d["src"]) == (0, 1) and d["old"] == HYP
    new = d["new"]
    assert math.isclose(new["alpha"], 6e-4) and new["beta"] == 1.5e-3 and math.isclose(new["tau"], 1e-2)
    assert math.isclose(1.0 - new["gamma"], 2.0 * 0.02)
    # lower bounds, and explore limited to some keys (the rest is src's, unchanged)
    p = _pbt(2, factors=(1e-9,), explore=("alpha", "gamma"))
    p.observe([_rec([1.0] * 4), _rec([2.0] * 4)])
    new = p.decide(10, [dict(HYP), src])[0]["new"]
    assert new["alpha"] == BOUNDS["alpha"][0] and new["gamma"] == BOUNDS["gamma"][1]
    assert new["beta"] == src["beta"] and new["tau"] == src["tau"]


def test_window_is_reset_for_dst_only():
    p = _pbt(4, quantile=0.25)
    p.observe([_rec([float(a)] * 6) for a in range(4)])
    assert all(len(w) == 4 for w in p.windows)                # the last `window` episodes
    d = p.decide(10, _hypers(4))
    assert [x["dst"] for x in d] == [0]
    assert len(p.windows[0]) == 0 and all(len(p.windows[a]) == 4 for a in (1, 2, 3))
    assert p.history == d


def test_state_dict_round_trip_reproduces_later_decisions():
    from ddpg_trucktrailer_amd.pbt import PBT
    gen = torch.Generator().manual_seed(3)
    K = 6
    batches = [[_rec((torch.rand(3, generator=gen) * 100).tolist(), (torch.rand(3, generator=gen) < 0.3).tolist())
                for _ in range(K)] for _ in range(12)]
    a = PBT(K, 2, seed=9, window=5, metric="success", quantile=0.34)
    for i in range(6):
        a.observe(batches[i])
        a.decide(2 * (i + 1), _hypers(K))
    b = PBT(K, 2, seed=123, window=5, metric="success", quantile=0.34)
    b.load_state_dict(a.state_dict())
    out_a, out_b = [], []
    for i in range(6, 12):
        for p, out in ((a, out_a), (b, out_b)):
            p.observe(batches[i])
            out.append(p.decide(2 * (i + 1), _hypers(K)))
    assert any(out_a) and out_a == out_b and a.history == b.history


def test_bad_arguments():
    from ddpg_trucktrailer_amd.pbt import PBT
    for kw in (dict(metric="loss"), dict(quantile=0.0), dict(explore=("lr",)), dict(window=4, min_episodes=5), dict(factors=(0.0,))):
        with pytest.raises(ValueError):
            PBT(4, 10, **kw)
    with pytest.raises(ValueError):
        PBT(4, 10).observe([_rec([])] * 3)


# ---- the library -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib as L
    return L


def test_exploit_kernel_has_no_scratch_and_no_spill(lib):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    found = kr.find(kr.kernels(), "13k_pop_exploit")
    assert len(found) == 1, sorted(found)
    (n, v), = found.items()
    assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["max_threads"] == 256, (n, v)


def test_exploit_and_hyper_refuse_a_null_handle(lib):
    dll = lib.load()
    pairs = (lib.TTPopExploitPair * 1)(lib.TTPopExploitPair(1, 0, 1e-4, 1e-3, 1e-3, 0.99))
    assert dll.tt_pop_exploit(None, 1, pairs, None) == lib.TT_EINVAL
    assert b"tt_pop_exploit" in dll.tt_last_error(None) and b"NULL" in dll.tt_last_error(None)
    out = (C.c_float * 4)()
    assert dll.tt_pop_hyper(None, 0, C.byref(out)) == lib.TT_EINVAL
    assert b"tt_pop_hyper" in dll.tt_last_error(None)
