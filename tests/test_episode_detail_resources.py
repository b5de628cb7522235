"""CPU: the detailed episode log's kernels, C-ABI argument checks and objectives (include/ttenv.h: tt_env_set_episode_log2).

* k_step_tally has its 16 variants, and the ones the loop launches (PER_ENV = INFO = false) keep four waves per SIMD with no
  scratch and no spill -- the bar k_step and k_step_log are held to;
* the plain log's kernels (k_step_log, k_log_zero, k_log_drain) keep the resource rows they had before the detailed log
  (tests/golden/kernel_resources_step_log.json);
* bad arguments are TT_EINVAL with a message before any HIP call (no GPU here);
* episode_metrics restates viz_how_agent_learn.compute_metrics and its 100-episode running averages."""
import ctypes as C
import json
import os
from collections import deque

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def ks(lib):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    return kr.kernels()


def test_tally_kernel_has_sixteen_variants_and_is_not_matched_as_the_others(ks):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    tally = kr.find(ks, "12k_step_tally")
    assert len(tally) == 16, sorted(tally)
    assert not [n for n in tally if "10k_step_log" in n or "6k_step" in n]


def test_loop_variants_of_the_tally_kernel_keep_four_waves_per_simd(ks):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    loop = kr.find(ks, "12k_step_tallyILb0ELb0E")
    assert len(loop) == 4
    for n, v in loop.items():
        assert v["vgpr"] <= 128 and kr.waves_per_simd(v["vgpr"]) >= 4, (n, v)
        assert v["scratch"] == 0 and v["vgpr_spills"] == 0, (n, v)
    for n, v in kr.find(ks, "12k_step_tally").items():
        assert v["vgpr_spills"] == 0, (n, v)


def test_plain_log_kernels_are_unchanged(ks):
    before = json.load(open(os.path.join(GOLDEN, "kernel_resources_step_log.json")))
    assert len(before) == 18
    changed = {n: (v, ks.get(n)) for n, v in before.items() if ks.get(n) != v}
    assert not changed, changed


def test_arguments_are_refused_before_any_hip_call(lib):
    dll = lib.load()
    assert lib.LOG_COMPONENTS == lib.INFO_ROWS[1:10] and len(lib.LOG_COMPONENTS) == 9
    # unknown flag bits come first: no handle is needed to see them
    for bad in (2, 0x80000000, lib.LOG_DETAIL | 4):
        assert dll.tt_env_set_episode_log2(None, 64, bad, None) == lib.TT_EINVAL
        assert b"unknown flag bits" in dll.tt_last_error(None)
    assert dll.tt_env_set_episode_log2(None, 64, lib.LOG_DETAIL, None) == lib.TT_EINVAL
    assert b"tt_env_set_episode_log2: NULL handle" in dll.tt_last_error(None)
    assert dll.tt_env_set_episode_log2(None, 64, 0, None) == lib.TT_EINVAL
    out = C.c_void_p(0x1000)
    assert dll.tt_env_drain_episode_log2(None, out, out, out, out, out, out, out, out, out, out, None) == lib.TT_EINVAL
    assert b"tt_env_drain_episode_log2: NULL handle" in dll.tt_last_error(None)
    # the plain entry point keeps its own name in its messages
    assert dll.tt_env_drain_episode_log(None, None, None, None, None, None, None, None, None, None) == lib.TT_EINVAL
    assert b"tt_env_drain_episode_log: NULL handle" in dll.tt_last_error(None)


def compute_metrics(steps):
    """viz_how_agent_learn.py:13-33 written out over a list of per-step reward_info dicts."""
    s = lambda k: sum([st[k] for st in steps])
    efficiency = s("progress_reward") + s("staged_success") + s("exploration_bonus") + s("final_success_bonus") + \
        s("backward_penalty")
    return efficiency, s("smoothness_penalty"), s("heading_reward") + s("orientation_reward"), s("safety_penalty")


def test_objectives_and_running_averages_follow_the_reference(lib):
    import torch
    from ddpg_trucktrailer_amd import episode_metrics as em
    rng = np.random.RandomState(4)
    names = lib.LOG_COMPONENTS
    episodes = []
    for _ in range(260):
        steps = [{k: float(rng.normal(0, 30)) for k in names} for _ in range(rng.randint(1, 12))]
        episodes.append(steps)
    # what the detailed log records: each term summed in step order
    comp = np.array([[sum([st[k] for st in ep]) for k in names] for ep in episodes])
    want = np.array([compute_metrics(ep) for ep in episodes])
    got = em.objectives({"components": torch.from_numpy(comp)})
    for j, k in enumerate(em.OBJECTIVES):
        assert np.allclose(got[k].numpy(), want[:, j], rtol=1e-12, atol=1e-9), k
    # plot_running_average: deque(maxlen=100) per objective, averaged after every episode -- fed in uneven drains
    hist = [deque(maxlen=100) for _ in em.OBJECTIVES]
    ref = []
    for row in want:
        for h, x in zip(hist, row):
            h.append(x)
        ref.append([np.mean(h) for h in hist])
    ref = np.array(ref)
    run = em.RunningObjectives()
    assert run.last() == {k: None for k in em.OBJECTIVES}
    k0, parts = 0, []
    for cut in (1, 40, 99, 100, 101, 230, 260):
        parts.append(run.update({"components": torch.from_numpy(comp[k0:cut])}))
        k0 = cut
    for j, k in enumerate(em.OBJECTIVES):
        series = np.concatenate([p[k].numpy() for p in parts])
        assert np.allclose(series, ref[:, j], rtol=1e-10, atol=1e-8), k
        assert abs(run.last()[k] - ref[-1, j]) <= 1e-8 * max(1.0, abs(ref[-1, j]))
    with pytest.raises(ValueError):
        em.objectives({"components": torch.zeros(5, 8, dtype=torch.float64)})
