"""CPU: the four kernels of the TD3 learner (csrc/tttd3.hip) exist in libttenv.so with the budgets of the launches they are modelled on
(tests/test_kernel_resources.py, tests/test_population_resources.py): the weight-gradient launch fits three workgroups per CU, the
three row kernels keep two waves per SIMD, and nothing spills."""
import pytest


@pytest.fixture(scope="module")
def ks():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import kernel_resources as kr
    return kr.kernels()


def _one(ks, part):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    found = kr.find(ks, part)
    assert len(found) == 1, (part, sorted(found))
    return next(iter(found.items()))


def test_the_four_td3_kernels_exist(ks):
    names = sorted(n for n in ks if "k_td3_" in n)
    assert len(names) == 4, names
    for part in ("15k_td3_fwd_multi", "14k_td3_bwd_rows", "17k_td3_bwd_weights", "16k_td3_actor_tail"):
        _one(ks, part)


@pytest.mark.parametrize("part", ["15k_td3_fwd_multi", "14k_td3_bwd_rows", "16k_td3_actor_tail"])
def test_td3_row_kernels_keep_two_waves_per_simd(ks, part):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    n, v = _one(ks, part)
    assert v["max_threads"] == 512 and kr.waves_per_simd(v["vgpr"]) >= 2, (n, v)
    assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["lds"] <= 160 * 1024, (n, v)


def test_td3_weight_kernel_fits_three_workgroups_per_cu(ks):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    n, v = _one(ks, "17k_td3_bwd_weights")
    assert v["vgpr"] <= 168 and kr.waves_per_simd(v["vgpr"]) >= 3, (n, v)
    assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and 3 * v["lds"] <= 160 * 1024, (n, v)
