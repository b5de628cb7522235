"""Register budgets of the hot kernels, read from the code objects inside libttenv.so (no GPU needed).

The loop's speed hangs on a few occupancy facts that no numerics test sees (DESIGN.md sections 4.1, 4.2): the policy kernel must not
spill (one wave per SIMD, all 512 registers: a spilled build ran at 0.144 ms per step instead of 0.085), the weight-gradient
kernels must fit THREE workgroups on a CU (<= 168 registers: beside the policy's 171 workgroups 85 CUs are free for their 200-210;
the actor's variant sat at 192 for three rounds and its last 30 workgroups started 5 us late), the row kernels two waves per SIMD
(eight waves per workgroup), the env step four."""
import pytest

from ddpg_trucktrailer_amd import kernel_resources as kr


@pytest.fixture(scope="module")
def ks():
    out = kr.kernels()
    assert len(out) >= 40, "the library's gfx950 code objects were not found"
    return out


def the(ks, *parts):
    found = kr.find(ks, *parts)
    assert found, f"no kernel named like {parts}"
    return found


def test_no_kernel_spills_vector_registers(ks):
    bad = {n: v["vgpr_spills"] for n, v in ks.items() if v["vgpr_spills"]}
    assert not bad, bad


def test_policy_kernel_takes_one_wave_per_simd_without_scratch_traffic(ks):
    for n, v in the(ks, "k_mlp_split").items():
        assert v["vgpr"] <= 512 and v["vgpr_spills"] == 0, (n, v)
        assert v["scratch"] <= 16, (n, v)          # (a few spilled SGPRs' worth of lanes, no vector spill)


def test_weight_gradient_kernels_fit_three_workgroups_per_cu(ks):
    for n, v in the(ks, "k_bwd_weights").items():
        assert v["vgpr"] <= 168 and kr.waves_per_simd(v["vgpr"]) >= 3, (n, v)
        assert v["scratch"] == 0 and 3 * v["lds"] <= 160 * 1024, (n, v)


def test_row_kernels_fit_their_eight_waves_on_a_cu(ks):
    for part in ("k_fwd_multi", "k_fwd_small", "k_bwd_rows_pair", "k_actor_tail"):
        for n, v in the(ks, part).items():
            assert kr.waves_per_simd(v["vgpr"]) >= 2 and v["scratch"] == 0 and v["lds"] <= 160 * 1024, (n, v)


def test_env_step_of_the_loop_keeps_four_waves_per_simd(ks):
    # k_step<PER_ENV = false, INFO = false, AUTO_RESET, RANDOM_POLICY>: the variants bench.py and the DDPG loop launch
    for n, v in the(ks, "6k_stepILb0ELb0E").items():
        assert kr.waves_per_simd(v["vgpr"]) >= 4 and v["scratch"] == 0, (n, v)


def test_text_sections_lists_every_code_object_once_and_is_stable():
    """One (size, sha256) per code object, in the order of build.SRC: hipcc makes one code object per source that defines a kernel
    (csrc/ttp2p.hip is host code only and has none), so that is what the library must hold.  The table is what
    `kernel_resources --text before.so after.so` compares (csrc/ttlearn_sites.h)."""
    from ddpg_trucktrailer_amd import build

    with_kernels = [p for p in build.SRC if "__global__" in open(p).read()]
    assert len(build.SRC) - len(with_kernels) <= 1, "more than ttp2p.hip without a kernel: look at this test's premise"
    ts = kr.text_sections()
    assert len(ts) == len(with_kernels)
    for size, digest in ts:
        assert size > 0 and len(digest) == 64 and int(digest, 16) >= 0
    assert kr.text_sections() == ts


def test_build_hdr_holds_every_header_the_sources_include():
    """build.stale() and build_variant() compare the library's time with build.SRC + build.HDR: a header missing from HDR lets an
    edit of it pass for a fresh library.  Followed from every source through the quoted #include lines (the angle-bracket ones are
    the toolchain's), each must resolve -- next to the including file or under include/, as the compiler looks -- to a file of
    HDR; and HDR holds every csrc/*.h, included yet or not."""
    import glob
    import os
    import re

    from ddpg_trucktrailer_amd import build

    hdr = {os.path.realpath(p) for p in build.HDR}
    assert len(hdr) == len(build.HDR) and all(os.path.isfile(p) for p in hdr)
    quoted = re.compile(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', re.M)
    todo, seen = [os.path.realpath(p) for p in build.SRC], set()
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.add(path)
        for name in quoted.findall(open(path).read()):
            places = [os.path.join(os.path.dirname(path), name), os.path.join(build.ROOT, "include", name)]
            found = [os.path.realpath(p) for p in places if os.path.isfile(p)]
            assert found, f"{path} includes \"{name}\", which is neither next to it nor under include/"
            assert found[0] in hdr, f"{path} includes {found[0]}, which build.HDR does not list"
            todo.append(found[0])
    assert len(seen) > len(build.SRC), "no #include line was followed: look at this test's pattern"
    csrc = glob.glob(os.path.join(build.HERE, "csrc", "*.h"))
    assert csrc and {os.path.realpath(p) for p in csrc} <= hdr
