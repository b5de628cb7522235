"""GPU (-m gpu): the two policy forward kernels -- split-f16 k_mlp_split (csrc/ttnet_split.hip) and exact-f32 k_mlp_forward_v2
(csrc/ttnet.hip) -- on the rows of tests/policy_edges.py: at the edge of the split's stated range, where LayerNorm's eps carries
the result, beyond the range, and not finite; PLANTED among ordinary rows at the seams of the kernels' tiles.

Geometries: "split" = n 1079 through fused.actor_forward / critic_forward (9 tiles of 128 rows, the last ragged, one per
workgroup); "split_wg2" = the same rows through the packed entry points on max_workgroups = 2 (chains of 5 and 4 tiles: the
planted rows 128.. sit in tiles whose observations were loaded a tile ahead); "f32_200" / "f32_1079" = under fused.exact_f32
(n 200: three workgroups of 64 rows + 8).  Planted rows: policy_edges.SPLIT_POSITIONS / F32_POSITIONS.

(a) accuracy, every row: |kernel - f64| <= 3 x max(error of the torch f32 modules on the GPU, error of policy_edges.numpy_f32)
    on that case + 1e-7 (Q: + 1e-6 x max(1, max |q|)) -- the factor and constants of
    test_gpu_fused_net.py::test_split_f16_kernel_is_f32_accurate; no kernel under test is part of the yardstick;
(b) isolation: every row that is not planted has the same BITS as in a second run whose planted rows are ordinary ones;
(c) the contract: a row is NaN exactly where the torch f32 module's is -- plus, for the split kernel, the rows beyond its
    range (a weight beyond the range: every row); the exact-f32 kernel stays inside (a) on those;
(d) fused.actor_act with noise: mu, raw and scaled are NaN on a non-finite row (torch.clamp(raw, -1, 1) * high), whose OU state
    advances as ever; every other row's raw, scaled and OU state keep their bits.

Measured on MI355X.  Each cell: max error over all rows that have a number, max error over the planted rows alone (NaN: they
have none), the bound; the split kernel's two geometries give the same bits, hence one column:

    case       net     split (both geometries)    exact f32, n 200           exact f32, n 1079
    ordinary   actor   1.0e-06 4.3e-07 4.5e-06    6.3e-07 3.5e-07 2.0e-06    1.2e-06 3.5e-07 4.5e-06
    ordinary   critic  1.5e-06 7.3e-07 1.1e-05    1.2e-06 6.8e-07 7.4e-06    2.1e-06 6.3e-07 1.1e-05
    large4000  actor   1.0e-06 4.2e-07 4.5e-06    6.3e-07 4.1e-07 2.0e-06    1.2e-06 4.1e-07 4.5e-06
    large4000  critic  1.5e-06 4.9e-07 1.1e-05    1.2e-06 4.6e-07 7.4e-06    2.1e-06 5.4e-07 1.1e-05
    one4090    actor   1.0e-06 1.2e-07 4.5e-06    6.3e-07 4.2e-07 3.3e-06    1.2e-06 4.2e-07 4.5e-06
    one4090    critic  1.5e-06 6.4e-07 1.1e-05    1.2e-06 8.5e-07 7.4e-06    2.1e-06 8.6e-07 1.1e-05
    mixed      actor   1.0e-06 8.4e-07 4.9e-06    6.3e-07 5.3e-07 2.0e-06    1.2e-06 1.2e-06 4.9e-06
    mixed      critic  1.5e-06 5.5e-07 1.1e-05    1.2e-06 6.2e-07 7.4e-06    2.1e-06 9.2e-07 1.1e-05
    tiny       actor   1.0e-06 3.4e-08 4.5e-06    6.3e-07 3.2e-08 2.0e-06    1.2e-06 3.2e-08 4.5e-06
    tiny       critic  1.5e-06 5.4e-07 1.1e-05    1.2e-06 6.3e-07 7.4e-06    2.1e-06 7.7e-07 1.1e-05
    zero       actor   1.0e-06 1.9e-08 4.5e-06    6.3e-07 1.9e-08 2.0e-06    1.2e-06 1.9e-08 4.5e-06
    zero       critic  1.5e-06 4.0e-07 1.1e-05    1.2e-06 4.7e-07 7.4e-06    2.1e-06 4.0e-07 1.1e-05
    eps        actor   1.0e-06 2.9e-08 4.7e-06    7.8e-07 2.8e-08 2.8e-06    9.7e-07 2.9e-08 4.7e-06
    eps        critic  1.6e-06 1.0e-06 9.8e-06    1.2e-06 6.8e-07 7.3e-06    1.5e-06 6.1e-07 9.8e-06
    const      actor   3.6e-06 1.1e-08 5.3e-06    1.5e-06 1.7e-07 3.7e-06    1.5e-06 1.7e-07 5.3e-06
    const      critic  3.8e-06 2.4e-07 1.0e-05    3.3e-06 3.3e-06 1.0e-05    3.4e-06 3.4e-06 1.0e-05
    dead       actor   2.2e-08 2.2e-08 2.1e-07    2.2e-08 2.2e-08 2.1e-07    2.2e-08 2.2e-08 2.1e-07
    dead       critic  8.0e-07 5.9e-07 8.1e-06    5.5e-07 2.3e-07 7.4e-06    5.8e-07 3.6e-07 8.1e-06
    w_near     actor   2.2e-07 6.8e-08 1.3e-06    1.4e-07 1.2e-07 1.2e-06    2.0e-07 1.2e-07 1.3e-06
    w_near     critic  1.7e-06 7.2e-07 1.1e-05    1.4e-06 6.7e-07 8.0e-06    1.1e-06 7.3e-07 1.1e-05
    act_edge   actor   1.0e-06 3.3e-07 4.5e-06    6.3e-07 3.3e-07 2.0e-06    1.2e-06 3.3e-07 4.5e-06
    act_edge   critic  1.3e-04 1.3e-04 1.5e-03    7.3e-05 7.3e-05 1.4e-03    7.3e-05 7.3e-05 1.5e-03
    out4096    actor   1.0e-06 NaN     4.5e-06    6.3e-07 6.2e-07 2.0e-06    1.2e-06 6.2e-07 4.5e-06
    out4096    critic  1.5e-06 NaN     1.1e-05    1.2e-06 8.0e-07 7.4e-06    2.1e-06 7.8e-07 1.1e-05
    out1e6     actor   1.0e-06 NaN     4.5e-06    6.3e-07 2.3e-07 2.0e-06    1.2e-06 5.7e-07 4.5e-06
    out1e6     critic  1.5e-06 NaN     1.1e-05    1.2e-06 4.1e-07 7.4e-06    2.1e-06 5.6e-07 1.1e-05
    w_beyond   actor   all rows NaN               3.3e-07 4.9e-08 1.3e-06    1.6e-06 4.9e-08 4.8e-06
    w_beyond   critic  all rows NaN               2.6e-06 5.8e-07 1.5e-05    6.0e-06 8.1e-07 9.3e-05
    nan        actor   1.0e-06 NaN     4.5e-06    6.3e-07 NaN     2.0e-06    1.2e-06 NaN     4.5e-06
    nan        critic  1.5e-06 NaN     1.1e-05    1.2e-06 NaN     7.4e-06    2.1e-06 NaN     1.1e-05
    pinf       actor   1.0e-06 NaN     4.5e-06    6.3e-07 NaN     2.0e-06    1.2e-06 NaN     4.5e-06
    pinf       critic  1.5e-06 NaN     1.1e-05    1.2e-06 NaN     7.4e-06    2.1e-06 NaN     1.1e-05
    ninf       actor   1.0e-06 NaN     4.5e-06    6.3e-07 NaN     2.0e-06    1.2e-06 NaN     4.5e-06
    ninf       critic  1.5e-06 NaN     1.1e-05    1.2e-06 NaN     7.4e-06    2.1e-06 NaN     1.1e-05
    act_nan    actor   1.0e-06 7.0e-07 4.5e-06    6.3e-07 4.6e-07 2.0e-06    1.2e-06 4.6e-07 4.5e-06
    act_nan    critic  1.5e-06 NaN     1.1e-05    1.2e-06 NaN     7.4e-06    2.1e-06 NaN     1.1e-05
"""
import ctypes as C
import math

import numpy as np
import pytest

import policy_edges as E

pytestmark = pytest.mark.gpu

GEOMETRIES = ("split", "split_wg2", "f32_200", "f32_1079")
_nets, _clean = {}, {}


def _gpu_nets(dev, variant):
    """{"actor": (cpu module, gpu module), "critic": ...} of one variant, the packed images made once."""
    if variant not in _nets:
        from ddpg_trucktrailer_amd import fused
        a, c = E.nets(variant)
        ga, gc = E.to_device(a, dev), E.to_device(c, dev)
        assert fused.supported(ga) and fused.supported(gc)
        fused.pack(ga, 1)
        fused.pack(gc, 1)
        _nets[variant] = {"actor": (a, ga), "critic": (c, gc)}
    return _nets[variant]


def _run(net, geometry, obs, act):
    """One forward of `net` on the GPU through `geometry` -> out [n] (a fresh tensor)."""
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    from ddpg_trucktrailer_amd import fused
    critic, n = hasattr(net, "q"), obs.shape[0]
    if geometry == "split_wg2":
        w = fused.packed_weights_of(net, 1, 2, 0)
        out = torch.full((n,), 12345.0, device=obs.device)
        stream = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        if critic:
            L.check(L.load().tt_critic_forward(n, C.c_void_p(obs.data_ptr()), C.c_void_p(act.data_ptr()), C.byref(w),
                                               C.c_void_p(out.data_ptr()), stream))
        else:
            L.check(L.load().tt_actor_forward(n, C.c_void_p(obs.data_ptr()), C.byref(w), C.c_void_p(out.data_ptr()), stream))
        fused.packed_weights_of(net, 1, 0, 0)
        return out
    if geometry == "split":
        assert n >= 1024
        return (fused.critic_forward(net, obs, act) if critic else fused.actor_forward(net, obs)).view(-1).clone()
    with fused.exact_f32(net):
        return (fused.critic_forward(net, obs, act) if critic else fused.actor_forward(net, obs)).view(-1).clone()


def _shape(geometry):
    return (E.N_F32, E.F32_POSITIONS) if geometry == "f32_200" else (E.N_SPLIT, E.SPLIT_POSITIONS(E.N_SPLIT))


def _same_bits(a, b):
    """Row by row: the same 32 bits (two NaNs count as the same whatever their payload)."""
    import torch
    return (a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))


@pytest.mark.parametrize("case", list(E.CASES))
def test_planted_rows_accuracy_isolation_and_nan_contract(gpu_device, case):
    import torch
    spec = E.CASES[case]
    nets = _gpu_nets(gpu_device, spec["variant"])
    refs = {}
    for geometry in GEOMETRIES:
        n, positions = _shape(geometry)
        obs_h, act_h, mask, clean_obs_h, clean_act_h = E.build_case(case, n, positions)
        obs, act = torch.from_numpy(obs_h).to(gpu_device), torch.from_numpy(act_h).to(gpu_device)
        planted = torch.from_numpy(mask).to(gpu_device)
        for name in ("actor", "critic"):
            cpu_net, net = nets[name]
            if (n, name) not in refs:          # the references of this case: once per row count, shared by the geometries
                with torch.no_grad():
                    out_t = (net(obs, act) if name == "critic" else net(obs)).view(-1).double().cpu().numpy()
                refs[(n, name)] = (E.ref64(cpu_net, obs_h, act_h)[0], out_t, E.numpy_f32(cpu_net, obs_h, act_h).astype(np.float64))
            ref, out_t, out_np = refs[(n, name)]
            out = _run(net, geometry, obs, act)
            # (c) which rows are NaN
            torch_nan = np.isnan(out_t)
            designed = mask if name in spec.get("nan_for", ()) else np.zeros_like(mask)
            assert np.array_equal(torch_nan, designed), (case, name, "the torch f32 module is not NaN where the case says")
            want_nan = torch_nan.copy()
            if geometry.startswith("split") and spec["kind"] == "outside":
                want_nan |= np.ones_like(mask) if case == "w_beyond" else mask
            got_nan = torch.isnan(out).cpu().numpy()
            assert np.array_equal(got_nan, want_nan), (case, name, geometry, "NaN rows", np.flatnonzero(got_nan != want_nan)[:20])
            # (a) every row that has a number: against f64, the yardstick's own error on the same rows
            rows = ~want_nan
            if rows.any():
                err = np.abs(out.double().cpu().numpy() - ref)[rows]
                yard = max(np.abs(out_t - ref)[rows].max(), np.abs(out_np - ref)[rows].max())
                bound = 3 * yard + (1e-7 if name == "actor" else E.q_floor(ref[rows]))
                line = f"{case:10s} {name:6s} {geometry:9s} error {err.max():.2e}  bound {bound:.2e}"
                # (printed, not asserted: the same figures over the planted rows alone.  Eleven rows -- in "const", for the actor,
                # eleven times the SAME row -- are too few for their own yardstick: there the exact-f32 kernel misses f64 by
                # 1.7e-7 = 2.8 ulp of a tanh output of 0.99 where numpy's and torch's f32 happen to miss it by 1.1e-8.)
                sub = rows & mask
                if sub.any():
                    err_p = np.abs(out.double().cpu().numpy() - ref)[sub]
                    yard_p = max(np.abs(out_t - ref)[sub].max(), np.abs(out_np - ref)[sub].max())
                    bound_p = 3 * yard_p + (1e-7 if name == "actor" else E.q_floor(ref[sub]))
                    line += f"   planted rows: error {err_p.max():.2e}  bound {bound_p:.2e}"
                print(line)
                assert (err <= bound).all(), (case, name, geometry, float(err.max()), bound, np.flatnonzero(rows)[err > bound][:20])
            else:
                print(f"{case:10s} {name:6s} {geometry:9s} every row NaN")
            # (b) the other rows do not know what was planted
            key = (spec["variant"], geometry, name)
            if key not in _clean:
                _clean[key] = _run(net, geometry, torch.from_numpy(clean_obs_h).to(gpu_device), torch.from_numpy(clean_act_h).to(gpu_device))
            same = _same_bits(out, _clean[key])
            assert same[~planted].all(), (case, name, geometry, "rows changed by their neighbours",
                                          torch.nonzero(~same & ~planted).view(-1)[:20].tolist())
            # (the planted rows really were other rows -- except where no row can differ: the dead net's output does not depend on
            # the observation, and beyond-range weights leave the split kernel nothing but NaN)
            if case != "dead" and not (case == "w_beyond" and geometry.startswith("split")):
                assert not same[planted].all()


@pytest.mark.parametrize("geometry", ["split_wg2", "f32_200"])
def test_choose_action_keeps_nan_rows_nan_and_their_neighbours_bits(gpu_device, geometry):
    """(d): fused.actor_act with noise -- n 1079 on two workgroups of the split kernel (finish_row_noise), n 200 on the
    exact-f32 kernel (finish_row).  Planted rows: one component NaN, +inf, -inf in turn."""
    import contextlib
    import torch
    from ddpg_trucktrailer_amd import fused
    _, actor = _gpu_nets(gpu_device, "base")["actor"]
    n, positions = _shape(geometry)
    clean_h = E.rows_ordinary(n, 100 + n)
    obs_h = clean_h.copy()
    mask = E.plant(obs_h, E.rows_nonfinite(len(positions)), positions)
    planted = torch.from_numpy(mask).to(gpu_device)
    high = float(np.float32(math.pi / 4))
    ou0 = torch.from_numpy(np.random.RandomState(5).normal(0, 0.1, n).astype(np.float32)).to(gpu_device)
    runs = []
    for rows in (obs_h, clean_h):
        obs = torch.from_numpy(rows).to(gpu_device)
        ou = ou0.clone()
        raw, scaled, mu = (torch.full((n,), 12345.0, device=gpu_device) for _ in range(3))
        steps = []
        if geometry == "split_wg2":
            w, ctx = fused.packed_weights_of(actor, 1, 2, 0), contextlib.nullcontext()
        else:
            w, ctx = None, fused.exact_f32(actor)
        with ctx:
            for step in range(3):
                fused.actor_act(actor, obs, ou, raw, scaled, seed=27, step=step, mu_out=mu, high=high, weights=w)
                steps.append((mu.clone(), raw.clone(), scaled.clone(), ou.clone()))
        fused.packed_weights_of(actor, 1, 0, 0)
        runs.append(steps)
    for step, ((mu, raw, scaled, ou), (mu_c, raw_c, scaled_c, ou_c)) in enumerate(zip(*runs)):
        for name, x in (("mu", mu), ("raw", raw), ("scaled", scaled)):
            assert torch.isnan(x[planted]).all(), (geometry, step, name, "a non-finite row came out finite")
            assert torch.isfinite(x[~planted]).all(), (geometry, step, name)
        assert torch.isfinite(ou).all() and torch.equal(ou.view(torch.int32), ou_c.view(torch.int32)), (geometry, step, "OU state")
        assert (ou != (ou0 if step == 0 else runs[0][step - 1][3])).all()          # ... and advanced in every row
        # the reference's own arithmetic on what the kernel stored: clip(raw, -1, 1) * high, NaN kept (trainv2.py:516)
        ref_scaled = torch.clamp(raw, -1, 1) * high
        assert _same_bits(scaled, ref_scaled).all() and torch.isnan(ref_scaled[planted]).all()
        for name, x, y in (("mu", mu, mu_c), ("raw", raw, raw_c), ("scaled", scaled, scaled_c)):
            assert torch.equal(x[~planted].view(torch.int32), y[~planted].view(torch.int32)), (geometry, step, name)
        assert torch.isfinite(scaled_c).all() and torch.allclose(raw_c, mu_c + ou_c, atol=1e-7)
