"""CPU: the cases of tests/policy_edges.py really are the edges they claim, and the references agree among themselves.

Nothing here runs a kernel.  tests/test_gpu_policy_edges.py holds the two policy forward kernels to 3 x (the f32 yardstick's
error against f64) + 1e-7; this file shows that the split SCHEME itself (policy_edges.split_model: two rn16 pieces, three
products, no accumulation order) stays inside that yardstick on every finite case, so a kernel that misses it has a fault of
its own.  Measured here (max over the planted rows, actor | critic, against f64):

    case        numpy-f32 error      split-model error
    ordinary    5.2e-07 | 1.2e-06    2.2e-07 | 5.5e-07
    large4000   4.6e-07 | 1.1e-06    1.6e-07 | 5.8e-07
    one4090     2.4e-07 | 8.5e-07    3.8e-07 | 4.3e-07
    mixed       4.4e-07 | 7.6e-07    3.0e-07 | 5.9e-07
    tiny        4.5e-08 | 1.2e-06    4.5e-08 | 4.5e-07
    zero        1.9e-08 | 6.4e-07    4.1e-08 | 2.6e-07
    eps         4.5e-08 | 1.0e-06    4.9e-08 | 9.1e-07
    const       1.1e-08 | 1.1e-06    1.1e-08 | 2.5e-07
    dead        2.2e-08 | 3.8e-07    2.2e-08 | 3.8e-07
    w_near      6.5e-08 | 8.5e-07    1.2e-07 | 6.0e-07
    act_edge    6.1e-07 | 9.4e-05    3.1e-07 | 9.4e-05      (|q| up to 1.0e3: 1e-7 relative)
"""
import numpy as np
import pytest

import policy_edges as E

K = 33                                     # rows per case here: three rounds of the 11 planted positions
FINITE = [c for c, v in E.CASES.items() if v["kind"] == "finite"]
OUTSIDE_ROWS = ("out4096", "out1e6")
_nets = {}


def nets(variant):
    if variant not in _nets:
        _nets[variant] = E.nets(variant)
    return _nets[variant]


def rows_of(case):
    c = E.CASES[case]
    act = (c.get("act") or E.actions_ordinary)(K)
    return c["rows"](K), act


def test_eps_dominated_rows_have_layer1_variance_far_below_eps():
    obs, act = rows_of("eps")
    for net in nets("b1_zero"):
        _, pre1, _ = E.ref64(net, obs, act)
        assert pre1.var(axis=1).max() < 1e-7
        # ... and eps really carries the result: without it the normalised values would be ~30 x larger
        assert (1.0 / np.sqrt(pre1.var(axis=1) + E.EPS)).max() * np.sqrt(pre1.var(axis=1)).max() < 0.1


def test_constant_row_has_variance_exactly_zero_in_f64_and_in_f32():
    obs, act = rows_of("const")
    for net in nets("b1_half"):
        _, pre1, h1 = E.ref64(net, obs, act)
        assert (pre1 == 0.5).all() and (pre1.var(axis=1) == 0).all()
        w1, b1 = net.fc1.weight.detach().numpy(), net.fc1.bias.detach().numpy()
        assert ((obs @ w1.T + b1) == np.float32(0.5)).all()
        # LayerNorm of a constant row is its bias: the hidden layer is relu(bn1.bias) in every row
        assert np.array_equal(h1, np.broadcast_to(np.maximum(net.bn1.bias.detach().double().numpy(), 0), h1.shape))


def test_dead_net_has_an_all_zero_hidden_layer():
    obs, act = rows_of("dead")
    for rows in (obs, E.rows_ordinary(K), E.rows_large(K), E.rows_zero(K)):
        for net in nets("dead"):
            _, _, h1 = E.ref64(net, rows, act)
            assert (h1 == 0).all()


@pytest.mark.parametrize("case", FINITE)
def test_in_range_cases_keep_every_split_operand_finite_in_f16(case):
    obs, _ = rows_of(case)
    for net in nets(E.CASES[case]["variant"]):
        x, h1, w = E.split_operands(net, obs)
        assert E.SX * np.abs(x).max() <= E.F16_MAX and E.SX * np.abs(h1).max() <= E.F16_MAX
        assert E.SW * np.abs(w).max() <= E.F16_MAX
        for operand, scale in ((x, E.SX), (h1.astype(np.float32), E.SX), (w, E.SW)):
            h, m = E.split_pieces(operand, scale)
            assert np.isfinite(h.astype(np.float32)).all() and np.isfinite(m.astype(np.float32)).all()


def test_cases_near_the_range_really_are_near_it():
    assert np.abs(rows_of("one4090")[0]).max() == 4090 and np.abs(rows_of("large4000")[0]).max() > 3900
    a, _ = nets("w_near")
    assert a.fc1.weight.abs().max().item() == 1020 and a.fc2.weight.abs().max().item() == 1022


@pytest.mark.parametrize("case", OUTSIDE_ROWS)
def test_outside_range_rows_make_a_piece_inf_and_the_split_model_nan(case):
    obs, act = rows_of(case)
    h, _ = E.split_pieces(obs, E.SX)
    assert np.isinf(h.astype(np.float32)).any(axis=1).all()                   # every row of the case
    assert np.isfinite(E.split_pieces(E.rows_ordinary(K), E.SX)[0].astype(np.float32)).all()
    for net in nets("base"):
        assert np.isnan(E.split_model(net, obs, act)).all()
        # ... while the row is an ordinary finite one to f32 and f64
        assert np.isfinite(E.numpy_f32(net, obs, act)).all() and np.isfinite(E.ref64(net, obs, act)[0]).all()
        assert np.isfinite(E.torch_f32(net, obs, act)).all()


def test_weight_beyond_the_range_makes_a_piece_inf_and_every_row_nan_in_the_split_model():
    obs, act = rows_of("w_beyond")
    for net in nets("w_beyond"):
        h, _ = E.split_pieces(net.fc2.weight.detach().numpy(), E.SW)
        assert np.isinf(h.astype(np.float32)).sum() == 1
        assert np.isnan(E.split_model(net, obs, act)).all()
        assert np.isfinite(E.numpy_f32(net, obs, act)).all() and np.isfinite(E.torch_f32(net, obs, act)).all()


@pytest.mark.parametrize("case", [c for c, v in E.CASES.items() if v["kind"] == "nonfinite"])
def test_torch_f32_answers_nan_on_exactly_the_non_finite_rows(case):
    obs, act, mask, clean_obs, clean_act = E.build_case(case, E.N_F32, E.F32_POSITIONS)
    assert mask.sum() == len(E.F32_POSITIONS)
    for name, net in zip(("actor", "critic"), nets("base")):
        want = mask if name in E.CASES[case]["nan_for"] else np.zeros_like(mask)
        assert np.array_equal(np.isnan(E.torch_f32(net, obs, act)), want), name
        assert np.array_equal(np.isnan(E.numpy_f32(net, obs, act)), want), name
        assert np.isfinite(E.torch_f32(net, clean_obs, clean_act)).all()


@pytest.mark.parametrize("case", [c for c, v in E.CASES.items() if v["kind"] != "nonfinite"])
def test_torch_f32_is_finite_on_every_other_case(case):
    obs, act = rows_of(case)
    for net in nets(E.CASES[case]["variant"]):
        assert np.isfinite(E.torch_f32(net, obs, act)).all()


@pytest.mark.parametrize("case", FINITE)
def test_split_scheme_stays_inside_the_f32_yardstick(case):
    """The bound of the GPU tests, on the scheme alone: error(split model) <= 3 x error(numpy f32) + 1e-7 (Q: + 1e-6 max(1, |q|))."""
    obs, act = rows_of(case)
    for name, net in zip(("actor", "critic"), nets(E.CASES[case]["variant"])):
        ref = E.ref64(net, obs, act)[0]
        e32 = np.abs(E.numpy_f32(net, obs, act).astype(np.float64) - ref).max()
        esp = np.abs(E.split_model(net, obs, act).astype(np.float64) - ref).max()
        et = np.abs(E.torch_f32(net, obs, act).astype(np.float64) - ref).max()
        floor = 1e-7 if name == "actor" else E.q_floor(ref)
        print(f"{case:10s} {name:6s} numpy-f32 {e32:.1e}  split model {esp:.1e}  torch-f32 {et:.1e}  max|ref| {np.abs(ref).max():.2e}")
        assert esp <= 3 * e32 + floor, (case, name, esp, e32)


def test_plant_overwrites_the_given_rows_only_and_returns_their_mask():
    base = E.rows_ordinary(50)
    before = base.copy()
    mask = E.plant(base, E.rows_zero(3), (0, 17, 49))
    assert mask.sum() == 3 and mask[[0, 17, 49]].all()
    assert (base[mask] == 0).all() and np.array_equal(base[~mask], before[~mask])
    obs, act, mask, clean_obs, clean_act = E.build_case("act_nan", E.N_SPLIT, E.SPLIT_POSITIONS(E.N_SPLIT))
    assert np.array_equal(np.flatnonzero(mask), sorted(E.SPLIT_POSITIONS(E.N_SPLIT)))
    assert np.array_equal(obs[~mask], clean_obs[~mask]) and np.array_equal(act[~mask], clean_act[~mask])
    assert np.isnan(act[mask]).all() and np.isfinite(clean_act).all() and not np.array_equal(obs[mask], clean_obs[mask])
