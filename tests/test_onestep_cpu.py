"""CPU: the one-step reference (tests/onestep_ref.py) and its fixture (tests/golden/f9_onestep.npz) against code the project
already trusts, and the teeth of the bound that tests/test_gpu_onestep.py holds the HIP kernel to.

  * the fixture regenerates bit for bit from tests/onestep_cases.py;
  * oracle.simv2_twin.FixedStepTwin and the C oracle, stepped once from the fixture's raw states in S1, S2 and S5, land within
    0.5 ulp64(new state) + 1 * E_q of the fixture and give its f32 observations; the twin's reward_step agrees with the
    reference's reward mirror on the S6 lanes through all four steps, up to the f32 ulp of its library atan2f;
  * E_q (the reference at float64 against itself at longdouble, S1, increments before the add) reproduces;
  * negative controls: the float64 reference run on a local copy of tt_sincos's scheme passes the kernel's bound
    (0.5 ulp + 4 E_q) as it stands and FAILS it with the sin series cut at x^11; the longdouble reference with the headings
    reduced by `psi - k * fl(2 pi)` instead of exactly FAILS it on the wound lanes."""
import functools
import os

import numpy as np
import pytest

import onestep_cases as K
import onestep_ref as R
from conftest import GOLDEN
from oracle import c_oracle, simv2_twin

LD, F64, F32 = R.LD, R.F64, R.F32
needs_x87 = pytest.mark.skipif(np.finfo(LD).eps >= 2e-19, reason="np.longdouble is not the 80-bit extended format on this machine")


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLDEN, "f9_onestep.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def lanes_of(*strata):
    return np.flatnonzero(np.isin(fixture()["stratum"], strata))


def state_ratio(new_f64, lanes, factor, E=None, unreduced=False):
    """|new state - fixture| / (0.5 ulp64 + factor * E_q), [len(lanes), 6], the subtraction in longdouble (exact to 2**-64).
    E: the fixture's yardstick (the kernel's bound) unless given.
    unreduced: the twin and the C oracle round each stage's headings y0 + h sum(a k) at ulp(psi), the reference (and E_q) at
    ulp(psi - 2 pi k); S2's seams reach 4 pi.  A stage heading off by half the difference d = ulp(psi) - ulp(reduced psi) moves
    a position increment by h |v| b_s d / 2, summed over the five later stages (sum |b_s| = 1.55) 0.31 d, and through the hitch
    the trailer's heading increment by h |v| / L2 * 1.55 * d <= 0.09 d: that much is added to their bound."""
    fx = fixture()
    ref = R.join(fx["new_hi"][lanes], fx["new_lo"][lanes])
    bound = K.state_bound(ref, fx["E"] if E is None else E, factor)
    if unreduced:
        psi = fx["state0"][lanes, :2]
        red = psi - 2 * np.pi * np.round(psi[:, 1:] / (2 * np.pi))
        d = (R.ulp64(psi) - R.ulp64(red)).clip(0).max(-1)
        bound = bound + d[:, None] * np.array([0, 0.09, 0.31, 0.31, 0.31, 0.31])
    return (np.abs(np.asarray(new_f64, F64).astype(LD) - ref) / bound.astype(LD)).astype(F64)


def own_yardstick(lanes):
    """E_q of the twin's formula on the lanes it is checked on: the reference at float64 (FixedStepTwin.integrate operation for
    operation) against the fixture's longdouble increments, before the add.  The fixture's E_q is the same figure over S1 alone,
    a maximum over 160 lanes that three times as many other lanes exceed by a third."""
    fx = fixture()
    got = R.step(fx["state0"][lanes], fx["actions"][0, lanes], fx["goal"][lanes], fx["L2"][lanes], F64)["inc"]
    return np.abs(got.astype(LD) - R.join(fx["inc_hi"][lanes], fx["inc_lo"][lanes])).max(0).astype(F64)


@needs_x87
def test_fixture_regenerates_bit_for_bit():
    fx, fresh = fixture(), K.build_fixture()
    assert sorted(fx) == sorted(fresh)
    for k in fx:
        a, b = fx[k], np.asarray(fresh[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert os.path.getsize(os.path.join(GOLDEN, "f9_onestep.npz")) < 1_000_000
    assert (fx["redraws"] < K.REDRAW_CAP * K.PER).all()


@needs_x87
def test_yardsticks_reproduce():
    """E_q is measured from the reference alone; the figures (headings 1.8e-17, positions 1.3e-16 to 1.8e-16) are the rounding of
    an f64 chain of about ten operations on increments of 0.08 rad and 0.4 m."""
    fx = fixture()
    s1 = lanes_of(K.S1)
    want = R.step(fx["state0"][s1], fx["actions"][0, s1], fx["goal"][s1], fx["L2"][s1], LD)["inc"]
    assert np.array_equal(R.split(want)[0], fx["inc_hi"][s1])
    got = R.step(fx["state0"][s1], fx["actions"][0, s1], fx["goal"][s1], fx["L2"][s1], F64)["inc"]
    E = np.abs(got.astype(LD) - want).max(0).astype(F64)
    print("E_q", E.tolist())
    assert np.array_equal(E, fx["E"])
    assert (E[:2] < 8 * 2.0 ** -53 * 0.08).all() and (E[2:] < 8 * 2.0 ** -53 * 0.4).all()     # under eight roundings of the increment


def _twin_step(lanes):
    fx = fixture()
    states, obs, obs0 = [], [], []
    for i in lanes:
        tw = simv2_twin.FixedStepTwin()
        tw.set_pose(fx["start"][i], goal=fx["goal"][i], L2=float(fx["L2"][i]), state=fx["state0"][i])
        obs0.append(simv2_twin.observation(tw.state, F64(fx["actions"][0, i]), (tw.goalx, tw.goaly, tw.goalyaw), tw.p))
        o, *_ = tw.step(np.array([fx["actions"][0, i]], F32))
        states.append(tw.state)
        obs.append(o)
    return np.array(states), np.array(obs), np.array(obs0)


def _check_trusted(tag, states, obs, obs0, lanes):
    fx = fixture()
    E = own_yardstick(lanes)
    r = state_ratio(states, lanes, 1, E, unreduced=True)
    print(f"RATIOS {tag} state / (0.5 ulp + 1 E_q) per component", r.max(0).round(3).tolist(), "own E_q", E.tolist(),
          "; against the fixture's E_q", state_ratio(states, lanes, 1).max(0).round(3).tolist())
    assert (E <= 2 * fx["E"]).all()
    assert (r <= 1.0).all(), (tag, np.argwhere(r > 1)[:5].tolist(), r.max())
    for got, want, exact in ((obs, fx["obs_step"], fx["exact_step"]), (obs0, fx["obs_observe"], fx["exact_observe"])):
        if got is None:
            continue
        same = got.view(np.uint32) == want[lanes].view(np.uint32)
        bad = np.argwhere(~same & exact[lanes])
        assert not len(bad), (tag, "f32 observations differ at (lane, entry)", bad[:5].tolist())


def test_twin_agrees_with_the_fixture():
    """S1, S2, S5 (in-range headings: the twin rounds y0 + h sum(a k) at ulp(psi), so wound lanes are not its ground).
    The fixture marks the entries a seam forces to be tiny; no other entry may differ in its f32 bits."""
    lanes = lanes_of(K.S1, K.S2, K.S5)
    fx = fixture()
    assert not (~fx["exact_step"][lanes_of(K.S1, K.S5)]).any() and not (~fx["exact_observe"][lanes_of(K.S1, K.S5)]).any()
    _check_trusted("twin", *_twin_step(lanes), lanes)


def test_c_oracle_agrees_with_the_fixture():
    fx = fixture()
    lanes = lanes_of(K.S1, K.S2, K.S5)
    ora = c_oracle.COracle(len(lanes))
    ora.place(fx["start"][lanes], goal=fx["goal"][lanes], L2=fx["L2"][lanes])
    for n, i in enumerate(lanes):
        ora.set_state(n, fx["state0"][i])
    obs0 = np.stack([ora.observe(n, float(fx["actions"][0, i])) for n, i in enumerate(lanes)])
    obs, *_ = ora.step(fx["actions"][0, lanes])
    _check_trusted("C oracle", ora.state(), obs, obs0, lanes)


def test_reward_mirror_agrees_with_the_twin():
    """The twin's reward_step on the S6 lanes, four steps, against the fixture's info rows.  The twin calls the library's f32
    arctan2, which may sit one f32 ulp off the correctly rounded value (onestep_ref.atan2_f32): the heading term moves by up to
    15 * ulp32(pi) = 3.6e-6 and the smoothness term, a difference of two such values, by 2 * 25 / (pi / 2) * ulp32(pi / 2) =
    3.8e-6, so the rows agree to 5e-6 (measured: heading 3.5e-6, smoothness 3.8e-6, every other row 0 to 1e-12), the labels
    exactly."""
    fx = fixture()
    lanes = lanes_of(K.S6)
    worst = np.zeros(12)
    for n, i in enumerate(lanes):
        tw = simv2_twin.FixedStepTwin()
        tw.set_pose(fx["start"][i], goal=fx["goal"][i], L2=float(fx["L2"][i]), state=fx["state0"][i])
        assert tw.max_episode_steps == fx["max_episode_steps"][i]
        for t in range(K.T):
            _, total, done, info = tw.step(np.array([fx["actions"][t, i]], F32))
            row = np.array([float(info[k]) for k in R.INFO_ROWS])
            worst = np.maximum(worst, np.abs(row - fx["info_s6"][t, n]))
            assert info["violation"] == fx["viol"][t, n], (i, t)
            bits = sum(int(tw.flags[k]) << b for b, k in enumerate(tw.flags)) | (R.F_SUCCESS if info["success"] else 0)
            assert bits == fx["flags"][t, n], (i, t)
            assert done == bool(bits & simv2_twin.TERM_ALL)
    print("WORST |twin - fixture| per info row", dict(zip(R.INFO_ROWS, worst.round(12).tolist())))
    assert worst.max() <= 5e-6


# ---- negative controls: a local copy of the kernel's reduction-plus-Taylor scheme (csrc/ttenv_math.h tt_sincos) in numpy f64
P1, P2, P3, P3T = (float.fromhex(h) for h in ("0x1.921fb54400000p+0", "0x1.0b4611a600000p-34", "0x1.3198a2e000000p-69",
                                                "0x1.b839a252049c1p-104"))


def _taylor_sincos(x, sin_terms):
    """Cody-Waite by pi/2 in four pieces, sin to x^(2 sin_terms + 1), cos to x^16."""
    x = np.asarray(x, F64)
    k = np.rint(x * 0.6366197723675814)
    r = (((x - k * P1) - k * P2) - k * P3) - k * P3T
    u = -(r * r)
    f = [1.0]
    for n in range(1, 17):
        f.append(f[-1] / n)
    ps = np.full_like(r, f[2 * sin_terms + 1])
    for n in range(2 * sin_terms - 1, 2, -2):
        ps = ps * u + f[n]
    sr = r * u * ps + r
    pc = np.full_like(r, f[16])
    for n in range(14, 1, -2):
        pc = pc * u + f[n]
    cr = u * pc + 1.0
    q = k.astype(np.int64)
    a, b = np.where(q & 1, cr, sr), np.where(q & 1, sr, cr)
    return np.where(q & 2, -a, a), np.where((q + 1) & 2, -b, b)


def _scheme(sin_terms):
    return dict(sin=lambda x: _taylor_sincos(x, sin_terms)[0], cos=lambda x: _taylor_sincos(x, sin_terms)[1])


def _control(lanes, dtype, **how):
    fx = fixture()
    res = R.step(fx["state0"][lanes], fx["actions"][0, lanes], fx["goal"][lanes], fx["L2"][lanes], dtype, **how)
    return state_ratio(res["new"].astype(F64), lanes, 4)


def test_negative_control_sin_series_cut_at_x11():
    lanes = lanes_of(K.S1, K.S2)
    whole, cut = _control(lanes, F64, **_scheme(7)), _control(lanes, F64, **_scheme(5))
    print("RATIOS control sincos scheme whole", whole.max(0).round(3).tolist(), "cut at x^11", cut.max(0).round(3).tolist())
    assert (whole <= 1.0).all(), "the scheme as the kernel has it must pass: the control would prove nothing"
    assert (cut > 1.0).any(0)[2:].all(), "a sin series cut at x^11 must fail the bound in every position component"


@needs_x87
def test_negative_control_inexact_heading_reduction():
    wound = lanes_of(K.S4)
    exact, trap = _control(wound, LD), _control(wound, LD, exact=False)
    print("RATIOS control reduction exact", exact.max(0).round(3).tolist(), "by fl(2 pi)", trap.max(0).round(3).tolist())
    assert (exact <= 1.0).all()
    assert (trap > 1.0).any(0)[2:].all(), "psi - k * fl(2 pi) must fail the bound on the wound lanes"
