"""GPU (-m gpu): ONE step of the HIP env from set states against the extended-precision reference (tests/onestep_ref.py through
the fixture tests/golden/f9_onestep.npz; lanes and rejection rules: tests/onestep_cases.py; DESIGN.md "One-step tests").

The free-running parity tests hold the env step to 1e-5; its hand-written f64 numerics (tt_sincos and the stage rotations,
tt_exp_neg and the three tanh on one division, tt_wrap_pi, the atan-free f32 read-back) are good to about 1e-16, and a lost
reduction piece or series term changes every trajectory long before 1e-5 sees it.  Here, 960 lanes of six strata mixed in every
wave, one handle, five launches:

  a. state after one step, every stratum but S6: |kernel - reference| <= 0.5 ulp64(new state) + 4 E_q per component, E_q the
     reference's own float64-against-longdouble error from the fixture (never measured from the kernel);
  b. the 23 f32 observations of step(), observe(steering) and set_pose(out=) bit for bit, signs of zero included; the entries
     the fixture marks as forced tiny by a seam within the absolute f64 error of their formula;
  c. S6, steps 1 to 4: the 12 info rows within 1e-9 (tests/test_oracle_golden.py's figure for "the same reward"), flags,
     violation and done exactly, the f32 reward the rounded f64 total, the observations of every step bit for bit;
  d. S3 (tt_wrap_pi's cut) and every other stratum: heading and orientation terms of step 1 within 1e-9.

The kernel's five launches are made once per process and shared."""
import functools
import os

import numpy as np
import pytest

import onestep_cases as K
import onestep_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
LD, F64, F32 = R.LD, R.F64, R.F32
QS = ("psi1", "psi2", "x1", "y1", "x2", "y2")
REWARD_TOL = 1e-9


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLDEN, "f9_onestep.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def kernel():
    """set_pose(out=), set_state, observe(steering), four steps with info: every output, as numpy."""
    import torch
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    fx = fixture()
    n = len(fx["state0"])
    env = TruckTrailerVecEnv(n)
    assert env.max_steer == R.P.max_steer and int(env.params.term_mask) == 0x3F
    out = torch.full((n, 23), float("nan"), dtype=torch.float32, device=env.device)
    k = dict(obs_pose=env.set_pose(fx["start"], goal=fx["goal"], L2=fx["L2"], out=out).cpu().numpy().copy())
    k["max_episode_steps"] = env.episode()["max_episode_steps"].cpu().numpy()
    env.set_state(fx["state0"])
    assert np.array_equal(env.state.cpu().numpy().view(np.int64), fx["state0"].view(np.int64))
    k["obs_observe"] = env.observe(torch.from_numpy(fx["actions"][0].copy()).to(env.device)).cpu().numpy().copy()
    rec = {q: [] for q in ("obs", "rew", "done", "info", "flags", "viol", "state")}
    for a in fx["actions"]:
        obs, rew, done, info = env.step(torch.from_numpy(a.copy()).to(env.device), auto_reset=False, info=True)
        for q, v in zip(rec, (obs, rew, done, info["comp"].t(), info["flags"], info["violation"], env.state)):
            rec[q].append(v.cpu().numpy().copy())
    env.close()
    k.update({q: np.stack(v) for q, v in rec.items()})
    return k


def lanes_of(*strata):
    return np.flatnonzero(np.isin(fixture()["stratum"], strata))


def test_a_state_after_one_step(gpu_device):
    """Headings: the kernel's psi_after - psi_0 against the reference's increment; positions: the kernel's new position against
    the reference's.  The subtractions are made in longdouble from f64 operands: exact wherever the operands' exponents lie
    within 11 bits of each other (every heading here), within 2**-64 of the result otherwise.
    Measured on an MI355X, worst error / (0.5 ulp64 + 4 E_q) over psi1, psi2, x1, y1, x2, y2:
      S1 generic   0.754 0.700 0.873 0.766 0.793 0.813
      S2 seams     0.886 0.868 0.868 0.771 0.747 0.760
      S3 cut       0.913 0.907 0.865 0.829 0.839 0.843
      S4 wound     1.000 0.996 0.869 0.824 0.812 0.845   (headings: the half ulp of 6.3e5; 4 E_q is 1e-6 of the bound there)
      S5 steering  0.748 0.742 0.827 0.773 0.837 0.799"""
    fx, k = fixture(), kernel()
    s0, s1 = fx["state0"].astype(LD), k["state"][0].astype(LD)
    inc, new = R.join(fx["inc_hi"], fx["inc_lo"]), R.join(fx["new_hi"], fx["new_lo"])
    err = np.abs(np.concatenate([(s1 - s0)[:, :2] - inc[:, :2], s1[:, 2:] - new[:, 2:]], axis=1))
    ratio = (err / K.state_bound(new, fx["E"], 4).astype(LD)).astype(F64)
    worst = None
    for s in range(K.NS - 1):
        m = lanes_of(s)
        print(f"RATIOS onestep state {K.STRATA[s]}: " + " ".join(f"{q}={r:.3g}" for q, r in zip(QS, ratio[m].max(0))))
        if ratio[m].max() > 1.0 and worst is None:
            i, q = np.unravel_index(np.argmax(ratio[m]), ratio[m].shape)
            worst = f"{K.STRATA[s]} lane {m[i]} {QS[q]}: {ratio[m][i, q]:.3g} x the bound, state0 {fx['state0'][m[i]].tolist()}"
    assert worst is None, worst


def _obs_check(tag, got, want, exact, floor, lanes=None):
    """f32 bits where `exact`, |difference| <= the formula's absolute f64 error + one f32 spacing elsewhere."""
    lanes = np.arange(len(want)) if lanes is None else lanes
    got, want, exact = got[lanes], want[lanes], exact[lanes]
    same = got.view(np.uint32) == want.view(np.uint32)
    bad = np.argwhere(~same & exact)
    loose = np.abs(got.astype(F64) - want.astype(F64)) <= floor[None, :] + np.spacing(np.abs(want)).astype(F64)
    print(f"OBS {tag}: {int((~same & exact).sum())} of {int(exact.sum())} exact entries differ; {int((~exact).sum())} seam-forced "
          f"entries held to their formula's error, {int((~exact & ~same).sum())} of them not the reference's bits, "
          f"{int((~exact & ~loose).sum())} outside")
    msg = ""
    if len(bad):
        i, j = bad[0]
        msg = (f"{tag}: {len(bad)} entries differ, by entry {np.bincount(bad[:, 1], minlength=23).tolist()}; first lane "
               f"{lanes[i]} ({K.STRATA[lanes[i] % K.NS]}) entry {j}: kernel {got[i, j]!r} ({got[i, j].view(np.uint32):#x}) "
               f"reference {want[i, j]!r} ({want[i, j].view(np.uint32):#x})")
    assert not len(bad), msg
    assert (loose | exact).all(), (tag, np.argwhere(~loose & ~exact)[:5].tolist())


def test_b_observations_bit_for_bit(gpu_device):
    """Measured on an MI355X: 0 of 20973 (set_pose), 21797 (observe), 22080 (step) exact entries differ; of the 1107 / 283 / 0
    entries a seam forces tiny, 1013 / 141 are not the reference's bits and none is outside its formula's error.  Before
    tt_sincos kept the sign of a zero argument, 4 entries of set_pose differed (sin of a heading that rounds to -0.0f)."""
    fx, k = fixture(), kernel()
    assert np.array_equal(k["max_episode_steps"], fx["max_episode_steps"])
    _obs_check("set_pose(out=)", k["obs_pose"], fx["obs_pose"], fx["exact_pose"], K.FLOOR_DIRECT)
    _obs_check("observe(steering)", k["obs_observe"], fx["obs_observe"], fx["exact_observe"], K.FLOOR_DIRECT)
    _obs_check("step", k["obs"][0], fx["obs_step"], fx["exact_step"], K.FLOOR_STEP)


def test_c_reward_over_four_steps(gpu_device):
    """S6.  Step 1 is the `first` branch; steps 2 to 4 read the carry (prev, the window, closest, the first steering) and take the
    three tanh at non-zero arguments, 40 lanes with |inst| < 1e-3 among them.  No S6 lane is within 5 m of its goal; 13 lanes of
    the other strata start there, in 9 of the 15 waves, so the `__any(cur <= 5)` shortcut is taken in some waves and not in others.
    Measured on an MI355X, worst over 160 lanes: total 5.7e-14 at step 1, 1.3e-13 / 1.9e-13 / 1.7e-13 at steps 2 to 4 (all of it
    the progress term), heading 1.2e-14, orientation 6.2e-15, backward 6.6e-15, smoothness 3.6e-15, cumulative backward 1.0e-14;
    0 of 4 x 3680 observation entries differ."""
    fx, k = fixture(), kernel()
    m = lanes_of(K.S6)
    everything = np.ones_like(fx["exact_step"][m])
    _obs_check("S6 step 1", k["obs"][0], fx["obs_step"], fx["exact_step"], K.FLOOR_STEP, m)
    for t in range(1, K.T):
        _obs_check(f"S6 step {t + 1}", k["obs"][t][m], fx["obs_s6"][t - 1], everything, K.FLOOR_STEP)
    info = k["info"][:, m]
    err = np.abs(info - fx["info_s6"])
    for t in range(K.T):
        print(f"WORST S6 step {t + 1}: " + " ".join(f"{name.split('_')[0]}={e:.2g}" for name, e in zip(R.INFO_ROWS, err[t].max(0))))
    assert np.array_equal(k["flags"][:, m], fx["flags"]), np.argwhere(k["flags"][:, m] != fx["flags"])[:5].tolist()
    assert np.array_equal(k["viol"][:, m], fx["viol"]), np.argwhere(k["viol"][:, m] != fx["viol"])[:5].tolist()
    assert np.array_equal(k["done"][:, m].astype(bool), (fx["flags"] & 0x3F) != 0)
    assert np.array_equal(k["rew"][:, m].view(np.uint32), info[:, :, 0].astype(F32).view(np.uint32))
    t, i, j = np.unravel_index(np.argmax(err), err.shape)
    assert err.max() <= REWARD_TOL, f"step {t + 1}, lane {m[i]}, {R.INFO_ROWS[j]}: kernel {info[t, i, j]!r} reference {fx['info_s6'][t, i, j]!r}"


def test_d_heading_and_orientation_terms_on_the_cut(gpu_device):
    """On the cut the true np.arctan2 read-back of the trailer's heading is -pi where the kernel's wrapped angle is +pi + tiny,
    or the reverse; the kernel keeps the read-back's rounding error `eps` at about 1e-7 there instead of +-2 pi, by design: the
    heading term must come out the same.  Asserted for S3, then for every stratum (the terms are continuous: no margins).
    Measured on an MI355X, worst heading / orientation error: S1 5.8e-15 / 9.4e-16, S2 1.2e-14 / 1.6e-15, S3 2.6e-14 / 2.0e-15,
    S4 7.9e-10 / 1.1e-15, S5 1.2e-14 / 4.7e-15, S6 8.9e-15 / 5.3e-15.  S4's heading term is the stored heading's own rounding:
    at 1e5 turns ulp64(psi2) = 1.2e-10, the wrapped angle and with it the read-back's eps are off by up to half of that, the
    term by 15 * 5.8e-11 = 8.7e-10."""
    fx, k = fixture(), kernel()
    err = np.abs(k["info"][0][:, 2:4] - fx["info_step1"][:, 2:4])
    for s in range(K.NS):
        m = lanes_of(s)
        print(f"WORST onestep {K.STRATA[s]}: heading={err[m, 0].max():.2g} orientation={err[m, 1].max():.2g}")
    m = lanes_of(K.S3)
    assert err[m].max() <= REWARD_TOL, ("S3", m[np.argmax(err[m].max(1))], err[m].max())
    assert err.max() <= REWARD_TOL, (np.argmax(err.max(1)), err.max())
