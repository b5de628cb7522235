"""GPU (-m gpu): gradient-norm clipping in the lone learn() (csrc/ttclip.hip; ddpg_trucktrailer_amd/grad_clip.py; DESIGN.md section
34) -- clip_grad_norm_ in front of each optimizer step, as the norm's launch and a clipped optimizer launch.

    entry     tt_adam_soft_update_clipped alone on planted tensors between fences: norm, coefficient, counts, gradients untouched
    inactive  a learner with GradClip(1e30, 1e30) against the plain learner's separate-optimizer chain, bit for bit
    f64       one update against tests/clip_ref.py: every check of learn_checks.against_f64 in front of the optimizer, the norms, and
              the optimizer arithmetic at the kernel's own gradient times the f64 coefficient of that gradient
    paths     sampled first launch, n-step draw: the same bits; with a LossShape against clip_ref; the learn log's norms
    loop      DDPGRollout(grad_clip=): graphs == eager in both orders and with two updates per step, resume, refusals

The optimizer's bounds are learn_checks.against_f64's (derived in tests/test_gpu_learn_shapes.py::test_one_learn_step_against_f64)
with the rounding counts raised by what the coefficient adds -- two roundings, coef's own to f32 and the product coef * grad:
    |m - m64| <= 6 2^-24 (|beta1 m0| + |(1 - beta1) g'|) + 2 2^-24 (1 - beta1) |wd p0|                        (4 -> 6)
    |v - v64| <= 10 2^-24 v64 + 4 2^-24 (1 - beta2) |g'| |wd p0| + 2^-149                                      (6 -> 10: g' enters squared)
    |p - p64| <= ulp32(p64) + max(2^-19, (20 + 6 kappa + 4 kappa_w + 4 rho_w) 2^-24) |p64 - p0|                (18 -> 20)
g' = coef64 g + wd p0 with g the kernel's own gradient and coef64 clip_grad_norm_'s coefficient of that gradient in f64.  The further
terms in wd: the two added roundings are relative to coef * g, not to g', and |coef g| <= |g'| + |wd p0| -- where the decay term
cancels the gradient the count of g' alone does not cover them.  In m that is 2 2^-24 (1 - beta1) |wd p0|; in v, where g' enters
squared, 2 |g'| times it with (1 - beta2); in p, by test_gpu_learn_shapes.py's rule (twice the count, a rounding that ends in m
counted relative to m, one that ends in v halved by the root), kappa_w = (1 - beta1) |wd p0| / |m64| and rho_w = (1 - beta2) |g'|
|wd p0| / v64, twice two roundings each.  All three vanish with wd = 0 (the actor of the fresh cases).  The test prints the worst
ratios with and without the further terms.
    |target - soft64(target0, p)| <= 2 ulp32 + tau ulp32(p - target0), with the kernel's own p
The target is fmaf(tau, p - target0, target0), k_adam_soft's line: the difference rounds once, and tau times that rounding is not small
against the ulp of a result that passes near zero.  learn_checks.against_f64 holds the target to 2 ulp32 alone, which the unclipped
steps of its cases meet (at most 0.67 of it); the clipped steps of the same states -- another p, the same targets -- reach 1.6 times
it in the trained-scale actor, and the planted tensors, whose normal targets come within 1e-6 of zero, 194 times.

Worst error / bound per check, measured on MI355X (the tests print them as RATIOS lines).  Cases: batch, state scale, (critic, actor)
max_norm over the reference's norm; "f32" = fc2 images off, "shaped" = with LossShape(1.19, 0.01); m, v, p, target, norms and coef: the
worse of the two nets.  The last four columns are figures, not checks: the same errors over the bounds WITHOUT the further terms.

    case                                 pre-ReLU        y        q     q_pi    dq_da   grad c   grad a norm own norm ref     coef        m        v        p   target    m -wd    v -wd    p -wd tgt 2ulp
    planted                                     -        -        -        -        -        -        -        -        -        -     0.43     0.42      0.5     0.46     0.43     0.42      0.5  1.9e+02
    B1 x1 (0.5, 0.5)                         0.11    0.016    0.022   0.0051  1.6e-05    0.069   0.0063      0.4    0.006     0.28     0.73     0.73      0.5     0.25  7.5e+02    9e+02       17     0.32
    B33 x1 (0.5, 0.5)                        0.19    0.012    0.015   0.0095   0.0004    0.018     0.02     0.34  0.00063     0.16     0.36      0.5      0.5     0.33  5.7e+02  6.8e+02       11     0.67
    B257 x1 (0.5, 0.5)                       0.26    0.012    0.017     0.02  0.00059    0.022   0.0072     0.36  0.00021     0.21     0.35     0.43      0.5     0.27    1e+03  1.2e+03       12      0.4
    B1 x20 (0.5, 0.5)                       0.098  0.00073   0.0028   0.0054  9.2e-05    0.013    0.028     0.28  0.00094     0.46      0.6     0.57     0.49      0.3      3.4      2.6     0.49      1.4
    B33 x20 (0.5, 0.5)                       0.27   0.0095    0.017    0.023  0.00054    0.014   0.0081     0.28  0.00064     0.12     0.39     0.38      0.5     0.32      3.1     0.58      0.5     0.52
    B257 x20 (0.5, 0.5)                       0.3    0.012    0.015    0.025  0.00055    0.014   0.0072     0.23  0.00068     0.22     0.53     0.29     0.49     0.26      4.1     0.59      0.5      1.6
    B33 x1 (0.5, 2.0)                        0.19    0.012    0.015   0.0095   0.0004    0.018     0.02     0.34  0.00063     0.16     0.36      0.5      0.5     0.33  5.7e+02  6.8e+02       11     0.67
    B33 x1 (2.0, 0.5)                        0.19    0.012    0.015     0.01   0.0005    0.018    0.019     0.34  0.00065     0.13     0.33     0.44      0.5     0.25     0.33     0.44      0.5     0.51
    B257 x20 (0.5, 2.0)                       0.3    0.012    0.015    0.025  0.00055    0.014   0.0072     0.23  0.00068     0.22     0.53     0.29      0.5     0.25      4.1     0.59      0.5     0.57
    B257 x20 (2.0, 0.5)                       0.3    0.012    0.015    0.022  0.00061    0.014   0.0076     0.23  0.00068     0.19     0.34     0.27      0.5     0.28     0.68     0.37      0.5     0.53
    B257 x20 (0.5, None)                      0.3    0.012    0.015    0.025  0.00055    0.014   0.0072     0.23  0.00068     0.22     0.53     0.29      0.5     0.25      4.1     0.59      0.5     0.57
    B257 x20 (None, 0.5)                      0.3    0.012    0.015    0.022  0.00061    0.014   0.0076     0.17  0.00024     0.19     0.34     0.27      0.5     0.28     0.68     0.37      0.5     0.53
    B257 x1 (0.5, 0.5) f32                   0.34    0.017    0.019    0.022  0.00057    0.013   0.0075     0.44   0.0001    0.055      0.3     0.38      0.5     0.27  2.5e+02    3e+02      3.5      0.4
    B257 x20 (0.5, 0.5) f32                  0.31    0.013    0.025    0.023  0.00053    0.016   0.0043     0.13  0.00024     0.16     0.43     0.28     0.49     0.26      3.3     0.39      0.5      1.6
    B33 x1 (0.5, 0.5) shaped                 0.19    0.012    0.015    0.007  0.00033    0.017   0.0083     0.21   0.0003     0.15     0.47     0.52      0.5     0.25  2.6e+03  3.1e+03       46     0.38

The largest share of any bound is 0.73 (m and v of the critic at B = 1).  Without the terms in wd the fresh critic (wd = 0.01, zero
moments) is 250 to 3100 times over m's and v's bound -- among 132201 elements some have coef g within 1e-3 of -wd p0 -- and 3.5 to 46
times over p's; the actor of the fresh cases (wd = 0) is the same with and without.  The target at 2 ulp alone: 1.4 to 1.6 times
in the trained-scale actor with both sites clipped, 194 times on the planted tensors."""
import ctypes as C
import math

import pytest

import clip_ref as CR
import learn_checks as K
import learn_ref as R
import shape_ref as S

pytestmark = pytest.mark.gpu

_id = K.case_id
_results, _same, _flat, _ring_with_batch = K.results, K.same, K.flat, K.ring_with_batch
_PATH_CASE = CR.TRAINED_CASES[1]          # B = 33, trained scale


def _clip(critic, actor):
    from ddpg_trucktrailer_amd.grad_clip import GradClip
    return GradClip(critic, actor)


def _learner(dev, state, hyper, batch, step, images=True, clip=None, shape=None):
    agent, fl, dbatch = K.learner(dev, state, hyper, batch, step, images, shape)
    if clip is not None:
        fl.set_grad_clip(clip)
    return agent, fl, dbatch


# ---- 1. the entry point alone ------------------------------------------------------------------------------------------------
_CRITIC_NUMEL = (9200, 400, 400, 400, 120000, 300, 300, 300, 300, 1, 300, 300)
_SETS = {"3-4": (3, 4), "1": (1,), "255-257": (255, 257), "ragged5": (1, 300, 400, 9200, 120000), "critic12": _CRITIC_NUMEL}
_HYP = (1e-3, 0.9, 0.999, 1e-8, 0.01, 5e-3)        # lr, beta1, beta2, eps, weight decay, tau


def _planted(dev, arena, numel, seed=5):
    """Per tensor p, g, m, v, target in the arena (the gradients at every 4-byte phase of a 16-byte line), and the clip's buffers."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    t = dict(p=[], g=[], m=[], v=[], t=[])
    for i, n in enumerate(numel):
        if numel == (3, 4):
            g = torch.tensor([[3.0, 0.0, 0.0], [0.0, 4.0, 0.0, 0.0]][i])
        else:
            g = torch.randn(n, generator=gen) * (0.5 if i % 2 else 3.0)
        t["g"].append(arena.inp(f"g{i}", g.to(dev), misalign=4 * (i % 4) if i else 12))
        t["p"].append(arena.inp(f"p{i}", (torch.randn(n, generator=gen) * 0.1).to(dev)))
        t["m"].append(arena.inp(f"m{i}", (torch.randn(n, generator=gen) * 0.01).to(dev)))
        t["v"].append(arena.inp(f"v{i}", (torch.rand(n, generator=gen) * 1e-3).to(dev)))
        t["t"].append(arena.inp(f"t{i}", (torch.randn(n, generator=gen) * 0.1).to(dev)))
    from ddpg_trucktrailer_amd import _lib as L
    t["partials"] = arena.out("partials", L.GRAD_CLIP_PARTIALS, dtype=torch.float64)
    t["out"] = arena.out("out", 2)
    t["counts"] = arena.inp("counts", torch.zeros(2, dtype=torch.int64, device=dev))
    t["step"] = arena.inp("step", torch.tensor([7], dtype=torch.int64, device=dev))
    return t


def _call(L, t, numel, max_norm, clipped=True):
    import torch
    cnt = len(numel)
    arr = lambda ts: (C.c_void_p * cnt)(*[x.data_ptr() for x in ts])
    args = [cnt, arr(t["p"]), arr(t["g"]), arr(t["m"]), arr(t["v"]), arr(t["t"]), (C.c_int32 * cnt)(*numel), L.ptr(t["step"]), *_HYP, None, None]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if clipped:
        clip = L.TTGradClip(max_norm=max_norm, partials=t["partials"].data_ptr(), out=t["out"].data_ptr(), counts=t["counts"].data_ptr())
        L.check(L.load().tt_adam_soft_update_clipped(*args, C.byref(clip), st))
    else:
        L.check(L.load().tt_adam_soft_update(*args, st))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", list(_SETS), ids=list(_SETS))
def test_the_entry_point_alone_on_planted_tensors_between_fences(gpu_device, name):
    """tt_adam_soft_update_clipped on tensors planted between fences (tests/fenced.py; NaN, huge and zero surrounds), the gradients at
    every 4-byte phase of a 16-byte line: [3] and [4] with max_norm = 1 -- coef = 1 / (5 + 1e-6): the norm is global, not per tensor
    --, one element, (255, 257), the five ragged lengths (1, 300, 400, 9200, 120000) and the critic's twelve tensors.
    out[0] is the f64 norm of the very buffers within 2^-23 relative (f64 accumulation; the one rounding is the store's), out[1] the
    f32 rounding of the formula at that norm within 1 ulp; the fences are intact whatever surrounds the payloads; the gradients keep
    their bits; counts advance by (1, coef < 1); a second call with max_norm far above the norm has coef = 1 and leaves the bits of
    tt_adam_soft_update on the same buffers."""
    import numpy as np
    import torch
    import fenced
    from ddpg_trucktrailer_amd import _lib as L
    dev, numel = gpu_device, _SETS[name]
    outs = []
    for surround in fenced.SURROUNDS:
        arena = fenced.Arena(dev, surround)
        t = _planted(dev, arena, numel)
        g0 = [g.clone() for g in t["g"]]
        norm = math.sqrt(math.fsum(float(x) ** 2 for g in g0 for x in g.double().cpu().tolist()))
        max_norm = 1.0 if name == "3-4" else float(np.float32(0.5 * norm))
        _call(L, t, numel, max_norm)
        arena.assert_clean(f"{name} {surround}")
        for g, want in zip(t["g"], g0):
            assert torch.equal(g, want), "a gradient buffer was rewritten"
        got_norm, got_coef = (float(x) for x in t["out"].cpu())
        want_coef = np.float32(min(1.0, max_norm / (norm + 1e-6)))
        print(f"{name} {surround}: norm {got_norm!r} want {norm!r}, coef {got_coef!r} want {float(want_coef)!r}")
        assert abs(got_norm - norm) <= 2.0 ** -23 * norm
        assert abs(got_coef - float(want_coef)) <= float(np.spacing(want_coef)) and got_coef < 1.0
        assert t["counts"].tolist() == [1, 1]
        if name == "3-4":
            assert norm == 5.0 and got_norm == 5.0 and got_coef == float(np.float32(1.0 / (5.0 + 1e-6)))
        outs.append((got_norm, got_coef))
        # inactive: the bits of tt_adam_soft_update on a copy of the buffers as they stand
        plain = fenced.Plain(dev)
        u = {k: [plain.inp(f"{k}{i}", x) for i, x in enumerate(t[k])] for k in ("p", "g", "m", "v", "t")}
        u["step"] = t["step"]
        _call(L, u, numel, None, clipped=False)
        _call(L, t, numel, float(np.float32(4.0 * norm)))
        arena.assert_clean(f"{name} {surround} inactive")
        assert t["counts"].tolist() == [2, 1] and float(t["out"][1]) == 1.0
        for k in ("p", "m", "v", "t", "g"):
            for x, y in zip(t[k], u[k]):
                assert torch.equal(x, y), (k, "inactive clip against tt_adam_soft_update")
    assert outs[0] == outs[1] == outs[2]          # nothing read from the surrounds


def test_the_clipped_optimizer_applies_the_coefficient_to_every_element(gpu_device):
    """The critic's twelve planted tensors, max_norm = half the norm: m, v, p and target of every element against learn_ref.adam64 at
    coef64 g, under the bounds of the f64 test (module docstring), and NOT within ten times m's bound of the unclipped step."""
    import numpy as np
    import torch
    import fenced
    from ddpg_trucktrailer_amd import _lib as L
    dev, numel = gpu_device, _CRITIC_NUMEL
    t = _planted(dev, fenced.Plain(dev), numel)
    before = {k: [x.clone() for x in t[k]] for k in ("p", "m", "v", "t")}
    norm = math.sqrt(math.fsum(float(x) ** 2 for g in t["g"] for x in g.double().cpu().tolist()))
    max_norm = float(np.float32(0.5 * norm))
    _call(L, t, numel, max_norm)
    hyper = dict(lr=float(np.float32(_HYP[0])), betas=(float(np.float32(_HYP[1])), float(np.float32(_HYP[2]))), eps=float(np.float32(_HYP[3])),
                 weight_decay=float(np.float32(_HYP[4])), tau=float(np.float32(_HYP[5])))
    worst = _check_optimizer(lambda n, e, tol: None, "planted", hyper, CR.coef64(max_norm, norm), 7,
                             [(before["p"][i], before["m"][i], before["v"][i], before["t"][i], t["g"][i], t["p"][i], t["m"][i], t["v"][i],
                               t["t"][i]) for i in range(len(numel))], must_differ=True)
    print("RATIOS planted: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v <= 1.0 for k, v in worst.items() if not k.startswith("(")), worst


def _check_optimizer(check, key, h, coef, t, tensors, must_differ=False):
    """m, v, p, target of every element against adam64 at coef * g (f64), with the module docstring's bounds.  tensors: (p0, m0, v0,
    target0, g, p, m, v, target) per parameter tensor.  Returns the worst ratios; "(...)" entries are figures: the same errors over the
    bounds WITHOUT the further terms in wd."""
    import torch
    worst = {}

    def note(name, err, tol):
        ratio = (err / tol).max().item()
        worst[name] = max(worst.get(name, 0.0), ratio)
        if not name.startswith("("):
            check(name, err, tol)

    b1, b2 = h["betas"]
    wd = h["weight_decay"]
    for p0, m0, v0, t0, g, p, m, v, tg in tensors:
        p0, m0, v0, t0, g, p, m, v, tg = (x.detach().double().reshape(-1) for x in (p0, m0, v0, t0, g, p, m, v, tg))
        p64, m64, v64, _, g2 = R.adam64(p0, m0, v0, t0, coef * g, t, h)
        terms = (b1 * m0).abs() + ((1 - b1) * g2).abs()
        wdp = (wd * p0).abs()
        u = 2.0 ** -24
        note("adam m " + key, (m - m64).abs(), (6 * u * terms + 2 * u * (1 - b1) * wdp).clamp_min(2.0 ** -149))
        note("(m without wd term) " + key, (m - m64).abs(), (6 * u * terms).clamp_min(2.0 ** -149))
        note("adam v " + key, (v - v64).abs(), 10 * u * v64 + 4 * u * (1 - b2) * g2.abs() * wdp + 2.0 ** -149)
        note("(v without wd term) " + key, (v - v64).abs(), 10 * u * v64 + 2.0 ** -149)
        kappa = terms / m64.abs().clamp_min(1e-300)
        kappa_w = (1 - b1) * wdp / m64.abs().clamp_min(1e-300)
        rho_w = (1 - b2) * g2.abs() * wdp / v64.clamp_min(1e-300)
        rel = ((20 + 6 * kappa + 4 * kappa_w + 4 * rho_w) * u).clamp_min(2.0 ** -19)
        note("adam p " + key, (p - p64).abs(), K.ulp32(p64) + rel * (p64 - p0).abs())
        note("(p without wd terms) " + key, (p - p64).abs(), K.ulp32(p64) + ((20 + 6 * kappa) * u).clamp_min(2.0 ** -19) * (p64 - p0).abs())
        tg64 = R.soft64(t0, p, h["tau"])
        note("target " + key, (tg - tg64).abs(), 2 * K.ulp32(tg64) + h["tau"] * K.ulp32(p - t0))
        note("(target at 2 ulp alone) " + key, (tg - tg64).abs(), 2 * K.ulp32(tg64))
        if must_differ and g.numel() >= 300:
            _, m_un, _, _, _ = R.adam64(p0, m0, v0, t0, g, t, h)
            assert ((m - m_un).abs() > 10 * (6 * u * terms + 2 * u * (1 - b1) * wdp).clamp_min(2.0 ** -149)).any()
    return worst


# ---- 2. inactive equals the plain learner's separate-optimizer chain -------------------------------------------------------------
@pytest.mark.parametrize("images", [True, False], ids=["images", "f32"])
@pytest.mark.parametrize("case", S.OFF_CASES, ids=_id)
def test_an_inactive_clip_leaves_the_bits_of_the_separate_optimizer_chain(gpu_device, case, images):
    """Three updates from the trained-scale state, B = 1 and 257: a learner with GradClip(1e30, 1e30) -- coef = 1 at both sites --
    against a plain FusedLearner driven through phase_a(fuse_adam=False), phase_b(separate_adam=True) (which opens with the critic's
    _adam) and phase_c, the launches data-parallel ranks make: the four nets, all moments, both flat gradients, y, q, q_pi, dq_da
    and the step count, bit for bit."""
    import torch
    state, hyper, batch, _, _ = R.case(*case)
    runs = []
    for clip in (None, _clip(1e30, 1e30)):
        _, fl, dbatch = _learner(gpu_device, state, hyper, batch, case[3], images, clip)
        for _ in range(3):
            if clip is None:
                fl.phase_a(*dbatch, fuse_adam=False)
                fl.phase_b(dbatch[0], separate_adam=True)
                fl.phase_c()
            else:
                fl.learn_batch(*dbatch)
        torch.cuda.synchronize()
        assert int(fl.step_dev.item()) == case[3] + 3
        if clip is not None:
            stats = fl.clip_stats()
            assert all(stats[k]["coef"] == 1.0 and stats[k]["updates"] == 3 and stats[k]["clipped"] == 0 for k in ("critic", "actor"))
        runs.append(_results(fl))
    assert all(torch.isfinite(x).all() for x in runs[0])
    _same(runs[1], runs[0], "inactive")


# ---- 3. one update against f64 ------------------------------------------------------------------------------------------------
def _against_f64(dev, case, factors, *, images=True, delta=None, c=0.0, prepare=None):
    """One learn_batch of a learner with GradClip(max_norm critic, max_norm actor) of clip_ref.clipped(case, factors) against f64.
    In front of the optimizer, every check of learn_checks.against_f64 under its bounds: no unit changes side, y, q, q_pi, dq_da
    with its choices, both gradients (the buffers keep the UNCLIPPED gradient).  Then the norms and the optimizer (module docstring);
    targets and fc2 images as there.  Returns (worst ratios, the learner)."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    state, hyper, batch, (max_c, max_a), ref = CR.clipped(case, factors, delta, c)
    B, step0 = batch[0].shape[0], state["step"]
    tag = f"B{B} x{case[1]:g} clip {factors}" + (f" delta {delta:.3g} c {c:g}" if (delta or c) else "")
    shape = K.loss_shape(delta, c) if (delta is not None or c) else None
    h32 = R.f32_hyper(hyper)
    clip = _clip(max_c, max_a)
    agent, fl, (s, a, r, s2, d8) = _learner(dev, state, hyper, batch, step0, images, clip, shape)
    if prepare is not None:
        prepare(fl)
    twin = R.load_agent(state, hyper, dev, torch.float32)
    before = {st: dict(p=[x.detach().clone() for x in st.params], t=[x.detach().clone() for x in st.targets],
                       m=[x.clone() for x in st.ms], v=[x.clone() for x in st.vs]) for st in (fl.critic, fl.actor)}
    fl.learn_batch(s, a, r, s2, d8)
    torch.cuda.synchronize()
    worst = {}

    def check(name, err, tol):
        ratio = (err / tol).max().item() if torch.is_tensor(err) else err / tol
        worst[name] = max(worst.get(name, 0.0), ratio)
        assert ratio <= 1.0, (tag, name, B, ratio)

    # ---- no unit changes side
    for st, key in ((fl.critic, "critic"), (fl.actor, "actor")):
        sd = {k: v.to(dev).double() for k, v in state["nets"][key].items()}
        z1 = st.saved_t["xh1"].double() * sd["bn1.weight"] + sd["bn1.bias"]
        z2 = st.saved_t["xh2"].double() * sd["bn2.weight"] + sd["bn2.bias"]
        if st.critic:
            z2 = z2 + a.double().view(-1, 1) * sd["action_value.weight"].view(1, -1) + sd["action_value.bias"]
        for got, want in zip((z1, z2), ref["z"][key]):
            check("pre-relu", (got.cpu() - want).abs().max().item(), R.MARGIN / 3)
    # ---- outputs
    done = d8.bool()
    assert torch.equal(fl.y[done], r[done])
    for name in ("y", "q"):
        check(name, (getattr(fl, name).double().cpu() - ref[name]).abs().max().item(), 2e-5 * max(1.0, ref[name].abs().max().item()))
    nets = dict(state["nets"], critic={k: v.detach().cpu() for k, v in agent.critic.state_dict().items()})
    a64 = R.load_agent(dict(state, nets=nets), hyper, torch.device("cpu"), torch.float64)
    s64, act64 = s.double().cpu(), a.double().cpu()
    half = R.actor_half(a64.critic, a64.actor, s64, act64, c=c)          # the third forward, in f64 on the critic this learn() left
    check("q_pi", (fl.q_pi.double().cpu() - half["q_pi"]).abs().max().item(), 2e-5 * max(1.0, half["q_pi"].abs().max().item()))
    got_dq, dq64 = fl.dq_da.double().cpu(), half["dq_da"].clone()
    choices = R.dq_da_choices(a64.critic, half["z_pi"][1], half["dq_da"])
    for b, values in choices.items():
        dq64[b] = min(values, key=lambda x: abs(x - got_dq[b].item()))
    check("dq_da", (got_dq - dq64).abs().max().item(), 2e-5 * max(1.0, dq64.abs().max().item()))
    if shape is not None:
        check("pre", (fl.pre.double().cpu() - half["pre"]).abs().max().item(), 2e-5 * max(1.0, half["pre"].abs().max().item()))
    # ---- the gradients at both sites: the buffers hold the unclipped ones
    half_dq = R.actor_half(a64.critic, a64.actor, s64, act64, dq_da=dq64, c=c)
    g64 = dict(critic=ref["grads"]["critic"], actor=half_dq["grads"])
    twin.loss_shape = shape
    g32 = dict(actor=R.actor_half(twin.critic, twin.actor, s, a, dq_da=dq64.to(dev), c=c)["grads"])
    with torch.no_grad():
        q_next = twin.target_critic(s2, twin.target_actor(s2)).masked_fill(done.view(-1, 1), 0.0).view(-1)
        y32 = (r + h32["gamma"] * q_next).view(-1, 1)
    q32 = twin.critic(s, a)
    loss32 = F.mse_loss(y32, q32) if delta is None else F.huber_loss(q32, y32, delta=delta)
    g32["critic"] = dict(zip([k for k, _ in twin.critic.named_parameters()], torch.autograd.grad(loss32, list(twin.critic.parameters()))))
    norm_tol = {}
    for st, key, names in ((fl.critic, "critic", K.CRITIC_NAMES), (fl.actor, "actor", K.ACTOR_NAMES)):
        assert len(st.grads) == len(names) == len(g64[key])
        sq = 0.0
        for name, g in zip(names, st.grads):
            want = g64[key][name]
            e32 = (g32[key][name].double().cpu() - want).abs().max().item()
            tol = max(3e-5 * want.abs().max().item() + 1e-7, 3 * e32)
            check("grad " + key, (g.double().cpu() - want).abs().max().item(), tol)
            sq += want.numel() * tol * tol
        norm_tol[key] = math.sqrt(sq)
    # ---- the norms and the coefficient
    stats = fl.clip_stats()
    coefs = {}
    for st, key, max_norm in ((fl.critic, "critic", max_c), (fl.actor, "actor", max_a)):
        own = float(torch.sqrt((st.flat_grad.double() ** 2).sum()).item())
        coefs[key] = CR.coef64(None if max_norm is None else float(np.float32(max_norm)), own)
        if max_norm is None:
            assert key not in stats
            continue
        got = stats[key]
        check("norm own " + key, abs(got["norm"] - own), 2.0 ** -23 * own)
        check("norm ref " + key, abs(got["norm"] - CR.norm64(g64[key])), norm_tol[key] + 2.0 ** -23 * own)
        check("coef " + key, abs(got["coef"] - coefs[key]), 2.0 ** -23 * coefs[key])
        active = factors[0 if key == "critic" else 1] == CR.ACTIVE
        assert (got["coef"] < 1.0) == active and (got["updates"], got["clipped"]) == (1, int(active)), (tag, key, got)
    # ---- the optimizer at the kernel's own gradient times the f64 coefficient of that gradient
    t = step0 + 1
    assert int(fl.step_dev.item()) == t
    for st, key in ((fl.critic, "critic"), (fl.actor, "actor")):
        tensors = [(before[st]["p"][i], before[st]["m"][i], before[st]["v"][i], before[st]["t"][i], st.grads[i], st.params[i], st.ms[i],
                    st.vs[i], st.targets[i]) for i in range(len(st.params))]
        worst.update(_check_optimizer(check, key, R.net_hyper(h32, key), coefs[key], t, tensors,
                                      must_differ=factors[0 if key == "critic" else 1] == CR.ACTIVE))
        for i in range(len(st.params)):
            assert not torch.equal(st.params[i].detach(), before[st]["p"][i]), (key, i)
    # ---- images
    if images:
        fwd = 2 * 20 * 13 * 512
        assert fl.images_current()
        for net in (agent.actor, agent.critic, agent.target_actor, agent.target_critic):
            kept, fresh = fl._img[id(net)], K.scratch_image(fl, net, dev)
            if net in (agent.target_actor, agent.target_critic):
                assert torch.equal(kept.view(torch.float16)[:fwd], fresh.view(torch.float16)[:fwd]), "target image differs"
            else:
                assert torch.equal(kept, fresh), "maintained image differs from one made from scratch"
    print(f"RATIOS {tag} {'images' if images else 'f32'}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) +
          f", rows near a boundary in Q(s, mu(s)) {len(choices)}")
    return worst, fl


_F64 = [(case, CR.BOTH, True) for case in CR.CASES] + [(CR.CASES[i], f, True) for i in (1, 5) for f in (CR.CRITIC_ONLY, CR.ACTOR_ONLY)] + \
       [(CR.TRAINED_CASES[2], (CR.ACTIVE, None), True), (CR.TRAINED_CASES[2], (None, CR.ACTIVE), True)] + \
       [(case, CR.BOTH, False) for case in (CR.FRESH_CASES[2], CR.TRAINED_CASES[2])]


@pytest.mark.parametrize("case, factors, images", _F64,
                         ids=[f"{_id(k)}-{f[0]}-{f[1]}-{'images' if im else 'f32'}" for k, f, im in _F64])
def test_one_clipped_learn_step_against_f64(gpu_device, case, factors, images):
    """B = 1, 33, 257 from fresh and trained-scale states with max_norm = 0.5 x the f64 reference's own norm at both sites (active, coef
    just below 0.5); at B = 33 active at one site and inactive (2 x norm, coef exactly 1) at the other; at B = 257 one site with no
    clip at all (its step is tt_adam_soft_update's); with and without fc2 images.  See _against_f64."""
    _against_f64(gpu_device, case, factors, images=images)


# ---- 4. the draw, the loss shape and the log ----------------------------------------------------------------------------------
def _path_clip():
    _, _, _, (max_c, max_a), _ = CR.clipped(_PATH_CASE, CR.BOTH)
    return _clip(max_c, max_a)


def test_clipped_learn_with_the_draw_made_by_its_first_launch(gpu_device):
    """The sampled first launch (tt_mlp_forward_multi_sampled) against a batch drawn before, with an active clip: the same bits."""
    import torch
    dev = gpu_device
    state, hyper, batch, _, _ = R.case(*_PATH_CASE)
    B, step0 = _PATH_CASE[0], _PATH_CASE[3]
    runs = []
    for sampled in (False, True):
        _, fl, dbatch = _learner(dev, state, hyper, batch, step0, True, _path_clip())
        ring, seed = _ring_with_batch(dev, B, dbatch)
        for _ in range(2):
            if sampled:
                for t in ring._batch_bufs(B)[:5]:
                    t.zero_()
                args = ring.sample_args(B, seed=seed)
                s, a, r, s2, d = ring._batch_bufs(B)[:5]
                fl.learn_batch(s, a, r, s2, d, sample=args)
            else:
                fl.learn_batch(*dbatch)
        torch.cuda.synchronize()
        stats = fl.clip_stats()
        assert stats["critic"]["updates"] == 2 and stats["critic"]["clipped"] >= 1
        runs.append(_results(fl) + [fl._clip[k]["out"].clone() for k in ("critic", "actor")])
    _same(runs[1], runs[0], "sampled")


def test_clipped_learn_with_an_n_step_draw(gpu_device):
    """n_step = 3: tt_mlp_forward_multi_sampled_nstep's draw against tt_ring_sample_nstep followed by the same clipped learn()."""
    import torch
    import nstep_ref
    dev, n_step = gpu_device, 3
    state, hyper, batch, _, _ = R.case(*_PATH_CASE)
    B, step0 = _PATH_CASE[0], _PATH_CASE[3]
    ring = nstep_ref.synthetic_ring(dev)
    learners = [_learner(dev, state, hyper, batch, step0, True, _path_clip())[1] for _ in range(2)]
    gamma = float(learners[0].agent.gamma)
    res = lambda fl: _results(fl) + [fl._clip[k]["out"].clone() for k in ("critic", "actor")]
    for step in range(2):
        kw = dict(seed=1234 + step)
        s, a, r, s2, d = ring.sample_fused(B, done_as_bool=False, n_step=n_step, gamma=gamma, **kw)
        drawn = [t.clone() for t in (s, a, r, s2, d)]
        learners[0].learn_batch(s, a, r, s2, d, n_step=n_step)
        for t in ring._batch_bufs(B)[:5]:
            t.zero_()
        args = ring.sample_args(B, **kw)
        s, a, r, s2, d = ring._batch_bufs(B)[:5]
        learners[1].learn_batch(s, a, r, s2, d, sample=args, n_step=n_step)
        torch.cuda.synchronize()
        for x, y in zip(drawn, (s, a, r, s2, d)):
            assert torch.equal(x, y), step
        _same(res(learners[1]), res(learners[0]), f"n-step {step}")
    assert all(torch.isfinite(x).all() for x in res(learners[0]))


def test_a_clipped_step_with_a_loss_shape_and_the_learn_log(gpu_device):
    """B = 33, fresh state, LossShape(delta = the case's median |q - y|, c = 0.01) and an active clip at both sites, against clip_ref
    extended by delta and c: every check of the f64 test.  With the learn log on, the record's two gradient norms are those of the
    gradient buffers -- the UNCLIPPED gradient, so out[0] of each site: within out[0]'s own rounding to f32, 2^-24 relative, plus the
    bound tests/test_gpu_learn_log.py holds those fields to, (numel + 2) 2^-52 relative."""
    case = CR.FRESH_CASES[1]
    _, _, _, ref, _ = R.case(*case)
    _, fl = _against_f64(gpu_device, case, CR.BOTH, delta=S.delta_of(ref), c=0.01, prepare=lambda fl: fl.enable_learn_log(4))
    rec = fl.drain_learn_log()
    stats = fl.clip_stats()
    assert rec["step"].tolist() == [1] and int(rec["nonfinite"].sum()) == 0
    for key, st in (("critic", fl.critic), ("actor", fl.actor)):
        got, out0 = float(rec["grad_norm_" + key][0]), stats[key]["norm"]
        tol = (2.0 ** -24 + (st.flat_grad.numel() + 2) * 2.0 ** -52) * got
        print(f"learn log grad_norm_{key} {got!r}, out[0] {out0!r}, |diff| {abs(got - out0):.3g}, tol {tol:.3g}")
        assert got > 0 and abs(got - out0) <= tol and stats[key]["coef"] < 0.5


# ---- 5. the loop ----------------------------------------------------------------------------------------------------------------
_LOOP_CLIP = (0.5, 0.01)


def _loop(seed=6, graph_steps=4, pipeline=False, clip="default", **kw):
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    env = TruckTrailerVecEnv(64)
    env.reset(seed=seed)
    if clip == "default":
        clip = _clip(*_LOOP_CLIP)
    return DDPGRollout(env, batch_size=33, replay_slots=16, seed=seed, graph_steps=graph_steps, pipeline=pipeline, grad_clip=clip, **kw)


@pytest.mark.parametrize("updates", [1, 2], ids=["1-update", "2-updates"])
@pytest.mark.parametrize("pipeline", [False, True], ids=["serial", "pipelined"])
def test_vector_loop_with_a_clip_graphs_equal_eager(gpu_device, pipeline, updates):
    """DDPGRollout(grad_clip=GradClip(0.5, 0.01)) at N = 64, B = 33, 12 steps: whole-step graphs == eager steps over the flat weights and
    in clip_stats(), bit for bit; finite; every update counted, some clipped at each site; other bits than the loop without a clip."""
    import torch
    flats, stats = [], []
    for graph_steps in (4, 0):
        loop = _loop(graph_steps=graph_steps, pipeline=pipeline, updates_per_step=updates)
        assert loop.pipeline == pipeline and loop.graph_steps == graph_steps and loop.learner.grad_clip == _clip(*_LOOP_CLIP)
        assert loop.agent.grad_clip == _clip(*_LOOP_CLIP)
        loop.run(5)
        loop.run(7)
        torch.cuda.synchronize()
        assert loop.handover_gave_up == [] and loop.ring.policy_gave_up() == 0 and loop.learner.tail_gave_up() == 0
        steps = int(loop.learner.step_dev.item())
        assert int(loop.ring.k_dev.item()) == 12 and steps >= 9 * updates
        flats.append(_flat(loop).clone())
        st = loop.learner.clip_stats()
        assert all(st[k]["updates"] == steps and 1 <= st[k]["clipped"] <= steps for k in ("critic", "actor")), st
        stats.append(st)
        loop.env.close()
    assert torch.equal(flats[0], flats[1]) and torch.isfinite(flats[0]).all() and stats[0] == stats[1]
    plain = _loop(graph_steps=4, pipeline=pipeline, clip=None, updates_per_step=updates)
    plain.run(12)
    torch.cuda.synchronize()
    assert not torch.equal(_flat(plain), flats[0])
    plain.env.close()


def test_vector_loop_with_an_inactive_clip_graphs_equal_eager(gpu_device):
    """GradClip(1e30, 1e30): the loop in graphs against itself eager, bit for bit, and no update clipped."""
    import torch
    flats = []
    for graph_steps in (4, 0):
        loop = _loop(graph_steps=graph_steps, pipeline=True, clip=_clip(1e30, 1e30))
        loop.run(12)
        torch.cuda.synchronize()
        st = loop.learner.clip_stats()
        assert all(st[k]["clipped"] == 0 and st[k]["coef"] == 1.0 and st[k]["updates"] == int(loop.learner.step_dev.item()) for k in st)
        flats.append(_flat(loop).clone())
        loop.env.close()
    assert torch.equal(flats[0], flats[1]) and torch.isfinite(flats[0]).all()


def test_vector_loop_with_a_clip_resumes_bitwise(gpu_device, tmp_path):
    """A checkpoint taken at step 6 and resumed in another loop ends step 12 with the same bits; the checkpoint carries the clip, and a
    loop with another clip (or none) refuses it."""
    import torch
    from ddpg_trucktrailer_amd import checkpoint
    a = _loop(seed=21)
    a.run(6)
    path = checkpoint.save_loop_checkpoint(str(tmp_path / "loop.pt"), a)
    assert a.state_dict()["grad_clip"] == list(_LOOP_CLIP) and a.state_dict()["fused_adam"]["grad_clip"] == list(_LOOP_CLIP)
    a.run(6)
    b = _loop(seed=99)
    b.run(5)                           # its graphs are already captured when the file is loaded
    checkpoint.load_loop_checkpoint(path, b)
    assert b.ring.k == 6
    b.run(6)
    torch.cuda.synchronize()
    assert torch.equal(_flat(a), _flat(b))
    for st_a, st_b in ((a.learner.actor, b.learner.actor), (a.learner.critic, b.learner.critic)):
        assert torch.equal(st_a.m, st_b.m) and torch.equal(st_a.v, st_b.v)
    assert int(a.learner.step_dev.item()) == int(b.learner.step_dev.item())
    for other in (_clip(1.0, 0.01), _clip(0.5, None), None):
        c = _loop(seed=3, clip=other)
        with pytest.raises(ValueError, match="grad_clip"):
            checkpoint.load_loop_checkpoint(path, c)
        c.env.close()
    for lp in (a, b):
        lp.env.close()


def test_refused_combinations_raise(gpu_device, monkeypatch):
    import torch
    from ddpg_trucktrailer_amd.agent import Agent
    from ddpg_trucktrailer_amd.demo_loss import DemoLoss
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    from ddpg_trucktrailer_amd.mpc import ExpertLanes
    from ddpg_trucktrailer_amd.population import PopulationLearner
    from ddpg_trucktrailer_amd.td3 import TD3Config
    with pytest.raises(ValueError, match="grad_clip with td3"):
        _loop(td3=TD3Config(), updates_per_step=2)
    with pytest.raises(ValueError, match="grad_clip with data-parallel"):
        _loop(data_parallel=True, dp_exchange="p2p")
    with pytest.raises(ValueError, match="grad_clip with data-parallel"):
        _loop(dp_exchange="p2p")
    with pytest.raises(ValueError, match="grad_clip with demo_loss"):
        _loop(demo_loss=DemoLoss(0.1))
    with pytest.raises(ValueError, match="grad_clip with expert lanes"):
        _loop(expert=ExpertLanes(4))
    with pytest.raises(ValueError, match="grad_clip"):
        _loop(clip=(1.0, None))
    monkeypatch.setenv("TT_FORCE_DP", "1")
    with pytest.raises(ValueError, match="grad_clip with the data-parallel launch structure"):
        _loop()
    monkeypatch.delenv("TT_FORCE_DP")
    # an agent built with another clip than the loop's, a population given an agent with one, a learner whose ranks exchange gradients
    kw = dict(alpha=1e-4, beta=1e-3, input_dims=(23,), tau=1e-3, n_actions=1, batch_size=33, device=gpu_device, replay=False)
    with pytest.raises(ValueError, match="grad_clip"):
        _loop(agent=Agent(grad_clip=_clip(2.0, None), capturable=True, **kw))
    with pytest.raises(ValueError, match="grad_clip"):
        _loop(clip=None, agent=Agent(grad_clip=_clip(2.0, None), capturable=True, **kw))
    with pytest.raises(ValueError, match="grad_clip in a population"):
        PopulationLearner([Agent(grad_clip=_clip(2.0, None), **kw)], 33, rings=[None], seeds=[1])
    with pytest.raises(ValueError, match="grad_clip with demo_loss"):
        FusedLearner(Agent(**kw), 33, demo_loss=DemoLoss(0.1), grad_clip=_clip(1.0, None))
    fl = FusedLearner(Agent(**kw), 33, grad_clip=_clip(1.0, 0.5))
    with pytest.raises(ValueError, match="grad_clip"):
        fl.enable_p2p()
    with pytest.raises(ValueError, match="grad_clip"):
        fl.enable_data_parallel()
    fl.grad_sync_critic = fl.grad_sync_actor = lambda: None
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=gpu_device)
    with pytest.raises(ValueError, match="grad_clip"):
        fl.learn_batch(z(33, 23), z(33, 1), z(33), z(33, 23), z(33, dtype=torch.uint8))
    plain = FusedLearner(Agent(**kw), 33)
    plain.grad_sync_critic = plain.grad_sync_actor = lambda: None
    with pytest.raises(ValueError, match="grad_clip"):
        plain.set_grad_clip(_clip(1.0, None))
    with pytest.raises(ValueError, match="grad_clip is off"):
        FusedLearner(Agent(**kw), 33).clip_stats()
