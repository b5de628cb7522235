"""GPU (-m gpu): the TD3 launches (csrc/tttd3.hip, td3.TD3Learner) against the lone DDPG learn() bit for bit where TD3 degenerates to
it, against TD3 in f64 (tests/td3_ref.py) with the bounds of tests/test_gpu_learn_shapes.py unchanged, the delay's bookkeeping, the
smoothing noise against its host reproduction, and the loop (graphs against eager steps, resume).

Worst error / bound per check of test_one_full_update_against_f64 and test_delay..., and worst |eps - host| / bound of test_noise,
are printed by the tests ("RATIOS ..."); the figures measured on MI355X are in each test's docstring."""
import math

import numpy as np
import pytest

import learn_ref as R
import td3_ref as T

pytestmark = pytest.mark.gpu


def _cfg(**kw):
    from ddpg_trucktrailer_amd.td3 import TD3Config
    return TD3Config(**kw)


def _td3_learner(dev, state, hyper, cfg, batch, images, noise_seed=None):
    """(agent, TD3Learner, ring, batch on the device): f32 nets, moments and both step counts of `state`; the ring's draw IS the batch."""
    import torch
    from ddpg_trucktrailer_amd.td3 import TD3Learner
    from learn_checks import ring_with_batch as _ring_with_batch
    B = batch[0].shape[0]
    on_dev = [t.to(dev).contiguous() for t in batch]
    ring, seed = _ring_with_batch(dev, B, on_dev)
    agent = T.load_td3_agent(state, hyper, cfg, dev, torch.float32)
    fl = TD3Learner(agent, B, ring, seed, fc2_images=images, noise_seed=noise_seed)
    fl.import_from_optimizers()
    fl.set_step_counts({"step": state["step"], "actor_step": state["actor_step"]})      # (the optimizers' f32 step is exact below 2^24 only)
    assert fl.use_images == images and int(fl.step_dev.item()) == state["step"] and int(fl.actor_step_dev.item()) == state["actor_step"]
    return agent, fl, ring, on_dev


def _drawn(ring, B, batch):
    import torch
    for got, want in zip(ring._batch_bufs(B)[:5], batch):
        assert torch.equal(got.view(-1), want.view(-1)), "the launch's draw is not the batch"


@pytest.mark.parametrize("B", [1, 257])
def test_equal_critics_no_noise_delay_one_is_ddpg_bit_for_bit(gpu_device, B):
    """learn_ref's trained-scale state (step 999, TRAINED_HYPER), images on; critic_2 and target_critic_2 are copies of critic 1's
    (parameters and Adam moments), sigma = 0, delay 1.  After 3 updates everything equals a lone FusedLearner with the tail in one
    launch on the same batch, bit for bit: actor, critic, both targets, both m and v, both flat gradients, q_pi, dq_da, y and both
    step counts; critic_2 is critic 1, y2 is y, eps is zero, and no tail gave up."""
    import torch
    from test_gpu_learn_shapes import _learner, _results
    dev = gpu_device
    case = (B, 20.0, 3, 999, "trained", R.SEED)
    assert case in R.PATH_CASES
    state, hyper, batch, _, _ = R.case(*case)
    _, lone, on_dev = _learner(dev, case, True)
    lone.fuse_tail = True
    for _ in range(3):
        lone.learn_batch(*on_dev)
    torch.cuda.synchronize()
    assert lone.tail_gave_up() == 0
    want = _results(lone)
    twin = dict(state, actor_step=state["step"])
    twin["nets"] = dict(state["nets"], critic_2=state["nets"]["critic"], target_critic_2=state["nets"]["target_critic"])
    twin["m"], twin["v"] = dict(state["m"], critic_2=state["m"]["critic"]), dict(state["v"], critic_2=state["v"]["critic"])
    agent, fl, ring, _ = _td3_learner(dev, twin, hyper, _cfg(policy_delay=1, target_noise=0.0, noise_clip=0.5), batch, True)
    for _ in range(3):
        fl.learn_batch(u=0)
    torch.cuda.synchronize()
    _drawn(ring, B, on_dev)
    assert fl.tail_gave_up() == 0
    got = _results(fl)
    assert len(got) == len(want) and all(torch.isfinite(x).all() for x in want)
    for i, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(x, y), (B, i)
    assert int(fl.actor_step_dev.item()) == int(fl.step_dev.item()) == 1002
    assert torch.equal(fl.y, lone.y) and torch.equal(fl.y, fl.y2) and torch.equal(fl.q, lone.q) and torch.equal(fl.q, fl.q2)
    assert torch.equal(fl.q1t, fl.q2t) and fl.eps.eq(0).all()
    for a, b in ((agent.critic, agent.critic_2), (agent.target_critic, agent.target_critic_2)):
        for x, y in zip(a.parameters(), b.parameters()):
            assert torch.equal(x, y)
    assert torch.equal(fl.critic.m, fl.critic_2.m) and torch.equal(fl.critic.v, fl.critic_2.v)
    assert torch.equal(fl.critic.flat_grad, fl.critic_2.flat_grad)


def _ulp32(x64):
    import torch
    x = x64.float().abs()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def _adam_checks(check, key, st, before, grads, t, h, cancelling_targets=False):
    """test_one_learn_step_against_f64's four optimizer bounds for one net, at the kernel's own gradient.
    cancelling_targets (tests/test_gpu_big_counters.py): the target's 2 ulp are a bound of the f32 formats only while the rounding
    of the difference p - target0, carried through tau, stays below them: |err| <= ulp32(target) / 2 + tau ulp32(p - target0) / 2.
    Where tau (p - target0) cancels target0 -- the new target is orders of magnitude below the old one -- the second term is
    hundreds of ulps of the result, whatever the kernel does.  With the flag, an element whose second term alone exceeds 1.5 ulp of
    the f64 target is held to the f32 arithmetic itself instead: its bits must be those of the correctly rounded
    fmaf(tau, p - target0, target0) on the kernel's own f32 inputs; every other element keeps the 2 ulp."""
    import torch
    b1 = h["betas"][0]
    for i in range(len(st.params)):
        p0, m0, v0, t0 = (before[k][i].double().reshape(-1) for k in ("p", "m", "v", "t"))
        g = grads[i].double().reshape(-1)
        p64, m64, v64, _, g2 = R.adam64(p0, m0, v0, t0, g, t, h)
        p, m, v, tg = (x.detach().double().reshape(-1) for x in (st.params[i], st.ms[i], st.vs[i], st.targets[i]))
        terms = (b1 * m0).abs() + ((1 - b1) * g2).abs()
        check("adam m " + key, (m - m64).abs(), (4 * 2.0 ** -24 * terms).clamp_min(2.0 ** -149))
        check("adam v " + key, (v - v64).abs(), 6 * 2.0 ** -24 * v64 + 2.0 ** -149)
        kappa = terms / m64.abs().clamp_min(1e-300)
        rel = ((18 + 6 * kappa) * 2.0 ** -24).clamp_min(2.0 ** -19)
        check("adam p " + key, (p - p64).abs(), _ulp32(p64) + rel * (p64 - p0).abs())
        tg64 = R.soft64(t0, p, h["tau"])
        if cancelling_targets:
            d32 = (st.params[i].detach().reshape(-1) - before["t"][i].reshape(-1)).double()           # (the f32 difference, as formed)
            loose = 0.5 * h["tau"] * _ulp32(d32) > 1.5 * _ulp32(tg64)
            fma32 = (h["tau"] * d32 + t0).float()                  # (tau d32 is exact in f64: one rounding to f64, one to f32)
            assert torch.equal(st.targets[i].detach().reshape(-1)[loose], fma32[loose]), (key, i, "target where tau (p - t0) cancels t0")
            check("target " + key, ((tg - tg64).abs() / (2 * _ulp32(tg64)))[~loose], torch.ones((), dtype=torch.float64, device=tg.device))
        else:
            check("target " + key, (tg - tg64).abs(), 2 * _ulp32(tg64))
        assert not torch.equal(p, p0), (key, i)


def _before(st):
    return dict(p=[x.detach().clone() for x in st.params], t=[x.detach().clone() for x in st.targets],
                m=[x.clone() for x in st.ms], v=[x.clone() for x in st.vs])


@pytest.mark.parametrize("images", [True, False], ids=["images", "f32"])
@pytest.mark.parametrize("case", T.F64_CASES, ids=lambda c: f"B{c[0]}")
def test_one_full_update_against_f64(gpu_device, case, images):
    """One full TD3 update (distinct critics, sigma 0.2, c 0.5) from td3_ref.case(*case), every result against td3_ref.td3_step fed
    the kernel's own eps.  |eps| <= c; y, q, q2, q1t, q2t, q_pi, dq_da within 2e-5 max(1, max |ref|); y[done] == r[done]; y2 == y;
    dq_da of a row with a unit of Q1(s, mu(s)) within 3e-5 of zero is compared with the nearest of learn_ref.dq_da_choices.  Both
    critics' and the actor's gradients within max(3e-5 max |g64| + 1e-7, 3 e32), e32 from the torch f32 twin's TD3 learn_batch with
    the same eps.  Adam m, v, p and the soft-updated targets of all three trained nets: the four bounds of
    tests/test_gpu_learn_shapes.py::test_one_learn_step_against_f64, unchanged.  All six fc2 images equal ones packed from scratch
    (targets over their forward planes).

    Worst error / bound per check, measured on MI355X (fc2 images on | off; adam m, v, p and target: the worst of the three nets;
    "near": rows of Q1(s, mu(s)) with a unit within 3e-5 of zero):

        case   pre-ReLU            y            q           q2          q1t          q2t         q_pi           dq_da
        B1    0.18|0.17  0.026|0.0007  0.020|0.004  0.0004|0.021  0.0004|0.004  0.026|0.0008  0.002|0.002     8e-5|8e-5
        B250  0.28|0.35   0.016|0.019  0.020|0.019   0.022|0.032   0.017|0.021   0.020|0.022  0.009|0.013  0.0005|0.0005
        B257  0.33|0.31   0.014|0.019  0.023|0.024   0.026|0.040   0.019|0.023   0.015|0.021  0.010|0.011  0.0007|0.0007

        case  grad critic  grad critic_2   grad actor          m          v          p     target  near
        B1    0.018|0.014    0.027|0.034  0.017|0.017  0.43|0.43  0.61|0.62  0.50|0.50  0.47|0.47     0
        B250  0.014|0.010    0.015|0.019  0.006|0.009  0.43|0.43  0.64|0.61  0.50|0.50  0.42|0.42     6
        B257  0.012|0.013    0.013|0.012  0.005|0.009  0.43|0.43  0.62|0.63  0.50|0.50  0.42|0.42     1"""
    state, hyper, batch, _ = T.case(*case)
    full_update_against_f64(gpu_device, state, hyper, batch, images)


def full_update_against_f64(dev, state, hyper, batch, images, cancelling_targets=False):
    """The body of test_one_full_update_against_f64 on any state (tests/test_gpu_big_counters.py gives one with large step counts;
    cancelling_targets: see _adam_checks).  Returns (worst error / bound per check, the learner after the update)."""
    import torch
    from learn_checks import ACTOR_NAMES as _ACTOR_NAMES, CRITIC_NAMES as _CRITIC_NAMES, scratch_image as _scratch_image
    B = batch[0].shape[0]
    cfg, h32 = T.default_cfg(), R.f32_hyper(hyper)
    agent, fl, ring, (s, a, r, s2, d8) = _td3_learner(dev, state, hyper, cfg, batch, images, noise_seed=77)
    states = (("critic", fl.critic), ("critic_2", fl.critic_2), ("actor", fl.actor))
    before = {key: _before(st) for key, st in states}
    fl.learn_batch(u=0, full=True)
    torch.cuda.synchronize()
    _drawn(ring, B, (s, a, r, s2, d8))
    assert fl.tail_gave_up() == 0
    worst = {}

    def check(name, err, tol):
        ratio = (err / tol).max().item() if torch.is_tensor(err) else err / tol
        worst[name] = max(worst.get(name, 0.0), ratio)
        assert ratio <= 1.0, (name, B, ratio)

    eps = fl.eps.double().cpu()
    assert eps.abs().max().item() <= float(np.float32(cfg.noise_clip))
    host_eps, _ = T.noise_eps(77, state["step"], B, cfg.target_noise, cfg.noise_clip)
    assert np.abs(eps.numpy() - host_eps).max() <= 1e-5          # (test_noise holds the tight bound)
    ref = T.td3_step(state, batch, hyper, cfg, eps.numpy(), full=True)
    # ---- no unit changes side in the three forwards that depend on a row alone
    for key, st in states:
        sd = {k: v.to(dev).double() for k, v in state["nets"][key].items()}
        z1 = st.saved_t["xh1"].double() * sd["bn1.weight"] + sd["bn1.bias"]
        z2 = st.saved_t["xh2"].double() * sd["bn2.weight"] + sd["bn2.bias"]
        if st.critic:
            z2 = z2 + a.double().view(-1, 1) * sd["action_value.weight"].view(1, -1) + sd["action_value.bias"]
        for got, want in zip((z1, z2), ref["z"][key]):
            check("pre-relu", (got.cpu() - want).abs().max().item(), R.MARGIN / 3)
    # ---- outputs
    done = d8.bool()
    assert torch.equal(fl.y[done], r[done]) and torch.equal(fl.y, fl.y2)
    for name in ("y", "q", "q2", "q1t", "q2t"):
        check(name, (getattr(fl, name).double().cpu() - ref[name]).abs().max().item(), 2e-5 * max(1.0, ref[name].abs().max().item()))
    nets = dict(state["nets"], critic={k: v.detach().cpu() for k, v in agent.critic.state_dict().items()})
    a64 = T.load_td3_agent(dict(state, nets=nets), hyper, cfg, torch.device("cpu"), torch.float64)
    s64 = s.double().cpu()
    half = R.actor_half(a64.critic, a64.actor, s64)
    check("q_pi", (fl.q_pi.double().cpu() - half["q_pi"]).abs().max().item(), 2e-5 * max(1.0, half["q_pi"].abs().max().item()))
    got_dq, dq64 = fl.dq_da.double().cpu(), half["dq_da"].clone()
    choices = R.dq_da_choices(a64.critic, half["z_pi"][1], half["dq_da"])
    for b, values in choices.items():
        dq64[b] = min(values, key=lambda x: abs(x - got_dq[b].item()))
    check("dq_da", (got_dq - dq64).abs().max().item(), 2e-5 * max(1.0, dq64.abs().max().item()))
    # ---- gradients at the three optimizer sites
    g64 = dict(critic=ref["grads"]["critic"], critic_2=ref["grads"]["critic_2"],
               actor=R.actor_half(a64.critic, a64.actor, s64, dq_da=dq64)["grads"])
    twin, g32 = T.load_td3_agent(state, hyper, cfg, dev, torch.float32), {}
    for key in T.TRAINED:
        net = getattr(twin, key)

        def step(*args, _net=net, _key=key, _orig=net.optimizer.step, **kw):
            g32[_key] = {k: p.grad.clone() for k, p in _net.named_parameters()}
            return _orig(*args, **kw)
        net.optimizer.step = step
    twin.learn_batch(s, a, r, s2, done, eps=fl.eps.clone(), full=True)
    for key, st in states:
        names = _ACTOR_NAMES if key == "actor" else _CRITIC_NAMES
        assert len(st.grads) == len(names) == len(g64[key])
        for name, g in zip(names, st.grads):
            want = g64[key][name]
            e32 = (g32[key][name].double().cpu() - want).abs().max().item()
            tol = max(3e-5 * want.abs().max().item() + 1e-7, 3 * e32)
            check("grad " + key, (g.double().cpu() - want).abs().max().item(), tol)
    # ---- optimizer arithmetic at the kernel's own gradient: the critics at the shared step, the actor at its own
    assert int(fl.step_dev.item()) == state["step"] + 1 and int(fl.actor_step_dev.item()) == state["actor_step"] + 1
    for key, st in states:
        t = (state["actor_step"] if key == "actor" else state["step"]) + 1
        _adam_checks(check, key, st, before[key], st.grads, t, R.net_hyper(h32, "actor" if key == "actor" else "critic"), cancelling_targets)
    # ---- images
    if images:
        fwd = 2 * 20 * 13 * 512
        assert fl.images_current()
        for net in fl._nets():
            kept, fresh = fl._img[id(net)], _scratch_image(fl, net, dev)
            if net in (agent.target_actor, agent.target_critic, agent.target_critic_2):
                assert torch.equal(kept.view(torch.float16)[:fwd], fresh.view(torch.float16)[:fwd]), "target image differs"
            else:
                assert torch.equal(kept, fresh), "maintained image differs from one made from scratch"
    print(f"RATIOS td3 B{B} {'images' if images else 'f32'}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) +
          f", rows near a boundary in Q1(s, mu(s)) {len(choices)}")
    return worst, fl


def test_delay_two_first_update_trains_the_critics_only(gpu_device):
    """Delay 2, two updates at B = 257 by the learner's own count.  After the first the actor, its m and v, its step word, the three
    targets and the three target images keep their bits and the critic step is 1; after the second the actor step is 1 and the
    critic step 2, and the actor's p is adam64 WITH t = 1 at the kernel's own gradient inside test_one_full_update_against_f64's
    bound (with the shared count t = 2 the bias corrections 0.1 and 0.001 would be 0.19 and 0.002: a step 0.74 times as long).
    Measured on MI355X, worst error / bound of the actor: m 0.24, v 0.32, p 0.50, target 0.31."""
    import torch
    dev = gpu_device
    case = T.DELAY_CASE
    B = case[0]
    state, hyper, batch, _ = T.case(*case)
    cfg, h32 = T.default_cfg(), R.f32_hyper(hyper)
    agent, fl, ring, _ = _td3_learner(dev, state, hyper, cfg, batch, True, noise_seed=5)
    fl.refresh_images()
    torch.cuda.synchronize()
    targets = (agent.target_actor, agent.target_critic, agent.target_critic_2)

    def frozen():
        out = [p.detach().clone() for p in agent.actor.parameters()] + [fl.actor.m.clone(), fl.actor.v.clone(), fl.actor_step_dev.clone()]
        out += [p.detach().clone() for n in targets for p in n.parameters()] + [fl._img[id(n)].clone() for n in targets]
        return out
    before, actor_before = frozen(), _before(fl.actor)
    critic_before = [p.detach().clone() for p in agent.critic.parameters()]
    fl.learn_batch(u=0)
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(frozen(), before)):
        assert torch.equal(x, y), i
    assert int(fl.step_dev.item()) == 1 and int(fl.actor_step_dev.item()) == 0
    assert not any(torch.equal(x, y) for x, y in zip(agent.critic.parameters(), critic_before))
    fl.learn_batch(u=0)
    torch.cuda.synchronize()
    assert int(fl.step_dev.item()) == 2 and int(fl.actor_step_dev.item()) == 1 and fl.tail_gave_up() == 0 and fl.images_current()
    worst = {}

    def check(name, err, tol):
        ratio = (err / tol).max().item()
        worst[name] = max(worst.get(name, 0.0), ratio)
        assert ratio <= 1.0, (name, ratio)
    _adam_checks(check, "actor", fl.actor, actor_before, fl.actor.grads, 1, R.net_hyper(h32, "actor"))
    print("RATIOS td3 delay: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def _phi(x):
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


def test_noise(gpu_device):
    """B = 1024, sigma 0.2, c 0.5, 8 updates.  eps equals the host reproduction (td3_ref.noise_eps: the kernel's f32 uniforms and
    angle, then f64 log / sqrt / cos, then the clip) within 1e-5 sigma max(1, |N|) -- a few ulps of logf, cosf and sqrtf.  The noise
    differs from step to step and with the seed and repeats when step and seed repeat.  Over the 8192 samples the share of clipped
    rows, the mean and the variance are within 5 standard errors of the clipped normal's analytic values.

    Measured on MI355X: worst |eps - host| / bound 0.019; clipped share 0.0131 (analytic 0.0124, 0.5 standard errors), mean 2.5e-3
    (1.1 standard errors), variance 0.03864 (analytic 0.03910, 0.5 standard errors)."""
    import torch
    dev = gpu_device
    B, sigma, c, updates = 1024, 0.2, 0.5, 8
    cfg = _cfg(policy_delay=2, target_noise=sigma, noise_clip=c)
    state = T.make_td3_state(T.SEED, 1.0, 0)
    batch = R._candidates(B, torch.Generator().manual_seed(123))
    _, fl, _, _ = _td3_learner(dev, state, R.DEFAULT_HYPER, cfg, batch, True, noise_seed=4711)

    def run(n):
        out = []
        for _ in range(n):
            fl.learn_batch(u=0)
            out.append(fl.eps.clone())
        torch.cuda.synchronize()
        return [e.double().cpu().numpy() for e in out]
    got = run(updates)
    worst = 0.0
    for t, e in enumerate(got):
        host, nrm = T.noise_eps(4711, t, B, sigma, c)
        assert np.abs(e).max() <= c
        ratio = (np.abs(e - host) / (1e-5 * sigma * np.maximum(1.0, np.abs(nrm)))).max()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (t, ratio)
    assert all(not np.array_equal(got[i], got[j]) for i in range(updates) for j in range(i))
    # the same steps again: the same noise; another seed: another noise
    fl.step_dev.fill_(0)
    again = run(2)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    fl.set_noise_seed(4712)
    fl.step_dev.fill_(0)
    other = run(1)
    assert not np.array_equal(other[0], got[0])
    # the clipped normal's moments
    x = np.concatenate(got)
    n, k = x.size, c / sigma
    p_clip = 2.0 * (1.0 - _phi(k))
    pdf = math.exp(-0.5 * k * k) / math.sqrt(2.0 * math.pi)
    inside = 2.0 * _phi(k) - 1.0
    var = sigma ** 2 * (inside - 2.0 * k * pdf) + c ** 2 * p_clip
    mu4 = sigma ** 4 * (3.0 * inside - 2.0 * (k ** 3 + 3.0 * k) * pdf) + c ** 4 * p_clip
    share = float((np.abs(x) >= c).mean())
    assert abs(share - p_clip) <= 5.0 * math.sqrt(p_clip * (1.0 - p_clip) / n), (share, p_clip)
    assert abs(x.mean()) <= 5.0 * math.sqrt(var / n), x.mean()
    assert abs(x.var() - var) <= 5.0 * math.sqrt((mu4 - var ** 2) / n), (x.var(), var)
    print(f"RATIOS td3 noise: worst |eps - host| / bound {worst:.3g}, clipped share {share:.4f} (analytic {p_clip:.4f}), "
          f"mean {x.mean():.2e}, variance {x.var():.5f} (analytic {var:.5f})")


def _loop_state(loop):
    import torch
    fl = loop.learner
    out = [p.detach().clone() for net in loop.agent._nets() for p in net.parameters()]
    out += [fl.actor.m, fl.actor.v, fl.critic.m, fl.critic.v, fl.critic_2.m, fl.critic_2.v, fl.step_dev, fl.actor_step_dev]
    return out + [getattr(loop.ring, name) for name in ("obs", "act", "rew", "done")] + [loop.noise.x, loop.env.state]


def test_loop_graphs_equal_eager_steps_and_resume_is_bitwise(gpu_device, tmp_path):
    """DDPGRollout(td3=TD3Config(), updates_per_step=2) at N = 1024, B = 256, 8 ring slots: 12 vector steps through graphs equal 12
    eager step()s bit for bit -- six nets, the three nets' moments, both counters, ring, noise and env -- and a loop saved after 6
    steps and restored into a fresh loop (another seed) ends the 12 steps with the same bits.  updates_per_step = 1 with the
    default config raises."""
    import torch
    from ddpg_trucktrailer_amd import checkpoint
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.td3 import TD3Learner
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv

    def make(seed, graph_steps, **kw):
        env = TruckTrailerVecEnv(1024)
        env.reset(seed=seed)
        kw.setdefault("updates_per_step", 2)
        return DDPGRollout(env, batch_size=256, replay_slots=8, seed=seed, graph_steps=graph_steps, td3=_cfg(), **kw)
    a, b = make(5, 4), make(5, 0)
    assert isinstance(a.learner, TD3Learner) and a.pipeline is False and a.graph_steps == 4 and b.graph_steps == 0
    a.run(6)
    path = checkpoint.save_loop_checkpoint(str(tmp_path / "td3_loop.pt"), a)
    a.run(6)
    for _ in range(12):
        b.step()
    torch.cuda.synchronize()
    assert a.graph1 is not None and a.graphG is not None and a.ring.k == b.ring.k == 12
    sa, sb = _loop_state(a), _loop_state(b)
    assert len(sa) == len(sb)
    for i, (x, y) in enumerate(zip(sa, sb)):
        assert torch.equal(x, y), i
    steps, actor_steps = int(a.learner.step_dev.item()), int(a.learner.actor_step_dev.item())
    assert steps == 2 * actor_steps and steps >= 2 * 10 and a.learner.tail_gave_up() == 0
    c = make(99, 4)
    checkpoint.load_loop_checkpoint(path, c)
    assert c.ring.k == 6
    c.run(6)
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(_loop_state(c), sa)):
        assert torch.equal(x, y), i
    # a checkpoint without TD3 is refused by a TD3 loop, and the other way round
    env = TruckTrailerVecEnv(1024)
    env.reset(seed=5)
    plain = DDPGRollout(env, batch_size=256, replay_slots=8, seed=5, graph_steps=0, pipeline=False)
    with pytest.raises(ValueError, match="td3"):
        plain.load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="td3"):
        c.load_state_dict(plain.state_dict())
    with pytest.raises(ValueError, match="updates_per_step"):
        make(5, 4, updates_per_step=1)
    for lp in (a, b, c, plain):
        lp.env.close()


def test_descriptor_is_rewritten_in_place_when_a_parameter_storage_moves(gpu_device):
    """Two learners from the same state take one eager update and then replay a captured graph of one update twice; in one of them
    every parameter of critic_2 and of the target actor is given a new storage (same values) and the noise seed is set again
    between the replays.  That learner writes the new description over its descriptor at the same device address (new weight
    structs, fc2 images and optimizer tables), so the graph captured before stays valid, and it ends with the other's bits."""
    import torch
    from ddpg_trucktrailer_amd.rollout import _CAPTURE_MODE
    dev = gpu_device
    state, hyper, batch, _ = T.case(*T.DELAY_CASE)
    runs = []
    for move in (False, True):
        agent, fl, _, _ = _td3_learner(dev, state, hyper, T.default_cfg(), batch, True, noise_seed=5)
        fl.learn_batch(u=0, full=False)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side, capture_error_mode=_CAPTURE_MODE):
            fl.learn_batch(u=0, full=True)
        torch.cuda.current_stream().wait_stream(side)
        g.replay()
        torch.cuda.synchronize()
        handle, key = fl._h.value, fl._key
        if move:
            with torch.no_grad():
                for net in (agent.critic_2, agent.target_actor):
                    for p in net.parameters():
                        p.data = p.data.clone()
            fl.set_noise_seed(5)
        fl.refresh_images()                # (what a loop calls before it replays)
        g.replay()
        torch.cuda.synchronize()
        assert fl._h.value == handle and (fl._key != key) == move and fl.tail_gave_up() == 0 and fl.images_current()
        assert int(fl.step_dev.item()) == 3 and int(fl.actor_step_dev.item()) == 2
        runs.append([p.detach().clone() for n in fl._nets() for p in n.parameters()] +
                    [fl.critic.m, fl.critic_2.m, fl.actor.m, fl.critic_2.v, fl.y, fl.eps, fl.q_pi])
    for i, (x, y) in enumerate(zip(*runs)):
        assert torch.equal(x, y), i
