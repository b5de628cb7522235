"""What the GPU tests of the lone learn() share (tests/test_gpu_learn_shapes.py plain, tests/test_gpu_loss_shape.py with a LossShape,
tests/test_gpu_demo_loss.py with a DemoLoss): a FusedLearner that holds a learn_ref state (learner), and the comparison of one update
with f64 (against_f64), whose options are arguments -- every check and bound is written here once.  No GPU is touched on import."""
import ctypes as C

import demo_ref as D
import learn_ref as R

CRITIC_NAMES = ["fc1.weight", "fc1.bias", "bn1.weight", "bn1.bias", "fc2.weight", "fc2.bias", "bn2.weight", "bn2.bias", "q.weight",
                "q.bias", "action_value.weight", "action_value.bias"]
ACTOR_NAMES = CRITIC_NAMES[:8] + ["mu.weight", "mu.bias"]          # the order of FusedLearner's gradient views (tt_mlp_weights)


def case_id(case):
    return "B{}-x{:g}".format(case[0], case[1])


def loss_shape(delta, c):
    from ddpg_trucktrailer_amd.loss_shape import LossShape
    return LossShape(delta, c)


def learner(dev, state, hyper, batch, step, images=True, shape=None, tail=False, demo=None):
    """(agent, FusedLearner, batch on the device) holding `state`: f32 nets, Adam moments and step count."""
    import torch
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    agent = R.load_agent(state, hyper, dev, torch.float32)
    fl = FusedLearner(agent, batch[0].shape[0], fc2_images=images, loss_shape=shape, demo_loss=demo)
    fl.import_from_optimizers()
    fl.step_dev.fill_(int(step))          # (the optimizers' f32 step holds it exactly only below 2^24)
    fl.refresh_images()
    fl.fuse_tail = tail
    assert fl.use_images == images and int(fl.step_dev.item()) == step
    return agent, fl, [t.to(dev).contiguous() for t in batch]


def ulp32(x64):
    import torch
    x = x64.float().abs()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def scratch_image(fl, net, dev):
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    w = L.TTMlpWeights()
    C.memmove(C.byref(w), C.byref(fl.w(net)), C.sizeof(w))
    img = torch.zeros(int(fl.lib.tt_mlp_fc2_image_bytes()), dtype=torch.uint8, device=dev)
    w.fc2_img = img.data_ptr()
    L.check(fl.lib.tt_mlp_fc2_image_pack(C.byref(w), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return img


def ring_with_batch(dev, B, batch):
    """A ring of one stored step whose draw with `seed` IS the batch, in order (as tests/test_gpu_population.py lays out F5's): with
    2^20 envs the first seed of a short list whose B rows pick distinct envs."""
    from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing
    s, a, r, s2, d8 = batch
    ring = TrajectoryRing(1 << 20, 3, 23, dev)
    ring.k = 1
    ring.k_dev.fill_(1)
    for seed in range(4242, 4242 + 32):
        idx = ring.sample_fused(B, seed=seed, return_index=True)[-1]
        env = idx[:, 1].long()
        if env.unique().numel() == B:
            break
    assert idx[:, 0].eq(0).all() and env.unique().numel() == B
    ring.obs[0, env] = s
    ring.obs[1, env] = s2
    ring.act[0, env] = a.view(-1)
    ring.rew[0, env] = r
    ring.done[0, env] = d8
    return ring, seed


def results(fl):
    ag = fl.agent
    out = [p.detach().clone() for n in (ag.actor, ag.critic, ag.target_actor, ag.target_critic) for p in n.parameters()]
    return out + [t.clone() for t in (fl.actor.m, fl.actor.v, fl.critic.m, fl.critic.v, fl.actor.flat_grad, fl.critic.flat_grad,
                                      fl.y, fl.q, fl.q_pi, fl.dq_da, fl.step_dev)]


def same(a, b, what):
    import torch
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (what, i)


def flat(loop):
    import torch
    return torch.cat([p.detach().reshape(-1) for net in loop.agent._nets() for p in net.parameters()])


def against_f64(dev, state, hyper, batch, ref, *, delta=None, c=0.0, demo=None, images, tag, frozen=(), tail=False, prepare=None):
    """One learn_batch of a FusedLearner that holds `state` -- with LossShape(delta, c) unless both are off, with the DemoLoss `demo`
    and demo_ref.demo_index's rows when one is given -- every result against f64: `ref` is learn_ref.ref_step's result on the same
    state, batch and options.

    The checks and bounds without an option are told, and the optimizer's bound justified, in the docstring of
    tests/test_gpu_learn_shapes.py::test_one_learn_step_against_f64: no unit changes side; y, q, q_pi, dq_da; the gradients at both
    optimizer sites; m, v, p and target of every element; every tensor moved (but the critic's named in `frozen`); the step count;
    the fc2 images.  The options add:
    With a shape, pre -- the head's pre-activation as the rows launch recomputed it, a head output of the same dot product -- within
    the outputs' bound, 2e-5 max(1, max |pre64|); the f32 twin and the f64 actor half carry the penalty.
    With a demonstration loss: code is the reference's -- the filter compares q of the critic before its step with q_pi through the
    critic the learner left -- except on undecided rows (at most MAX_UNDECIDED of the demonstration rows from 33 rows on), where
    either code of a demonstration row is accepted and the reference gradient is formed with the learner's choice; dq_da stays the
    TRUE derivative; dq_eff within the outputs' bound, and it holds dq_da's bits on every row the learner did not apply;
    demo_stats() counts the mask's and the applied rows and its bc_loss is the f64 one within 1e-5 relative.

    Prints the worst error / bound per check (RATIOS) and, as figures, not checks: kappa, p's error over the bound with 2^-19 alone
    (no kappa), and the rows whose dQ/da was taken from the other side of a ReLU boundary than f64's.
    tail: the actor tail in one launch (fuse_tail); prepare: called with the learner before its update (e.g. to turn its learn log on).
    Returns (worst ratios, the learner, the f64 actor half at dq64, dq64)."""
    import torch
    B, step0 = batch[0].shape[0], state["step"]
    shape = loss_shape(delta, c) if (delta is not None or c) else None
    lam = demo.bc_weight if demo is not None else 0.0
    h32 = R.f32_hyper(hyper)
    agent, fl, (s, a, r, s2, d8) = learner(dev, state, hyper, batch, step0, images, shape, tail=tail, demo=demo)
    if prepare is not None:
        prepare(fl)
    twin = R.load_agent(state, hyper, dev, torch.float32)
    twin.loss_shape = shape
    before = {st: dict(p=[x.detach().clone() for x in st.params], t=[x.detach().clone() for x in st.targets],
                       m=[x.clone() for x in st.ms], v=[x.clone() for x in st.vs]) for st in (fl.critic, fl.actor)}
    if demo is not None:
        mask = ref["demo"]
        idx = D.demo_index(B, dev)
        assert torch.equal(idx[:, 0].cpu() < 0, mask)
        fl.learn_batch(s, a, r, s2, d8, demo_index=idx)
    else:
        fl.learn_batch(s, a, r, s2, d8)
    torch.cuda.synchronize()
    worst, figures = {}, {}

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
    # the third forward, in f64 on the critic this learn() left
    nets = dict(state["nets"], critic={k: v.detach().cpu() for k, v in agent.critic.state_dict().items()})
    a64 = R.load_agent(dict(state, nets=nets), hyper, torch.device("cpu"), torch.float64)
    s64, act64 = s.double().cpu(), a.double().cpu()
    half = R.actor_half(a64.critic, a64.actor, s64, act64, c=c)
    check("q_pi", (fl.q_pi.double().cpu() - half["q_pi"]).abs().max().item(), 2e-5 * max(1.0, half["q_pi"].abs().max().item()))
    got_dq, dq64 = fl.dq_da.double().cpu(), half["dq_da"].clone()
    choices = R.dq_da_choices(a64.critic, half["z_pi"][1], half["dq_da"])
    for b, values in choices.items():
        dq64[b] = min(values, key=lambda x: abs(x - got_dq[b].item()))
    figures["other side"] = sum(1 for b in choices if dq64[b] != half["dq_da"][b])
    check("dq_da", (got_dq - dq64).abs().max().item(), 2e-5 * max(1.0, dq64.abs().max().item()))
    if shape is not None:
        check("pre", (fl.pre.double().cpu() - half["pre"]).abs().max().item(), 2e-5 * max(1.0, half["pre"].abs().max().item()))
    # ---- the filter
    applied = None
    if demo is not None:
        filt = D.filter_of(ref["q"], half["q_pi"], mask)
        want_code = D.codes(mask, filt["above"] if demo.q_filter else mask)
        code = fl.code.cpu()
        und = filt["undecided"] if demo.q_filter else torch.zeros_like(mask)
        assert int(und.sum()) <= D.MAX_UNDECIDED * int(mask.sum()) or B < 33, (tag, int(und.sum()))
        assert torch.equal(code[~und], want_code[~und]), (tag, "code")
        assert bool(((code[und] == 1) | (code[und] == 2)).all())
        applied = code == 2
    # ---- gradients at both optimizer sites, the actor's with the rows the learner applied
    half_dq = R.actor_half(a64.critic, a64.actor, s64, act64, dq_da=dq64, c=c, lam=lam, applied=applied)
    if demo is not None:
        check("dq_eff", (fl.dq_eff.double().cpu() - half_dq["dq_eff"]).abs().max().item(), 2e-5 * max(1.0, half_dq["dq_eff"].abs().max().item()))
        assert torch.equal(fl.dq_eff[~applied.to(dev)], fl.dq_da[~applied.to(dev)])          # (a row without the term keeps dQ/da's bits)
    g64 = dict(critic=ref["grads"]["critic"], actor=half_dq["grads"])
    g32 = dict(actor=R.actor_half(twin.critic, twin.actor, s, a, dq_da=dq64.to(dev), c=c, lam=lam,
                                  applied=None if applied is None else applied.to(dev))["grads"])
    seen, orig = {}, twin.critic.optimizer.step

    def step(*args, **kw):
        seen.update({k: p.grad.clone() for k, p in twin.critic.named_parameters()})
        return orig(*args, **kw)
    twin.critic.optimizer.step = step
    twin.learn_batch(s, a, r, s2, done)
    g32["critic"] = seen
    for st, key, names in ((fl.critic, "critic", CRITIC_NAMES), (fl.actor, "actor", ACTOR_NAMES)):
        assert len(st.grads) == len(names) == len(g64[key])
        for name, g in zip(names, st.grads):
            want = g64[key][name]
            e32 = (g32[key][name].double().cpu() - want).abs().max().item()
            tol = max(3e-5 * want.abs().max().item() + 1e-7, 3 * e32)
            check("grad " + key, (g.double().cpu() - want).abs().max().item(), tol)
            worst["e32 share " + key] = max(worst.get("e32 share " + key, 0.0), 3 * e32 / (3e-5 * want.abs().max().item() + 1e-7))
    # ---- optimizer arithmetic at the kernel's own gradient
    t = step0 + 1
    assert int(fl.step_dev.item()) == t
    for st, key, names in ((fl.critic, "critic", CRITIC_NAMES), (fl.actor, "actor", ACTOR_NAMES)):
        h = R.net_hyper(h32, key)
        b1 = h["betas"][0]
        for i in range(len(st.params)):
            p0, m0, v0, t0 = (before[st][k][i].double().reshape(-1) for k in ("p", "m", "v", "t"))
            g = st.grads[i].double().reshape(-1)
            p64, m64, v64, _, g2 = R.adam64(p0, m0, v0, t0, g, t, h)
            p, m, v, tg = (x.detach().double().reshape(-1) for x in (st.params[i], st.ms[i], st.vs[i], st.targets[i]))
            terms = (b1 * m0).abs() + ((1 - b1) * g2).abs()
            check("adam m " + key, (m - m64).abs(), (4 * 2.0 ** -24 * terms).clamp_min(2.0 ** -149))
            check("adam v " + key, (v - v64).abs(), 6 * 2.0 ** -24 * v64 + 2.0 ** -149)
            kappa = terms / m64.abs().clamp_min(1e-300)
            rel = ((18 + 6 * kappa) * 2.0 ** -24).clamp_min(2.0 ** -19)
            check("adam p " + key, (p - p64).abs(), ulp32(p64) + rel * (p64 - p0).abs())
            flat_p = ((p - p64).abs() / (ulp32(p64) + 2.0 ** -19 * (p64 - p0).abs())).max().item()       # (a figure, not a check)
            figures["p at 2^-19 without kappa " + key] = max(figures.get("p at 2^-19 without kappa " + key, 0.0), flat_p)
            figures["kappa " + key] = max(figures.get("kappa " + key, 0.0), kappa[terms > 0].max().item() if (terms > 0).any() else 0.0)
            tg64 = R.soft64(t0, p, h["tau"])
            check("target " + key, (tg - tg64).abs(), 2 * ulp32(tg64))
            if not (key == "critic" and names[i] in frozen):
                assert not torch.equal(p, p0), (key, i)                                          # the step moved the tensor
    # ---- images
    if images:
        fwd = 2 * 20 * 13 * 512                              # halves of the two forward planes (test_fc2_images_follow_the_weights)
        assert fl.images_current()
        for net in (agent.actor, agent.critic, agent.target_actor, agent.target_critic):
            kept, fresh = fl._img[id(net)], scratch_image(fl, net, dev)
            if net in (agent.target_actor, agent.target_critic):
                assert torch.equal(kept.view(torch.float16)[:fwd], fresh.view(torch.float16)[:fwd]), "target image differs"
            else:
                assert torch.equal(kept, fresh), "maintained image differs from one made from scratch"
    line = f"RATIOS {tag} {'images' if images else 'f32'}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + \
           f", rows near a boundary in Q(s, mu(s)) {len(choices)}"
    # ---- demo_stats of this update
    if demo is not None:
        st = fl.demo_stats()
        assert st["demo_rows"] == int(mask.sum()) and st["applied"] == int(applied.sum())
        assert abs(st["bc_loss"] - half_dq["bc_part"]) <= 1e-5 * max(1e-3, abs(half_dq["bc_part"]))
        line += f", demonstration rows {int(mask.sum())}, applied {int(applied.sum())}, undecided {int(und.sum())}"
    print(line + "; figures: " + ", ".join(f"{k} {v:.3g}" for k, v in figures.items()))
    return worst, fl, half_dq, dq64
