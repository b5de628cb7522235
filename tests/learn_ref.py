"""What tests/test_learn_ref.py (CPU) and tests/test_gpu_learn_shapes.py (GPU) share: learn() restated in f64 with the project's own
modules, autograd and torch.optim.Adam (ref_step, actor_half: the loss shape and the demonstration loss are arguments of the one
step; tests/shape_ref.py and tests/demo_ref.py hold what is those options' own), the optimizer formula of adam_finish (csrc/ttlearn_bodies.h) in f64
(adam64), and a builder of states and batches whose ReLU units stay clear of zero (make_state, make_batch).

A unit whose pre-ReLU value lies within rounding of zero can fall on the other side in f32 than in f64, and its row's whole
contribution to a gradient then changes.  The tests built on this module do not bound that with a tolerance that gives way.

  * critic(s, a) and actor(s), the two forwards whose backward passes learn() runs, depend on a row alone.  make_batch replaces
    every row that has a unit within `margin` of zero in either until none is left: by construction no unit of the batch can
    change side.
  * The third forward, the UPDATED critic on (s, mu(s)), depends on the whole batch through the critic's Adam step, and that
    dependence is far steeper than `margin`: replacing 1 % of the rows moves the median pre-ReLU value of every other row by
    1e-2 at step 1 (zero moments: the step is lr * sign(g), and the exchange flips the sign of ~1 / sqrt(B) of the elements per
    row) and by 5e-4 from warmed moments at step 1000, measured with these networks at B = 250 .. 1024.  Each pass therefore
    deals all B rows a new hand -- 7 to 25 rows of 1000 are within 3e-5 after every one of 8 passes -- and no batch that is
    clean in this forward can be constructed.  It does not have to be: Q(s, mu(s)) is continuous in its pre-ReLU values, and the
    only quantity of learn() that is not is dQ/da = sum_j w3_j [z2_j > 0] wa_j, which enters the actor's gradient as one factor
    per row.  near_units() names the (few) units of that forward within `margin` of zero and dq_da_choices() the exact values
    dQ/da can take when they fall on either side; a test demands that the kernel's value is one of them, and forms the actor's
    reference gradient (actor_half's `dq_da`) with the value so identified.  For the same reason the third forward's reference
    is evaluated on the critic weights the code under test left, which the gradient and optimizer checks tie to f64: an Adam
    step that differs in the sign of one element whose gradient is ~0 moves Q(s, mu(s)) by 1e-3.

Everything is built on the CPU from seeded CPU generators, so a case tuple names the same state and batch on every machine: the
CPU tests vouch for the very batches the GPU tests run."""
import functools
import itertools

import numpy as np
import torch
import torch.nn.functional as F

MARGIN = 3e-5          # ten times tests/test_gpu_fused_learn.py's _RELU_BOUNDARY
MAX_PASSES = 8
MAX_DISCARD = 0.10
NETS = ("actor", "critic", "target_actor", "target_critic")

DEFAULT_HYPER = dict(actor=dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
                     critic=dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01), tau=1e-3, gamma=0.99)
# the actor's betas differ from the critic's: the actor's optimizer launch finds the critic's betas in the bias-correction buffer
# and must evaluate its own (adam_bias_corrections' fallback)
TRAINED_HYPER = dict(actor=dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=1e-3),
                     critic=dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01), tau=5e-3, gamma=0.95)
HYPERS = dict(default=DEFAULT_HYPER, trained=TRAINED_HYPER)

SEED = 7
# (B, scale, warm_steps, incoming step, hyperparameters, seed) of every state and batch the GPU tests use
FRESH_CASES = [(B, 1.0, 0, 0, "default", SEED) for B in (1, 250, 257, 1000, 1024)]
TRAINED_CASES = [(B, 20.0, 3, 999, "trained", SEED) for B in (257, 1024)]
PATH_CASES = [(B, 20.0, 3, 999, "trained", SEED) for B in (1, 257, 1000, 1024)]
ALL_CASES = sorted(set(FRESH_CASES + TRAINED_CASES + PATH_CASES))


def f32_hyper(hyper):
    """The hyperparameters as the kernels hold them: every one is an f32 argument of the C entry points."""
    r = lambda x: float(np.float32(x))
    out = dict(tau=r(hyper["tau"]), gamma=r(hyper["gamma"]))
    for name in ("actor", "critic"):
        h = hyper[name]
        out[name] = dict(lr=r(h["lr"]), betas=(r(h["betas"][0]), r(h["betas"][1])), eps=r(h["eps"]), weight_decay=r(h["weight_decay"]))
    return out


def net_hyper(hyper, name):
    """adam64's hyperparameters of one net: its optimizer's and tau."""
    return dict(hyper[name], tau=hyper["tau"])


def load_agent(state, hyper, device, dtype):
    """An Agent (replay=False) of `dtype` on `device` that holds `state`: four nets, both optimizers' hyperparameters, Adam
    moments and step count.  The optimizers' step is torch.optim.Adam's own f32 tensor while that holds it exactly (below 2^24:
    every case that existed before steps beyond it were tested keeps its bits); from 2^24 on it is an f64 tensor on the CPU, where
    Adam reads the step as a Python float either way, and stays f32 -- rounded -- on a GPU, whose fused Adam reads f32 steps: the
    f32 twin there only lends its gradients, and a learner takes its exact count from learn_checks.learner."""
    from ddpg_trucktrailer_amd.agent import Agent
    step = int(state["step"])
    step_dtype = torch.float64 if step >= 2 ** 24 and torch.device(device).type == "cpu" else torch.float32
    agent = Agent(alpha=hyper["actor"]["lr"], beta=hyper["critic"]["lr"], input_dims=(23,), tau=hyper["tau"], n_actions=1,
                  gamma=hyper["gamma"], batch_size=1, device=device, replay=False)
    for name in NETS:
        net = getattr(agent, name).to(dtype)
        net.load_state_dict({k: v.to(device=device, dtype=dtype) for k, v in state["nets"][name].items()})
    for name in ("actor", "critic"):
        net = getattr(agent, name)
        group = net.optimizer.param_groups[0]
        h = hyper[name]
        group["lr"], group["betas"], group["eps"], group["weight_decay"] = h["lr"], tuple(h["betas"]), h["eps"], h["weight_decay"]
        for k, p in net.named_parameters():
            net.optimizer.state[p] = {"step": torch.tensor(float(step), dtype=step_dtype, device=p.device),
                                      "exp_avg": state["m"][name][k].to(device=device, dtype=dtype).clone(),
                                      "exp_avg_sq": state["v"][name][k].to(device=device, dtype=dtype).clone()}
    return agent


def forward_z(net, s, a=None):
    """net(s) / net(s, a) of ddpg_trucktrailer_amd.networks, keeping the values in front of its two ReLUs: (out, z1, z2)."""
    z1 = net.bn1(net.fc1(s))
    z2 = net.bn2(net.fc2(F.relu(z1)))
    if a is not None:
        z2 = z2 + net.action_value(a)
        return net.q(F.relu(z2)), z1, z2
    return torch.tanh(net.mu(F.relu(z2))), z1, z2


def _moments(net, key):
    return {k: net.optimizer.state[p][key].detach().clone() for k, p in net.named_parameters()}


def actor_half(critic, actor, s, a=None, dq_da=None, c=0.0, lam=0.0, applied=None):
    """The actor half of learn() in f64 on modules: mu(s); Q(s, mu(s)) and dQ/da at a = mu(s) through `critic` (the updated one);
    the actor's gradients of mean(-Q(s, mu(s))), formed as the gradient of sum_b c_b mu_b with c_b = -(1/B) dQ/da[b] (the chain
    rule through the critic written out: what tt_mlp_backward_weights' row factor is).  dq_da: per-row values to use for c_b in
    place of this function's own.  With a loss shape (c) and a demonstration loss (lam, the stored actions `a` and the APPLIED mask;
    None: no row) the loss is -mean Q(s, mu(s)) + c mean(pre^2) + lam (1/B) sum_b m_b (mu_b - a_b)^2, pre the value in front of tanh.
    Returns dict(mu, pre, q_pi, dq_da, z_actor, z_pi, grads {name: tensor}, q_part = -mean q_pi, pen_part, bc_part -- the three
    parts of the loss --, dq_eff = dQ/da - 2 lam m (mu - a) of the dq_da used)."""
    B = s.shape[0]
    z1 = actor.bn1(actor.fc1(s))
    z2 = actor.bn2(actor.fc2(F.relu(z1)))
    pre = actor.mu(F.relu(z2))
    mu = torch.tanh(pre)
    at_mu = mu.detach().clone().requires_grad_(True)
    q_pi, *z_pi = forward_z(critic, s, at_mu)
    own = torch.autograd.grad(q_pi.sum(), at_mu)[0].view(-1)
    used = own if dq_da is None else dq_da.to(mu).view(-1)
    cb = -used / B
    m = torch.zeros(B, dtype=mu.dtype, device=mu.device) if applied is None else applied.to(mu).view(-1)
    d = mu.view(-1) - (0.0 if a is None else a.to(mu).view(-1))
    bc = lam * (m * d * d).sum() / B
    loss = (cb.view(-1, 1) * mu).sum() + c * (pre * pre).mean() + bc
    g = torch.autograd.grad(loss, list(actor.parameters()))
    names = [k for k, _ in actor.named_parameters()]
    return dict(mu=mu.detach().view(-1), pre=pre.detach().view(-1), q_pi=q_pi.detach().view(-1), dq_da=own,
                z_actor=(z1.detach(), z2.detach()), z_pi=tuple(t.detach() for t in z_pi),
                grads=dict(zip(names, (x.clone() for x in g))), q_part=float(-q_pi.mean().item()),
                pen_part=float(c * (pre * pre).mean().item()), bc_part=float(bc.item()),
                dq_eff=(used - 2.0 * lam * m * d).detach())


def near_units(z2_pi, margin=MARGIN):
    """[(row, [units])] of the third forward's second ReLU within `margin` of zero."""
    near = z2_pi.abs() < margin
    return [(int(b), near[b].nonzero().view(-1).tolist()) for b in near.any(1).nonzero().view(-1)]


def dq_da_choices(critic, z2_pi, dq_da, margin=MARGIN):
    """{row: [every value dQ/da[row] = sum_j w3_j [z2_j > 0] wa_j takes as the row's units within `margin` of zero fall on either
    side]} (the first is dq_da[row] itself), for the rows that have such units."""
    w = (critic.q.weight.view(-1) * critic.action_value.weight.view(-1)).detach().double()
    out = {}
    for b, units in near_units(z2_pi, margin):
        assert len(units) <= 8, (b, units)
        flip = [(-w[j] if z2_pi[b, j] > 0 else w[j]).item() for j in units]
        out[b] = [dq_da[b].item() + sum(c) for k in range(len(units) + 1) for c in itertools.combinations(flip, k)]
    return out


def ref_step(state, batch, hyper, delta=None, c=0.0, lam=0.0, q_filter=True, mask=None):
    """One learn() in f64 (DDPG_agent.py:72-106 as agent.py's learn_batch orders it).  batch = (s, a, r, s2, done), done bool or
    uint8.  The options: the critic loss huber_loss(q, y, delta) (delta None: mse_loss), the actor's pre-activation penalty c
    mean(pre^2), and the demonstration loss lam on the rows `mask` [B] bool names (None: no row), gated by the filter q > q_pi -- q of
    the critic BEFORE its step, q_pi through the UPDATED one -- when q_filter.  Returns a dict: y, q, mu, pre, q_pi (Q(s, mu(s))
    through the updated critic), dq_da (its derivative at a = mu(s)), grads {critic, actor: {name: tensor}} as the optimizers saw
    them, nets / m / v / step after the step, z {critic, actor, critic_pi: (z1, z2)} in front of the ReLUs of the three forwards
    that carry a gradient, margin = per row the smallest |z| of the two forwards that depend on the row alone (critic, actor),
    critic_loss, actor_loss, and of the demonstration loss demo (the mask), applied, dq_eff, bc_loss."""
    s, a, r, s2, done = (t.detach().cpu() for t in batch)
    s, a, r, s2, done = s.double(), a.double().view(-1, 1), r.double().view(-1), s2.double(), done.bool().view(-1)
    mask = torch.zeros(s.shape[0], dtype=torch.bool) if mask is None else mask.cpu().bool().view(-1)
    agent = load_agent(state, hyper, torch.device("cpu"), torch.float64)
    with torch.no_grad():
        q_next = agent.target_critic(s2, agent.target_actor(s2)).view(-1)
        y = r + hyper["gamma"] * q_next.masked_fill(done, 0.0)
    grads, z = {}, {}
    q, *z["critic"] = forward_z(agent.critic, s, a)
    names = [k for k, _ in agent.critic.named_parameters()]
    critic_loss = F.mse_loss(y.view(-1, 1), q) if delta is None else F.huber_loss(q, y.view(-1, 1), delta=delta)
    g = torch.autograd.grad(critic_loss, list(agent.critic.parameters()))
    for p, gp in zip(agent.critic.parameters(), g):
        p.grad = gp
    grads["critic"] = dict(zip(names, (x.clone() for x in g)))
    agent.critic.optimizer.step()
    q = q.detach().view(-1)
    with torch.no_grad():
        q_pi = agent.critic(s, agent.actor(s)).view(-1)              # through the UPDATED critic
    applied = mask & (q > q_pi) if q_filter else mask.clone()
    half = actor_half(agent.critic, agent.actor, s, a, c=c, lam=lam, applied=applied)      # the actor step, through the UPDATED critic
    for k, p in agent.actor.named_parameters():
        p.grad = half["grads"][k]
    grads["actor"] = half["grads"]
    agent.actor.optimizer.step()
    agent.update_network_parameters()
    z = dict(critic=tuple(t.detach() for t in z["critic"]), actor=half["z_actor"], critic_pi=half["z_pi"])
    margin = torch.stack([t.abs().min(1).values for k in ("critic", "actor") for t in z[k]]).min(0).values
    return dict(y=y, q=q, q_pi=half["q_pi"], dq_da=half["dq_da"], mu=half["mu"], pre=half["pre"], grads=grads,
                nets={n: {k: v.detach().clone() for k, v in getattr(agent, n).state_dict().items()} for n in NETS},
                m={n: _moments(getattr(agent, n), "exp_avg") for n in ("actor", "critic")},
                v={n: _moments(getattr(agent, n), "exp_avg_sq") for n in ("actor", "critic")},
                step=int(state["step"]) + 1, z=z, margin=margin, critic_loss=float(critic_loss.item()),
                actor_loss=half["q_part"] + half["pen_part"] + half["bc_part"], demo=mask, applied=applied, dq_eff=half["dq_eff"],
                bc_loss=half["bc_part"])


def soft64(tgt, p, tau):
    return tgt + tau * (p - tgt)


def adam64(p, m, v, tgt, g, t, hyper):
    """adam_finish (csrc/ttlearn_bodies.h) in f64, elementwise: torch.optim.Adam's step t (weight decay as L2 in the gradient, bias
    corrections 1 - beta^t) and the soft update of the target towards the NEW parameter.  hyper: net_hyper().  Returns
    (p, m, v, tgt, g') after the step, g' the gradient with the L2 term."""
    b1, b2 = hyper["betas"]
    g = g + hyper["weight_decay"] * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    denom = v.sqrt() / bc2 ** 0.5 + hyper["eps"]
    p = p - (hyper["lr"] / bc1) * (m / denom)
    return p, m, v, soft64(tgt, p, hyper["tau"]), g


def _candidates(B, g):
    """Rows with the distributions of tests/test_gpu_fused_learn.py's _setup: s, s' U(-1, 1), a U(-1.2, 1.2), r N(0, 1), done
    with probability 0.3."""
    s = torch.rand((B, 23), generator=g) * 2 - 1
    a = torch.rand((B, 1), generator=g) * 2.4 - 1.2
    r = torch.randn(B, generator=g)
    s2 = torch.rand((B, 23), generator=g) * 2 - 1
    done = (torch.rand(B, generator=g) < 0.3).to(torch.uint8)
    return [s, a, r, s2, done]


def make_state(seed, scale, warm_steps, device="cpu"):
    """A learn() state as f32 tensors: {"nets": {actor, critic, target_actor, target_critic: state_dict}, "m" / "v": {actor,
    critic: {parameter name: tensor}}, "step": 0 (the caller sets the incoming step count it wants)}.  The nets are
    tests/test_gpu_fused_net.py's _nets(seed) with fc1 and fc2 weights times `scale`, the targets those nets perturbed by about
    1 %; warm_steps > 0: that many f64 learn() steps on throw-away batches of 64 rows, which leave Adam moments that are not zero
    and that belong to these weights."""
    from test_gpu_fused_net import _nets
    cpu = torch.device("cpu")
    actor, critic = _nets(cpu, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    nets = {}
    for name, net in (("actor", actor), ("critic", critic)):
        with torch.no_grad():
            net.fc1.weight.mul_(scale)
            net.fc2.weight.mul_(scale)
        nets[name] = {k: v.detach().clone() for k, v in net.state_dict().items()}
        nets["target_" + name] = {k: v * (1 + 0.01 * torch.randn(v.shape, generator=g)) + 1e-3 * torch.randn(v.shape, generator=g)
                                  for k, v in nets[name].items()}
    zeros = lambda: {name: {k: torch.zeros_like(p) for k, p in net.named_parameters()} for name, net in (("actor", actor), ("critic", critic))}
    state = dict(nets=nets, m=zeros(), v=zeros(), step=0)
    for _ in range(int(warm_steps)):
        out = ref_step(state, _candidates(64, g), DEFAULT_HYPER)
        state = dict(nets=out["nets"], m=out["m"], v=out["v"], step=out["step"])
    dev = torch.device(device)
    move = lambda tree: {k: (move(v) if isinstance(v, dict) else v.float().to(dev)) for k, v in tree.items()}
    return dict(move(dict(nets=state["nets"], m=state["m"], v=state["v"])), step=0)


def make_batch(state, hyper, B, seed, margin=MARGIN):
    """A batch of B rows none of whose ReLU units, in f64, lies within `margin` of zero in critic(s, a) or actor(s) of this very
    learn() step (for the third forward see the module's docstring): candidates are drawn, the step is run (ref_step), every row
    with such a unit is replaced by a fresh candidate, and that is repeated for at most MAX_PASSES passes.  Returns (batch of f32 /
    uint8 CPU tensors, ref_step's result on it, share of all candidates drawn that were discarded); asserts that the share is at
    most MAX_DISCARD and that a clean batch was reached."""
    g = torch.Generator().manual_seed(seed)
    batch = _candidates(B, g)
    drawn, discarded = B, 0
    for _ in range(MAX_PASSES):
        ref = ref_step(state, batch, hyper)
        bad = (ref["margin"] < margin).nonzero().view(-1)
        if bad.numel() == 0:
            break
        fresh = _candidates(bad.numel(), g)
        for t, f in zip(batch, fresh):
            t[bad] = f
        drawn += bad.numel()
        discarded += bad.numel()
    else:
        raise AssertionError(f"B = {B}: rows within {margin} of a ReLU boundary are left after {MAX_PASSES} passes")
    share = discarded / drawn
    assert share <= MAX_DISCARD, f"B = {B}: {discarded} of {drawn} candidate rows discarded"
    return batch, ref, share


@functools.lru_cache(maxsize=None)
def case(B, scale, warm_steps, step, hyper_name, seed):
    """(state, hyperparameters, batch, ref_step's result, share discarded) of one tuple of ALL_CASES; made once per process and
    shared: do not write to it."""
    state = make_state(seed, scale, warm_steps)
    state["step"] = step
    hyper = HYPERS[hyper_name]
    batch, ref, share = make_batch(state, hyper, B, seed + B)
    return state, hyper, batch, ref, share
