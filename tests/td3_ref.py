"""What tests/test_td3_cpu.py (CPU) and tests/test_gpu_td3.py (GPU) share: one TD3 update restated in f64 on the project's own modules
(td3_step, built on learn_ref's load_agent recipe, forward_z, actor_half, adam64 and soft64), the target-smoothing noise of
csrc/tttd3.hip reproduced on the host (Philox4x32-10 and Box-Muller in numpy: noise_normal, noise_eps), and a builder of TD3 states
and of batches whose ReLU units stay clear of zero in all THREE forwards that carry a gradient and depend on a row alone:
critic(s, a), critic_2(s, a) and actor(s) (make_td3_state, make_td3_batch; learn_ref's docstring has the reasons, and its caps
MAX_PASSES and MAX_DISCARD hold here unchanged).

The smoothing noise eps is an INPUT of td3_step: a test feeds it the kernel's own eps (checked separately against noise_eps), so
that no bound has to absorb a unit of the target critics changing side under a different eps."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import learn_ref as R

NETS = R.NETS + ("critic_2", "target_critic_2")
TRAINED = ("actor", "critic", "critic_2")
NOISE_TAG = 0x7D3E             # csrc/tttd3.hip: TD3_NOISE_TAG
SEED = 11
# (B, scale, warm_steps, incoming critic step, incoming actor step, hyperparameters, seed) of every state and batch the tests use
F64_CASES = [(B, 1.0, 0, 0, 0, "default", SEED) for B in (1, 250, 257)]
DELAY_CASE = (257, 1.0, 0, 0, 0, "default", SEED)
ALL_CASES = sorted(set(F64_CASES + [DELAY_CASE]))


# ---- the noise ------------------------------------------------------------------------------------------------------
def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (csrc/ttphilox.h) on uint32 arrays / scalars; returns the four output words as uint64 arrays holding 32 bits."""
    M0, M1, W0, W1, mask = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) & mask for x in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & mask, int(k1) & mask
    for _ in range(10):
        p0, p1 = c0 * np.uint64(M0), c2 * np.uint64(M1)
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(mask), p1 >> np.uint64(32), p1 & np.uint64(mask)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & mask, (k1 + W1) & mask
    return c0, c1, c2, c3


def noise_normal(seed, t, rows):
    """N_b of csrc/tttd3.hip for rows b = 0 .. rows - 1 at critic step count t: the two uniforms exactly as the kernel forms them in
    f32 ((r >> 8) + 0.5) 2^-24, the angle 2 pi u2 as the f32 product, then log, sqrt and cos in f64."""
    seed, t = int(seed) & (2 ** 64 - 1), int(t)
    r0, r1, _, _ = philox4x32(np.arange(rows), t & 0xFFFFFFFF, t >> 32, NOISE_TAG, seed & 0xFFFFFFFF, seed >> 32)
    f32 = np.float32
    u1 = (r0 >> np.uint64(8)).astype(f32) + f32(0.5)
    u2 = (r1 >> np.uint64(8)).astype(f32) + f32(0.5)
    u1, u2 = u1 * f32(1.0 / 16777216.0), u2 * f32(1.0 / 16777216.0)
    angle = (f32(6.28318530717958647692) * u2).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(angle)


def noise_eps(seed, t, rows, sigma, clip):
    """(eps, N): eps_b = clip(sigma N_b, -clip, clip) in f64, sigma and clip rounded to f32 as the C struct holds them."""
    n = noise_normal(seed, t, rows)
    sigma, clip = float(np.float32(sigma)), float(np.float32(clip))
    return np.clip(sigma * n, -clip, clip), n


# ---- states and agents ----------------------------------------------------------------------------------------------
def load_td3_agent(state, hyper, cfg, device, dtype):
    """learn_ref.load_agent for an Agent(td3=cfg): six nets, three optimizers' hyperparameters (critic_2 has the critic's), Adam
    moments, and the step counts -- state["step"] for both critics, state["actor_step"] for the actor."""
    from ddpg_trucktrailer_amd.agent import Agent
    agent = Agent(alpha=hyper["actor"]["lr"], beta=hyper["critic"]["lr"], input_dims=(23,), tau=hyper["tau"], n_actions=1,
                  gamma=hyper["gamma"], batch_size=1, device=device, replay=False, td3=cfg)
    for name in NETS:
        net = getattr(agent, name).to(dtype)
        net.load_state_dict({k: v.to(device=device, dtype=dtype) for k, v in state["nets"][name].items()})
    for name in TRAINED:
        net = getattr(agent, name)
        group = net.optimizer.param_groups[0]
        h = hyper["actor" if name == "actor" else "critic"]
        group["lr"], group["betas"], group["eps"], group["weight_decay"] = h["lr"], tuple(h["betas"]), h["eps"], h["weight_decay"]
        step = state["actor_step"] if name == "actor" else state["step"]
        for k, p in net.named_parameters():
            exact = torch.float64 if step >= 2 ** 24 and p.device.type == "cpu" else torch.float32      # (learn_ref.load_agent's rule)
            net.optimizer.state[p] = {"step": torch.tensor(float(step), dtype=exact, device=p.device),
                                      "exp_avg": state["m"][name][k].to(device=device, dtype=dtype).clone(),
                                      "exp_avg_sq": state["v"][name][k].to(device=device, dtype=dtype).clone()}
    return agent


def make_td3_state(seed, scale, warm_steps, twin_copy=False):
    """learn_ref.make_state plus a second critic: another seed's critic at the same scale with a target perturbed the same way and
    zero moments (twin_copy: critic_2 and its target, moments included, are copies of critic 1's)."""
    from test_gpu_fused_net import _nets
    state = R.make_state(seed, scale, warm_steps)
    state["actor_step"] = 0
    if twin_copy:
        for key in ("critic", "target_critic"):
            state["nets"][key + "_2"] = {k: v.clone() for k, v in state["nets"][key].items()}
        for key in ("m", "v"):
            state[key]["critic_2"] = {k: v.clone() for k, v in state[key]["critic"].items()}
        return state
    _, critic = _nets(torch.device("cpu"), seed + 1)
    g = torch.Generator().manual_seed(seed + 2000)
    with torch.no_grad():
        critic.fc1.weight.mul_(scale)
        critic.fc2.weight.mul_(scale)
    net = {k: v.detach().clone().float() for k, v in critic.state_dict().items()}
    state["nets"]["critic_2"] = net
    state["nets"]["target_critic_2"] = {k: (v * (1 + 0.01 * torch.randn(v.shape, generator=g)) + 1e-3 * torch.randn(v.shape, generator=g)).float()
                                        for k, v in net.items()}
    for key in ("m", "v"):
        state[key]["critic_2"] = {k: torch.zeros_like(p) for k, p in critic.named_parameters()}
    return state


def row_margin(state, hyper, cfg, batch):
    """Per row the smallest |pre-ReLU value|, in f64, over critic(s, a), critic_2(s, a) and actor(s) of the incoming state."""
    s, a = batch[0].double(), batch[1].double().view(-1, 1)
    agent = load_td3_agent(state, hyper, cfg, torch.device("cpu"), torch.float64)
    with torch.no_grad():
        zs = list(R.forward_z(agent.critic, s, a)[1:]) + list(R.forward_z(agent.critic_2, s, a)[1:]) + list(R.forward_z(agent.actor, s)[1:])
    return torch.stack([z.abs().min(1).values for z in zs]).min(0).values


def make_td3_batch(state, hyper, cfg, B, seed, margin=R.MARGIN):
    """learn_ref.make_batch with the three-net filter, under learn_ref's own caps.  Returns (batch, share of candidates discarded)."""
    g = torch.Generator().manual_seed(seed)
    batch = R._candidates(B, g)
    drawn, discarded = B, 0
    for _ in range(R.MAX_PASSES):
        bad = (row_margin(state, hyper, cfg, batch) < margin).nonzero().view(-1)
        if bad.numel() == 0:
            break
        for t, fresh in zip(batch, R._candidates(bad.numel(), g)):
            t[bad] = fresh
        drawn += bad.numel()
        discarded += bad.numel()
    else:
        raise AssertionError(f"B = {B}: rows within {margin} of a ReLU boundary are left after {R.MAX_PASSES} passes")
    share = discarded / drawn
    assert share <= R.MAX_DISCARD, f"B = {B}: {discarded} of {drawn} candidate rows discarded"
    return batch, share


def default_cfg():
    from ddpg_trucktrailer_amd.td3 import TD3Config
    return TD3Config(policy_delay=2, target_noise=0.2, noise_clip=0.5)


@functools.lru_cache(maxsize=None)
def case(B, scale, warm_steps, step, actor_step, hyper_name, seed):
    """(state, hyperparameters, batch, share discarded) of one tuple of ALL_CASES; made once per process: do not write to it."""
    state = make_td3_state(seed, scale, warm_steps)
    state["step"], state["actor_step"] = step, actor_step
    hyper = R.HYPERS[hyper_name]
    batch, share = make_td3_batch(state, hyper, default_cfg(), B, seed + B)
    return state, hyper, batch, share


# ---- the update -----------------------------------------------------------------------------------------------------
def _moments(net, key):
    return {k: net.optimizer.state[p][key].detach().clone() for k, p in net.named_parameters()}


def td3_step(state, batch, hyper, cfg, eps, full):
    """One TD3 update in f64.  eps [B]: the smoothing noise (normalised action units).  Returns a dict: eps, a2 (the smoothed target
    action), q1t, q2t, y, q, q2, grads {critic, critic_2[, actor]}, z {critic, critic_2[, actor, critic_pi]}, and after a full update
    mu, q_pi, dq_da; nets / m / v after the update, step and actor_step after it."""
    s, a, r, s2, done = (t.detach().cpu() for t in batch)
    s, a, r, s2, done = s.double(), a.double().view(-1, 1), r.double().view(-1), s2.double(), done.bool().view(-1)
    eps = torch.as_tensor(np.asarray(eps, dtype=np.float64)).view(-1, 1)
    agent = load_td3_agent(state, hyper, cfg, torch.device("cpu"), torch.float64)
    with torch.no_grad():
        a2 = (agent.target_actor(s2) + eps).clamp(-1.0, 1.0)
        q1t, q2t = agent.target_critic(s2, a2).view(-1), agent.target_critic_2(s2, a2).view(-1)
        y = r + hyper["gamma"] * torch.min(q1t, q2t).masked_fill(done, 0.0)
    out = dict(eps=eps.view(-1), a2=a2.view(-1), q1t=q1t, q2t=q2t, y=y, grads={}, z={})
    for name, key in (("critic", "q"), ("critic_2", "q2")):
        net = getattr(agent, name)
        q, *z = R.forward_z(net, s, a)
        g = torch.autograd.grad(F.mse_loss(y.view(-1, 1), q), list(net.parameters()))
        for p, gp in zip(net.parameters(), g):
            p.grad = gp
        out["grads"][name] = dict(zip([k for k, _ in net.named_parameters()], (x.clone() for x in g)))
        out["z"][name] = tuple(t.detach() for t in z)
        out[key] = q.detach().view(-1)
        net.optimizer.step()
    if full:
        half = R.actor_half(agent.critic, agent.actor, s)          # through the UPDATED critic 1
        for k, p in agent.actor.named_parameters():
            p.grad = half["grads"][k]
        agent.actor.optimizer.step()
        agent.update_network_parameters()
        out["grads"]["actor"] = half["grads"]
        out["z"].update(actor=half["z_actor"], critic_pi=half["z_pi"])
        out.update(mu=half["mu"], q_pi=half["q_pi"], dq_da=half["dq_da"])
    out.update(nets={n: {k: v.detach().clone() for k, v in getattr(agent, n).state_dict().items()} for n in NETS},
               m={n: _moments(getattr(agent, n), "exp_avg") for n in TRAINED},
               v={n: _moments(getattr(agent, n), "exp_avg_sq") for n in TRAINED},
               step=int(state["step"]) + 1, actor_step=int(state["actor_step"]) + (1 if full else 0))
    return out


def next_state(state, out):
    """The state after td3_step's update `out`, as td3_step / load_td3_agent take it."""
    return dict(nets=out["nets"], m=out["m"], v=out["v"], step=out["step"], actor_step=out["actor_step"])
