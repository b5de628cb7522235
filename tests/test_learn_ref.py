"""The f64 restatement of learn() that tests/test_gpu_learn_shapes.py measures the HIP kernels against (tests/learn_ref.py), checked
on the CPU: against fixture F5 (the reference's own learn()), against torch.optim.Adam, and that every batch the GPU tests use can
be built with all its row-local ReLU units clear of zero."""
import os
import types

import numpy as np
import pytest
import torch

import learn_ref as R
from conftest import GOLDEN


@pytest.mark.parametrize("case", R.ALL_CASES, ids=lambda c: "B{}-x{:g}-warm{}-seed{}".format(c[0], c[1], c[2], c[5]))
def test_every_gpu_case_builds_with_its_units_clear_of_zero(case):
    """make_batch ends within its passes (it raises otherwise), discards at most 10 % of its candidates, and leaves no unit of
    critic(s, a) or actor(s) within 3e-5 of zero; the units of the third forward that are within it are few enough to enumerate."""
    B = case[0]
    state, hyper, batch, ref, share = R.case(*case)
    assert all(t.shape[0] == B for t in batch) and state["step"] == case[3]
    assert share <= 0.10
    assert ref["margin"].shape == (B,) and ref["margin"].min().item() >= 3e-5 == R.MARGIN
    for k in ("critic", "actor"):
        assert min(t.abs().min().item() for t in ref["z"][k]) >= 3e-5
    near = R.near_units(ref["z"]["critic_pi"][1])
    print(f"B {B}: discarded {share:.4f}, margin {ref['margin'].min().item():.2e}, third forward: {len(near)} rows near a boundary")
    assert len(near) <= 0.05 * B + 1 and all(len(units) <= 3 for _, units in near)
    if case[2]:                                              # warmed: the moments are there, and they are f32 numbers
        assert all(v.abs().max() > 0 and v.dtype == torch.float32 for v in state["v"]["critic"].values())
        assert not torch.equal(state["nets"]["critic"]["fc2.weight"], state["nets"]["target_critic"]["fc2.weight"])


def test_ref_step_matches_the_reference_fixture():
    """ref_step at B = 256 on F5's batch and initial weights against what the reference's own learn() left (after1, grad1/*,
    target_y), with tests/test_learner.py's bounds; its forward_z is the modules' forward."""
    from test_learner import _batch, _check_grads, _check_snapshot
    z = np.load(os.path.join(GOLDEN, "f5_learner.npz"), allow_pickle=False)
    nets = {}
    for name in ("actor", "critic"):
        keys = [k[len(f"init/{name}/"):] for k in z.files if k.startswith(f"init/{name}/")]
        nets[name] = {k: torch.tensor(z[f"init/{name}/{k}"]) for k in keys}
        nets["target_" + name] = {k: v.clone() for k, v in nets[name].items()}
    zeros = {name: {k: torch.zeros_like(v) for k, v in nets[name].items()} for name in ("actor", "critic")}
    state = dict(nets=nets, m=zeros, v=zeros, step=0)
    batch = _batch(z, torch.device("cpu"))
    ref = R.ref_step(state, batch, R.DEFAULT_HYPER)
    assert ref["step"] == 1
    assert np.abs(ref["y"].numpy() - z["target_y"]).max() <= 1e-5 * np.abs(z["target_y"]).max()
    for name in ("critic", "actor"):
        _check_grads(z, 1, name, list(ref["grads"][name].items()))
    after = types.SimpleNamespace(**{n: types.SimpleNamespace(state_dict=lambda n=n: ref["nets"][n]) for n in R.NETS})
    _check_snapshot(after, z, "after1", 1e-5)
    agent = R.load_agent(state, R.DEFAULT_HYPER, torch.device("cpu"), torch.float64)
    s, a = batch[0].double(), batch[1].double()
    with torch.no_grad():
        assert torch.equal(R.forward_z(agent.critic, s, a)[0], agent.critic(s, a))
        assert torch.equal(R.forward_z(agent.actor, s)[0], agent.actor(s))
    # the actor's gradient as actor_half forms it (sum_b c_b mu_b) is autograd's of mean(-Q(s, mu(s)))
    loss = torch.mean(-agent.critic(s, agent.actor(s)))
    half = R.actor_half(agent.critic, agent.actor, s)
    for (k, g64), g in zip(half["grads"].items(), torch.autograd.grad(loss, list(agent.actor.parameters()))):
        assert (g64 - g).abs().max().item() <= 1e-13 * g.abs().max().item(), k


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("t", [1, 1000])
def test_adam64_is_torch_adam_and_the_soft_update(t, weight_decay):
    """adam64 == torch.optim.Adam's step t followed by the soft update, on f64 tensors, to 1e-14 relative (m: relative to the two
    terms it is the sum of)."""
    g = torch.Generator().manual_seed(t)
    n = 4096
    p0, tgt0, grad = (torch.randn(n, generator=g, dtype=torch.float64) for _ in range(3))
    m0 = torch.randn(n, generator=g, dtype=torch.float64) * (t > 1)
    v0 = torch.rand(n, generator=g, dtype=torch.float64) * (t > 1)
    hyper = dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=weight_decay, tau=5e-3)
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=hyper["lr"], betas=hyper["betas"], eps=hyper["eps"], weight_decay=weight_decay)
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    p.grad = grad.clone()
    opt.step()
    tgt = tgt0.clone().lerp_(p.detach(), hyper["tau"])                   # Agent.update_network_parameters
    p64, m64, v64, tgt64, g2 = R.adam64(p0, m0, v0, tgt0, grad, t, hyper)
    st = opt.state[p]
    assert float(st["step"]) == t
    b1 = hyper["betas"][0]
    assert ((st["exp_avg"] - m64).abs() <= 1e-14 * ((b1 * m0).abs() + ((1 - b1) * g2).abs())).all()
    assert ((st["exp_avg_sq"] - v64).abs() <= 1e-14 * v64).all()
    assert ((p.detach() - p64).abs() <= 1e-14 * p64.abs()).all()
    assert ((tgt - tgt64).abs() <= 1e-14 * tgt64.abs()).all()
    assert (p64 - p0).abs().min().item() > 0 and torch.equal(g2, grad + weight_decay * p0)


def test_dq_da_choices_are_the_values_on_either_side():
    """dq_da_choices: with a unit of the third forward moved across zero (through its action_value bias), autograd's dQ/da is the
    value listed for that unit's flip."""
    state, hyper, batch, ref, _ = R.case(*R.ALL_CASES[-1])
    nets = dict(ref["nets"], actor=state["nets"]["actor"])               # the updated critic, the actor as mu(s) was formed
    agent = R.load_agent(dict(state, nets=nets), hyper, torch.device("cpu"), torch.float64)
    s = batch[0].double()
    z2 = ref["z"]["critic_pi"][1]
    row = 5
    units = z2[row].abs().argsort()[:2].tolist()
    wide = z2[row, units[1]].abs().item() * (1 + 1e-9)
    choices = R.dq_da_choices(agent.critic, z2[row:row + 1], ref["dq_da"][row:row + 1], margin=wide)[0]
    assert len(choices) == 4 and choices[0] == ref["dq_da"][row].item()
    with torch.no_grad():
        for j in units:
            agent.critic.action_value.bias[j] -= 2 * z2[row, j]
    flipped = R.actor_half(agent.critic, agent.actor, s)["dq_da"][row].item()
    assert min(abs(c - flipped) for c in choices[1:]) <= 1e-12 and abs(choices[0] - flipped) > 1e-6
