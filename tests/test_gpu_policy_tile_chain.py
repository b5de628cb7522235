"""GPU (-m gpu): the split-f16 policy kernel (csrc/ttnet_split.hip) where a workgroup takes SEVERAL tiles in turn.  The kernel
requests the next tile's packed fc1 and first fc2 steps under the running tile's last layer-2 steps, into ring slots the
running tile has just left, and a workgroup's last tile drains what it requested before it ends: the places to go wrong are the
hand-over from tile to tile and the exit, so the grids here are small and the chains of tiles long (8..38 tiles on 1..3
workgroups), not the row counts large.

Yardstick: the torch modules evaluated in f64; bound = the one tests/test_gpu_fused_net.py::test_split_f16_kernel_is_f32_accurate
uses (3 x the larger of the exact-f32 kernel's and torch-f32's own error, + 1e-7 on the actor's tanh output, + 1e-6 on Q).  A
fragment from a wrong step or slot is an error of order 1."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = (1024, 1024 + 55, 128 * 37 + 55)          # 8 tiles (where the split kernel takes over), 9 and 38 with a ragged last one
_cache = {}


def _nets(dev, seed):
    import torch
    from ddpg_trucktrailer_amd.networks import ActorNetwork, CriticNetwork
    torch.manual_seed(seed)
    a = ActorNetwork(1e-4, (23,), 400, 300, 1, name="actor", device=dev)
    c = CriticNetwork(1e-3, (23,), 400, 300, 1, name="critic", device=dev)
    with torch.no_grad():    # non-trivial LayerNorm affines + bigger heads so that mistakes show
        for net in (a, c):
            net.bn1.weight.uniform_(0.5, 1.5); net.bn1.bias.uniform_(-0.3, 0.3)
            net.bn2.weight.uniform_(0.5, 1.5); net.bn2.bias.uniform_(-0.3, 0.3)
        a.mu.weight.uniform_(-0.2, 0.2); c.q.weight.uniform_(-0.2, 0.2)
    return a, c


def _case(dev, n):
    """Nets, inputs and the references of one row count: computed once, shared by the tests, never changed."""
    if n in _cache:
        return _cache[n]
    import torch
    from ddpg_trucktrailer_amd import fused
    actor, critic = _nets(dev, seed=100 + n)
    g = torch.Generator(device=dev).manual_seed(n)
    obs = torch.rand((n, 23), device=dev, generator=g) * 2 - 1
    act = torch.rand((n, 1), device=dev, generator=g) * 2.4 - 1.2
    with torch.no_grad():
        mu64 = actor.double()(obs.double()).float().view(-1)
        q64 = critic.double()(obs.double(), act.double()).float().view(-1)
        actor.float(); critic.float()
        mu_t, q_t = actor(obs).view(-1), critic(obs, act).view(-1)
    with fused.exact_f32(actor), fused.exact_f32(critic):
        mu_e = fused.actor_forward(actor, obs).clone().view(-1)
        q_e = fused.critic_forward(critic, obs, act).clone().view(-1)
    err = lambda x, ref: (x - ref).abs().max().item()
    fused.pack(actor, 1)
    fused.pack(critic, 1)
    _cache[n] = dict(actor=actor, critic=critic, obs=obs, act=act, mu64=mu64, q64=q64,
                     bound_mu=3 * max(err(mu_e, mu64), err(mu_t, mu64)) + 1e-7,
                     bound_q=3 * max(err(q_e, q64), err(q_t, q64)) + 1e-6)
    return _cache[n]


def _geometries(n):
    tiles = (n + 127) // 128
    # a workgroup takes all the tiles, half, an uneven share, exactly one, or what the chip-wide grid gives it;
    # the last: one capped round of 3 tiles, the rest in a second launch over the whole chip
    return [(1, 0), (2, 0), (3, 0), (tiles, 0), (0, 0), (3, 1)]


def _forward(c, critic, wg, capped):
    """One launch of the packed image (tt_actor_forward / tt_critic_forward) into a fresh NaN-filled output."""
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    from ddpg_trucktrailer_amd import fused
    net, obs = (c["critic"] if critic else c["actor"]), c["obs"]
    n = obs.shape[0]
    w = fused.packed_weights_of(net, 1, wg, capped)
    out = torch.full((n,), float("nan"), device=obs.device)
    stream = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
    if critic:
        L.check(L.load().tt_critic_forward(n, C.c_void_p(obs.data_ptr()), C.c_void_p(c["act"].data_ptr()), C.byref(w),
                                           C.c_void_p(out.data_ptr()), stream))
    else:
        L.check(L.load().tt_actor_forward(n, C.c_void_p(obs.data_ptr()), C.byref(w), C.c_void_p(out.data_ptr()), stream))
    return out


@pytest.mark.parametrize("n", NS)
def test_every_geometry_is_f32_accurate_and_geometries_agree(gpu_device, n):
    import torch
    c = _case(gpu_device, n)
    for critic, ref, bound in ((False, c["mu64"], c["bound_mu"]), (True, c["q64"], c["bound_q"])):
        outs = []
        for wg, capped in _geometries(n):
            out = _forward(c, critic, wg, capped)
            e = (out - ref).abs().max().item()
            print(f"n={n} {'critic' if critic else 'actor'} max_workgroups={wg} capped_grids={capped}: error {e:.3e}, bound {bound:.3e}")
            assert torch.isfinite(out).all(), (n, critic, wg, capped)
            assert e <= bound, (n, critic, wg, capped, e, bound)
            outs.append(out)
        for o, geo in zip(outs[1:], _geometries(n)[1:]):      # the same rows computed by the same code: bit-identical
            assert torch.equal(o, outs[0]), (n, critic, geo)


@pytest.mark.parametrize("n", NS)
def test_long_tile_chains_repeat_bit_for_bit(gpu_device, n):
    """A slot overwritten too early, or a piece that lands after a workgroup's exit in the next workgroup's LDS, tends to show as
    run-to-run differences: 30 launches each with all / half of the tiles on one workgroup."""
    import torch
    c = _case(gpu_device, n)
    for critic in (False, True):
        for wg in (1, 2):
            first = _forward(c, critic, wg, 0)
            assert torch.isfinite(first).all()
            for rep in range(29):
                assert torch.equal(_forward(c, critic, wg, 0), first), (n, critic, wg, rep)


def test_choose_action_on_a_capped_grid(gpu_device):
    """fused.actor_act with noise, 9 tiles on 2 workgroups: a = mu + noise and mu is the module's, over 3 steps."""
    import torch
    from ddpg_trucktrailer_amd import fused
    n = 1024 + 55
    c = _case(gpu_device, n)
    actor, obs = c["actor"], c["obs"]
    w = fused.packed_weights_of(actor, 1, 2, 0)
    ou = torch.zeros(n, device=gpu_device)
    raw, scaled, mu = (torch.full((n,), float("nan"), device=gpu_device) for _ in range(3))
    high = float(np.float32(math.pi / 4))
    with torch.no_grad():
        ref = actor(obs).view(-1)
    for step in range(3):
        before = ou.clone()
        fused.actor_act(actor, obs, ou, raw, scaled, seed=27, step=step, mu_out=mu, high=high, weights=w)
        assert (mu - ref).abs().max().item() <= 2e-5
        assert torch.allclose(raw, mu + ou, atol=1e-7)
        assert torch.equal(scaled, torch.clamp(raw, -1, 1) * high)
        assert not torch.equal(ou, before)                   # the noise advanced for every row
        assert (ou != before).all()
    fused.packed_weights_of(actor, 1, 0, 0)
