"""GPU (-m gpu): a population of K independent agents (ddpg_trucktrailer_amd/population.py, csrc/ttpop.hip) against K lone agents.

Every agent has its own seed, alpha, beta, tau and gamma.  The population's learn() must give each agent the bits of a lone
FusedLearner with the tail in one launch; the population loop must give each agent the bits of a lone serial-order DDPGRollout."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STRIDE = 0x9E3779B97F4A7C15
HYP = [dict(seed=11 + 7 * a, alpha=1e-4 * (1 + 0.25 * a), beta=1e-3 * (1 + 0.5 * a), tau=1e-3 * (1 + a), gamma=0.99 - 0.01 * a)
       for a in range(8)]


def _agent(dev, h):
    import torch
    from ddpg_trucktrailer_amd.agent import Agent
    torch.manual_seed(h["seed"])
    return Agent(alpha=h["alpha"], beta=h["beta"], input_dims=(23,), tau=h["tau"], n_actions=1, gamma=h["gamma"], batch_size=256,
                 device=dev, replay=False)


def _ring(dev, seed, n=512, slots=16, k=37):
    import torch
    from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    ring = TrajectoryRing(n, slots, 23, dev)
    ring.obs.copy_(torch.rand(ring.obs.shape, device=dev, generator=g) * 2 - 1)
    ring.act.copy_(torch.rand(ring.act.shape, device=dev, generator=g) * 2 - 1)
    ring.rew.copy_(torch.rand(ring.rew.shape, device=dev, generator=g) * 10 - 5)
    ring.done.copy_((torch.rand(ring.done.shape, device=dev, generator=g) < 0.05).to(torch.uint8))
    ring.k = k
    ring.k_dev.fill_(k)
    return ring


def _lone_learn(fl, ring, seed, u, B):
    args = ring.sample_args(B, seed=(seed + u * STRIDE) & (2 ** 64 - 1))
    s, a, r, s2, d = ring._batch_bufs(B)[:5]
    fl.learn_batch(s, a, r, s2, d, sample=args)


def _state(fl):
    ag = fl.agent
    out = [p.detach().clone() for n in (ag.actor, ag.critic, ag.target_actor, ag.target_critic) for p in n.parameters()]
    return out + [t.clone() for t in (fl.actor.m, fl.actor.v, fl.critic.m, fl.critic.v, fl.step_dev, fl.q, fl.y, fl.mu)]


def _equal(x, y):
    import torch
    return len(x) == len(y) and all(torch.equal(a, b) for a, b in zip(x, y))


@pytest.mark.parametrize("images", [True, False])
@pytest.mark.parametrize("B", [256, 64])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_population_learn_is_bitwise_the_lone_learners(gpu_device, K, B, images):
    """K rings filled, 5 population updates (u = 0..4) == K lone FusedLearners (tail in one launch) on the same rings with the
    same sampling keys: the four networks, Adam moments, step_dev, q, y and mu, bit for bit."""
    import torch
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    from ddpg_trucktrailer_amd.population import PopulationLearner
    dev = gpu_device
    hyp = HYP[:K]
    pop = PopulationLearner([_agent(dev, h) for h in hyp], B, fc2_images=images, rings=[_ring(dev, 100 + a) for a in range(K)],
                            seeds=[h["seed"] for h in hyp])
    for u in range(5):
        pop.learn(u)
    lone = []
    for a, h in enumerate(hyp):
        fl = FusedLearner(_agent(dev, h), B, fc2_images=images)
        fl.fuse_tail = True
        ring = _ring(dev, 100 + a)
        for u in range(5):
            _lone_learn(fl, ring, h["seed"], u, B)
        lone.append(fl)
    torch.cuda.synchronize()
    assert pop.tail_gave_up() == [0] * K
    for a in range(K):
        got, want = _state(pop.learners[a]), _state(lone[a])
        assert int(want[-4].item()) == 5
        assert _equal(got, want), f"agent {a}"
        assert pop.state_dict(a)["step"] == 5 and torch.equal(pop.state_dict(a)["critic"]["m"], lone[a].critic.m.cpu())


def test_population_agents_are_isolated(gpu_device):
    """One agent's critic moved by one ulp and its actor's learning rate zeroed: every other agent's results stay bit-identical,
    that agent's differ."""
    import torch
    from ddpg_trucktrailer_amd.population import PopulationLearner
    dev, K, B = gpu_device, 3, 256
    runs = []
    for perturb in (False, True):
        agents = [_agent(dev, h) for h in HYP[:K]]
        if perturb:
            with torch.no_grad():
                w = agents[1].critic.fc1.weight
                w[0, 0] = torch.nextafter(w[0, 0], torch.tensor(float("inf"), device=dev))
            agents[1].actor.optimizer.param_groups[0]["lr"] = 0.0
        pop = PopulationLearner(agents, B, rings=[_ring(dev, 100 + a) for a in range(K)], seeds=[h["seed"] for h in HYP[:K]])
        for u in range(5):
            pop.learn(u)
        torch.cuda.synchronize()
        runs.append([_state(fl) for fl in pop.learners])
    assert _equal(runs[0][0], runs[1][0]) and _equal(runs[0][2], runs[1][2])
    assert not _equal(runs[0][1], runs[1][1])
    actor_params = 10           # the actor's parameters come first in _state: with lr = 0 its weights did not move
    before = [p.detach() for p in _agent(dev, HYP[1]).actor.parameters()]
    assert _equal(runs[1][1][:actor_params], before)


def test_population_agent_matches_the_reference_fixture(gpu_device):
    """A population agent with fixture F5's networks and batch (the ring laid out so that its draw IS that batch, in order) beside
    another agent: its gradients and losses at learn() steps 1..3 against the reference's own learn(), at the tolerances of
    tests/test_gpu_fused_learn.py::test_fused_gradients_and_losses_match_the_reference."""
    import torch
    from conftest import GOLDEN
    from ddpg_trucktrailer_amd.fused_learn import _ORDER
    from ddpg_trucktrailer_amd.population import PopulationLearner
    from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing
    from test_gpu_fused_learn import _RELU_BOUNDARY, _agent as f5_agent, _ln_params, _relu_margin
    from test_learner import _batch, _check_grads, _check_snapshot
    z = np.load(os.path.join(GOLDEN, "f5_learner.npz"), allow_pickle=False)
    dev, B, seed = gpu_device, 256, 4242
    s, a, r, s2, d = _batch(z, dev)
    # one stored step (k = 1): every draw takes slot 0 of a random env; with 2^20 envs the 256 rows pick distinct envs
    ring = TrajectoryRing(1 << 20, 3, 23, dev)
    ring.k = 1
    ring.k_dev.fill_(1)
    idx = ring.sample_fused(B, seed=seed, return_index=True)[-1]
    env = idx[:, 1].long()
    assert idx[:, 0].eq(0).all() and env.unique().numel() == B
    ring.obs[0, env] = s
    ring.obs[1, env] = s2
    ring.act[0, env] = a.view(-1)
    ring.rew[0, env] = r
    ring.done[0, env] = d.to(torch.uint8)
    agent = f5_agent(dev, z)
    pop = PopulationLearner([_agent(dev, HYP[1]), agent], B, rings=[_ring(dev, 7), ring], seeds=[HYP[1]["seed"], seed])
    fl = pop.learners[1]

    def named(st):
        head = "q" if st.critic else "mu"
        names = list(_ORDER) + [head + ".weight", head + ".bias"] + (["action_value.weight", "action_value.bias"] if st.critic else [])
        return [(n, g.clone()) for n, g in zip(names, st.grads)]
    for i in (1, 2, 3):
        params = _ln_params(fl)
        pop.learn(0)                 # (update 0 every time: the same key, the same draw -- F5's batch, as the reference's 3 steps)
        torch.cuda.synchronize()
        assert torch.equal(ring._batch_bufs(B)[0], s) and torch.equal(ring._batch_bufs(B)[2], r)
        rtol = 3e-5 if _relu_margin(fl, a, params) >= _RELU_BOUNDARY else 1e-4
        _check_grads(z, i, "critic", named(fl.critic), rtol)
        _check_grads(z, i, "actor", named(fl.actor), rtol)
        loss_c = torch.mean((fl.q - fl.y) ** 2).item()
        assert abs(loss_c - float(z[f"loss{i}/critic"])) <= 1e-5 * float(z[f"loss{i}/critic"])
        loss_a = -fl.q_pi.mean().item()
        assert abs(loss_a - float(z[f"loss{i}/actor"])) <= 2e-5 * max(0.1, abs(float(z[f"loss{i}/actor"])))
    _check_snapshot(agent, z, "after3", 4e-5)


K_LOOP, N_LOOP, UPS, STEPS = 3, 2048, 2, 40


@pytest.fixture(scope="module")
def loop_runs(gpu_device):
    """The population loop (graphs, and eager steps) and three lone loops, 40 vector steps each, episode logs on."""
    import torch
    from ddpg_trucktrailer_amd.population import PopulationRollout
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    hyp = HYP[:K_LOOP]
    kw = dict(batch_size=256, replay_slots=16, updates_per_step=UPS, episode_log=1 << 16)
    pops = {}
    for mode in ("graph", "eager"):
        pop = PopulationRollout(N_LOOP, [h["seed"] for h in hyp], alphas=[h["alpha"] for h in hyp], betas=[h["beta"] for h in hyp],
                                taus=[h["tau"] for h in hyp], gammas=[h["gamma"] for h in hyp], graph_steps=4 if mode == "graph" else 0,
                                **kw)
        if mode == "graph":
            pop.run(STEPS)
            assert pop.graph1 is not None
        else:
            for _ in range(STEPS):
                pop.step()
        torch.cuda.synchronize()
        pops[mode] = pop
    old = os.environ.get("TT_ACTOR_TAIL")
    os.environ["TT_ACTOR_TAIL"] = "1"
    try:
        lone = []
        for h in hyp:
            env = TruckTrailerVecEnv(N_LOOP, device=gpu_device)
            env.reset(seed=h["seed"])
            lp = DDPGRollout(env, seed=h["seed"], alpha=h["alpha"], beta=h["beta"], tau=h["tau"], gamma=h["gamma"], pipeline=False, **kw)
            assert lp.learner.fuse_tail and not lp.pipeline
            lp.run(STEPS)
            lone.append(lp)
    finally:
        if old is None:
            os.environ.pop("TT_ACTOR_TAIL")
        else:
            os.environ["TT_ACTOR_TAIL"] = old
    torch.cuda.synchronize()
    return pops, lone


def _loop_state(lp, fl):
    ag = lp.agent
    out = [p.detach().clone() for n in (ag.actor, ag.critic, ag.target_actor, ag.target_critic) for p in n.parameters()]
    out += [lp.ring.obs.clone(), lp.ring.act.clone(), lp.ring.rew.clone(), lp.ring.done.clone(), lp.ring.k_dev.clone(),
            lp.noise.x.clone(), lp.env.state.clone(), fl.actor.m.clone(), fl.critic.v.clone(), fl.step_dev.clone()]
    return out


def test_population_loop_equals_lone_loops(loop_runs):
    """Every agent's weights, ring contents, OU state, env state and Adam state after run(40) in graphs == its lone
    DDPGRollout(pipeline=False) with the tail in one launch; the population's graph replays == its eager step() loop."""
    import torch
    pops, lone = loop_runs
    for a in range(K_LOOP):
        g = _loop_state(pops["graph"].loops[a], pops["graph"].learner.learners[a])
        e = _loop_state(pops["eager"].loops[a], pops["eager"].learner.learners[a])
        w = _loop_state(lone[a], lone[a].learner)
        assert int(w[-1].item()) == (STEPS - 1) * UPS
        assert torch.isfinite(g[0]).all()
        assert _equal(g, w), f"agent {a}: population graphs against the lone loop"
        assert _equal(g, e), f"agent {a}: population graphs against its eager steps"
    assert pops["graph"].vector_steps == STEPS and pops["graph"].k == STEPS


def test_population_episode_logs_are_per_agent(loop_runs):
    import torch
    pops, lone = loop_runs
    logs = pops["graph"].drain_episodes()
    assert len(logs) == K_LOOP
    for a in range(K_LOOP):
        want = lone[a].drain_episodes()
        got = logs[a]
        assert len(want["ret"]) > 0 and set(got) == set(want)
        for key in want:
            x, y = got[key], want[key]
            assert (torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y), (a, key)


def test_population_runs_at_size(gpu_device):
    """K = 8 x n = 8192 envs at 8 updates per step, 200 graph-replayed steps: weights finite, no give-up, agents pairwise apart."""
    import torch
    from ddpg_trucktrailer_amd.population import PopulationRollout
    hyp = HYP[:8]
    pop = PopulationRollout(8192, [h["seed"] for h in hyp], alphas=[h["alpha"] for h in hyp], betas=[h["beta"] for h in hyp],
                            taus=[h["tau"] for h in hyp], gammas=[h["gamma"] for h in hyp], batch_size=256, replay_slots=64,
                            updates_per_step=8, graph_steps=20)
    pop.run(204)
    torch.cuda.synchronize()
    assert pop.learner.tail_gave_up() == [0] * 8
    flat = [torch.cat([p.detach().reshape(-1) for n in ag._nets() for p in n.parameters()]) for ag in pop.agents]
    assert all(torch.isfinite(f).all() for f in flat)
    for i in range(8):
        assert int(pop.learner.learners[i].step_dev.item()) == 203 * 8
        for j in range(i):
            assert not torch.equal(flat[i], flat[j]), (i, j)
