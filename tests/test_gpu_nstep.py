"""GPU: n-step returns in the replay draw (csrc/ttnstep.hip): the lone draw against tt_ring_sample (n = 1, bit for bit) and
against an f64 restatement of the walk, learn()'s own draw against the lone one, the TD target the learner really forms, and the
vector loop with n_step = 5 (graphs == eager, resume) and n_step = 1 (== the loop without the option)."""
import os

import numpy as np
import pytest

import nstep_ref as ref

pytestmark = pytest.mark.gpu


def _flat(loop):
    import torch
    return torch.cat([p.detach().reshape(-1) for net in loop.agent._nets() for p in net.parameters()])


@pytest.mark.parametrize("window", [dict(), dict(reserve=2, lag=1)])
def test_lone_draw_with_one_step_is_tt_ring_sample(gpu_device, window):
    import torch
    ring = ref.synthetic_ring(gpu_device)
    one = [t.clone() for t in ring.sample_fused(ref.BATCH, seed=77, done_as_bool=False, return_index=True, **window)]
    for t in ring._batch_bufs(ref.BATCH):
        t.zero_()
    import ctypes as C
    from ddpg_trucktrailer_amd import _lib as L
    args = ring.sample_args(ref.BATCH, seed=77, **window)
    L.check(L.load().tt_ring_sample_nstep(C.byref(args), 1, 0.99, C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)))
    torch.cuda.synchronize()
    for x, y in zip(one, ring._batch_bufs(ref.BATCH)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("window", [dict(), dict(reserve=2, lag=1)])
@pytest.mark.parametrize("n_step", [3, 5, 8])
def test_lone_draw_against_the_walk_in_f64(gpu_device, n_step, window):
    """tt_ring_sample_nstep: exact fields exact, R within the derived bound (nstep_ref.walk64), both branches of the walk
    populated, and the base step uniform over the avail_n positions that have their n steps: each position's share within 0.03
    of 1 / avail_n at B = 4096."""
    import torch
    ring = ref.synthetic_ring(gpu_device)
    gamma = 0.99
    out = ring.sample_fused(ref.BATCH, seed=1234 + n_step, done_as_bool=False, return_index=True, n_step=n_step, gamma=gamma, **window)
    torch.cuda.synchronize()
    k = ref.K - window.get("lag", 0)
    avail = min(k, ref.SLOTS - 1 - window.get("reserve", 0))
    _, back = ref.check_rows(ring, out, n_step, gamma, k=k, avail=avail)
    avail_n = avail - (n_step - 1)
    share = np.bincount(back - (n_step - 1), minlength=avail_n) / len(back)
    print("shares of the base positions:", np.round(share, 4))
    assert len(share) == avail_n and np.abs(share - 1.0 / avail_n).max() <= 0.03, share
    env_share = np.bincount(out[5][:, 1].cpu().numpy() // 64, minlength=8) / len(back)       # eight blocks of 64 envs
    assert np.abs(env_share - 0.125).max() <= 0.03, env_share


def test_learn_with_the_n_step_draw_made_by_its_first_launch(gpu_device):
    """tt_mlp_forward_multi_sampled_nstep == tt_ring_sample_nstep followed by the same learn(), bit for bit: batch buffers, the
    four networks, Adam's moments; three steps, the last with the pipelined loop's window."""
    import torch
    from conftest import GOLDEN
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    from test_gpu_fused_learn import _agent
    z = np.load(os.path.join(GOLDEN, "f5_learner.npz"), allow_pickle=False)
    dev, B, n_step = gpu_device, 256, 5
    ring = ref.synthetic_ring(dev)
    agents = [_agent(dev, z), _agent(dev, z)]
    learners = [FusedLearner(a, B) for a in agents]
    gamma = float(agents[0].gamma)
    for step in range(3):
        kw = dict(seed=1234 + step) if step < 2 else dict(seed=99, reserve=2, lag=1)
        s, a, r, s2, d = ring.sample_fused(B, done_as_bool=False, n_step=n_step, gamma=gamma, **kw)
        drawn = [t.clone() for t in (s, a, r, s2, d)]
        assert 0.1 < d.float().mean().item() < 0.9
        learners[0].learn_batch(s, a, r, s2, d, n_step=n_step)
        for t in ring._batch_bufs(B)[:5]:
            t.zero_()                                    # the sampled launch must fill them itself
        args = ring.sample_args(B, **kw)
        s, a, r, s2, d = ring._batch_bufs(B)[:5]
        learners[1].learn_batch(s, a, r, s2, d, sample=args, n_step=n_step)
        torch.cuda.synchronize()
        for x, y in zip(drawn, (s, a, r, s2, d)):
            assert torch.equal(x, y), step
        for name in ("actor", "critic", "target_actor", "target_critic"):
            for x, y in zip(getattr(agents[0], name).state_dict().values(), getattr(agents[1], name).state_dict().values()):
                assert torch.equal(x, y), (step, name)
        for st0, st1 in ((learners[0].critic, learners[1].critic), (learners[0].actor, learners[1].actor)):
            assert torch.equal(st0.m, st1.m) and torch.equal(st0.v, st1.v)
        assert torch.equal(learners[0].y, learners[1].y)


def test_the_target_is_the_n_step_target(gpu_device):
    """After a learn() whose first launch drew with n = 5 the learner's y is R + gamma^n q'(s2) (1 - D), q' from the torch target
    networks on the drawn s2, to the tolerance test_fused_learn_matches_reference_fixture_and_torch_path has for fl.y (1e-5 of
    max |y|) -- and NOT the one-step target of the same base steps: with rewards U(-5, 5) the two differ by the order of |r|,
    more than 100 times that tolerance on at least half of the full rows."""
    import torch
    from conftest import GOLDEN
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    from test_gpu_fused_learn import _agent
    z = np.load(os.path.join(GOLDEN, "f5_learner.npz"), allow_pickle=False)
    dev, B, n_step = gpu_device, 256, 5
    ring = ref.synthetic_ring(dev)
    agent = _agent(dev, z)
    fl = FusedLearner(agent, B)
    gamma = float(agent.gamma)
    # the rows this learn() will draw, and q' on them from the torch target networks as they are BEFORE it moves them
    lone = ring.sample_fused(B, seed=31, done_as_bool=False, return_index=True, n_step=n_step, gamma=gamma)
    idx = lone[5].clone()
    t0, e = idx[:, 0].long(), idx[:, 1].long()
    with torch.no_grad():
        def q_target(obs):
            return agent.target_critic.forward(obs, agent.target_actor.forward(obs)).view(-1).double().cpu().numpy()
        q_n = q_target(lone[3].clone())
        q_1 = q_target(ring.obs[(t0 + 1) % ring.slots, e])
    for t in ring._batch_bufs(B):
        t.zero_()
    args = ring.sample_args(B, seed=31)
    s, a, r, s2, d, idx2 = ring._batch_bufs(B)
    fl.learn_batch(s, a, r, s2, d, sample=args, n_step=n_step)
    torch.cuda.synchronize()
    assert torch.equal(idx, idx2)
    y = fl.y.clone().double().cpu().numpy().reshape(-1)
    want = ref.walk64(ring, idx, n_step, gamma)
    assert np.array_equal(s2.cpu().numpy(), want["s2"]) and np.array_equal(d.cpu().numpy().astype(bool), want["D"])
    g32 = float(np.float32(gamma))
    y_n = want["R"] + np.where(want["D"], 0.0, float(np.float32(gamma ** n_step)) * q_n)
    tol = 1e-5 * np.abs(y_n).max()
    print(f"max |y - y_n| = {np.abs(y - y_n).max():.3e}, tolerance {tol:.3e}")
    assert np.abs(y - y_n).max() <= tol
    r1 = ring.rew[t0, e].double().cpu().numpy()
    d1 = ring.done[t0, e].cpu().numpy() != 0
    y_1 = r1 + np.where(d1, 0.0, g32 * q_1)
    full = ~want["D"]
    assert full.sum() >= B // 4
    far = np.abs(y - y_1)[full] > 100 * tol
    print(f"full rows {full.sum()}, of which {far.sum()} differ from the one-step target by more than {100 * tol:.3e}")
    assert far.mean() >= 0.5


@pytest.mark.parametrize("pipeline", [False, True])
def test_vector_loop_with_n_step_graphs_equal_eager(gpu_device, pipeline):
    """DDPGRollout(n_step=5) at N = 512 with a 16-slot ring, strict and pipelined order: whole-step graphs == eager steps over
    the flat weights, bit for bit; finite; learn() ran from the step its window allows; no launch gave up a hand-over."""
    import torch
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    flats = []
    for graph_steps in (4, 0):
        env = TruckTrailerVecEnv(512)
        env.reset(seed=6)
        loop = DDPGRollout(env, batch_size=128, replay_slots=16, seed=6, graph_steps=graph_steps, pipeline=pipeline, n_step=5)
        assert loop.pipeline == pipeline and loop.graph_steps == graph_steps
        loop.run(8)
        loop.run(13)
        torch.cuda.synchronize()
        assert loop.handover_gave_up == [] and loop.ring.policy_gave_up() == 0
        # learn() starts at the step its window allows: vector steps 0 .. 4 of the strict order and 0 .. 5 of the pipelined one make none
        assert int(loop.learner.step_dev.item()) == 21 - (6 if pipeline else 5)
        assert int(loop.ring.k_dev.item()) == 21
        flats.append(_flat(loop).clone())
        env.close()
    assert torch.equal(flats[0], flats[1]) and torch.isfinite(flats[0]).all()


def test_vector_loop_with_n_step_resumes_bitwise(gpu_device, tmp_path):
    import torch
    from ddpg_trucktrailer_amd import checkpoint
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv

    def make(seed, n_step=5):
        env = TruckTrailerVecEnv(512)
        env.reset(seed=seed)
        return DDPGRollout(env, batch_size=128, replay_slots=16, seed=seed, graph_steps=4, n_step=n_step)
    a = make(21)
    a.run(10)
    path = checkpoint.save_loop_checkpoint(str(tmp_path / "loop.pt"), a, training_state={"episode_num": 7})
    a.run(9)
    b = make(99)
    b.run(8)                           # its graphs are already captured when the file is loaded
    ts = checkpoint.load_loop_checkpoint(path, b)
    assert ts == {"episode_num": 7} and b.ring.k == 10 and b.n_step == 5
    b.run(9)
    torch.cuda.synchronize()
    assert torch.equal(_flat(a), _flat(b))
    for name in ("obs", "act", "rew", "done"):
        assert torch.equal(getattr(a.ring, name), getattr(b.ring, name)), name
    for st_a, st_b in ((a.learner.actor, b.learner.actor), (a.learner.critic, b.learner.critic)):
        assert torch.equal(st_a.m, st_b.m) and torch.equal(st_a.v, st_b.v)
    assert int(a.learner.step_dev.item()) == int(b.learner.step_dev.item())
    c = make(3, n_step=1)
    with pytest.raises(ValueError, match="n_step"):
        checkpoint.load_loop_checkpoint(path, c)
    for lp in (a, b, c):
        lp.env.close()


@pytest.mark.parametrize("pipeline", [False, True])
def test_n_step_one_is_the_loop_without_the_option(gpu_device, pipeline):
    import torch
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    flats = []
    for kw in (dict(), dict(n_step=1)):
        env = TruckTrailerVecEnv(512)
        env.reset(seed=8)
        loop = DDPGRollout(env, batch_size=128, replay_slots=16, seed=8, graph_steps=4, pipeline=pipeline, **kw)
        loop.run(12)
        torch.cuda.synchronize()
        flats.append(_flat(loop).clone())
        env.close()
    assert torch.equal(flats[0], flats[1]) and torch.isfinite(flats[0]).all()
