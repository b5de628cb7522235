"""GPU (-m gpu): population-based training's exploit/explore launch (csrc/ttpop.hip: k_pop_exploit; population.py: exploit / hyper)
and the controller driving a live population (pbt.py).

The copy must be complete (dst then IS src: four networks, Adam moments, fc2 images) and isolated (nothing else of any agent moves);
the new hyperparameters must take effect in the descriptors bit for bit (a lone FusedLearner built with them and loaded with src's
state learns the same bits); captured graphs must keep working across an exploit."""
import ctypes as C

import pytest
from test_gpu_population import HYP, _agent, _equal, _lone_learn, _loop_state, _ring, _state

pytestmark = pytest.mark.gpu

B = 256
NEW = dict(alpha=2.5e-4, beta=7e-4, tau=4e-3, gamma=0.985)       # differs from every HYP[a] in each key


def _pop(dev, K, images):
    from ddpg_trucktrailer_amd.population import PopulationLearner
    hyp = HYP[:K]
    return PopulationLearner([_agent(dev, h) for h in hyp], B, fc2_images=images, rings=[_ring(dev, 100 + a) for a in range(K)],
                             seeds=[h["seed"] for h in hyp])


def _learning_state(fl):
    """What an exploit copies: the four networks' parameters, both networks' m and v, the four fc2 images (when on)."""
    ag = fl.agent
    nets = (ag.actor, ag.critic, ag.target_actor, ag.target_critic)
    out = [p.detach().clone() for n in nets for p in n.parameters()]
    out += [t.clone() for t in (fl.actor.m, fl.actor.v, fl.critic.m, fl.critic.v)]
    if fl.use_images:
        out += [fl._img[id(n)].clone() for n in nets]
    return out


def _own_state(fl, ring):
    """What an exploit must not touch: the step count, bias corrections, tail words, the ring."""
    return [t.clone() for t in (fl.step_dev, fl.bias_corr, fl.tail_words, ring.obs, ring.act, ring.rew, ring.done, ring.k_dev)]


def _f32(x):
    import numpy as np
    return float(np.float32(x))


@pytest.mark.parametrize("images", [True, False])
def test_exploit_copy_is_complete_and_isolated(gpu_device, images):
    import torch
    dev, K = gpu_device, 4
    pop = _pop(dev, K, images)
    for u in range(3):
        pop.learn(u)
    torch.cuda.synchronize()
    before = [_learning_state(fl) for fl in pop.learners]
    own = [_own_state(fl, r) for fl, r in zip(pop.learners, pop.rings)]
    assert not _equal(before[0], before[3]) and not _equal(before[0], before[2])
    h1 = dict(alpha=3e-4, beta=2e-3, tau=2e-3, gamma=0.97)
    pop.exploit([(3, 0, NEW), (2, 0, dict(NEW, alpha=1e-5)), (1, 1, h1)])
    torch.cuda.synchronize()
    after = [_learning_state(fl) for fl in pop.learners]
    assert _equal(after[0], before[0]), "src changed"
    assert _equal(after[1], before[1]), "a hyperparameters-only pair moved tensors"
    assert _equal(after[2], before[0]) and _equal(after[3], before[0]), "dst is not src bit for bit"
    for a in range(K):
        assert _equal(_own_state(pop.learners[a], pop.rings[a]), own[a]), f"agent {a}: step / tail words / ring moved"
        assert int(pop.learners[a].step_dev.item()) == 3
    want = {0: {k: HYP[0][k] for k in NEW}, 1: h1, 2: dict(NEW, alpha=1e-5), 3: NEW}
    for a, w in want.items():
        got = pop.hyper(a)
        assert got == {k: _f32(v) for k, v in w.items()}, (a, got, w)
        ag, fl = pop.agents[a], pop.learners[a]
        assert (ag.alpha, ag.beta, ag.tau, ag.gamma) == (w["alpha"], w["beta"], w["tau"], w["gamma"])
        assert ag.actor.optimizer.param_groups[0]["lr"] == w["alpha"] and ag.critic.optimizer.param_groups[0]["lr"] == w["beta"]
        assert fl.hyp_actor[0] == w["alpha"] and fl.hyp_critic[0] == w["beta"]
        assert fl.hyp_actor[1:] == pop.learners[0].hyp_actor[1:]
    assert pop.tail_gave_up() == [0] * K


@pytest.mark.parametrize("images", [True, False])
def test_exploited_agent_learns_with_its_new_hyperparameters(gpu_device, images):
    """After 3 <- 0 with new alpha, beta, tau and gamma, three more population updates leave agent 3 bit-identical to a lone
    FusedLearner (tail in one launch) built with the new hyperparameters, loaded with agent 0's networks and Adam state at the
    exploit point, learning from agent 3's ring with agent 3's keys; with agent 0's hyperparameters the lone run differs."""
    import torch
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    dev, K = gpu_device, 4
    pop = _pop(dev, K, images)
    for u in range(3):
        pop.learn(u)
    torch.cuda.synchronize()
    src = pop.agents[0]
    nets = {n: {k: v.clone() for k, v in getattr(src, n).state_dict().items()}
            for n in ("actor", "critic", "target_actor", "target_critic")}
    adam = pop.state_dict(0)
    assert adam["step"] == 3
    pop.exploit([(3, 0, NEW)])
    for u in range(3, 6):
        pop.learn(u)
    torch.cuda.synchronize()
    assert pop.tail_gave_up() == [0] * K
    got = _state(pop.learners[3])

    def lone(hyp):
        ag = _agent(dev, dict(HYP[3], **hyp))
        for n, sd in nets.items():
            getattr(ag, n).load_state_dict(sd)
        fl = FusedLearner(ag, B, fc2_images=images)
        fl.fuse_tail = True
        fl.load_state_dict(adam)
        ring = _ring(dev, 103)
        for u in range(3, 6):
            _lone_learn(fl, ring, HYP[3]["seed"], u, B)
        torch.cuda.synchronize()
        assert fl.tail_gave_up() == 0
        return _state(fl)
    want = lone(NEW)
    assert int(want[-4].item()) == 6
    assert _equal(got, want), "agent 3 after the exploit is not the lone learner with the new hyperparameters"
    control = lone({k: HYP[0][k] for k in NEW})
    assert not _equal(got, control), "agent 0's hyperparameters give the same bits: the new ones did not take effect"
    for k in NEW:                      # each hyperparameter on its own matters
        assert not _equal(got, lone(dict(NEW, **{k: HYP[0][k]}))), k


def test_exploit_between_graph_replays_equals_eager_steps(gpu_device):
    """PopulationRollout: run(12) in graphs, exploit, run(12) == the same sequence through eager step(); no re-capture."""
    import torch
    from ddpg_trucktrailer_amd.population import PopulationRollout
    K, hyp = 3, HYP[:3]
    pairs = [(2, 0, NEW), (1, 1, dict(alpha=3e-4, beta=2e-3, tau=2e-3, gamma=0.97))]
    kw = dict(alphas=[h["alpha"] for h in hyp], betas=[h["beta"] for h in hyp], taus=[h["tau"] for h in hyp],
              gammas=[h["gamma"] for h in hyp], batch_size=B, replay_slots=16, updates_per_step=2)
    states = {}
    for mode in ("graph", "eager"):
        pop = PopulationRollout(2048, [h["seed"] for h in hyp], graph_steps=4 if mode == "graph" else 0, **kw)
        if mode == "graph":
            pop.run(12)
            g1, gG = pop.graph1, pop.graphG
            assert g1 is not None and gG is not None
            pop.exploit(pairs)
            pop.run(12)
            assert pop.graph1 is g1 and pop.graphG is gG, "an exploit made run() capture again"
        else:
            for _ in range(12):
                pop.step()
            pop.exploit(pairs)
            for _ in range(12):
                pop.step()
        torch.cuda.synchronize()
        assert pop.learner.tail_gave_up() == [0] * K
        states[mode] = [_loop_state(pop.loops[a], pop.learner.learners[a]) for a in range(K)]
        states[mode + "_hyper"] = [pop.hyper(a) for a in range(K)]
    for a in range(K):
        assert torch.isfinite(states["graph"][a][0]).all()
        assert _equal(states["graph"][a], states["eager"][a]), f"agent {a}"
    assert states["graph_hyper"] == states["eager_hyper"]
    assert states["graph_hyper"][2] == {k: _f32(v) for k, v in NEW.items()}


def test_exploit_arguments_are_checked_on_a_live_handle(gpu_device):
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    dev, K = gpu_device, 4
    pop = _pop(dev, K, True)
    with pytest.raises(RuntimeError):
        pop.exploit([(1, 0, NEW)])                 # no learn() yet: no descriptors
    pop.learn(0)
    torch.cuda.synchronize()
    before = [_learning_state(fl) + _own_state(fl, r) for fl, r in zip(pop.learners, pop.rings)]
    hyp = [pop.hyper(a) for a in range(K)]
    dll = pop.lib
    ok = dict(alpha=1e-4, beta=1e-3, tau=1e-3, gamma=0.99)

    def P(dst, src, **kw):
        h = dict(ok, **kw)
        return L.TTPopExploitPair(dst, src, h["alpha"], h["beta"], h["tau"], h["gamma"])
    inf, nan = float("inf"), float("nan")
    bad = [[P(1, 0), P(2, 0), P(3, 0), P(0, 0), P(0, 1)],                 # pairs = K + 1
           [P(4, 0)], [P(1, -1)], [P(-1, 0)], [P(1, 0), P(1, 2)],          # out of range, duplicate dst
           [P(1, 0), P(2, 1)], [P(1, 1), P(2, 1)],                         # a dst that is another pair's src
           [P(1, 0, alpha=nan)], [P(1, 0, gamma=inf)], [P(1, 0, tau=-inf)],
           [P(1, 0, alpha=0.0)], [P(1, 0, alpha=1.5)], [P(1, 0, beta=0.0)], [P(1, 0, beta=2.0)], [P(1, 0, tau=0.0)],
           [P(1, 0, tau=1.01)], [P(1, 0, gamma=1.0)], [P(1, 0, gamma=0.0)]]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for lst in bad:
        arr = (L.TTPopExploitPair * len(lst))(*lst)
        assert dll.tt_pop_exploit(pop._h, len(lst), arr, stream) == L.TT_EINVAL, [(p.dst, p.src) for p in lst]
        assert dll.tt_last_error(None)
    one = (L.TTPopExploitPair * 1)(P(1, 0))
    assert dll.tt_pop_exploit(pop._h, 0, one, stream) == L.TT_EINVAL
    assert dll.tt_pop_exploit(pop._h, 1, None, stream) == L.TT_EINVAL
    assert dll.tt_pop_hyper(pop._h, K, C.byref((C.c_float * 4)())) == L.TT_EINVAL
    torch.cuda.synchronize()
    after = [_learning_state(fl) + _own_state(fl, r) for fl, r in zip(pop.learners, pop.rings)]
    assert all(_equal(x, y) for x, y in zip(after, before))
    assert [pop.hyper(a) for a in range(K)] == hyp


def test_pbt_drives_a_population(gpu_device):
    """K = 4 x 4096 envs, a short window: PBT rounds every 20 vector steps for 300 steps.  At least one decision; right after it
    dst holds src's networks and moments; every weight finite at the end; no hand-over gave up."""
    import torch
    from ddpg_trucktrailer_amd.pbt import PBT
    from ddpg_trucktrailer_amd.population import PopulationRollout
    K, hyp = 4, HYP[:4]
    pop = PopulationRollout(4096, [h["seed"] for h in hyp], alphas=[h["alpha"] for h in hyp], betas=[h["beta"] for h in hyp],
                            taus=[h["tau"] for h in hyp], gammas=[h["gamma"] for h in hyp], batch_size=B, replay_slots=16,
                            updates_per_step=2, graph_steps=4, episode_log=1 << 18)
    pbt = PBT(K, 20, seed=1, window=20, quantile=0.25)
    checked = 0
    for _ in range(15):
        pop.run(20)
        out = pbt.step(pop, pop.drain_episodes())
        if out and not checked:
            torch.cuda.synchronize()
            for d in out:
                s, t = pop.learner.learners[d["src"]], pop.learner.learners[d["dst"]]
                assert _equal(_learning_state(t), _learning_state(s)), d
                assert pop.hyper(d["dst"]) == {k: _f32(v) for k, v in d["new"].items()}
            checked = len(out)
    torch.cuda.synchronize()
    assert checked >= 1 and len(pbt.history) >= 1
    assert pop.learner.tail_gave_up() == [0] * K
    for ag in pop.agents:
        assert all(torch.isfinite(p).all() for n in ag._nets() for p in n.parameters())
    assert pop.vector_steps == 300
