"""GPU (-m gpu): per-agent n-step returns in a population (csrc/ttpop_nstep.hip: k_pop_fwd_multi_nstep; population.py: n_steps /
n_step; pbt.py: n_step_choices) against lone learners and lone loops with the same n.

Each agent draws with its own n and gamma inside the shared first launch; its results must be the bits of a lone FusedLearner /
DDPGRollout with that n.  The C-side refusals that need a live handle are here too (tests/test_population_nstep_cpu.py has those
reachable without one)."""
import ctypes as C
import os

import numpy as np
import pytest
from test_gpu_pbt import NEW, _learning_state, _own_state
from test_gpu_population import HYP, STRIDE, _agent, _equal, _loop_state, _ring, _state

pytestmark = pytest.mark.gpu

SLOTS = 24                  # k = 37 wraps it


def _f32(x):
    return float(np.float32(x))


def _pop(dev, n_steps, B, images=None, K=None, slots=SLOTS):
    from ddpg_trucktrailer_amd.population import PopulationLearner
    K = len(n_steps) if K is None else K
    hyp = HYP[:K]
    return PopulationLearner([_agent(dev, h) for h in hyp], B, fc2_images=images, rings=[_ring(dev, 100 + a, slots=slots) for a in range(K)],
                             seeds=[h["seed"] for h in hyp], n_steps=n_steps)


def _lone(dev, a, B, images, n_step, updates, fl=None, hyp=None):
    """A lone FusedLearner (tail in one launch) of agent a's making on agent a's ring with agent a's keys, drawing with n_step."""
    import torch
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    if fl is None:
        fl = FusedLearner(_agent(dev, hyp or HYP[a]), B, fc2_images=images)
    fl.fuse_tail = True
    ring = _ring(dev, 100 + a, slots=SLOTS)
    for u in updates:
        args = ring.sample_args(B, seed=(HYP[a]["seed"] + u * STRIDE) & (2 ** 64 - 1))
        s, act, r, s2, d = ring._batch_bufs(B)[:5]
        fl.learn_batch(s, act, r, s2, d, sample=args, n_step=n_step)
    torch.cuda.synchronize()
    assert fl.tail_gave_up() == 0
    return fl


@pytest.mark.parametrize("images", [True, False])
@pytest.mark.parametrize("B", [64, 250])
def test_population_learn_with_mixed_n_is_bitwise_the_lone_learners(gpu_device, B, images):
    """K = 3 with n = 1, 5, 16 on wrapped rings with 5 % done flags, five population updates == per agent a lone FusedLearner
    drawing with that n; the batch buffers and index after the last update == the lone n-step draw with the last key; the n = 5
    agent's draw has rows that stop early at a done and rows that run all five steps; a lone learner with n = 4 differs."""
    import torch
    dev, n_steps = gpu_device, [1, 5, 16]
    pop = _pop(dev, n_steps, B, images)
    for u in range(5):
        pop.learn(u)
    torch.cuda.synchronize()
    assert pop.tail_gave_up() == [0] * 3
    for a, n in enumerate(n_steps):
        want = _state(_lone(dev, a, B, images, n, range(5)))
        assert int(want[-4].item()) == 5
        assert _equal(_state(pop.learners[a]), want), f"agent {a}, n = {n}"
        assert pop.n_step_of(a) == (n, _f32(HYP[a]["gamma"]), _f32(float(HYP[a]["gamma"]) ** n if n > 1 else HYP[a]["gamma"]))
        got = [t.clone() for t in pop.rings[a]._batch_bufs(B)]
        ring = _ring(dev, 100 + a, slots=SLOTS)
        drawn = ring.sample_fused(B, seed=(HYP[a]["seed"] + 4 * STRIDE) & (2 ** 64 - 1), n_step=n, gamma=HYP[a]["gamma"],
                                  return_index=True, done_as_bool=False)
        torch.cuda.synchronize()
        assert _equal(got, list(drawn)), f"agent {a}: batch buffers and index"
        if n == 5 and B == 250:
            idx, D = drawn[5].long().cpu(), drawn[4].cpu()
            done = ring.done.cpu()
            steps = torch.full((B,), 5)
            for j in reversed(range(5)):          # the first done of the walk ends it after j + 1 steps
                steps[done[(idx[:, 0] + j) % SLOTS, idx[:, 1]] != 0] = j + 1
            hit = done[(idx[:, 0] + steps - 1) % SLOTS, idx[:, 1]] != 0
            assert torch.equal(D != 0, hit)
            assert int(((D != 0) & (steps < 5)).sum()) >= 10 and int((D == 0).sum()) >= 100, (steps.bincount(), D.sum())
    assert not _equal(_state(pop.learners[1]), _state(_lone(dev, 1, B, images, 4, range(5)))), "n = 4 gives agent 1's bits as well"


def test_all_ones_through_the_table_is_the_one_step_population(gpu_device):
    """n_steps = [1, 1, 1] runs k_pop_fwd_multi_nstep; without the argument the population runs k_pop_fwd_multi: the same bits."""
    import torch
    dev, B = gpu_device, 64
    table, plain = _pop(dev, [1, 1, 1], B), _pop(dev, None, B, K=3)
    assert table.nstep_table and not plain.nstep_table
    for u in range(5):
        table.learn(u)
        plain.learn(u)
    torch.cuda.synchronize()
    for a in range(3):
        assert _equal(_state(table.learners[a]), _state(plain.learners[a])), f"agent {a}"
        assert _equal(list(table.rings[a]._batch_bufs(B)), list(plain.rings[a]._batch_bufs(B)))
        assert table.n_step_of(a) == plain.n_step_of(a) == (1, _f32(HYP[a]["gamma"]), _f32(HYP[a]["gamma"]))
        assert table.hyper(a) == plain.hyper(a)


def test_exploited_agent_learns_with_its_new_n_and_gamma(gpu_device):
    """K = 4, n = 5, 5, 3, 1; after 3 <- 0 with NEW and n_step = 8 three more updates leave agent 3 bit-identical to a lone learner
    built with NEW and n = 8 from agent 0's state at the exploit point, on agent 3's ring with agent 3's keys; with n = 5 or with
    agent 0's gamma the lone run differs; nothing else of any agent moved."""
    import torch
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    dev, K, B, images = gpu_device, 4, 256, True
    pop = _pop(dev, [5, 5, 3, 1], B, images)
    for u in range(3):
        pop.learn(u)
    torch.cuda.synchronize()
    src = pop.agents[0]
    nets = {n: {k: v.clone() for k, v in getattr(src, n).state_dict().items()} for n in ("actor", "critic", "target_actor", "target_critic")}
    adam = pop.state_dict(0)
    before = [_learning_state(fl) for fl in pop.learners]
    own = [_own_state(fl, r) for fl, r in zip(pop.learners, pop.rings)]
    pop.exploit([(3, 0, dict(NEW, n_step=8))])
    torch.cuda.synchronize()
    after = [_learning_state(fl) for fl in pop.learners]
    for a in range(3):
        assert _equal(after[a], before[a]), f"agent {a}'s learning state moved"
    assert _equal(after[3], before[0]), "dst is not src bit for bit"
    for a in range(K):
        assert _equal(_own_state(pop.learners[a], pop.rings[a]), own[a]), f"agent {a}: step / tail words / ring moved"
    g = NEW["gamma"]
    assert pop.n_step_of(3) == (8, _f32(g), _f32(float(g) ** 8))
    assert pop.hyper(3) == {k: _f32(v) for k, v in NEW.items()}
    assert pop.n_steps == [5, 5, 3, 8] and pop.rings[3].n_step == 8 and pop.agents[3].gamma == g
    for a, n in enumerate((5, 5, 3)):
        assert pop.n_step_of(a) == (n, _f32(HYP[a]["gamma"]), _f32(float(HYP[a]["gamma"]) ** n))
        assert pop.hyper(a)["gamma"] == _f32(HYP[a]["gamma"])
    for u in range(3, 6):
        pop.learn(u)
    torch.cuda.synchronize()
    assert pop.tail_gave_up() == [0] * K
    got = _state(pop.learners[3])

    def lone(hyp, n):
        ag = _agent(dev, dict(HYP[3], **hyp))
        for name, sd in nets.items():
            getattr(ag, name).load_state_dict(sd)
        fl = FusedLearner(ag, B, fc2_images=images)
        fl.load_state_dict(adam)
        return _state(_lone(dev, 3, B, images, n, range(3, 6), fl=fl))
    want = lone(NEW, 8)
    assert int(want[-4].item()) == 6
    assert _equal(got, want), "agent 3 after the exploit is not the lone learner with NEW and n = 8"
    assert not _equal(got, lone(NEW, 5)), "src's n gives the same bits: the new n did not take effect"
    assert not _equal(got, lone(dict(NEW, gamma=HYP[0]["gamma"]), 8)), "src's gamma gives the same bits"
    # agents 0 .. 2 went on as if nothing had happened
    for a, n in enumerate((5, 5, 3)):
        assert _equal(_state(pop.learners[a]), _state(_lone(dev, a, B, images, n, range(6)))), f"agent {a}"


def test_refusals_on_a_live_handle(gpu_device):
    """Every refusal of tt_pop_learn_set_nstep / tt_pop_exploit_nstep that needs a handle, plain tt_pop_exploit on a population
    with a table, and tt_pop_exploit_nstep on one without: TT_EINVAL, a message that names the entry point and the agent or pair,
    and nothing moved."""
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    dev, K, B = gpu_device, 3, 64
    pop, plain = _pop(dev, [1, 5, 3], B, slots=8), _pop(dev, None, B, K=3, slots=8)
    pop.learn(0)
    plain.learn(0)
    torch.cuda.synchronize()
    before = [_learning_state(fl) + _own_state(fl, r) for fl, r in zip(pop.learners, pop.rings)]
    table = [pop.n_step_of(a) for a in range(K)]
    lib, stream = pop.lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = 0.99

    def refused(rc, *words):
        msg = lib.tt_last_error(None).decode()
        assert rc == L.TT_EINVAL, (rc, msg)
        assert all(w in msg for w in words), msg
    bad = [((0, g, g), "n_step"), ((17, g, g ** 17), "n_step"), ((-1, g, g), "n_step"),
           ((5, 0.0, 0.5), "gamma"), ((5, 1.0, 0.5), "gamma"), ((5, float("nan"), 0.5), "gamma"), ((1, 1.5, 1.5), "gamma"),
           ((1, g, g ** 2), "discount"), ((5, g, g), "discount"), ((5, g, 0.0), "discount"), ((5, g, 0.995), "discount"),
           ((5, g, float("nan")), "discount"),
           ((7, g, g ** 7), "slots")]                    # 3 + (7 - 1) = 9 slots; the rings have 8 (n = 6 fits)
    ok = L.TTPopNstep(6, g, g ** 6)
    for (n, gamma, disc), word in bad:
        ns = (L.TTPopNstep * K)(ok, L.TTPopNstep(n, gamma, disc), ok)
        refused(lib.tt_pop_learn_set_nstep(pop._h, ns), "tt_pop_learn_set_nstep", "agent 1", word)
        pairs = (L.TTPopExploitPair * 2)(L.TTPopExploitPair(0, 0, 1e-4, 1e-3, 1e-3, g),
                                         L.TTPopExploitPair(2, 1, 1e-4, 1e-3, 1e-3, gamma if 0.0 < gamma < 1.0 else g))
        if not 0.0 < gamma < 1.0:
            word = "gamma"
        ns2 = (L.TTPopNstep * 2)(ok, L.TTPopNstep(n, gamma, disc))
        refused(lib.tt_pop_exploit_nstep(pop._h, 2, pairs, ns2, stream), "tt_pop_exploit_nstep", "pair 1", word)
    one = (L.TTPopExploitPair * 1)(L.TTPopExploitPair(2, 1, 1e-4, 1e-3, 1e-3, g))
    refused(lib.tt_pop_exploit_nstep(pop._h, 1, one, (L.TTPopNstep * 1)(L.TTPopNstep(5, 0.98, 0.98 ** 5)), stream),
            "tt_pop_exploit_nstep", "pair 0", "gamma")                                            # ns.gamma != the pair's
    refused(lib.tt_pop_learn_set_nstep(pop._h, None), "tt_pop_learn_set_nstep", "NULL")
    refused(lib.tt_pop_exploit_nstep(pop._h, 1, None, (L.TTPopNstep * 1)(ok), stream), "tt_pop_exploit_nstep", "list is NULL")
    refused(lib.tt_pop_exploit_nstep(pop._h, 1, one, None, stream), "tt_pop_exploit_nstep", "ns is NULL")
    refused(lib.tt_pop_exploit_nstep(pop._h, 4, one, (L.TTPopNstep * 1)(ok), stream), "tt_pop_exploit_nstep", "pairs = 4")
    bad_pair = (L.TTPopExploitPair * 1)(L.TTPopExploitPair(3, 1, 1e-4, 1e-3, 1e-3, g))
    refused(lib.tt_pop_exploit_nstep(pop._h, 1, bad_pair, (L.TTPopNstep * 1)(ok), stream), "tt_pop_exploit_nstep", "pair 0")
    refused(lib.tt_pop_nstep(pop._h, K, C.byref(L.TTPopNstep())), "tt_pop_nstep", "agent 3")
    refused(lib.tt_pop_nstep(pop._h, 0, None), "tt_pop_nstep", "out is NULL")
    # plain exploit where gamma ** n belongs, and the n-step exploit where there is no table
    refused(lib.tt_pop_exploit(pop._h, 1, one, stream), "tt_pop_exploit:", "table")
    refused(lib.tt_pop_exploit_nstep(plain._h, 1, one, (L.TTPopNstep * 1)(L.TTPopNstep(1, g, g)), stream), "tt_pop_exploit_nstep", "table")
    with pytest.raises(ValueError, match="n_step"):
        plain.exploit([(2, 1, dict(n_step=3))])
    with pytest.raises(ValueError, match="slots"):
        pop.exploit([(2, 1, dict(n_step=7))])
    torch.cuda.synchronize()
    assert [pop.n_step_of(a) for a in range(K)] == table and pop.n_steps == [1, 5, 3]
    after = [_learning_state(fl) + _own_state(fl, r) for fl, r in zip(pop.learners, pop.rings)]
    assert all(_equal(x, y) for x, y in zip(after, before))
    assert plain.n_step_of(1) == (1, _f32(HYP[1]["gamma"]), _f32(HYP[1]["gamma"]))
    plain.exploit([(2, 1, dict(NEW, n_step=1))])             # the one-step population's exploit, as it was
    assert plain.hyper(2) == {k: _f32(v) for k, v in NEW.items()}


N_LOOP, B_LOOP, UPS, STEPS, RING = 512, 128, 2, 30, 24


def _population_loop(n_step, graph, K=3, **kw):
    import torch
    from ddpg_trucktrailer_amd.population import PopulationRollout
    hyp = HYP[:K]
    pop = PopulationRollout(N_LOOP, [h["seed"] for h in hyp], alphas=[h["alpha"] for h in hyp], betas=[h["beta"] for h in hyp],
                            taus=[h["tau"] for h in hyp], gammas=[h["gamma"] for h in hyp], batch_size=B_LOOP, replay_slots=RING,
                            updates_per_step=UPS, graph_steps=4 if graph else 0, n_step=n_step, **kw)
    if graph:
        pop.run(STEPS)
        assert pop.graph1 is not None and pop.graphG is not None
    else:
        for _ in range(STEPS):
            pop.step()
    torch.cuda.synchronize()
    assert pop.learner.tail_gave_up() == [0] * K and pop.vector_steps == STEPS and pop.k == STEPS
    return pop


@pytest.fixture(scope="module")
def lone_loops(gpu_device):
    """Three lone serial-order loops with n = 5 and the tail in one launch, 30 vector steps each (made once, never changed)."""
    import torch
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    old = os.environ.get("TT_ACTOR_TAIL")
    os.environ["TT_ACTOR_TAIL"] = "1"
    try:
        lone = []
        for h in HYP[:3]:
            env = TruckTrailerVecEnv(N_LOOP, device=gpu_device)
            env.reset(seed=h["seed"])
            lp = DDPGRollout(env, seed=h["seed"], alpha=h["alpha"], beta=h["beta"], tau=h["tau"], gamma=h["gamma"], pipeline=False,
                             batch_size=B_LOOP, replay_slots=RING, updates_per_step=UPS, n_step=5)
            assert lp.learner.fuse_tail and not lp.pipeline
            lp.run(STEPS)
            lone.append(lp)
    finally:
        if old is None:
            os.environ.pop("TT_ACTOR_TAIL")
        else:
            os.environ["TT_ACTOR_TAIL"] = old
    torch.cuda.synchronize()
    return [_loop_state(lp, lp.learner) for lp in lone]


def test_population_loop_with_one_n_equals_lone_loops(gpu_device, lone_loops):
    """n_step = 5 for all: the population's graphs == its eager step() loop == three lone DDPGRollout(n_step=5, pipeline=False)."""
    import torch
    graphs, eager = _population_loop(5, True), _population_loop(5, False)
    assert graphs.n_steps == [5, 5, 5] and graphs.learner.nstep_table
    for a in range(3):
        g = _loop_state(graphs.loops[a], graphs.learner.learners[a])
        e = _loop_state(eager.loops[a], eager.learner.learners[a])
        assert int(g[-1].item()) == (STEPS - 5) * UPS
        assert torch.isfinite(g[0]).all()
        assert _equal(g, e), f"agent {a}: population graphs against its eager steps"
        assert _equal(g, lone_loops[a]), f"agent {a}: population graphs against the lone loop"


def test_population_loop_with_mixed_n(gpu_device, lone_loops):
    """n_step = 1, 3, 5: graphs == eager steps, and the agent with n = 5 = n_max is its lone loop bit for bit, because its start
    step coincides.  Agents 0 and 1 start learning at vector step 1 + n_max = 6 like everyone in the population, later than their
    lone loops would (steps 2 and 4), so they have no lone loop to equal."""
    import torch
    graphs, eager = _population_loop([1, 3, 5], True), _population_loop([1, 3, 5], False)
    assert graphs.n_steps == [1, 3, 5] and graphs.learner.nstep_table
    states = []
    for a in range(3):
        g = _loop_state(graphs.loops[a], graphs.learner.learners[a])
        e = _loop_state(eager.loops[a], eager.learner.learners[a])
        assert int(g[-1].item()) == (STEPS - 5) * UPS and torch.isfinite(g[0]).all()
        assert _equal(g, e), f"agent {a}: population graphs against its eager steps"
        states.append(g)
    assert _equal(states[2], lone_loops[2]), "the n = 5 agent against its lone loop"
    assert not _equal(states[1], lone_loops[1])               # (n = 3 is not n = 5)
    assert [graphs.learner.n_step_of(a)[0] for a in range(3)] == [1, 3, 5]


def test_pbt_explores_n_on_a_live_loop(gpu_device):
    """K = 4, n = 1, 3, 5, 5 with room for 8: after a round that fires, dst's table entry is the decision's "new"; the graphs are
    the ones captured before; weights finite, no tail give-up."""
    import torch
    from ddpg_trucktrailer_amd.pbt import PBT
    from ddpg_trucktrailer_amd.population import PopulationRollout
    K, hyp = 4, HYP[:4]
    pop = PopulationRollout(2048, [h["seed"] for h in hyp], alphas=[h["alpha"] for h in hyp], betas=[h["beta"] for h in hyp],
                            taus=[h["tau"] for h in hyp], gammas=[h["gamma"] for h in hyp], batch_size=B_LOOP, replay_slots=16,
                            updates_per_step=UPS, graph_steps=4, episode_log=1 << 18, n_step=[1, 3, 5, 5], n_step_max=8)
    assert pop._learn_from == 9 and pop._warm_steps == 9
    pbt = PBT(K, 10, seed=1, window=20, min_episodes=4, quantile=0.25, n_step_choices=(1, 3, 5, 8))
    pop.run(20)
    g1, gG = pop.graph1, pop.graphG
    assert g1 is not None and gG is not None
    fired = 0
    for _ in range(30):
        out = pbt.step(pop, pop.drain_episodes())
        if out:
            torch.cuda.synchronize()
            for d in out:
                n, g = d["new"]["n_step"], d["new"]["gamma"]
                assert n in (1, 3, 5, 8) and d["old"]["n_step"] in (1, 3, 5, 8)
                assert pop.learner.n_step_of(d["dst"]) == (n, _f32(g), _f32(float(g) ** n if n > 1 else g)), d
                assert pop.hyper(d["dst"]) == {k: _f32(d["new"][k]) for k in ("alpha", "beta", "tau", "gamma")}
                assert pop.n_steps[d["dst"]] == n
            fired += len(out)
        pop.run(10)
        if fired:
            break
    torch.cuda.synchronize()
    assert fired >= 1 and len(pbt.history) == fired
    assert pop.graph1 is g1 and pop.graphG is gG, "an exploit that changed n made run() capture again"
    assert pop.learner.tail_gave_up() == [0] * K
    for ag in pop.agents:
        assert all(torch.isfinite(p).all() for n in ag._nets() for p in n.parameters())
