"""GPU (-m gpu): per-agent gradient-norm clipping in a population (csrc/ttclip.hip: k_pop_grad_sqnorm, k_pop_adam_soft_clip,
k_pop_clip_write; population.py: grad_clips / grad_clip) against lone learners and lone loops.

Agent a with the values (c, a') must have, on the same draws, the bits of a lone FusedLearner(grad_clip=GradClip(c or None, a' or
None)); an agent with (0, 0) in a population that has the table, the bits of the lone separate-optimizer chain --
phase_a(fuse_adam=False), phase_b(separate_adam=True), phase_c --, the twin tests/test_gpu_grad_clip.py uses for an inactive clip.

max_norm comes from the lone twin's own norms, as in tests/clip_ref.py: a learner whose clip never acts (GradClip(1e30, 1e30)) runs
the test's updates once and reports the norm of every update at both sites.  "active" is 0.5 x the smallest of them, "inactive" 2 x
the largest.  An agent whose two values are inactive IS that run, so no update of it can clip; an active value clips the first update
for certain (the critic's first norm is that run's; the actor's differs only through the critic's first step).  The tests assert
what they rely on from the counts: an inactive site has clipped 0 and coef exactly 1.0, an active one clipped >= 1.

Shapes: B = 1 (one row), 33 (a ragged 16-row tile), 257 (one row past a tile); K = 3, so the agent arithmetic is exercised at the
first, a middle and the last agent; rings and envs as tests/test_gpu_population.py has them."""
import ctypes as C
import math

import pytest
from test_gpu_pbt import NEW, _f32, _learning_state
from test_gpu_population import HYP, STRIDE, _agent, _equal, _loop_state, _ring, _state

pytestmark = pytest.mark.gpu

UPDATES = 3
BATCHES = (1, 33, 257)
OFF = 1e30
FWD_HALVES = 2 * 20 * 13 * 512          # an fc2 image's forward half: h and m planes of [20 neuron tiles][13 k32 steps] x 512 halves


def _clip(c, a):
    from ddpg_trucktrailer_amd.grad_clip import GradClip
    return None if not c and not a else GradClip(c or None, a or None)


def _full(fl):
    """Everything an update leaves: _state's parameters, targets, moments, step count, q, y and mu; both flat gradients; q_pi and
    dq_da; the fc2 images -- of the two targets the forward half, the one a target's image is kept current in and read from (the
    comparison tests/test_gpu_grad_clip.py makes of a maintained target image)."""
    import torch
    ag = fl.agent
    out = _state(fl) + [t.clone() for t in (fl.critic.flat_grad, fl.actor.flat_grad, fl.q_pi, fl.dq_da)]
    if fl.use_images:
        out += [fl._img[id(n)].clone() for n in (ag.actor, ag.critic)]
        out += [fl._img[id(n)].view(torch.float16)[:FWD_HALVES].clone() for n in (ag.target_actor, ag.target_critic)]
    return out


def _differ(x, y):
    import torch
    return [i for i, (a, b) in enumerate(zip(x, y)) if not torch.equal(a, b)] + ([] if len(x) == len(y) else ["length"])


def _lone(dev, a, B, clip, updates=range(UPDATES), fl=None, ring=None, n_step=1, hyp=None, norms=None):
    """A lone FusedLearner of agent a's making on agent a's ring with agent a's keys.  clip: a GradClip, or None = the
    separate-optimizer chain.  norms: a list that takes (critic norm, actor norm) of every update."""
    import torch
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    if fl is None:
        fl = FusedLearner(_agent(dev, hyp or HYP[a]), B, fc2_images=True, grad_clip=clip)
    ring = _ring(dev, 100 + a) if ring is None else ring
    for u in updates:
        args = ring.sample_args(B, seed=(HYP[a]["seed"] + u * STRIDE) & (2 ** 64 - 1))
        s, act, r, s2, d = ring._batch_bufs(B)[:5]
        if clip is not None:
            fl.learn_batch(s, act, r, s2, d, sample=args, n_step=n_step)
        else:
            fl.phase_a(s, act, r, s2, d, fuse_adam=False, sample=args, n_step=n_step)
            fl.phase_b(s, separate_adam=True)
            fl.phase_c()
        if norms is not None:
            st = fl.clip_stats()
            norms.append((st["critic"]["norm"], st["actor"]["norm"]))
    torch.cuda.synchronize()
    return fl


_NORMS = {}


def _values(dev, a, B):
    """(active critic, active actor, inactive critic, inactive actor) for agent a at batch B (module docstring); made once."""
    if (a, B) not in _NORMS:
        norms = []
        _lone(dev, a, B, _clip(OFF, OFF), norms=norms)
        assert all(math.isfinite(x) and x > 0 for n in norms for x in n), norms
        c, ac = [n[0] for n in norms], [n[1] for n in norms]
        _NORMS[(a, B)] = (_f32(0.5 * min(c)), _f32(0.5 * min(ac)), _f32(2.0 * max(c)), _f32(2.0 * max(ac)))
    return _NORMS[(a, B)]


def _pop(dev, B, clips, K=3, n_steps=None, rings=None, **kw):
    from ddpg_trucktrailer_amd.population import PopulationLearner
    hyp = HYP[:K]
    return PopulationLearner([_agent(dev, h) for h in hyp], B, fc2_images=True, rings=rings or [_ring(dev, 100 + a) for a in range(K)],
                             seeds=[h["seed"] for h in hyp], n_steps=n_steps, grad_clips=clips, **kw)


def _same_bits(x, y):
    """_equal over the tensors' bytes: a NaN equals the NaN with the same bits."""
    import torch
    raw = lambda t: t.detach().contiguous().reshape(-1).view(torch.uint8)
    return len(x) == len(y) and all(a.shape == b.shape and a.dtype == b.dtype and torch.equal(raw(a), raw(b)) for a, b in zip(x, y))


def _same_stats(pop_stats, lone_stats):
    """clip_stats(a) of a population against the lone learner's, over the networks the lone learner clips (NaN equals NaN)."""
    for key, want in lone_stats.items():
        got = pop_stats[key]
        for k in ("norm", "coef"):
            assert got[k] == want[k] or (math.isnan(got[k]) and math.isnan(want[k])), (key, k, got, want)
        assert (got["updates"], got["clipped"]) == (want["updates"], want["clipped"]), (key, got, want)


# ---- 1. every agent against its lone twin ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_population_learn_with_clips_is_bitwise_the_lone_learners(gpu_device, B):
    """K = 3 with (active, active), (inactive, inactive), (0, active): three updates leave every agent's parameters, targets, m, v,
    step count, q, y, mu, q_pi, dq_da, fc2 images and both gradient buffers -- the UNCLIPPED gradients -- bit for bit its lone
    FusedLearner(grad_clip=)'s, and clip_stats(a) equal to the lone learner's out and counts.  A second population, (0, 0), (active,
    inactive), (inactive, active): its (0, 0) agent has the bits of the lone separate-optimizer chain, reports its norms with coef 1."""
    import torch
    dev = gpu_device
    v = [_values(dev, a, B) for a in range(3)]
    first = [(v[0][0], v[0][1]), (v[1][2], v[1][3]), (0.0, v[2][1])]
    second = [(0.0, 0.0), (v[1][0], v[1][3]), (v[2][2], v[2][1])]
    for values in (first, second):
        pop = _pop(dev, B, [_clip(c, a) for c, a in values])
        assert pop.clip_table and pop.grad_clips == [list(x) for x in values]
        for u in range(UPDATES):
            pop.learn(u)
        torch.cuda.synchronize()
        assert pop.tail_gave_up() == [0] * 3
        for a, (c, ac) in enumerate(values):
            assert pop.clip_of(a) == (c, ac)
            lone = _lone(dev, a, B, _clip(c, ac))
            got, want = _full(pop.learners[a]), _full(lone)
            assert int(lone.step_dev.item()) == UPDATES and all(torch.isfinite(x.float()).all() for x in want)
            assert _equal(got, want), f"B {B} agent {a} {(c, ac)}: entries {_differ(got, want)} differ"
            stats = pop.clip_stats(a)
            print(f"B {B} agent {a} max_norm {(c, ac)}: {stats}")
            if c or ac:
                _same_stats(stats, lone.clip_stats())
            for key, x, active in (("critic", c, c == v[a][0]), ("actor", ac, ac == v[a][1])):
                assert stats[key]["updates"] == UPDATES and stats[key]["norm"] > 0
                if active:
                    assert stats[key]["clipped"] >= 1
                else:       # inactive or 0: never clipped, and the last coefficient is exactly 1
                    assert stats[key]["clipped"] == 0 and stats[key]["coef"] == 1.0
    # the clip is not a no-op: the (active, active) agent differs from the chain without a clip
    assert not _equal(_full(_lone(dev, 0, B, _clip(*first[0]))), _full(_lone(dev, 0, B, None)))


# ---- 2. an all-zero table ------------------------------------------------------------------------------------------------------------
def test_an_all_zero_table_is_the_separate_optimizer_chain(gpu_device):
    """tt_pop_learn_set_clip with {0, 0} for every agent (through the C entry point: Python makes no table without a value): the eight
    launches leave every agent the bits of the lone separate-optimizer chain; coef is 1.0, nothing is counted as clipped, the norms
    are reported."""
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    dev, B, K = gpu_device, 33, 3
    pop = _pop(dev, B, None)
    assert not pop.clip_table
    pop._create()
    pop._key = pop._storage_key()
    L.check(pop.lib.tt_pop_learn_set_clip(pop._h, (L.TTPopClip * K)()))
    pop.clip_table = True
    for u in range(UPDATES):
        pop.learn(u)
    torch.cuda.synchronize()
    for a in range(K):
        got, want = _full(pop.learners[a]), _full(_lone(dev, a, B, None))
        assert _equal(got, want), f"agent {a}: entries {_differ(got, want)} differ"
        stats = pop.clip_stats(a)
        assert pop.clip_of(a) == (0.0, 0.0)
        assert all(s["coef"] == 1.0 and s["clipped"] == 0 and s["updates"] == UPDATES and s["norm"] > 0 for s in stats.values()), stats


# ---- 3. isolation ------------------------------------------------------------------------------------------------------------------
def test_a_poisoned_agent_does_not_reach_its_neighbours(gpu_device):
    """Agent 1's ring rewards are NaN: its norms and coefficients are NaN where its lone twin's are, and agents 0 and 2 keep the bits of
    a run without the poison."""
    import torch
    dev, B = gpu_device, 33
    v = [_values(dev, a, B) for a in range(3)]
    clips = [_clip(v[a][0], v[a][1]) for a in range(3)]
    runs = []
    for poison in (False, True):
        rings = [_ring(dev, 100 + a) for a in range(3)]
        if poison:
            rings[1].rew.fill_(float("nan"))
        pop = _pop(dev, B, clips, rings=rings)
        for u in range(UPDATES):
            pop.learn(u)
        torch.cuda.synchronize()
        runs.append(([_full(fl) for fl in pop.learners], [pop.clip_stats(a) for a in range(3)]))
    for a in (0, 2):
        assert _equal(runs[1][0][a], runs[0][0][a]) and runs[1][1][a] == runs[0][1][a], f"agent {a} saw agent 1's NaN"
    ring = _ring(dev, 101)
    ring.rew.fill_(float("nan"))
    lone = _lone(dev, 1, B, clips[1], ring=ring)
    want = lone.clip_stats()
    got = runs[1][1][1]
    assert math.isnan(want["critic"]["norm"]) and math.isnan(got["critic"]["norm"]) and math.isnan(got["critic"]["coef"])
    _same_stats(got, want)
    assert _same_bits(runs[1][0][1], _full(lone)), "the poisoned agent against its poisoned lone twin, NaN payloads included"


# ---- 4. a captured graph survives an exploit that changes the clip ----------------------------------------------------------------------
def test_a_captured_learn_takes_the_clip_an_exploit_wrote(gpu_device):
    """Two eager updates, a graph captured over learn(2), then exploit 2 <- 0 with NEW and a new clip, then the replay: agent 2 is
    the lone learner holding agent 0's state at the exploit point with NEW and the new clip; clip_of(2) reads the new values;
    agent 1 has the bits of a population that never exploited."""
    import torch
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    from ddpg_trucktrailer_amd.rollout import _CAPTURE_MODE, _gc_off
    dev, B = gpu_device, 33
    v = [_values(dev, a, B) for a in range(3)]
    clips = [_clip(v[a][0], v[a][1]) for a in range(3)]
    new_clip = (_f32(0.25 * v[0][0] / 0.5), _f32(3.0 * v[0][1]))          # a quarter of agent 0's critic norm, 1.5 x its actor norm
    plain = _pop(dev, B, clips)
    for u in range(3):
        plain.learn(u)
    pop = _pop(dev, B, clips)
    for u in range(2):
        pop.learn(u)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with _gc_off(), torch.cuda.graph(g, stream=side, capture_error_mode=_CAPTURE_MODE):
        pop.learn(2)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    src = pop.agents[0]
    nets = {n: {k: t.clone() for k, t in getattr(src, n).state_dict().items()} for n in ("actor", "critic", "target_actor", "target_critic")}
    adam = pop.state_dict(0)
    pop.exploit([(2, 0, dict(NEW, clip_critic=new_clip[0], clip_actor=new_clip[1]))])
    torch.cuda.synchronize()
    assert _equal(_learning_state(pop.learners[2]), _learning_state(pop.learners[0]))
    assert pop.clip_of(2) == new_clip and pop.grad_clips[2] == list(new_clip) and pop.clip_of(0) == (v[0][0], v[0][1])
    assert pop.hyper(2) == {k: _f32(x) for k, x in NEW.items()}
    g.replay()
    torch.cuda.synchronize()
    ag = _agent(dev, dict(HYP[2], **NEW))
    for name, sd in nets.items():
        getattr(ag, name).load_state_dict(sd)
    fl = FusedLearner(ag, B, fc2_images=True, grad_clip=_clip(*new_clip))
    fl.load_state_dict(dict(adam, grad_clip=list(_clip(*new_clip).as_tuple())))
    lone = _lone(dev, 2, B, _clip(*new_clip), updates=[2], fl=fl)
    got, want = _full(pop.learners[2]), _full(lone)
    assert _equal(got, want), f"dst after the replay: entries {_differ(got, want)} differ"
    st = pop.clip_stats(2)
    _same_stats({k: dict(s, updates=1, clipped=int(s["coef"] < 1.0)) for k, s in st.items()}, lone.clip_stats())
    assert st["critic"]["coef"] < 1.0, "the new critic clip, a quarter of agent 0's norm, did not act: the test shows nothing"
    for a in (0, 1):
        assert _equal(_full(pop.learners[a]), _full(plain.learners[a])), f"agent {a} moved with the exploit"
    # an exploit without the keys carries src's clip; a population without the table refuses the keys
    pop.exploit([(1, 0, NEW)])
    assert pop.clip_of(1) == pop.clip_of(0) and pop.grad_clips[1] == pop.grad_clips[0]
    bare = _pop(dev, B, None)
    bare.learn(0)
    with pytest.raises(ValueError, match="clip"):
        bare.exploit([(1, 0, dict(NEW, clip_critic=1.0))])
    with pytest.raises(ValueError, match="clip_actor"):
        pop.exploit([(1, 0, dict(NEW, clip_actor=-1.0))])


# ---- 5. with the n-step table, in both orders of the two set_ calls -------------------------------------------------------------------
@pytest.mark.parametrize("clip_first", [False, True], ids=["nstep-then-clip", "clip-then-nstep"])
def test_clip_with_the_n_step_table(gpu_device, clip_first):
    """K = 2, n = [1, 3], a clip on both: every agent is the lone FusedLearner(grad_clip=) drawing with its n, whichever of
    tt_pop_learn_set_nstep and tt_pop_learn_set_clip came first."""
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    dev, B, n_steps = gpu_device, 33, [1, 3]
    v = [_values(dev, a, B) for a in range(2)]
    clips = [_clip(v[0][0], v[0][1]), _clip(v[1][2], v[1][1])]
    pop = _pop(dev, B, clips, K=2, n_steps=n_steps)
    assert pop.nstep_table and pop.clip_table
    if clip_first:          # _create() makes the clip table alone; the n-step table follows by hand
        pop.nstep_table = False
        pop._create()
        pop._key = pop._storage_key()
        ns = (L.TTPopNstep * 2)(*[pop._nstep_struct(ag.gamma, n) for ag, n in zip(pop.agents, n_steps)])
        L.check(pop.lib.tt_pop_learn_set_nstep(pop._h, ns))
        pop.nstep_table = True
    for u in range(UPDATES):
        pop.learn(u)
    torch.cuda.synchronize()
    for a, n in enumerate(n_steps):
        lone = _lone(dev, a, B, clips[a], n_step=n)
        got, want = _full(pop.learners[a]), _full(lone)
        assert _equal(got, want), f"agent {a}, n = {n}: entries {_differ(got, want)} differ"
        _same_stats(pop.clip_stats(a), lone.clip_stats())
        assert pop.n_step_of(a)[0] == n
    assert pop.clip_stats(0)["critic"]["clipped"] >= 1


# ---- 6. the loop -------------------------------------------------------------------------------------------------------------------
N_LOOP, B_LOOP, RING, STEPS = 512, 33, 16, 12
LOOP_CLIPS = ((0.5, 0.01), (2.0, 0.0))


def _population_loop(ups, graph_steps=4, clips=LOOP_CLIPS, **kw):
    from ddpg_trucktrailer_amd.population import PopulationRollout
    hyp = HYP[:len(clips)]
    return PopulationRollout(N_LOOP, [h["seed"] for h in hyp], alphas=[h["alpha"] for h in hyp], betas=[h["beta"] for h in hyp],
                             taus=[h["tau"] for h in hyp], gammas=[h["gamma"] for h in hyp], batch_size=B_LOOP, replay_slots=RING,
                             updates_per_step=ups, graph_steps=graph_steps, grad_clip=[_clip(*c) for c in clips], **kw)


@pytest.mark.parametrize("ups", [1, 3])
def test_population_loop_with_clips_equals_lone_loops(gpu_device, ups):
    """PopulationRollout(grad_clip=[GradClip(0.5, 0.01), GradClip(2.0, None)]), K = 2, 12 vector steps -- eager warm-up, then graph
    replays -- against a lone DDPGRollout(pipeline=False, grad_clip=) per agent: weights, ring, env state, noise and moments."""
    import torch
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    pop = _population_loop(ups)
    pop.run(STEPS)
    torch.cuda.synchronize()
    assert pop.graph1 is not None and pop.learner.tail_gave_up() == [0, 0]
    for a, (h, c) in enumerate(zip(HYP, LOOP_CLIPS)):
        env = TruckTrailerVecEnv(N_LOOP, device=gpu_device)
        env.reset(seed=h["seed"])
        lp = DDPGRollout(env, seed=h["seed"], alpha=h["alpha"], beta=h["beta"], tau=h["tau"], gamma=h["gamma"], pipeline=False,
                         batch_size=B_LOOP, replay_slots=RING, updates_per_step=ups, grad_clip=_clip(*c))
        lp.run(STEPS)
        torch.cuda.synchronize()
        got, want = _loop_state(pop.loops[a], pop.learner.learners[a]), _loop_state(lp, lp.learner)
        assert int(want[-1].item()) == (STEPS - 1) * ups and torch.isfinite(want[0]).all()
        assert _equal(got, want), f"agent {a}: entries {_differ(got, want)} differ"
        _same_stats(pop.clip_stats(a), lp.learner.clip_stats())
        assert pop.clip_stats(a)["critic"]["updates"] == (STEPS - 1) * ups
        env.close()
    assert pop.clip_stats(0)["critic"]["clipped"] >= 1 and pop.clip_stats(1)["actor"]["clipped"] == 0


# ---- 7. the learn log ------------------------------------------------------------------------------------------------------------------
def test_the_learn_log_of_a_clipped_population(gpu_device):
    """Records exist for every update of every agent, and the last record's gradient norms are out[0] of the two sites -- the norm of
    the UNCLIPPED gradient -- within tests/test_gpu_grad_clip.py's tolerance for the same comparison: out[0]'s rounding to f32,
    2^-24 relative, plus the learn log's own (numel + 2) 2^-52."""
    import torch
    dev, B = gpu_device, 33
    v = [_values(dev, a, B) for a in range(3)]
    pop = _pop(dev, B, [_clip(v[a][0], v[a][1]) for a in range(3)], learn_log=8)
    for u in range(UPDATES):
        pop.learn(u)
    torch.cuda.synchronize()
    for a, rec in enumerate(pop.drain_learn_log()):
        assert rec["step"].tolist() == [1, 2, 3] and int(rec["nonfinite"].sum()) == 0
        stats = pop.clip_stats(a)
        for key, st in (("critic", pop.learners[a].critic), ("actor", pop.learners[a].actor)):
            got, out0 = float(rec["grad_norm_" + key][-1]), stats[key]["norm"]
            tol = (2.0 ** -24 + (st.flat_grad.numel() + 2) * 2.0 ** -52) * got
            print(f"agent {a} learn log grad_norm_{key} {got!r}, out[0] {out0!r}, |diff| {abs(got - out0):.3g}, tol {tol:.3g}")
            assert got > 0 and abs(got - out0) <= tol


# ---- 8. checkpoint -----------------------------------------------------------------------------------------------------------------
def test_a_clipped_population_resumes_bitwise(gpu_device, tmp_path):
    """Six steps, an exploit that changes agent 1's clip, a checkpoint, six more steps == a fresh population that loads the file and
    runs six steps; the file carries the clips, the resumed table holds them, and a population without the option refuses the file."""
    import torch
    from ddpg_trucktrailer_amd import checkpoint
    a = _population_loop(1)
    a.run(6)
    a.exploit([(1, 0, dict(NEW, clip_critic=0.75, clip_actor=0.02))])
    path = checkpoint.save_population_checkpoint(str(tmp_path / "pop.pt"), a)
    sd = a.state_dict()
    assert sd["grad_clip_table"] is True and [st["clip"] for st in sd["agents"]] == [[0.5, 0.01], [0.75, 0.02]]
    a.run(6)
    b = _population_loop(1)
    b.run(5)
    checkpoint.load_population_checkpoint(path, b)
    assert b.grad_clips == [[0.5, 0.01], [0.75, 0.02]] and b.clip_of(1) == (0.75, _f32(0.02))
    b.run(6)
    torch.cuda.synchronize()
    for i in range(2):
        got, want = _loop_state(b.loops[i], b.learner.learners[i]), _loop_state(a.loops[i], a.learner.learners[i])
        assert _equal(got, want), f"agent {i}: entries {_differ(got, want)} differ"
        assert _equal([b.learner.learners[i].critic.m, b.learner.learners[i].actor.v], [a.learner.learners[i].critic.m, a.learner.learners[i].actor.v])
    from ddpg_trucktrailer_amd.population import PopulationRollout
    hyp = HYP[:2]
    bare = PopulationRollout(N_LOOP, [h["seed"] for h in hyp], batch_size=B_LOOP, replay_slots=RING)
    with pytest.raises(ValueError, match="grad_clip"):
        checkpoint.load_population_checkpoint(path, bare)


# ---- 9. the refusals that need a live handle ----------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle(gpu_device):
    """tt_pop_learn_set_clip, tt_pop_clip_write and tt_pop_clip on live handles: value ranges, agent indices, duplicates, counts, no
    table -- TT_EINVAL, a message naming the entry point and the agent or entry, and nothing moved."""
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    dev, K, B = gpu_device, 3, 33
    pop, bare = _pop(dev, B, [_clip(1.0, 0.5)] * K), _pop(dev, B, None)
    pop.learn(0)
    bare.learn(0)
    torch.cuda.synchronize()
    before = [_full(fl) for fl in pop.learners]
    lib, stream = pop.lib, L.stream()

    def refused(rc, *words):
        msg = lib.tt_last_error(None).decode()
        assert rc == L.TT_EINVAL, (rc, msg)
        assert all(w in msg for w in words), msg
    ok = L.TTPopClip(1.0, 0.5)
    one = (C.c_int32 * 1)(1)
    for bad, word in ((L.TTPopClip(-1.0, 0.5), "max_norm_critic"), (L.TTPopClip(float("nan"), 0.5), "max_norm_critic"),
                      (L.TTPopClip(1.0, float("inf")), "max_norm_actor"), (L.TTPopClip(1.0, -0.0001), "max_norm_actor")):
        refused(lib.tt_pop_learn_set_clip(pop._h, (L.TTPopClip * K)(ok, bad, ok)), "tt_pop_learn_set_clip", "agent 1", word)
        refused(lib.tt_pop_clip_write(pop._h, 2, (C.c_int32 * 2)(0, 2), (L.TTPopClip * 2)(ok, bad), stream), "tt_pop_clip_write", "entry 1", word)
    refused(lib.tt_pop_learn_set_clip(pop._h, None), "tt_pop_learn_set_clip", "per_agent is NULL")
    refused(lib.tt_pop_clip_write(pop._h, 1, None, (L.TTPopClip * 1)(ok), stream), "tt_pop_clip_write", "agents is NULL")
    refused(lib.tt_pop_clip_write(pop._h, 1, one, None, stream), "tt_pop_clip_write", "values is NULL")
    for count in (0, -1, K + 1):
        refused(lib.tt_pop_clip_write(pop._h, count, one, (L.TTPopClip * 1)(ok), stream), "tt_pop_clip_write", f"count = {count}")
    for agent in (-1, K):
        refused(lib.tt_pop_clip_write(pop._h, 1, (C.c_int32 * 1)(agent), (L.TTPopClip * 1)(ok), stream), "tt_pop_clip_write", f"agent {agent}")
    refused(lib.tt_pop_clip_write(pop._h, 2, (C.c_int32 * 2)(2, 2), (L.TTPopClip * 2)(ok, ok), stream), "tt_pop_clip_write", "both name agent 2")
    value, out, counts = L.TTPopClip(), (C.c_float * 4)(), (C.c_int64 * 4)()
    refused(lib.tt_pop_clip(pop._h, K, C.byref(value), C.byref(out), C.byref(counts)), "tt_pop_clip", "agent 3")
    refused(lib.tt_pop_clip(pop._h, 0, None, C.byref(out), C.byref(counts)), "tt_pop_clip", "NULL")
    refused(lib.tt_pop_clip_write(bare._h, 1, one, (L.TTPopClip * 1)(ok), stream), "tt_pop_clip_write", "no clip table")
    refused(lib.tt_pop_clip(bare._h, 0, C.byref(value), C.byref(out), C.byref(counts)), "tt_pop_clip", "no clip table")
    with pytest.raises(ValueError, match="grad_clip is off"):
        bare.clip_stats(0)
    torch.cuda.synchronize()
    assert [pop.clip_of(a) for a in range(K)] == [(1.0, 0.5)] * K
    assert all(_equal(x, _full(fl)) for x, fl in zip(before, pop.learners))
