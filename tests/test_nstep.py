"""CPU: n-step returns in the replay draw (csrc/ttnstep.hip, include/ttenv.h: tt_ring_sample_nstep) -- the two kernels' budgets,
every refusal of the two entry points over made-up addresses (nothing reaches a GPU), the torch twin of the draw against an f64
restatement of the walk, and what the Python classes refuse."""
import ctypes as C

import numpy as np
import pytest

import nstep_ref as ref


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib
    return _lib


def test_both_kernels_exist_within_their_budgets(L):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    ks = kr.kernels()
    fwd, lone = kr.find(ks, "k_fwd_multi_nstep"), kr.find(ks, "k_ring_sample_nstep")
    assert len(fwd) == 1 and len(lone) == 1, (list(fwd), list(lone))
    (v,), (w,) = fwd.values(), lone.values()
    assert v["max_threads"] == 512 and kr.waves_per_simd(v["vgpr"]) >= 2, v
    assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["lds"] <= 160 * 1024, v
    assert w["scratch"] == 0 and w["vgpr_spills"] == 0 and w["sgpr_spills"] == 0, w


class _Fake:
    """A plausible draw and learn()'s four forward jobs over made-up device addresses: the library checks them on the host, and
    with one bad argument nothing reaches the GPU."""

    def __init__(self, L, B=256, slots=16, reserve=0, draws=1, side_count=0):
        addr = iter(range(0x10000, 0x10000 + 0x1000 * 200, 0x1000))
        nxt = lambda: next(addr)
        self.w = [L.TTMlpWeights(*[nxt() for _ in range(12)], 23, 400, 300) for _ in range(4)]
        self.side = L.TTSideBuffer(nxt(), nxt(), nxt(), nxt(), nxt(), side_count, 0) if side_count else None
        self.sample = L.TTSampleArgs(B, 1024, slots, reserve, nxt(), nxt(), nxt(), nxt(), nxt(), 5,
                                     C.pointer(self.side) if self.side is not None else None,
                                     nxt(), nxt(), nxt(), nxt(), nxt(), None, 0, draws, 77, None)
        self.saved = [L.TTMlpSaved(*[nxt() for _ in range(6)]) for _ in range(2)]
        self.jobs = (L.TTFwdJob * 4)()
        smp = self.sample
        for j, (wi, crit, obs, act, out, saved, z) in enumerate(((2, 0, smp.s2_out, None, nxt(), None, None),
                                                                 (3, 1, smp.s2_out, None, None, None, nxt()),
                                                                 (1, 1, smp.s_out, smp.a_out, nxt(), self.saved[0], None),
                                                                 (0, 0, smp.s_out, None, nxt(), self.saved[1], None))):
            self.jobs[j].critic, self.jobs[j].obs, self.jobs[j].action = crit, obs, act
            self.jobs[j].w, self.jobs[j].out = C.pointer(self.w[wi]), out
            self.jobs[j].saved = C.pointer(saved) if saved is not None else None
            self.jobs[j].z_state = z


def _refused(L, who, rc, *words):
    msg = L.load().tt_last_error(None).decode()
    assert rc == L.TT_EINVAL, (who, rc)
    assert who in msg and all(w in msg for w in words), msg


@pytest.mark.parametrize("entry", ["tt_ring_sample_nstep", "tt_mlp_forward_multi_sampled_nstep"])
def test_entry_points_refuse_with_a_message_before_any_hip_call(L, entry):
    lib = L.load()
    assert L.NSTEP_MAX == 16

    def call(f, n_step, gamma, n=None, count=4, sample=True, jobs=True):
        smp = C.byref(f.sample) if sample else None
        if entry == "tt_ring_sample_nstep":
            return lib.tt_ring_sample_nstep(smp, n_step, gamma, None)
        return lib.tt_mlp_forward_multi_sampled_nstep(f.sample.batch if n is None else n, count, f.jobs if jobs else None, smp,
                                                      n_step, gamma, None, None)
    for n_step in (0, -1, 17):
        _refused(L, entry, call(_Fake(L), n_step, 0.99), "n_step")
    for gamma in (0.0, 1.0, -0.5, 1.5, float("nan")):
        _refused(L, entry, call(_Fake(L), 5, gamma), "gamma")
    # the window: slots >= 3 + reserve + (n_step - 1)
    _refused(L, entry, call(_Fake(L, slots=6), 5, 0.99), "slots")
    _refused(L, entry, call(_Fake(L, slots=8, reserve=2), 5, 0.99), "slots")
    _refused(L, entry, call(_Fake(L, slots=18, reserve=2), 16, 0.99), "slots")
    _refused(L, entry, call(_Fake(L, side_count=300), 2, 0.99), "side")
    _refused(L, entry, call(_Fake(L, draws=2), 5, 0.99), "draws")
    # ... and what make_ring_sample refuses
    _refused(L, entry, call(_Fake(L), 5, 0.99, sample=False))
    f = _Fake(L)
    f.sample.rew = None
    _refused(L, entry, call(f, 5, 0.99), "tt_sample_args")
    f = _Fake(L)
    f.sample.lag = -1
    _refused(L, entry, call(f, 5, 0.99), "tt_sample_args")
    if entry == "tt_mlp_forward_multi_sampled_nstep":      # the argument checks of tt_mlp_forward_multi_sampled
        _refused(L, entry, call(_Fake(L), 5, 0.99, n=128))
        _refused(L, entry, call(_Fake(L), 5, 0.99, count=5))
        _refused(L, entry, call(_Fake(L), 5, 0.99, jobs=False))
        f = _Fake(L)
        f.jobs[3].obs = 0x7000                              # a job that reads neither s nor s'
        _refused(L, entry, call(f, 5, 0.99), "job 3")
        f = _Fake(L)
        f.jobs[0].obs = f.jobs[1].obs = f.sample.s_out      # nobody leaves s', R, D for the later launches
        _refused(L, entry, call(f, 5, 0.99))


@pytest.mark.parametrize("gamma", [0.99, 0.95])
@pytest.mark.parametrize("n_step", [1, 3, 5, 8])
def test_torch_twin_of_the_draw_against_the_walk_in_f64(L, n_step, gamma):
    """TrajectoryRing.sample(n_step=..., return_index=True) on the CPU: every row recomputed in f64 numpy from the base step the
    draw reports.  s, a, s2, done and the index exact; |R - R64| <= 4 n 2^-24 sum_j |gamma^j r_j| (nstep_ref.walk64 has the
    derivation); for n >= 3 at least 10 % of the rows end at a done and at least 10 % run their full n steps; the base step
    never leaves the part of the window that has its n steps."""
    import torch
    ring = ref.synthetic_ring("cpu")
    g = torch.Generator().manual_seed(11 + n_step)
    out = ring.sample(ref.BATCH, generator=g, n_step=n_step, gamma=gamma, return_index=True)
    assert out[2].dtype == torch.float32 and out[4].dtype == torch.bool and out[5].shape == (ref.BATCH, 2)
    r64, back = ref.check_rows(ring, out, n_step, gamma, k=ref.K, avail=ref.SLOTS - 1)
    assert len(np.unique(back)) == ref.SLOTS - 1 - (n_step - 1)          # every base position of the window is drawn
    if n_step == 1:      # the one-step draw, as it always was: r and done are the stored ones
        idx = out[5].numpy()
        assert np.array_equal(out[2].numpy(), ring.rew.numpy()[idx[:, 0], idx[:, 1]])
        g2 = torch.Generator().manual_seed(11 + n_step)
        for x, y in zip(ring.sample(ref.BATCH, generator=g2), out[:5]):
            assert torch.equal(x, y)


def test_torch_twin_refuses_what_the_kernel_refuses(L):
    import torch
    ring = ref.synthetic_ring("cpu")
    with pytest.raises(ValueError, match="n_step"):
        ring.sample(8, n_step=17, gamma=0.99)
    with pytest.raises(ValueError, match="gamma"):
        ring.sample(8, n_step=3)
    with pytest.raises(ValueError, match="gamma"):
        ring.sample(8, n_step=3, gamma=1.0)
    ring.load_side(torch.zeros(4, 23), torch.zeros(4), torch.zeros(4), torch.zeros(4, 23), torch.zeros(4))
    with pytest.raises(ValueError, match="not supported"):
        ring.sample(8, n_step=3, gamma=0.99)
    assert len(ring.sample(8)) == 5                                       # one step: side tuples are part of the draw, as before


class _Env:
    """What DDPGRollout's constructor asks of an env (the refusals below come before anything else is asked)."""
    n_envs, observation_dim = 8, 23

    def __init__(self):
        import torch
        self.device = torch.device("cpu")

    def observe(self, out):
        out.zero_()


def test_python_side_refuses_what_n_step_does_not_support(L):
    import torch
    from ddpg_trucktrailer_amd.agent import Agent
    from ddpg_trucktrailer_amd.population import PopulationRollout
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    with pytest.raises(ValueError, match="not supported"):
        PopulationRollout(64, [1, 2], device="cpu", n_step=5)
    with pytest.raises(ValueError, match="not supported"):
        DDPGRollout(_Env(), n_step=5, data_parallel=True)
    with pytest.raises(ValueError, match="not supported"):
        DDPGRollout(_Env(), n_step=5, replay_slots=6)
    for n in (0, 17):
        with pytest.raises(ValueError, match="n_step"):
            DDPGRollout(_Env(), n_step=n)
    loop = DDPGRollout(_Env(), n_step=5, replay_slots=16, batch_size=4)
    assert loop.n_step == 5 and loop._learn_from == 6 and loop._draws_per_opening() == 1
    with pytest.raises(ValueError, match="not supported"):               # a side buffer later
        loop.ring.load_side(torch.zeros(2, 23), torch.zeros(2), torch.zeros(2), torch.zeros(2, 23), torch.zeros(2))
    loop.ring.side_count = 1                                             # ... or one that got there another way
    with pytest.raises(ValueError, match="not supported"):
        loop.run(1)
    loop.ring.side_count = 0
    sd = loop.state_dict()
    assert sd["n_step"] == 5
    with pytest.raises(ValueError, match="n_step"):
        DDPGRollout(_Env(), replay_slots=16, batch_size=4).load_state_dict(sd)
    one = DDPGRollout(_Env(), replay_slots=16, batch_size=4)
    assert one.n_step == 1 and one._learn_from == 2 and one._warm_steps == 4 and one.state_dict()["n_step"] == 1
    # the torch learner's discount: gamma ** n in the target, gamma when nothing is said
    torch.manual_seed(0)
    s, a, r, s2 = torch.rand(16, 23), torch.rand(16, 1), torch.rand(16), torch.rand(16, 23)
    d = torch.zeros(16, dtype=torch.bool)
    ends = []
    for discount in (None, 0.99, 0.99 ** 5):
        torch.manual_seed(1)
        ag = Agent(alpha=1e-4, beta=1e-3, input_dims=(23,), tau=1e-3, n_actions=1, gamma=0.99, batch_size=16, device="cpu", replay=False)
        ag.learn_batch(s, a, r, s2, d, **({} if discount is None else dict(discount=discount)))
        ends.append(torch.cat([p.detach().reshape(-1) for p in ag.critic.parameters()]))
    assert torch.equal(ends[0], ends[1]) and not torch.equal(ends[0], ends[2])
