"""CPU: the population learn() of K agents (csrc/ttpop.hip, include/ttenv.h: tt_pop_learn_*) -- its kernels exist in libttenv.so
with the budgets of the lone launches they wrap (tests/test_kernel_resources.py), and every bad argument of its C ABI is TT_EINVAL
with a message, found before any HIP call (no GPU here)."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def ks(lib):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    return kr.kernels()


def _one(ks, part):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    found = kr.find(ks, part)
    assert len(found) == 1, (part, sorted(found))
    return next(iter(found.items()))


@pytest.mark.parametrize("part", ["15k_pop_fwd_multi", "19k_pop_bwd_rows_pair", "16k_pop_actor_tail"])
def test_population_row_kernels_keep_two_waves_per_simd(ks, part):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    n, v = _one(ks, part)
    assert v["max_threads"] == 512 and kr.waves_per_simd(v["vgpr"]) >= 2, (n, v)
    assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["lds"] <= 160 * 1024, (n, v)


def test_population_weight_kernel_fits_three_workgroups_per_cu(ks):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    n, v = _one(ks, "17k_pop_bwd_weightsILb0E")
    assert v["vgpr"] <= 168 and kr.waves_per_simd(v["vgpr"]) >= 3, (n, v)
    assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and 3 * v["lds"] <= 160 * 1024, (n, v)


class _Fake:
    """A plausible agent description over made-up device addresses (the library checks them on the host and copies them; with
    one bad argument in the population nothing reaches the GPU)."""

    def __init__(self, L, B, batch=None):
        addr = iter(range(0x10000, 0x10000 + 0x1000 * 400, 0x1000))
        nxt = lambda: next(addr)
        self.w = [L.TTMlpWeights(*[nxt() for _ in range(12)], 23, 400, 300) for _ in range(4)]  # actor, critic, target a, target c
        self.sample = L.TTSampleArgs(B if batch is None else batch, 1024, 8, 0, nxt(), nxt(), nxt(), nxt(), nxt(), 5, None,
                                     nxt(), nxt(), nxt(), nxt(), nxt(), None, 0, 1, 77, None)
        sv = lambda: L.TTMlpSaved(*[nxt() for _ in range(6)])
        self.saved = [sv(), sv()]
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
        self.td = L.TTTdInput(z_state=nxt(), mu_target=nxt(), target_critic=C.pointer(self.w[3]), reward=nxt(), done=nxt(), gamma=0.99,
                              y_out=nxt(), q_out=nxt(), step_dev=nxt(), window_dev=None, bias_corr_out=nxt(), adam_beta1=0.9,
                              adam_beta2=0.999)
        self.ws = [L.TTMlpBwdWs(*[nxt() for _ in range(5)]) for _ in range(2)]
        self.grads = [L.TTMlpWeights(*[nxt() for _ in range(12)], 23, 400, 300) for _ in range(2)]
        self.tables = [(C.c_void_p * 12)(*[nxt() for _ in range(12)]) for _ in range(8)]
        nets = []
        for i, count in enumerate((12, 10)):
            p, m, v, t = self.tables[4 * i:4 * i + 4]
            nets.append(L.TTPopNet(C.pointer(self.ws[i]), C.pointer(self.grads[i]), count, 0, C.cast(p, C.c_void_p), C.cast(m, C.c_void_p),
                                   C.cast(v, C.c_void_p), C.cast(t, C.c_void_p), 1e-3, 0.9, 0.999, 1e-8, 0.01, 1e-3, None))
        self.agent = L.TTPopAgent(C.pointer(self.sample), self.jobs, C.pointer(self.td), nets[0], nets[1], nxt(), nxt(), nxt(), None)


def _create(L, count, batch, agents):
    h = C.c_void_p()
    rc = L.load().tt_pop_learn_create(count, batch, agents, C.byref(h))
    return rc, L.load().tt_last_error(None).decode(), h


def _population(L, fakes):
    arr = (L.TTPopAgent * len(fakes))()
    for i, f in enumerate(fakes):
        arr[i] = f.agent
    return arr


def test_population_arguments_are_checked_before_any_hip_call(lib):
    L, B = lib, 256
    good = [_Fake(L, B) for _ in range(3)]

    def refused(count, batch, agents, words):
        rc, msg, h = _create(L, count, batch, agents)
        assert rc == L.TT_EINVAL and not h.value, (rc, msg)
        assert msg.startswith("tt_pop_learn_create") and all(w in msg for w in words), msg

    pop = _population(L, good)
    refused(0, B, pop, ["count = 0"])
    refused(17, B, pop, ["count = 17"])
    refused(3, 0, pop, ["batch = 0"])
    refused(3, 1025, pop, ["batch = 1025"])
    refused(3, B, None, ["agents is NULL"])
    # agents whose rings disagree on B (the last one is bad: the first two pass every check)
    refused(3, B, _population(L, good[:2] + [_Fake(L, B, batch=128)]), ["agent 2", "128"])
    # one missing pointer at a time
    for field, words in (("sample", ["agent 1", "sample"]), ("jobs", ["agent 1", "jobs"]), ("td", ["agent 1", "tt_td_input"])):
        bad = _Fake(L, B)
        setattr(bad.agent, field, None)
        refused(3, B, _population(L, [good[0], bad, good[2]]), words)
    bad = _Fake(L, B)
    bad.agent.tail_words = None
    refused(3, B, _population(L, [good[0], good[1], bad]), ["agent 2", "tail_words"])
    bad = _Fake(L, B)
    bad.td.step_dev = None
    refused(3, B, _population(L, [bad]), ["agent 0", "step counter"])
    bad = _Fake(L, B)
    bad.agent.critic.ws = None
    refused(3, B, _population(L, [good[0], bad, good[2]]), ["agent 1", "workspace"])
    bad = _Fake(L, B)
    bad.jobs[2].saved = None
    refused(3, B, _population(L, [good[0], bad, good[2]]), ["agent 1", "four forwards"])
    bad = _Fake(L, B)
    bad.agent.actor.count = 12
    refused(3, B, _population(L, [good[0], bad, good[2]]), ["agent 1", "optimizer step"])
    # out NULL, and the other two entry points
    assert L.load().tt_pop_learn_create(3, B, pop, None) == L.TT_EINVAL and b"out is NULL" in L.load().tt_last_error(None)
    assert L.load().tt_pop_learn(None, 0, None) == L.TT_EINVAL and b"handle is NULL" in L.load().tt_last_error(None)
    assert L.load().tt_pop_learn_destroy(None) == L.TT_OK
    assert L.load().tt_version() == 3


def test_population_python_side_refuses_what_it_does_not_support():
    from ddpg_trucktrailer_amd.population import PopulationRollout
    for kw in (dict(data_parallel=True), dict(pipeline=True), dict(side_buffer=object())):
        with pytest.raises(ValueError, match="not supported"):
            PopulationRollout(64, [1, 2], device="cpu", **kw)
    with pytest.raises(ValueError, match="1 to 16"):
        PopulationRollout(64, list(range(17)), device="cpu")
    with pytest.raises(ValueError, match="alphas"):
        PopulationRollout(64, [1, 2], alphas=[1e-4], device="cpu")
