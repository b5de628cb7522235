"""CPU: TD3 for populations (csrc/ttpop_td3.hip, include/ttenv.h: tt_pop_td3_*, td3.PopulationTD3Learner) without a GPU -- its
kernels exist in libttenv.so with the budgets of the lone TD3 launches they wrap, every bad argument of its C ABI is TT_EINVAL with a
message that names the entry point and the agent, found before any HIP call, the lone tt_td3_create keeps its messages, and
PopulationRollout(td3=...) names every option it refuses."""
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


# ---- kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", ["k_pop_td3_fwd_multi", "k_pop_td3_bwd_rows", "k_pop_td3_actor_tail"])
def test_population_td3_row_kernels_keep_two_waves_per_simd(ks, part):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    n, v = _one(ks, part)
    assert v["max_threads"] == 512 and kr.waves_per_simd(v["vgpr"]) >= 2, (n, v)
    assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and v["lds"] <= 160 * 1024, (n, v)


def test_population_td3_weight_kernel_fits_three_workgroups_per_cu(ks):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    n, v = _one(ks, "k_pop_td3_bwd_weights")
    assert v["vgpr"] <= 168 and kr.waves_per_simd(v["vgpr"]) >= 3, (n, v)
    assert v["scratch"] == 0 and v["vgpr_spills"] == 0 and 3 * v["lds"] <= 160 * 1024, (n, v)


def test_population_td3_exploit_kernel_has_no_scratch(ks):
    n, v = _one(ks, "k_pop_td3_exploit")
    assert v["scratch"] == 0 and v["vgpr_spills"] == 0, (n, v)


def test_new_kernels_leave_every_name_search_of_the_existing_tests_alone(ks):
    assert len([n for n in ks if "k_td3_" in n]) == 4
    for part in ("15k_td3_fwd_multi", "14k_td3_bwd_rows", "17k_td3_bwd_weights", "16k_td3_actor_tail", "15k_pop_fwd_multi",
                 "19k_pop_bwd_rows_pair", "16k_pop_actor_tail", "17k_pop_bwd_weightsILb0E"):
        _one(ks, part)
    assert len([n for n in ks if "k_pop_td3_" in n]) == 5


# ---- refusals of tt_pop_td3_create ------------------------------------------------------------------------------------
class _Fake:
    """A plausible TD3 agent description over made-up device addresses (tests/test_population_resources.py's _Fake with TD3's six
    jobs and three trained networks): the library checks it on the host, and with one bad argument in the population nothing reaches
    the GPU.  index: the agent's place in the population -- every agent has addresses of its own."""

    def __init__(self, L, B, index=0, batch=None):
        base = 0x10000 + 0x1000000 * index
        addr = iter(range(base, base + 0x1000 * 600, 0x1000))
        nxt = lambda: next(addr)
        # actor, critic, target actor, target critic, critic 2, target critic 2
        self.w = [L.TTMlpWeights(*[nxt() for _ in range(12)], 23, 400, 300) for _ in range(6)]
        self.sample = L.TTSampleArgs(B if batch is None else batch, 1024, 8, 0, nxt(), nxt(), nxt(), nxt(), nxt(), 5, None, nxt(), nxt(),
                                     nxt(), nxt(), nxt(), None, 0, 1, 77, None)
        smp = self.sample
        self.saved = [L.TTMlpSaved(*[nxt() for _ in range(6)]) for _ in range(3)]
        self.jobs = (L.TTFwdJob * 6)()
        for j, (wi, crit, obs, act, out, saved, z) in enumerate(((2, 0, smp.s2_out, None, nxt(), None, None),
                                                                 (3, 1, smp.s2_out, None, None, None, nxt()),
                                                                 (5, 1, smp.s2_out, None, None, None, nxt()),
                                                                 (1, 1, smp.s_out, smp.a_out, nxt(), self.saved[0], None),
                                                                 (4, 1, smp.s_out, smp.a_out, nxt(), self.saved[1], None),
                                                                 (0, 0, smp.s_out, None, nxt(), self.saved[2], None))):
            self.jobs[j].critic, self.jobs[j].obs, self.jobs[j].action = crit, obs, act
            self.jobs[j].w, self.jobs[j].out = C.pointer(self.w[wi]), out
            self.jobs[j].saved = C.pointer(saved) if saved is not None else None
            self.jobs[j].z_state = z
        self.td = L.TTTdInput(z_state=self.jobs[1].z_state, mu_target=self.jobs[0].out, target_critic=C.pointer(self.w[3]),
                              reward=smp.r_out, done=smp.d_out, gamma=0.99, y_out=nxt(), q_out=nxt(), step_dev=nxt(), window_dev=None,
                              bias_corr_out=nxt(), adam_beta1=0.9, adam_beta2=0.999)
        self.ws = [L.TTMlpBwdWs(*[nxt() for _ in range(5)]) for _ in range(3)]
        self.grads = [L.TTMlpWeights(*[nxt() for _ in range(12)], 23, 400, 300) for _ in range(3)]
        self.tables = [(C.c_void_p * 12)(*[nxt() for _ in range(12)]) for _ in range(12)]
        nets = []
        for i, count in enumerate((12, 12, 10)):
            p, m, v, t = self.tables[4 * i:4 * i + 4]
            nets.append(L.TTPopNet(C.pointer(self.ws[i]), C.pointer(self.grads[i]), count, 0, C.cast(p, C.c_void_p), C.cast(m, C.c_void_p),
                                   C.cast(v, C.c_void_p), C.cast(t, C.c_void_p), 1e-3, 0.9, 0.999, 1e-8, 0.01, 1e-3, None))
        self.agent = L.TTTd3Agent(C.pointer(self.sample), self.jobs, C.pointer(self.td), nets[0], nets[1], nets[2], self.jobs[2].z_state,
                                  C.pointer(self.w[5]), 0.2, 0.5, 9, nxt(), nxt(), nxt(), nxt(), nxt(), nxt(), nxt(), nxt(), nxt(), None)


def _population(L, fakes):
    arr = (L.TTTd3Agent * len(fakes))()
    for i, f in enumerate(fakes):
        arr[i] = f.agent
    return arr


def test_population_td3_create_arguments_are_checked_before_any_hip_call(lib):
    L, B = lib, 256
    good = [_Fake(L, B, a) for a in range(3)]

    def refused(count, batch, agents, words):
        h = C.c_void_p()
        rc = L.load().tt_pop_td3_create(count, batch, agents, C.byref(h))
        msg = L.load().tt_last_error(None).decode()
        assert rc == L.TT_EINVAL and not h.value, (rc, msg)
        assert msg.startswith("tt_pop_td3_create") and all(w in msg for w in words), msg

    def with_bad(place, spoil, **kw):
        bad = _Fake(L, B, place, **kw)
        if spoil is not None:
            spoil(bad)
        return _population(L, [bad if a == place else good[a] for a in range(3)]), bad

    pop = _population(L, good)
    refused(0, B, pop, ["count = 0"])
    refused(17, B, pop, ["count = 17"])
    refused(3, 0, pop, ["batch = 0"])
    refused(3, 1025, pop, ["batch = 1025"])
    refused(3, B, None, ["agents is NULL"])
    assert L.load().tt_pop_td3_create(3, B, pop, None) == L.TT_EINVAL and b"tt_pop_td3_create: out is NULL" in L.load().tt_last_error(None)
    # one agent with another batch: the first two pass every check
    arr, keep = with_bad(2, None, batch=128)
    refused(3, B, arr, ["agent 2", "128"])
    # one missing pointer at a time
    for place, obj, field, words in ((1, lambda f: f.agent, "sample", ["agent 1", "sample"]),
                                     (1, lambda f: f.agent, "jobs", ["agent 1", "jobs"]),
                                     (0, lambda f: f.agent, "td", ["agent 0", "tt_td_input"]),
                                     (2, lambda f: f.agent, "z_state_2", ["agent 2", "z_state_2"]),
                                     (2, lambda f: f.agent, "tail_words", ["agent 2", "tail_words"]),
                                     (1, lambda f: f.agent, "target_noise", ["agent 1", "target_noise"])):
        arr, keep = with_bad(place, lambda f: setattr(obj(f), field, -0.1 if field == "target_noise" else None))
        refused(3, B, arr, words)
    # what two agents may not share
    arr, keep = with_bad(2, lambda f: setattr(f.td, "step_dev", good[0].td.step_dev))
    refused(3, B, arr, ["agents 0 and 2", "step counter"])
    arr, keep = with_bad(1, lambda f: setattr(f.agent, "actor_step_dev", good[0].agent.actor_step_dev))
    refused(3, B, arr, ["agents 0 and 1", "step counter"])
    arr, keep = with_bad(2, lambda f: setattr(f.agent, "tail_words", good[1].agent.tail_words))
    refused(3, B, arr, ["agents 1 and 2", "tail words"])
    arr, keep = with_bad(1, lambda f: setattr(f.ws[2], "dx2", good[0].ws[1].dx2))
    refused(3, B, arr, ["agents 0 and 1", "per-row workspace"])
    arr, keep = with_bad(2, lambda f: setattr(f.grads[0], "w1", good[0].grads[2].w1))
    refused(3, B, arr, ["agents 0 and 2", "gradient buffer"])


def test_the_other_population_td3_entry_points_refuse_before_any_hip_call(lib):
    dll = lib.load()
    err = lambda: dll.tt_last_error(None)
    assert dll.tt_pop_td3_learn(None, 0, 1, None) == lib.TT_EINVAL and b"tt_pop_td3_learn: handle is NULL" in err()
    pair = (lib.TTPopTd3Pair * 1)(lib.TTPopTd3Pair(0, 0, 1e-4, 1e-3, 1e-3, 0.99, 0.2, 0.5))
    assert dll.tt_pop_td3_exploit(None, 1, pair, None) == lib.TT_EINVAL and b"tt_pop_td3_exploit: handle is NULL" in err()
    out = (C.c_float * 6)()
    assert dll.tt_pop_td3_hyper(None, 0, C.byref(out)) == lib.TT_EINVAL and b"tt_pop_td3_hyper: handle is NULL" in err()
    assert dll.tt_pop_td3_destroy(None) == lib.TT_OK
    assert dll.tt_version() == 3


def test_update_below_zero_is_refused_without_a_launch(lib):
    """tt_pop_td3_learn looks at `update` before it looks at the handle, so the refusal can be seen without a handle (and a GPU)."""
    dll = lib.load()
    assert dll.tt_pop_td3_learn(None, -1, 0, None) == lib.TT_EINVAL
    assert dll.tt_last_error(None) == b"tt_pop_td3_learn: update = -1 < 0"


def test_lone_td3_create_keeps_its_messages(lib):
    """The lone entry point shares to_td3_agent with the population's: its messages are the ones it had before the move
    (literal strings of csrc/tttd3.hip as it was)."""
    L, B = lib, 256
    dll = L.load()

    def message(spoil, batch=B):
        f = _Fake(L, B)
        spoil(f)
        h = C.c_void_p()
        assert dll.tt_td3_create(batch, C.byref(f.agent), C.byref(h)) == L.TT_EINVAL and not h.value
        return dll.tt_last_error(None).decode()

    assert message(lambda f: setattr(f.agent, "sample", None)) == "tt_td3_create: sample (tt_sample_args) is NULL"
    assert message(lambda f: None, batch=128) == "tt_td3_create: the sample draws batches of 256 rows, not batch = 128"
    assert message(lambda f: setattr(f.ws[1], "dx2", f.ws[0].dx2)) == "tt_td3_create: two networks share a per-row workspace"
    assert message(lambda f: setattr(f.agent, "target_noise", -0.5)) == "tt_td3_create: target_noise = -0.5 is negative or not finite"
    assert message(lambda f: setattr(f.agent.actor, "count", 12)) == "tt_td3_create: network 2 has an incomplete optimizer step"


# ---- Python refusals ------------------------------------------------------------------------------------------------
def _cfg(**kw):
    from ddpg_trucktrailer_amd.td3 import TD3Config
    return TD3Config(**kw)


@pytest.mark.parametrize("kw, word", [(dict(updates_per_step=1), "updates_per_step"), (dict(updates_per_step=3), "updates_per_step"),
                                      (dict(updates_per_step=2, n_step=3), "n_step"),
                                      (dict(updates_per_step=2, n_step=[1, 2]), "n_step"),
                                      (dict(updates_per_step=2, n_step_max=2), "n_step_max"),
                                      (dict(updates_per_step=2, learn_log=128), "learn_log"),
                                      (dict(updates_per_step=2), "device")])
def test_population_rollout_with_td3_refuses(kw, word):
    """Built with device="cpu": every check precedes any GPU use, and the CPU device itself is the last refusal."""
    from ddpg_trucktrailer_amd.population import PopulationRollout
    with pytest.raises(ValueError, match="td3: .*" + word):
        PopulationRollout(64, [1, 2], device="cpu", replay_slots=8, td3=_cfg(), **kw)


def test_population_rollout_refuses_td3_lists_it_cannot_run():
    from ddpg_trucktrailer_amd.population import PopulationRollout
    with pytest.raises(ValueError, match="policy_delay"):
        PopulationRollout(64, [1, 2], device="cpu", updates_per_step=2, td3=[_cfg(policy_delay=2), _cfg(policy_delay=1)])
    with pytest.raises(ValueError, match="td3: 3 configurations for 2 agents"):
        PopulationRollout(64, [1, 2], device="cpu", updates_per_step=2, td3=[_cfg()] * 3)
    with pytest.raises(ValueError, match="TD3Config"):
        PopulationRollout(64, [1, 2], device="cpu", updates_per_step=2, td3=(2, 0.2))


def test_check_population_td3_accepts_the_supported_population():
    from ddpg_trucktrailer_amd.td3 import check_population_td3, same_policy_delay
    cfgs = check_population_td3([_cfg(target_noise=0.1), _cfg(noise_clip=0.05), _cfg()], 3, updates_per_step=4)
    assert [c.as_tuple() for c in cfgs] == [(2, 0.1, 0.5), (2, 0.2, 0.05), (2, 0.2, 0.5)] and same_policy_delay(cfgs) == 2
    one = _cfg(policy_delay=1)
    assert check_population_td3(one, 2, updates_per_step=1) == [one, one]


def test_without_td3_the_population_refuses_as_before():
    from ddpg_trucktrailer_amd.population import PopulationRollout
    with pytest.raises(ValueError, match="1 to 16"):
        PopulationRollout(64, list(range(17)), device="cpu")
