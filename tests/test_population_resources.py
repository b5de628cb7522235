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
    bad = _Fake(L, B)
    bad.jobs[0].action = bad.sample.a_out          # an action on s' (a lone sampled launch refuses it as well)
    refused(3, B, _population(L, [good[0], bad, good[2]]), ["agent 1", "forward job 0"])
    # out NULL, and the other two entry points
    assert L.load().tt_pop_learn_create(3, B, pop, None) == L.TT_EINVAL and b"out is NULL" in L.load().tt_last_error(None)
    assert L.load().tt_pop_learn(None, 0, None) == L.TT_EINVAL and b"handle is NULL" in L.load().tt_last_error(None)
    assert L.load().tt_pop_learn_destroy(None) == L.TT_OK
    assert L.load().tt_version() == 3


def _lone_args(L, f, B):
    """The arguments of learn()'s lone entry points over f's made-up addresses, by entry point and parameter: each set would pass
    every check (and launch), so a test only ever calls them with one argument spoiled."""
    smp, ag, tb = f.sample, f.agent, [C.cast(t, C.c_void_p) for t in f.tables]
    adam = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, tau=1e-3, images=None, bias_corr=None)
    fwd = dict(n=B, count=4, jobs=f.jobs)
    rows = dict(n=B, scale_critic=2.0 / B, q_out=f.jobs[2].out, critic=C.pointer(f.w[1]), saved_critic=C.pointer(f.saved[0]),
                ws_critic=C.pointer(f.ws[0]), tdi=C.pointer(f.td), mu_out=f.jobs[3].out, actor=C.pointer(f.w[0]),
                saved_actor=C.pointer(f.saved[1]), ws_actor=C.pointer(f.ws[1]), image=None)
    critic_weights = dict(n=B, critic=1, obs=smp.s_out, action=smp.a_out, saved=C.pointer(f.saved[0]), ws=C.pointer(f.ws[0]),
                          grads=C.pointer(f.grads[0]), row_dq_da=None, row_mu=None, row_scale=1.0, count=12, params=tb[0], exp_avg=tb[1],
                          exp_avg_sq=tb[2], targets=tb[3], step_dev=f.td.step_dev, **adam)
    actor_weights = dict(critic_weights, critic=0, action=None, saved=C.pointer(f.saved[1]), ws=C.pointer(f.ws[1]),
                         grads=C.pointer(f.grads[1]), row_dq_da=ag.dq_da, row_mu=f.jobs[3].out, row_scale=-1.0 / B, count=10,
                         params=tb[4], exp_avg=tb[5], exp_avg_sq=tb[6], targets=tb[7])
    tail = dict(n=B, obs=smp.s_out, mu=f.jobs[3].out, critic=C.pointer(f.w[1]), q_out=ag.q_pi, dq_da=ag.dq_da,
                saved=C.pointer(f.saved[1]), ws=C.pointer(f.ws[1]), grads=C.pointer(f.grads[1]), row_scale=-1.0 / B, count=10,
                params=tb[4], exp_avg=tb[5], exp_avg_sq=tb[6], targets=tb[7], step_dev=f.td.step_dev, **adam, tail_words=ag.tail_words,
                gave_up_host=None)
    return {"tt_mlp_forward_multi": fwd, "tt_mlp_forward_multi_sampled": dict(fwd, sample=C.pointer(smp), k_snapshot=None),
            "tt_mlp_backward_rows_pair": rows, "tt_mlp_backward_weights": critic_weights, "actor_weights": actor_weights,
            "tt_mlp_actor_tail": tail}


def test_lone_learn_arguments_are_checked_before_any_hip_call(lib):
    L, B = lib, 256

    def refused(entry, spoil=None, **args):
        f = _Fake(L, B)
        if spoil is not None:
            spoil(f)
        a = dict(_lone_args(L, f, B)[entry], **args)
        fn = "tt_mlp_backward_weights" if entry == "actor_weights" else entry
        rc = getattr(L.load(), fn)(*a.values(), None)         # (the stream)
        assert rc == L.TT_EINVAL, (entry, args, rc)

    def setter(obj, field, value):
        return lambda f: setattr(obj(f), field, value)

    for entry in ("tt_mlp_forward_multi", "tt_mlp_forward_multi_sampled"):
        refused(entry, n=-1)
        refused(entry, jobs=None)
        refused(entry, count=0)
        refused(entry, count=5)
        refused(entry, setter(lambda f: f.jobs[0], "obs", None))
        refused(entry, setter(lambda f: f.w[2], "fc1_dims", 256))                     # a bad shape
        refused(entry, setter(lambda f: f.w[3], "wa", None))                          # a critic without its action branch
        refused(entry, setter(lambda f: f.jobs[1], "z_state", None))                  # a critic with no action, no output
        refused(entry, setter(lambda f: f.saved[1], "h1", None))                      # an incomplete tt_mlp_saved
    sampled = "tt_mlp_forward_multi_sampled"
    refused(sampled, sample=None)
    refused(sampled, n=B // 2)                                                        # not the draw's batch
    refused(sampled, setter(lambda f: f.sample, "k_dev", None))
    refused(sampled, lambda f: setattr(f.jobs[0], "obs", f.td.reward))               # a job on neither s nor s'
    refused(sampled, lambda f: setattr(f.jobs[0], "action", f.sample.a_out))         # stray actions: on s' ...
    refused(sampled, lambda f: setattr(f.jobs[1], "action", f.sample.a_out))
    refused(sampled, lambda f: setattr(f.jobs[2], "action", f.td.reward))            # ... and not the draw's a
    refused(sampled, count=2)                                                         # no job on s: no one leaves s and a

    rows = "tt_mlp_backward_rows_pair"
    refused(rows, n=0)
    refused(rows, q_out=None)
    refused(rows, mu_out=None)
    refused(rows, setter(lambda f: f.w[1], "fc2_dims", 299))
    refused(rows, setter(lambda f: f.w[0], "w3", None))
    refused(rows, saved_critic=None)
    refused(rows, setter(lambda f: f.saved[1], "rstd2", None))
    refused(rows, ws_actor=None)
    refused(rows, lambda f: setattr(f.ws[1], "dx2", f.ws[0].dx2))                    # the two nets share a workspace
    refused(rows, tdi=None)
    refused(rows, setter(lambda f: f.td, "z_state", None))
    refused(rows, setter(lambda f: f.td, "y_out", None))
    refused(rows, setter(lambda f: f.w[3], "ba", None))                               # the target critic
    refused(rows, setter(lambda f: f.td, "target_critic", None))
    refused(rows, image=C.pointer(L.TTImageJob(C.pointer(_Fake(L, B).w[0]), None)))   # an image job without its cursor

    for entry, net in (("tt_mlp_backward_weights", 0), ("actor_weights", 1)):
        refused(entry, n=0)
        refused(entry, obs=None)
        refused(entry, saved=None)
        refused(entry, ws=None)
        refused(entry, setter(lambda f: f.grads[net], "in_dim", 24))
        refused(entry, count=11)
        refused(entry, params=None)
        refused(entry, step_dev=None)
        refused(entry, lambda f: f.tables[4 * net].__setitem__(3, None))             # one parameter tensor missing
    refused("tt_mlp_backward_weights", action=None)
    refused("tt_mlp_backward_weights", row_dq_da=0x1000)                              # row factors need both arrays
    refused("actor_weights", row_mu=None)
    refused("actor_weights", n=1025)                                                  # the row factors' table holds MAXB
    tail = "tt_mlp_actor_tail"
    refused(tail, n=0)
    refused(tail, n=1025)
    for arg in ("obs", "mu", "q_out", "dq_da", "critic", "saved", "ws", "grads", "params", "step_dev", "tail_words"):
        refused(tail, **{arg: None})
    refused(tail, setter(lambda f: f.w[1], "wa", None))
    refused(tail, count=12)


def test_population_python_side_refuses_what_it_does_not_support():
    from ddpg_trucktrailer_amd.population import PopulationRollout
    for kw in (dict(data_parallel=True), dict(pipeline=True), dict(side_buffer=object())):
        with pytest.raises(ValueError, match="not supported"):
            PopulationRollout(64, [1, 2], device="cpu", **kw)
    with pytest.raises(ValueError, match="1 to 16"):
        PopulationRollout(64, list(range(17)), device="cpu")
    with pytest.raises(ValueError, match="alphas"):
        PopulationRollout(64, [1, 2], alphas=[1e-4], device="cpu")
