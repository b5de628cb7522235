"""CPU: TD3 without a GPU -- the f64 restatement (tests/td3_ref.py) against learn_ref's DDPG step in the degenerate case, the torch
path Agent(td3=...) against the restatement, the delay's bookkeeping, the host reproduction of the smoothing noise, every refusal of
TD3Config / check_td3 (one test each) and of tt_td3_create (code and message, found before any HIP call)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import learn_ref as R
import td3_ref as T


def _cfg(**kw):
    from ddpg_trucktrailer_amd.td3 import TD3Config
    return TD3Config(**kw)


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) and a.keys() == b.keys()


@pytest.mark.parametrize("c", T.ALL_CASES, ids=lambda c: f"B{c[0]}")
def test_three_net_batches_stay_inside_learn_refs_caps(c):
    state, hyper, batch, share = T.case(*c)
    assert share <= R.MAX_DISCARD and R.MAX_PASSES == 8 and R.MAX_DISCARD == 0.10
    assert (T.row_margin(state, hyper, T.default_cfg(), batch) >= R.MARGIN).all()
    assert batch[0].shape == (c[0], 23)


def test_td3_ref_with_equal_critics_no_noise_delay_one_is_learn_refs_ddpg_step_exactly():
    B = 64
    state = T.make_td3_state(T.SEED, 1.0, 0, twin_copy=True)
    state["step"] = 5
    state["actor_step"] = 5
    hyper = R.DEFAULT_HYPER
    batch = R._candidates(B, torch.Generator().manual_seed(3))
    ddpg = R.ref_step(state, batch, hyper)
    td3 = T.td3_step(state, batch, hyper, _cfg(policy_delay=1, target_noise=0.0, noise_clip=0.5), np.zeros(B), full=True)
    for key in ("y", "q", "mu", "q_pi", "dq_da"):
        assert torch.equal(ddpg[key], td3[key]), key
    assert torch.equal(td3["q"], td3["q2"]) and torch.equal(td3["q1t"], td3["q2t"])
    for net in R.NETS:
        assert _same(ddpg["nets"][net], td3["nets"][net]), net
    assert _same(td3["nets"]["critic"], td3["nets"]["critic_2"]) and _same(td3["nets"]["target_critic"], td3["nets"]["target_critic_2"])
    for key in ("m", "v"):
        for net in ("actor", "critic"):
            assert _same(ddpg[key][net], td3[key][net]), (key, net)
    assert ddpg["step"] == td3["step"] == td3["actor_step"] == 6


def _rel(got, want):
    return ((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()


def test_agent_td3_in_f64_matches_td3_ref_over_a_critic_only_and_a_full_update():
    c = T.DELAY_CASE
    state, hyper, batch, _ = T.case(*c)
    cfg, B = T.default_cfg(), c[0]
    s, a, r, s2, d = batch
    agent = T.load_td3_agent(state, hyper, cfg, torch.device("cpu"), torch.float64)
    st = state
    for upd in range(2):
        eps, _ = T.noise_eps(99, upd, B, cfg.target_noise, cfg.noise_clip)
        out = T.td3_step(st, batch, hyper, cfg, eps, full=(upd == 1))
        agent.learn_batch(s.double(), a.double(), r.double(), s2.double(), d.bool(), eps=torch.as_tensor(eps))
        for net in T.NETS:
            for k, v in getattr(agent, net).state_dict().items():
                assert _rel(v, out["nets"][net][k]) <= 1e-9, (upd, net, k)
        for net in T.TRAINED:
            mod = getattr(agent, net)
            for k, p in mod.named_parameters():
                assert _rel(mod.optimizer.state[p]["exp_avg"], out["m"][net][k]) <= 1e-9, (upd, net, k)
                assert _rel(mod.optimizer.state[p]["exp_avg_sq"], out["v"][net][k]) <= 1e-9, (upd, net, k)
        st = T.next_state(st, out)
    assert st["step"] == 2 and st["actor_step"] == 1 and agent.td3_updates == 2


def test_delay_two_leaves_actor_and_targets_alone_on_the_first_update():
    c = T.DELAY_CASE
    state, hyper, batch, _ = T.case(*c)
    cfg = T.default_cfg()
    s, a, r, s2, d = batch
    agent = T.load_td3_agent(state, hyper, cfg, torch.device("cpu"), torch.float32)
    snap = lambda: {n: {k: v.clone() for k, v in getattr(agent, n).state_dict().items()}
                    for n in ("actor", "target_actor", "target_critic", "target_critic_2")}
    opt = lambda: {k: {kk: vv.clone() for kk, vv in agent.actor.optimizer.state[p].items()} for k, p in agent.actor.named_parameters()}
    step_of = lambda net: {float(net.optimizer.state[p]["step"]) for p in net.parameters()}
    before, opt_before, critic_before = snap(), opt(), {k: v.clone() for k, v in agent.critic.state_dict().items()}
    agent.learn_batch(s, a, r, s2, d.bool())
    after = snap()
    for n in before:
        assert _same(before[n], after[n]), n
    assert all(_same(opt_before[k], v) for k, v in opt().items())
    assert step_of(agent.actor) == {0.0} and step_of(agent.critic) == step_of(agent.critic_2) == {1.0}
    assert not _same(critic_before, dict(agent.critic.state_dict()))
    agent.learn_batch(s, a, r, s2, d.bool())
    assert step_of(agent.actor) == {1.0} and step_of(agent.critic) == step_of(agent.critic_2) == {2.0}
    after = snap()
    assert not any(_same(before[n], after[n]) for n in before)


def test_without_td3_the_agent_has_four_nets_and_no_td3_state():
    agent = R.load_agent(R.make_state(3, 1.0, 0), R.DEFAULT_HYPER, torch.device("cpu"), torch.float32)
    assert agent.td3 is None and len(agent._nets()) == 4 and not hasattr(agent, "critic_2")
    td3 = T.load_td3_agent(T.make_td3_state(3, 1.0, 0), R.DEFAULT_HYPER, T.default_cfg(), torch.device("cpu"), torch.float32)
    assert [n.name for n in td3._nets()][4:] == ["critic_2", "target_critic_2"]


def test_training_checkpoint_round_trip_carries_the_second_critic(tmp_path):
    """save_training_checkpoint / load_training_checkpoint with a TD3 agent: the six nets and all three optimizers' state come back
    bit for bit; a checkpoint written without TD3 is refused by a TD3 agent, and a TD3 checkpoint by a plain agent."""
    from ddpg_trucktrailer_amd import checkpoint
    state, hyper, batch, _ = T.case(*T.DELAY_CASE)
    cfg, cpu = T.default_cfg(), torch.device("cpu")
    s, a, r, s2, d = batch
    agent = T.load_td3_agent(state, hyper, cfg, cpu, torch.float32)
    for _ in range(2):
        agent.learn_batch(s, a, r, s2, d.bool())
    path = checkpoint.save_training_checkpoint(str(tmp_path / "td3.pt"), agent)
    other = T.load_td3_agent(T.make_td3_state(T.SEED + 5, 1.0, 0), hyper, cfg, cpu, torch.float32)
    checkpoint.load_training_checkpoint(path, other)
    for n in T.NETS:
        assert _same(dict(getattr(agent, n).state_dict()), dict(getattr(other, n).state_dict())), n
    for n in T.TRAINED:
        for p, q in zip(getattr(agent, n).parameters(), getattr(other, n).parameters()):
            sa, sb = getattr(agent, n).optimizer.state[p], getattr(other, n).optimizer.state[q]
            assert float(sa["step"]) == float(sb["step"]) and torch.equal(sa["exp_avg"], sb["exp_avg"]) \
                and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), n
    plain = R.load_agent(R.make_state(3, 1.0, 0), hyper, cpu, torch.float32)
    with pytest.raises(ValueError, match="td3"):
        checkpoint.load_training_checkpoint(path, plain)
    plain_path = checkpoint.save_training_checkpoint(str(tmp_path / "plain.pt"), plain)
    with pytest.raises(ValueError, match="td3"):
        checkpoint.load_training_checkpoint(plain_path, other)


def test_torch_path_noise_follows_the_seed_and_its_state_can_be_restored():
    state, hyper, batch, _ = T.case(*T.DELAY_CASE)
    cfg, cpu = T.default_cfg(), torch.device("cpu")
    s, a, r, s2, d = batch

    def run(seed, updates, resume=None):
        agent = T.load_td3_agent(state, hyper, cfg, cpu, torch.float32)
        agent.seed_td3_noise(seed)
        if resume is not None:
            agent.set_td3_noise_state(resume)
        for _ in range(updates):
            agent.learn_batch(s, a, r, s2, d.bool())
        return agent
    one, again, other = run(5, 1), run(5, 1), run(6, 1)
    flat = lambda ag: torch.cat([p.detach().reshape(-1) for p in ag.critic.parameters()])
    assert torch.equal(flat(one), flat(again)) and not torch.equal(flat(one), flat(other))
    # the generator's state after one update, restored into an agent seeded otherwise, gives the second update's noise
    two = run(5, 2)
    nrm_two = torch.randn(4, generator=two._td3_gen)
    resumed = run(99, 0, resume=one.td3_noise_state())
    resumed.learn_batch(s, a, r, s2, d.bool())
    assert torch.equal(torch.randn(4, generator=resumed._td3_gen), nrm_two)


# ---- the noise ------------------------------------------------------------------------------------------------------
def test_numpy_philox_reproduces_the_known_answer_vectors():
    """Philox4x32-10 known answers (Random123's kat_vectors): zeros; all ones; the digits of pi."""
    word = lambda xs: [int(x) for x in xs]
    assert word(T.philox4x32(0, 0, 0, 0, 0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xffffffff
    assert word(T.philox4x32(f, f, f, f, f, f)) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert word(T.philox4x32(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_host_noise_is_clipped_keyed_by_step_and_seed_and_standard_normal():
    n = 8192
    eps, nrm = T.noise_eps(5, 3, n, 0.2, 0.5)
    assert np.abs(eps).max() <= float(np.float32(0.5)) and np.isfinite(nrm).all()
    assert np.array_equal(eps, T.noise_eps(5, 3, n, 0.2, 0.5)[0])
    assert not np.array_equal(eps, T.noise_eps(5, 4, n, 0.2, 0.5)[0]) and not np.array_equal(eps, T.noise_eps(6, 3, n, 0.2, 0.5)[0])
    assert abs(nrm.mean()) <= 5 / math.sqrt(n) and abs(nrm.var() - 1) <= 5 * math.sqrt(2 / n)


# ---- refusals: TD3Config and check_td3, one test per refused combination ------------------------------------------------
@pytest.mark.parametrize("kw, word", [(dict(policy_delay=0), "policy_delay"), (dict(policy_delay=1.5), "policy_delay"),
                                      (dict(policy_delay=True), "policy_delay"), (dict(target_noise=-0.1), "target_noise"),
                                      (dict(target_noise=float("nan")), "target_noise"), (dict(noise_clip=-1.0), "noise_clip"),
                                      (dict(noise_clip=float("inf")), "noise_clip")])
def test_td3_config_refuses(kw, word):
    with pytest.raises(ValueError, match=word):
        _cfg(**kw)


def test_td3_config_defaults():
    assert _cfg().as_tuple() == (2, 0.2, 0.5) and _cfg() == _cfg(policy_delay=2)


@pytest.mark.parametrize("kw, word", [(dict(updates_per_step=1), "updates_per_step"), (dict(updates_per_step=3), "updates_per_step"),
                                      (dict(updates_per_step=2, n_step=3), "n_step"),
                                      (dict(updates_per_step=2, data_parallel=True), "data_parallel"),
                                      (dict(updates_per_step=2, pipeline=True), "pipeline"),
                                      (dict(updates_per_step=2, learn_log=128), "learn_log")])
def test_check_td3_refuses(kw, word):
    from ddpg_trucktrailer_amd.td3 import check_td3
    with pytest.raises(ValueError, match=word):
        check_td3(_cfg(), **kw)


def test_check_td3_accepts_the_supported_loop_and_refuses_a_non_config():
    from ddpg_trucktrailer_amd.td3 import check_td3
    cfg = _cfg()
    assert check_td3(cfg, updates_per_step=4, n_step=1, data_parallel=False, pipeline=None, learn_log=None) is cfg
    assert check_td3(cfg, updates_per_step=2, pipeline=False) is cfg
    with pytest.raises(ValueError, match="TD3Config"):
        check_td3((2, 0.2, 0.5), updates_per_step=2)


# ---- refusals of tt_td3_create ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib as L
    return L


class _Fake:
    """A plausible TD3 agent description over made-up device addresses: the library checks it on the host, and with one bad
    argument nothing reaches the GPU."""

    def __init__(self, L, B):
        addr = iter(range(0x10000, 0x10000 + 0x1000 * 600, 0x1000))
        nxt = lambda: next(addr)
        # actor, critic, target actor, target critic, critic 2, target critic 2
        self.w = [L.TTMlpWeights(*[nxt() for _ in range(12)], 23, 400, 300) for _ in range(6)]
        self.side = L.TTSideBuffer(nxt(), nxt(), nxt(), nxt(), nxt(), 4, 0)
        self.sample = L.TTSampleArgs(B, 1024, 8, 0, nxt(), nxt(), nxt(), nxt(), nxt(), 5, None, nxt(), nxt(), nxt(), nxt(), nxt(), None,
                                     0, 1, 77, None)
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
                              reward=smp.r_out, done=smp.d_out, gamma=0.99,
                              y_out=nxt(), q_out=nxt(), step_dev=nxt(), window_dev=None, bias_corr_out=nxt(), adam_beta1=0.9,
                              adam_beta2=0.999)
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


def test_td3_create_arguments_are_checked_before_any_hip_call(lib):
    L, B = lib, 256

    def refused(words, spoil=None, batch=B, agent=True):
        f = _Fake(L, B)
        if spoil is not None:
            spoil(f)
        h = C.c_void_p()
        rc = L.load().tt_td3_create(batch, C.byref(f.agent) if agent else None, C.byref(h))
        msg = L.load().tt_last_error(None).decode()
        assert rc == L.TT_EINVAL and not h.value, (rc, msg)
        assert msg.startswith("tt_td3_create") and all(w in msg for w in words), msg

    def setter(obj, field, value):
        return lambda f: setattr(obj(f), field, value)

    refused(["batch = 0"], batch=0)
    refused(["batch = 1025"], batch=1025)
    refused(["agent is NULL"], agent=False)
    refused(["target_noise"], setter(lambda f: f.agent, "target_noise", -0.1))
    refused(["target_noise"], setter(lambda f: f.agent, "target_noise", float("nan")))
    refused(["noise_clip"], setter(lambda f: f.agent, "noise_clip", -0.5))
    refused(["noise_clip"], setter(lambda f: f.agent, "noise_clip", float("inf")))
    refused(["sample"], setter(lambda f: f.agent, "sample", None))
    refused(["128"], batch=128)                                                       # not the draw's batch
    refused(["draws"], setter(lambda f: f.sample, "draws", 2))
    refused(["step_progress"], setter(lambda f: f.sample, "step_progress", 0x5000))
    refused(["side buffer"], lambda f: setattr(f.sample, "side", C.pointer(f.side)))
    refused(["tt_sample_args"], setter(lambda f: f.sample, "k_dev", None))
    refused(["jobs is NULL"], setter(lambda f: f.agent, "jobs", None))
    refused(["six forwards"], setter(lambda f: f.jobs[2], "z_state", None))
    refused(["six forwards"], setter(lambda f: f.jobs[4], "saved", None))
    refused(["forward job 3"], setter(lambda f: f.w[1], "wa", None))
    refused(["tt_td_input"], setter(lambda f: f.agent, "td", None))
    refused(["tt_td_input"], setter(lambda f: f.td, "step_dev", None))
    refused(["tt_td_input"], setter(lambda f: f.td, "q_out", None))
    refused(["window_dev"], setter(lambda f: f.td, "window_dev", 0x7000))
    # the parts of the description must belong together
    refused(["z_state", "jobs 1 and 2"], setter(lambda f: f.td, "z_state", 0x9000))
    refused(["z_state", "jobs 1 and 2"], setter(lambda f: f.agent, "z_state_2", 0x9000))
    refused(["mu_target", "job 0"], setter(lambda f: f.td, "mu_target", 0x9000))
    refused(["r_out"], setter(lambda f: f.td, "reward", 0x9000))
    refused(["d_out"], setter(lambda f: f.td, "done", 0x9000))
    refused(["target_critic", "jobs 1 and 2"], lambda f: setattr(f.td, "target_critic", C.pointer(f.w[1])))
    refused(["target_critic", "jobs 1 and 2"], lambda f: setattr(f.agent, "target_critic_2", C.pointer(f.w[3])))
    refused(["target_critic_2"], setter(lambda f: f.agent, "target_critic_2", None))
    refused(["z_state_2"], setter(lambda f: f.agent, "z_state_2", None))
    for field in ("eps_out", "y2_out", "q2t_out", "step_snapshot", "actor_step_dev", "actor_bias_corr_out", "q_pi", "dq_da",
                  "tail_words"):
        refused([field], setter(lambda f: f.agent, field, None))
    refused(["workspace"], setter(lambda f: f.agent.critic_2, "ws", None))
    refused(["share a per-row workspace"], lambda f: setattr(f.ws[1], "dx2", f.ws[0].dx2))
    refused(["share a per-row workspace"], lambda f: setattr(f.ws[2], "dx2", f.ws[1].dx2))
    refused(["share a gradient buffer"], lambda f: setattr(f.grads[1], "w1", f.grads[0].w1))
    refused(["network 1", "gradient buffers"], setter(lambda f: f.agent.critic_2, "grads", None))
    refused(["network 2", "optimizer step"], setter(lambda f: f.agent.actor, "count", 12))
    refused(["network 1", "optimizer step"], lambda f: f.tables[4].__setitem__(3, None))
    lib_ = L.load()
    f = _Fake(L, B)
    assert lib_.tt_td3_create(B, C.byref(f.agent), None) == L.TT_EINVAL and b"out is NULL" in lib_.tt_last_error(None)
    assert lib_.tt_td3_learn(None, 0, 1, None) == L.TT_EINVAL and b"handle is NULL" in lib_.tt_last_error(None)
    assert lib_.tt_td3_update(None, C.byref(f.agent)) == L.TT_EINVAL and b"handle is NULL" in lib_.tt_last_error(None)
    assert lib_.tt_td3_destroy(None) == L.TT_OK
