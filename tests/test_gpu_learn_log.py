"""GPU (-m gpu): the learn log (csrc/ttlearnlog.hip: k_learn_log; include/ttenv.h: tt_learn_log_*) -- a record per learn() update with
the losses, the Q / TD-target / dQ/da / mu statistics, both gradient norms and a non-finite count, reduced on the device.

  1  a record is the f64 reduction of the buffers learn() left (numpy on the host), at B = 1, 250, 257, 1024 and at trained scale
  2  its two losses are THIS update's: against learn() in f64 (tests/learn_ref.py), within what the output bounds of
     tests/test_gpu_learn_shapes.py already imply
  3  every row and every gradient element is counted, once: planted integers, 3-4-5 and 5-12-13 norms, planted NaN / inf
  4  ring, stride, drain cursor, dropped, clear on load_state_dict
  5  the vector loop: graph replays == eager launches record for record, and the log changes no result of the loop
  6  a population's records are each agent's lone records, bit for bit

States and batches: learn_ref.case (shared with tests/test_gpu_learn_shapes.py, made once per process)."""
import math

import numpy as np
import pytest

import learn_ref as R
from learn_checks import ring_with_batch as _ring_with_batch
from test_gpu_learn_shapes import _learner

pytestmark = pytest.mark.gpu

TRAINED_1024 = (1024, 20.0, 3, 999, "trained", 7)
RECORD_CASES = [c for c in R.FRESH_CASES if c[0] in (1, 250, 257, 1024)] + [TRAINED_1024]
LOSS_CASES = [c for c in R.FRESH_CASES if c[0] in (1, 257)]
ROWS = ("y", "q", "q_pi", "dq_da", "mu")


def _id(case):
    return "B{}-x{:g}".format(case[0], case[1])


def _columns():
    from ddpg_trucktrailer_amd import _lib as L
    return ("step", "nonfinite") + L.LEARN_LOG_VALUES


def _same_records(a, b):
    """Two drains hold the same records, bit for bit (NaN included)."""
    for k in _columns():
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].tobytes() == b[k].tobytes(), (k, a[k], b[k])


_ONE_UPDATE = {}


def _one_update(dev, case):
    """One learn_batch of the case with the log on (capacity 4, fc2 images on): the drained records, the host copies of the five row
    buffers and both flat gradients as f64, and the critic's state_dict as learn() left it.  Made once per case."""
    import torch
    if case not in _ONE_UPDATE:
        agent, fl, batch = _learner(dev, case, True)
        fl.enable_learn_log(4)
        fl.learn_batch(*batch)
        rec = fl.drain_learn_log()
        host = {n: getattr(fl, n).cpu().numpy().astype(np.float64) for n in ROWS}
        host["grad_critic"] = fl.critic.flat_grad.cpu().numpy().astype(np.float64)
        host["grad_actor"] = fl.actor.flat_grad.cpu().numpy().astype(np.float64)
        critic = {k: v.detach().cpu().clone() for k, v in agent.critic.state_dict().items()}
        assert int(fl.step_dev.item()) == case[3] + 1
        _ONE_UPDATE[case] = (rec, host, critic, batch[0].double().cpu())
        torch.cuda.synchronize()
    return _ONE_UPDATE[case]


@pytest.mark.parametrize("case", RECORD_CASES, ids=_id)
def test_record_is_the_f64_reduction_of_what_learn_left(gpu_device, case):
    """step, every min and max and the non-finite count exactly; a mean or loss of N terms t_i within (N + 2) 2^-52 sum |t_i| / N --
    (N - 1) 2^-53 is the first-order bound of ANY order of summation, two roundings per term and the last division fit into the
    factor 2; a norm over N elements within (N + 2) 2^-52 of itself."""
    B = case[0]
    rec, h, _, _ = _one_update(gpu_device, case)
    assert rec["step"].tolist() == [case[3] + 1] and rec["nonfinite"].tolist() == [0] and rec["dropped"] == 0
    y, q, q_pi, dq, mu = (h[n] for n in ROWS)
    assert all(x.shape == (B,) for x in (y, q, q_pi, dq, mu))
    got = {k: float(rec[k][0]) for k in rec if k not in ("step", "nonfinite", "dropped")}
    exact = dict(q_min=q.min(), q_max=q.max(), y_min=y.min(), y_max=y.max(), td_abs_max=np.abs(y - q).max(),
                 dq_da_abs_max=np.abs(dq).max())
    for k, want in exact.items():
        print(f"{_id(case)} {k}: got {got[k]!r} want {float(want)!r}")
        assert got[k] == float(want), k
    means = dict(critic_loss=(q - y) ** 2, actor_loss=-q_pi, q_mean=q, y_mean=y, td_abs_mean=np.abs(y - q), dq_da_abs_mean=np.abs(dq),
                 mu_abs_mean=np.abs(mu), gate_mean=1.0 - mu * mu)
    for k, t in means.items():
        want, tol = math.fsum(t) / B, (B + 2) * 2.0 ** -52 * math.fsum(np.abs(t)) / B
        print(f"{_id(case)} {k}: got {got[k]!r} want {want!r} |err| {abs(got[k] - want):.3g} tol {tol:.3g}")
        assert abs(got[k] - want) <= tol, k
    if B == 1:
        assert got["q_min"] == got["q_max"] == got["q_mean"] and got["y_min"] == got["y_max"] == got["y_mean"]
        assert got["td_abs_mean"] == got["td_abs_max"] and got["dq_da_abs_mean"] == got["dq_da_abs_max"]
    for k in ("grad_norm_critic", "grad_norm_actor"):
        g = h[k.replace("grad_norm", "grad")]
        assert g.size == (132201 if k.endswith("critic") else 131601)
        want = math.sqrt(math.fsum(g * g))
        tol = (g.size + 2) * 2.0 ** -52 * want
        print(f"{_id(case)} {k}: got {got[k]!r} want {want!r} |err| {abs(got[k] - want):.3g} tol {tol:.3g}")
        assert want > 0 and abs(got[k] - want) <= tol, k
    assert set(got) == set(means) | set(exact) | {"grad_norm_critic", "grad_norm_actor"}


@pytest.mark.parametrize("case", LOSS_CASES, ids=_id)
def test_losses_are_this_updates(gpu_device, case):
    """critic_loss against mean (q64 - y64)^2 and actor_loss against -mean q_pi64 of learn() in f64.  With d = max |q64 - y64| and
    e = 2e-5 (max(1, max |y64|) + max(1, max |q64|)) -- the sum of the bounds test_one_learn_step_against_f64 holds y and q to --
    every term (q - y)^2 is within 2 d e + e^2 of its f64 twin, and so is the mean; q_pi64 is Q(s, mu(s)) in f64 on the critic this
    learn() left (learn_ref's docstring says why), and every q_pi is within 2e-5 max(1, max |q_pi64|) of it."""
    import torch
    rec, _, critic, s64 = _one_update(gpu_device, case)
    state, hyper, _, ref, _ = R.case(*case)
    y64, q64 = ref["y"].numpy(), ref["q"].numpy()
    d = np.abs(q64 - y64).max()
    e = 2e-5 * (max(1.0, np.abs(y64).max()) + max(1.0, np.abs(q64).max()))
    mse64 = float(np.mean((q64 - y64) ** 2))
    got = float(rec["critic_loss"][0])
    print(f"{_id(case)} critic_loss: got {got!r} f64 {mse64!r} |err| {abs(got - mse64):.3g} tol {2 * d * e + e * e:.3g}")
    assert abs(got - mse64) <= 2 * d * e + e * e
    a64 = R.load_agent(dict(state, nets=dict(state["nets"], critic=critic)), hyper, torch.device("cpu"), torch.float64)
    q_pi64 = R.actor_half(a64.critic, a64.actor, s64)["q_pi"].numpy()
    got, tol = float(rec["actor_loss"][0]), 2e-5 * max(1.0, np.abs(q_pi64).max())
    print(f"{_id(case)} actor_loss: got {got!r} f64 {-float(q_pi64.mean())!r} |err| {abs(got + float(q_pi64.mean())):.3g} tol {tol:.3g}")
    assert abs(got + float(q_pi64.mean())) <= tol


def test_every_element_is_counted_once(gpu_device):
    """Planted data, the append alone (FusedLearner.append_learn_log).  Rows: q = 0, 1, .. B - 1 against y = 0 and friends, whose
    sums are exact in f64, so every statistic is exact -- a row dropped, or counted twice, moves them.  Gradients: zero but for the
    first and the last element (3, 4 and 5, 12: norms exactly 5 and 13 -- the ragged tail is covered), then all ones (norm exactly
    sqrt(numel): no chunk twice).  Then one NaN in y[B - 1], one inf in dq_da[0], one NaN in each gradient's last element: nonfinite
    = 4.  Plants are data: nothing faults."""
    import torch
    dev = gpu_device
    B = 257
    _, fl, _ = _learner(dev, R.FRESH_CASES[2], True)
    assert fl.B == B
    fl.enable_learn_log(4)
    i = torch.arange(B, dtype=torch.float32, device=dev)
    fl.y.zero_()
    fl.q.copy_(i)
    fl.q_pi.copy_(2 * i - 7)
    fl.dq_da.copy_(torch.where(i % 2 == 0, -i, i))
    fl.mu.copy_((i - 128) / 256)
    for st, (first, last) in ((fl.critic, (3.0, 4.0)), (fl.actor, (5.0, 12.0))):
        st.flat_grad.zero_()
        st.flat_grad[0], st.flat_grad[-1] = first, last
    fl.step_dev.fill_(1)
    fl.append_learn_log()
    for st in (fl.critic, fl.actor):
        st.flat_grad.fill_(1.0)
    fl.step_dev.fill_(2)
    fl.append_learn_log()
    fl.y[B - 1] = float("nan")
    fl.dq_da[0] = float("inf")
    fl.critic.flat_grad[-1] = float("nan")
    fl.actor.flat_grad[-1] = float("nan")
    fl.step_dev.fill_(3)
    fl.append_learn_log()
    rec = fl.drain_learn_log()
    assert rec["step"].tolist() == [1, 2, 3] and rec["nonfinite"].tolist() == [0, 0, 4] and rec["dropped"] == 0
    assert rec["grad_norm_critic"][0] == 5.0 and rec["grad_norm_actor"][0] == 13.0
    assert rec["grad_norm_critic"][1] == math.sqrt(132201) and rec["grad_norm_actor"][1] == math.sqrt(131601)
    n = np.arange(B, dtype=np.float64)
    mu = (n - 128) / 256
    want = dict(critic_loss=(n * n).sum() / B, actor_loss=-((2 * n - 7).sum() / B), q_mean=n.sum() / B, q_min=0.0, q_max=B - 1.0,
                y_mean=0.0, y_min=0.0, y_max=0.0, td_abs_mean=n.sum() / B, td_abs_max=B - 1.0, dq_da_abs_mean=n.sum() / B,
                dq_da_abs_max=B - 1.0, mu_abs_mean=np.abs(mu).sum() / B, gate_mean=(1.0 - mu * mu).sum() / B)
    for k, w in want.items():
        for r in (0, 1):                                         # (the rows were the same for the first two appends)
            assert rec[k][r] == w, (k, r, rec[k][r], w)
    torch.cuda.synchronize()


def test_ring_stride_drain_and_clear(gpu_device):
    """B = 16, capacity 4, every 2: eleven updates from step 0 leave steps 4, 6, 8, 10 (2 was overwritten: dropped = 1); a second
    drain has nothing new; two more updates give 12; after load_state_dict with step = 3 the log is empty and its cursor at 3, and
    two updates later it holds step 4 -- this run's, not the earlier one's."""
    import torch
    _, fl, batch = _learner(gpu_device, (16, 1.0, 0, 0, "default", R.SEED), True)
    fl.enable_learn_log(4, every=2)
    for _ in range(11):
        fl.learn_batch(*batch)
    rec = fl.drain_learn_log()
    assert rec["step"].tolist() == [4, 6, 8, 10] and rec["dropped"] == 1 and rec["nonfinite"].tolist() == [0] * 4
    first = {k: rec[k].copy() for k in _columns()}
    rec = fl.drain_learn_log()
    assert rec["step"].tolist() == [] and rec["dropped"] == 0 and all(len(rec[k]) == 0 for k in _columns())
    for _ in range(2):
        fl.learn_batch(*batch)
    rec = fl.drain_learn_log()
    assert rec["step"].tolist() == [12] and rec["dropped"] == 0
    sd = fl.state_dict()
    sd["step"] = 3
    fl.load_state_dict(sd)
    rec = fl.drain_learn_log()
    assert rec["step"].tolist() == [] and rec["dropped"] == 0
    for _ in range(2):
        fl.learn_batch(*batch)
    rec = fl.drain_learn_log()
    assert rec["step"].tolist() == [4] and rec["dropped"] == 0 and int(fl.step_dev.item()) == 5
    assert rec["critic_loss"][0] != first["critic_loss"][0]      # (the same batch on weights twelve updates older)
    torch.cuda.synchronize()


def _loop_state(lp):
    import torch
    ag = lp.agent
    return torch.cat([p.detach().reshape(-1) for n in (ag.actor, ag.critic, ag.target_actor, ag.target_critic) for p in n.parameters()])


@pytest.mark.parametrize("kw", [dict(updates_per_step=3), dict(n_step=3, updates_per_step=1)], ids=["u3", "n3"])
def test_loop_graph_equals_eager_and_the_log_changes_nothing(gpu_device, kw):
    """DDPGRollout at N = 256, batch 64, an 8-slot ring, 12 vector steps from one seed: replayed graphs and eager launches leave the
    same records, bit for bit -- one per update, consecutive steps, updates_per_step of them per vector step once learning has
    begun -- and the four networks end bitwise where the same loop ends with learn_log=None."""
    import torch
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    runs = {}
    for how, use_graph, log in (("graph", True, 64), ("eager", False, 64), ("off", True, None)):
        env = TruckTrailerVecEnv(256)
        env.reset(seed=11)
        lp = DDPGRollout(env, batch_size=64, replay_slots=8, seed=11, use_graph=use_graph, learn_log=log, **kw)
        assert bool(lp.graph_steps) == use_graph
        lp.run(12)
        torch.cuda.synchronize()
        runs[how] = (lp, lp.drain_learn_log() if log else None, _loop_state(lp), int(lp.learner.step_dev.item()))
    (_, rec, state, steps), (_, rec_e, state_e, steps_e), (off, _, state_off, steps_off) = runs["graph"], runs["eager"], runs["off"]
    u = kw["updates_per_step"]
    assert steps == steps_e == steps_off and steps % u == 0 and steps >= u * (12 - 1 - kw.get("n_step", 1) - 1)
    assert rec["step"].tolist() == list(range(1, steps + 1)) and rec["dropped"] == 0 and int(rec["nonfinite"].sum()) == 0
    _same_records(rec, rec_e)
    assert len(set(rec["critic_loss"].tolist())) == steps                    # (every update its own batch and weights)
    assert torch.equal(state, state_e) and torch.equal(state, state_off)
    with pytest.raises(ValueError, match="learn log is off"):
        off.drain_learn_log()
    for lp, *_ in runs.values():
        lp.env.close()


def test_population_records_are_each_agents_lone_records(gpu_device):
    """Two agents at B = 257 -- agent 0 the fresh state, agent 1 the x20 trained one -- two population updates: each agent's records are
    bitwise those of a lone FusedLearner with that agent's state and batch, and the two agents' differ.  And PopulationRollout with
    K = 2, 128 envs per agent, 8 steps: replayed graphs leave each agent the records eager launches leave."""
    import torch
    from ddpg_trucktrailer_amd.population import PopulationLearner, PopulationRollout
    dev = gpu_device
    B = 257
    cases = [(B, 1.0, 0, 0, "default", R.SEED), (B, 20.0, 3, 999, "trained", R.SEED)]
    lone = []
    for case in cases:
        _, fl, batch = _learner(dev, case, True)
        fl.fuse_tail = True
        fl.enable_learn_log(4)
        for _ in range(2):
            fl.learn_batch(*batch)
        lone.append(fl.drain_learn_log())
    agents, rings = [], []
    for case in cases:
        state, hyper, batch, _, _ = R.case(*case)
        agents.append(R.load_agent(state, hyper, dev, torch.float32))
        rings.append(_ring_with_batch(dev, B, [t.to(dev).contiguous() for t in batch]))
    pop = PopulationLearner(agents, B, fc2_images=True, rings=[ring for ring, _ in rings], seeds=[seed for _, seed in rings], learn_log=4)
    for fl in pop.learners:
        fl.import_from_optimizers()
    assert [len(r["step"]) for r in pop.drain_learn_log()] == [0, 0]         # (no learn() yet)
    for _ in range(2):
        pop.learn(0)
    recs = pop.drain_learn_log()
    assert pop.tail_gave_up() == [0, 0]
    assert recs[0]["step"].tolist() == [1, 2] and recs[1]["step"].tolist() == [1000, 1001]
    for got, want in zip(recs, lone):
        assert got["dropped"] == 0 and int(got["nonfinite"].sum()) == 0
        _same_records(got, want)
    assert recs[0]["critic_loss"].tolist() != recs[1]["critic_loss"].tolist()
    assert recs[0]["grad_norm_actor"].tolist() != recs[1]["grad_norm_actor"].tolist()
    # the loop
    runs = []
    for graph_steps in (4, 0):
        lp = PopulationRollout(128, [3, 4], batch_size=64, replay_slots=8, graph_steps=graph_steps, learn_log=16)
        lp.run(8)
        torch.cuda.synchronize()
        runs.append((lp, lp.drain_learn_log()))
    (a, rec_a), (b, rec_b) = runs
    assert a.graph1 is not None and b.graph1 is None
    for x, y in zip(rec_a, rec_b):
        assert len(x["step"]) >= 6 and x["step"].tolist() == list(range(1, len(x["step"]) + 1)) and x["dropped"] == 0
        _same_records(x, y)
    assert rec_a[0]["critic_loss"].tolist() != rec_a[1]["critic_loss"].tolist()
    for lp, _ in runs:
        for stepper in lp.loops:
            stepper.env.close()
