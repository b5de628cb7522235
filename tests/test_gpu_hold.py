"""GPU (-m gpu): greedy evaluation with held lanes (csrc/ttenv_hold.h: k_step_hold; evaluation.py).

    masked     step_hold against the host-masked loop of grid_eval on a twin env: returns, records and final states bit for bit
    held       lanes that finished do not move under 20 more launches; the episode log and the step counter are not touched
    oracle     the PER_ENV variant, free-running, against the C oracle
    graph      Evaluator: graph replays == eager launches, chunk 5 and 32; a second run() of the same graph == the first
    networks   K = 2 agents x 68 lanes == lone evaluators == the host loop; the captured graph follows learn()'s updates
    loop       DDPGRollout / PopulationRollout with evaluate() between their steps == without, bit for bit
    heatmap    generate_heatmap_data(hold=True) == hold=False

Episodes are kept short with per-lane step caps in [1, 48] (set_max_steps); actions come from seeded arrays, except where the test is
about networks."""
import functools

import numpy as np
import pytest

import learn_ref as R

pytestmark = pytest.mark.gpu

HIGH = float(np.float32(np.pi / 4))
T_MAX = 48
N1 = 600          # two full workgroups, one of 88 lanes


def _caps(n, seed):
    """Per-lane step caps: lanes 0..255 cap 1 (a workgroup wholly held from step 2), 256..319 cap 2 (a held wave inside a live
    workgroup), the rest mixed in [3, 48] (mixed waves)."""
    caps = np.random.RandomState(seed).randint(3, T_MAX + 1, n).astype(np.int32)
    caps[:256] = 1
    caps[256:320] = 2
    return caps


JACK = slice(320, 336)        # driven at full lock until the hitch folds
OUT = slice(336, 352)         # start at the map's edge, backing out of it


@functools.lru_cache(maxsize=None)
def _case1():
    """(start poses [N1,3], caps [N1], mu [T_MAX, N1] f32): seeded; the JACK and OUT lanes are made to end by their causes."""
    rng = np.random.RandomState(1234)
    lo, hi = np.array([-27.0, 0.0, np.deg2rad(45.0)]), np.array([27.0, 27.0, np.deg2rad(120.0)])
    start = lo + (hi - lo) * rng.uniform(size=(N1, 3))
    caps = _caps(N1, 99)
    mu = rng.uniform(-1.0, 1.0, size=(T_MAX, N1)).astype(np.float32)
    caps[JACK] = T_MAX
    mu[:, JACK] = np.where(np.arange(16) % 2 == 0, 1.0, -1.0).astype(np.float32)
    caps[OUT] = T_MAX
    start[OUT] = np.stack([np.full(16, -39.0) + 0.05 * np.arange(16), np.linspace(2.0, 25.0, 16), np.zeros(16)], 1)   # yaw 0: backs to -x
    return start, caps, mu


def _oracle_episodes(start, caps, mu, goal=None, L2=None):
    """The C oracle alone, free-running on the CPU, masked on the host: (ret, len, flags, end [n,3], success) of every lane's episode."""
    from oracle import c_oracle
    n = start.shape[0]
    ora = c_oracle.COracle(n)
    ora.place(start, goal, L2)
    for i in range(n):
        ora.set_max_steps(i, int(caps[i]))
    ret, length = np.zeros(n), np.zeros(n, np.int32)
    flags, end, succ = np.zeros(n, np.uint8), np.zeros((n, 3)), np.zeros(n, bool)
    fin = np.zeros(n, bool)
    high = np.float32(HIGH)
    for t in range(mu.shape[0]):
        _, rew, done, info = ora.step(mu[t] * high)           # (one f32 product, as the kernel forms it)
        live = ~fin
        ret[live] += rew[live]
        newly = live & done
        st = ora.state()
        length[newly] = t + 1
        flags[newly] = ora.flags()[newly]
        end[newly] = st[newly][:, [4, 5, 1]]
        succ[newly] = info[newly, c_oracle.INFO_KEYS.index("final_success_bonus")] > 0
        fin |= done
    assert fin.all()
    return ret, length, flags, end, succ


def _hold_env(dev, start, caps, goal=None, L2=None):
    import torch
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    env = TruckTrailerVecEnv(start.shape[0], device=dev)
    env.set_pose(start, goal=goal, L2=L2)
    env.set_max_steps(torch.from_numpy(caps))
    return env


def _lane_bytes(env, lanes):
    """Everything tt_env_export holds of the given lanes: hot tile rows, cold rows, episode number."""
    import torch
    blob = env.state_dict()["blob"]
    npad = (env.n_envs + 63) // 64 * 64
    hot = blob[:8 * 14 * npad].view(torch.int64).view(npad // 64, 14, 64)
    cold = blob[8 * 14 * npad:8 * 23 * npad].view(torch.int64).view(9, npad)
    eps = blob[8 * 23 * npad:].view(torch.int32)
    lanes = torch.as_tensor(lanes)
    return hot[lanes // 64, :, lanes % 64].clone(), cold[:, lanes].clone(), eps[lanes].clone()


# ---- 1. against the host-masked loop ---------------------------------------------------------------------------------------------
def test_step_hold_equals_the_host_masked_loop_bit_for_bit(gpu_device):
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    start, caps, mu = _case1()
    # the pose set covers the causes: asserted on the oracle alone
    _, o_len, o_flags, _, _ = _oracle_episodes(start, caps, mu)
    for bit, name in ((L.F_JACKKNIFE, "jackknife"), (L.F_OUT_OF_MAP, "out of map"), (L.F_MAX_STEPS, "max steps")):
        assert (o_flags & bit).any(), f"no lane of the oracle ends by {name}"
    assert (o_flags[JACK] & L.F_JACKKNIFE).any() and (o_flags[OUT] & L.F_OUT_OF_MAP).all()
    assert (o_len[:256] == 1).all() and (o_len[256:320] == 2).all() and len(set(o_len[352:].tolist())) > 10

    held, twin = _hold_env(gpu_device, start, caps), _hold_env(gpu_device, start, caps)
    held.enable_hold()
    held.hold_begin()
    assert int(held.hold_count_live().item()) == N1
    n, dev = N1, held.device
    mu_d = torch.from_numpy(mu).to(dev)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    ret, length, flags, succ = z(n, torch.float64), z(n, torch.int32), z(n, torch.uint8), z(n, torch.bool)
    end, state, obs_end = z((n, 3), torch.float64), z((n, 6), torch.float64), twin.obs.clone()
    fin = z(n, torch.bool)
    lives = []
    for t in range(T_MAX):
        held.step_hold(mu_d[t], HIGH)
        lives.append(int(held.hold_count_live().item()))
        obs, _, done, info = twin.step(mu_d[t] * HIGH, auto_reset=False, info=True)       # what grid_eval does
        live = ~fin
        ret += torch.where(live, info["comp"][0], torch.zeros_like(ret))
        newly = live & done.bool()
        st = twin.state
        length = torch.where(newly, twin.episode()["steps"], length)
        flags = torch.where(newly, info["flags"], flags)
        succ = torch.where(newly, info["comp"][L.INFO_ROWS.index("final_success_bonus")] > 0, succ)
        end = torch.where(newly.unsqueeze(1), st[:, [4, 5, 1]], end)
        state = torch.where(newly.unsqueeze(1), st, state)
        obs_end = torch.where(newly.unsqueeze(1), obs, obs_end)
        fin |= done.bool()
        assert lives[-1] == int((~fin).sum()), t
    assert lives[0] == N1 - 256 and lives[1] == N1 - 320 and lives[-1] == 0 and bool(fin.all())
    rec = held.hold_records()
    assert rec["live"] == 0
    assert torch.equal(rec["ret"], ret), float((rec["ret"] - ret).abs().max())
    assert torch.equal(rec["len"], length) and torch.equal(rec["len"].cpu(), torch.from_numpy(o_len))
    assert torch.equal(rec["flags"], flags) and torch.equal(rec["success"], succ) and torch.equal(rec["end"], end)
    assert torch.equal(rec["flags"].cpu(), torch.from_numpy(o_flags))
    assert torch.equal(held.state, state)
    assert torch.equal(held.obs, obs_end)
    assert torch.equal(held.episode()["steps"], length)


# ---- 2. held lanes do not move ------------------------------------------------------------------------------------------------
def test_held_lanes_do_not_move_and_the_log_and_the_counter_are_not_touched(gpu_device):
    import torch
    start, caps, mu = _case1()
    env = _hold_env(gpu_device, start, caps)
    dev = env.device
    env.enable_episode_log(1024)
    counter = torch.full((1,), 7, dtype=torch.int64, device=dev)
    env.set_step_counter(counter)
    env.enable_hold()
    env.hold_begin()
    mu_d = torch.from_numpy(mu).to(dev)
    env.step_hold(mu_d[0], HIGH)
    env.step_hold(mu_d[1], HIGH)
    held = np.arange(320)                      # caps 1 and 2: a whole workgroup and one wave of the next
    moving = np.nonzero(caps > 30)[0]
    before = dict(lanes=_lane_bytes(env, held), obs=env.obs[:320].clone(), rec=env.hold_records(),
                  log=env._episode_log_state()["blob"].clone(), moving=_lane_bytes(env, moving))
    assert before["rec"]["live"] == N1 - 320 and bool((before["rec"]["len"][:320] > 0).all())
    for t in range(2, 22):
        env.step_hold(mu_d[t], HIGH)
    after = dict(lanes=_lane_bytes(env, held), obs=env.obs[:320].clone(), rec=env.hold_records(),
                 log=env._episode_log_state()["blob"].clone(), moving=_lane_bytes(env, moving))
    for x, y in zip(before["lanes"], after["lanes"]):
        assert torch.equal(x, y)
    assert torch.equal(before["obs"].view(torch.int32), after["obs"].view(torch.int32))
    for k in ("ret", "len", "flags", "success", "end"):
        assert torch.equal(before["rec"][k][:320], after["rec"][k][:320]), k
    assert torch.equal(before["log"], after["log"])        # the whole block: launch count, write index, counters, running returns
    assert int(counter.item()) == 7
    assert not torch.equal(before["moving"][0], after["moving"][0])      # (the launches did step the others)
    assert after["rec"]["live"] < before["rec"]["live"]


# ---- 3. against the C oracle, per-lane goals and trailer lengths ----------------------------------------------------------------
def test_per_env_variant_against_the_c_oracle_free_running(gpu_device):
    import torch
    n = 136
    rng = np.random.RandomState(77)
    lo, hi = np.array([-27.0, 0.0, np.deg2rad(45.0)]), np.array([27.0, 27.0, np.deg2rad(120.0)])
    start = lo + (hi - lo) * rng.uniform(size=(n, 3))
    goal = np.stack([rng.uniform(-5, 5, n), rng.uniform(-32, -25, n), np.deg2rad(rng.uniform(80, 100, n))], 1)
    l2 = rng.uniform(5.0, 7.0, n)
    caps = rng.randint(1, T_MAX + 1, n).astype(np.int32)
    mu = rng.uniform(-1.0, 1.0, size=(T_MAX, n)).astype(np.float32)
    o_ret, o_len, o_flags, o_end, o_succ = _oracle_episodes(start, caps, mu, goal, l2)
    env = _hold_env(gpu_device, start, caps, goal, l2)
    env.enable_hold()
    env.hold_begin()
    mu_d = torch.from_numpy(mu).to(env.device)
    for t in range(T_MAX):
        env.step_hold(mu_d[t], HIGH)
    rec = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in env.hold_records().items()}
    assert rec["live"] == 0
    assert (rec["len"] == o_len).all() and (rec["flags"] == o_flags).all() and (rec["success"] == o_succ).all()
    d_ret, d_end = np.abs(rec["ret"] - o_ret), np.abs(rec["end"] - o_end).max()
    print(f"per-env hold against the oracle: max |ret| error / len = {(d_ret / o_len).max():.2e}, max |end| error = {d_end:.2e}")
    assert (d_ret <= o_len * 1e-5).all() and d_end <= 1e-5


# ---- networks -----------------------------------------------------------------------------------------------------------------
M, K = 68, 2      # the agent boundary lies inside a wave


@functools.lru_cache(maxsize=None)
def _poses_and_caps():
    rng = np.random.RandomState(5)
    lo, hi = np.array([-27.0, 0.0, np.deg2rad(45.0)]), np.array([27.0, 27.0, np.deg2rad(120.0)])
    return lo + (hi - lo) * rng.uniform(size=(M, 3)), rng.randint(1, T_MAX + 1, M).astype(np.int32)


def _trained(dev, seed):
    """(agent, FusedLearner, batch of 33 rows) at trained scale, as tests/test_gpu_loss_shape.py makes them."""
    import torch
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    state = R.make_state(seed, 20.0, 3)
    state["step"] = 999
    agent = R.load_agent(state, R.TRAINED_HYPER, dev, torch.float32)
    fl = FusedLearner(agent, 33, fc2_images=True)
    fl.import_from_optimizers()
    fl.refresh_images()
    batch = [t.to(dev).contiguous() for t in R._candidates(33, torch.Generator().manual_seed(seed + 33))]
    return agent, fl, batch


@pytest.fixture(scope="module")
def trained(gpu_device):
    return [_trained(gpu_device, s) for s in (7, 8)]


def _evaluator(dev, agents=K, **kw):
    from ddpg_trucktrailer_amd.evaluation import Evaluator
    poses, caps = _poses_and_caps()
    return Evaluator(M, agents=agents, poses=poses, max_steps=caps, device=dev, **kw)


def _same_records(a, b):
    import torch
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert set(x) == set(y) == {"ret", "len", "flags", "success", "end"}
        for k in x:
            assert x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]), k


@pytest.mark.parametrize("chunk", [5, 32])
def test_evaluator_graph_replays_equal_eager_launches(gpu_device, trained, chunk):
    import torch
    actors = [t[0].actor for t in trained]
    eager = _evaluator(gpu_device, chunk=chunk, use_graph=False)
    want = eager.run(actors)
    assert eager.captures == 0 and eager.live_left == 0
    ev = _evaluator(gpu_device, chunk=chunk)
    first = ev.run(actors)
    assert ev.captures == 1 and ev.live_left == 0 and ev.replays == -(-T_MAX // chunk) == eager.replays
    _same_records(first, want)
    _, caps = _poses_and_caps()
    assert torch.equal(first[0]["len"].cpu() <= torch.from_numpy(caps), torch.ones(M, dtype=torch.bool))
    assert first[0]["ret"].dtype == torch.float64 and first[0]["success"].dtype == torch.bool and tuple(first[0]["end"].shape) == (M, 3)
    assert not torch.equal(first[0]["ret"], first[1]["ret"])
    second = ev.run(actors)                       # the same captured graph, after hold_begin
    assert ev.captures == 1
    _same_records(second, first)


def test_evaluator_agents_equal_lone_evaluators_the_host_loop_and_follow_learn(gpu_device, trained):
    import torch
    from ddpg_trucktrailer_amd.checkpoint import BestModelTracker
    from ddpg_trucktrailer_amd.evaluation import summary
    from ddpg_trucktrailer_amd.pbt import PBT
    actors = [t[0].actor for t in trained]
    ev = _evaluator(gpu_device)
    recs = ev.run(actors)
    for a in range(K):
        lone = _evaluator(gpu_device, agents=1)
        _same_records(lone.run([actors[a]]), [recs[a]])
    host = _evaluator(gpu_device)
    _same_records(host.run(actors, host_loop=True), recs)
    assert host.captures == 0
    # the records go where drained episode records go
    PBT(K, 1, window=M).observe(recs)
    best, avg, rate = BestModelTracker().update_many(recs[0], 0)
    s = summary(recs[0])
    assert s["episodes"] == M and abs(s["mean_return"] - float(recs[0]["ret"].mean())) < 1e-9 and 0.0 <= rate <= 1.0
    # three updates of each agent: the SAME captured graph packs the image from the new weights
    for _, fl, batch in trained:
        for _ in range(3):
            fl.learn_batch(*batch)
    torch.cuda.synchronize()
    again = ev.run(actors)
    assert ev.captures == 1
    fresh = _evaluator(gpu_device)
    _same_records(again, fresh.run(actors))
    assert not torch.equal(again[0]["ret"], recs[0]["ret"])


# ---- 6. the loop is untouched ---------------------------------------------------------------------------------------------------
def _loop_state(lp, fl):
    ag = lp.agent
    out = [p.detach().clone() for n in (ag.actor, ag.critic, ag.target_actor, ag.target_critic) for p in n.parameters()]
    out += [lp.ring.obs.clone(), lp.ring.act.clone(), lp.ring.rew.clone(), lp.ring.done.clone(), lp.ring.k_dev.clone(),
            lp.noise.x.clone(), lp.env.state.clone(), fl.actor.m.clone(), fl.actor.v.clone(), fl.critic.m.clone(), fl.critic.v.clone(),
            fl.step_dev.clone(), torch_rng()]
    log = lp.drain_episodes()
    out += [log[k] for k in ("ret", "len", "flags", "success", "lane", "end_step")]
    return out


def torch_rng():
    import torch
    return torch.cuda.get_rng_state().clone()


def _all_equal(a, b):
    import torch
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("pipeline", [True, False], ids=["pipelined", "serial"])
def test_lone_loop_with_evaluations_equals_the_loop_without(gpu_device, pipeline, graphs):
    import torch
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    runs, evals = [], []
    for with_eval in (False, True):
        env = TruckTrailerVecEnv(64, device=gpu_device)
        env.reset(seed=3)
        lp = DDPGRollout(env, batch_size=33, replay_slots=16, seed=3, pipeline=pipeline, graph_steps=4 if graphs else 0, episode_log=4096)
        assert lp.pipeline == pipeline
        ev = _evaluator(gpu_device, agents=1, chunk=8) if with_eval else None
        for _ in range(3):
            if graphs:
                lp.run(4)
            else:
                for _ in range(4):
                    lp.step()
            if ev is not None and lp.vector_steps < 12:
                evals.append(lp.evaluate(ev))
        torch.cuda.synchronize()
        assert lp.vector_steps == 12 and (lp.graph1 is not None) == graphs
        runs.append(_loop_state(lp, lp.learner))
    assert len(evals) == 2 and set(evals[0]) == {"ret", "len", "flags", "success", "end"} and len(evals[0]["ret"]) == M
    assert not torch.equal(evals[0]["ret"], evals[1]["ret"])          # (the actor learned in between)
    assert _all_equal(runs[0], runs[1])


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
def test_population_with_evaluations_equals_the_population_without(gpu_device, graphs):
    import torch
    from ddpg_trucktrailer_amd.population import PopulationRollout
    runs, evals = [], []
    for with_eval in (False, True):
        pop = PopulationRollout(64, [11, 12], batch_size=33, replay_slots=16, graph_steps=4 if graphs else 0, episode_log=4096)
        ev = _evaluator(gpu_device, chunk=8) if with_eval else None
        for _ in range(3):
            if graphs:
                pop.run(4)
            else:
                for _ in range(4):
                    pop.step()
            if ev is not None and pop.vector_steps < 12:
                evals.append(pop.evaluate(ev))
        torch.cuda.synchronize()
        assert pop.vector_steps == 12 and (pop.graph1 is not None) == graphs
        runs.append([x for a in range(2) for x in _loop_state(pop.loops[a], pop.learner.learners[a])])
    assert len(evals) == 2 and len(evals[0]) == 2 and len(evals[0][1]["ret"]) == M
    assert _all_equal(runs[0], runs[1])


# ---- 7. the heat map ------------------------------------------------------------------------------------------------------------
def test_heatmap_with_held_lanes_equals_the_masked_loop(gpu_device, trained):
    from ddpg_trucktrailer_amd.grid_eval import generate_heatmap_data
    actor = trained[0][0].actor
    a = generate_heatmap_data(actor, grid_resolution=20, trials_per_cell=2, device=gpu_device)
    b = generate_heatmap_data(actor, grid_resolution=20, trials_per_cell=2, device=gpu_device, hold=True)
    assert len(a) == len(b) == 7 and a[0].shape == (4, 4) and len(a[5]) == 32 and len(a[6]) == 16
    for x, y in zip(a[:4], b[:4]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert a[4] == b[4] and a[5] == b[5] and a[6] == b[6]
    assert all(len(t["trailer_x"]) > 1 for t in a[6])
