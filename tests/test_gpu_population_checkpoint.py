"""GPU (-m gpu): whole-population checkpoints (PopulationRollout.state_dict / load_state_dict, checkpoint.save_population_checkpoint;
DESIGN.md section 21).  A population saved after an exploit() and continued must equal, bit for bit, a population built with other
seeds and hyperparameters that loads the file and continues -- whether it had captured graphs over a handle of its own or had
never stepped -- for DDPG, TD3, per-agent n-step returns and under a PBT controller; one agent of the file continues alone in a
lone loop; the learn log comes back empty; tools/train_population.py --resume prints the lines of the uninterrupted run.

The smallest sizes at which the pieces still differ per agent: K = 3 agents x 64 lanes, batch 16, 8 ring slots, graphs of 4 steps,
2 updates per step, every hyperparameter different per agent."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, N, B, SLOTS, UPS, G = 3, 64, 16, 8, 2, 4
BEFORE, AFTER, OTHER = 10, 9, 6          # vector steps before the save, after it, and of the population that loads, before it loads
HYP_A = dict(seeds=[11, 18, 25], alphas=[1e-4, 1.25e-4, 1.5e-4], betas=[1e-3, 1.5e-3, 2e-3], taus=[1e-3, 2e-3, 3e-3],
             gammas=[0.99, 0.98, 0.97])
HYP_B = dict(seeds=[5, 6, 7], alphas=[2e-4, 3e-4, 4e-4], betas=[3e-3, 4e-3, 5e-3], taus=[4e-3, 5e-3, 6e-3], gammas=[0.96, 0.95, 0.94])
# agent 2 takes agent 0's networks and new values; agent 1 keeps its networks and takes new values (dst == src)
EXPLOIT = [(2, 0, dict(alpha=3e-4, beta=2.5e-3, tau=5e-3, gamma=0.955)), (1, 1, dict(alpha=0.75e-4, beta=0.5e-3, tau=2.5e-3, gamma=0.985))]


def _f32(x):
    return float(np.float32(x))


def _pop(hyp, **kw):
    from ddpg_trucktrailer_amd.population import PopulationRollout
    return PopulationRollout(N, batch_size=B, replay_slots=SLOTS, updates_per_step=UPS, graph_steps=G, episode_log=1 << 12,
                             **dict(hyp, **kw))


def _agent_snapshot(agent, fl, ring, noise, env, records):
    """Everything the comparison helper holds of one agent, as {name: tensor or value}."""
    import torch
    out = {}
    for i, net in enumerate(fl._nets()):           # (actor, critic, their targets; with TD3 the second critic and its target)
        for name, p in net.named_parameters():
            out[f"net{i}.{name}"] = p.detach().clone()
    for st_name, st in zip(("actor", "critic", "critic_2"), fl._states()):
        out[f"adam.{st_name}.m"], out[f"adam.{st_name}.v"] = st.m.clone(), st.v.clone()
    out["step_dev"] = fl.step_dev.clone()
    if hasattr(fl, "actor_step_dev"):
        out["actor_step_dev"] = fl.actor_step_dev.clone()
    for name in ("obs", "act", "rew", "done", "k_dev"):
        out[f"ring.{name}"] = getattr(ring, name).clone()
    out["noise.x"], out["env.state"] = noise.x.clone(), env.state
    out.update({f"env.episode.{k}": v for k, v in env.episode().items()})
    out.update({f"records.{k}": v.clone() if torch.is_tensor(v) else v for k, v in records.items()})
    return out


def _snapshot(pop):
    """The comparison helper's view of a population, after draining every agent's episode log."""
    import torch
    torch.cuda.synchronize()
    records = pop.drain_episodes()
    snap = {"vector_steps": pop.vector_steps, "agents": []}
    for a, lp in enumerate(pop.loops):
        s = _agent_snapshot(lp.agent, pop.learner.learners[a], lp.ring, lp.noise, lp.env, records[a])
        s["hyper"] = pop.hyper(a)
        if pop.td3 is None and pop.learner.nstep_table:
            s["n_step_of"] = pop.n_step_of(a)
        snap["agents"].append(s)
    return snap


def _assert_agent_equal(got, want, who):
    import torch
    assert sorted(got) == sorted(want), (who, sorted(set(got) ^ set(want)))
    for k, w in want.items():
        if torch.is_tensor(w):
            assert got[k].dtype == w.dtype and torch.equal(got[k], w), f"{who}: {k} differs"
        else:
            assert got[k] == w, f"{who}: {k}: {got[k]} != {w}"


def _assert_equal(got, want):
    """THE comparison of two populations: per agent, by torch.equal, every network's parameters, every Adam m / v, step_dev (and
    actor_step_dev), the ring's obs / act / rew / done and k_dev, noise.x, env.state, env.episode() and the episode records drained
    over the run; by value, hyper(a) (and n_step_of(a)) read back from the device, and vector_steps."""
    assert got["vector_steps"] == want["vector_steps"]
    assert len(got["agents"]) == len(want["agents"])
    for a, (g, w) in enumerate(zip(got["agents"], want["agents"])):
        _assert_agent_equal(g, w, f"agent {a}")


def _saved_and_continued(path, hyp, exploit, **kw):
    """Population A: BEFORE steps, the exploit, the save (episode records of the first steps still undrained), AFTER more steps."""
    from ddpg_trucktrailer_amd.checkpoint import save_population_checkpoint
    pop = _pop(hyp, **kw)
    pop.run(BEFORE)
    pop.exploit(exploit)
    save_population_checkpoint(path, pop)
    pop.run(AFTER)
    return _snapshot(pop)


def _loaded_and_continued(path, hyp, steps_before_load, check=None, **kw):
    """A population built with `hyp` that runs steps_before_load steps, loads the file and runs AFTER steps."""
    from ddpg_trucktrailer_amd.checkpoint import load_population_checkpoint
    pop = _pop(hyp, **kw)
    if steps_before_load:
        pop.run(steps_before_load)
        assert pop.graph1 is not None and pop.learner.has_handle
    assert load_population_checkpoint(path, pop) == {}
    assert pop.graph1 is None
    if check is not None:
        check(pop)
    pop.run(AFTER)
    assert pop.graph1 is not None                      # (the continuation ran on captured graphs)
    return _snapshot(pop)


@pytest.fixture(scope="module")
def ddpg_file(gpu_device, tmp_path_factory):
    """(path of population A's file, A's snapshot after the continuation): computed once, shared by cases 1, 2, 6 and 7."""
    path = str(tmp_path_factory.mktemp("popck") / "ddpg.pt")
    return path, _saved_and_continued(path, HYP_A, EXPLOIT)


def test_resume_is_bitwise_ddpg(ddpg_file):
    """Case 1.  B -- other seeds, other hyperparameters, its own handle and captured graphs -- loads A's file: hyper(2) reads the
    exploited values back from the device before any step, and 9 steps later B equals A."""
    path, want = ddpg_file

    def exploited(pop):
        assert pop.learner.has_handle
        for dst, _, h in EXPLOIT:
            assert pop.hyper(dst) == {k: _f32(v) for k, v in h.items()}
        assert pop.hyper(0) == {k: _f32(HYP_A[k + "s"][0]) for k in ("alpha", "beta", "tau", "gamma")}
        assert pop.seeds == HYP_A["seeds"] and pop.learner.seeds == HYP_A["seeds"] and pop.vector_steps == BEFORE
    _assert_equal(_loaded_and_continued(path, HYP_B, OTHER, exploited), want)


def test_load_before_the_first_step(ddpg_file):
    """Case 2.  C never stepped: no handle yet, only the host changes, and run() goes on by itself -- and equals A."""
    path, want = ddpg_file

    def no_handle(pop):
        assert not pop.learner.has_handle and pop.k == BEFORE
        assert pop.agents[2].alpha == EXPLOIT[0][2]["alpha"] and pop.learner.learners[2].hyp_critic[0] == EXPLOIT[0][2]["beta"]
    _assert_equal(_loaded_and_continued(path, HYP_B, 0, no_handle), want)


def test_resume_is_bitwise_td3(gpu_device, tmp_path):
    """Case 3.  TD3 agents with their own target_noise and noise_clip: six networks, three moment pairs, both step counts, and
    hyper(a) reads all six values back."""
    from ddpg_trucktrailer_amd.td3 import TD3Config
    path = str(tmp_path / "td3.pt")
    cfg_a = [TD3Config(2, 0.2 + 0.05 * a, 0.5 - 0.1 * a) for a in range(K)]
    cfg_b = [TD3Config(2, 0.1, 0.3 + 0.01 * a) for a in range(K)]
    pairs = [(2, 0, dict(EXPLOIT[0][2], target_noise=0.15, noise_clip=0.35)), (1, 1, dict(EXPLOIT[1][2], target_noise=0.33))]
    want = _saved_and_continued(path, HYP_A, pairs, td3=cfg_a)
    assert sum(k.startswith("adam.") for k in want["agents"][0]) == 6 and "actor_step_dev" in want["agents"][0]
    assert any(k.startswith("net5.") for k in want["agents"][0])

    def six_values(pop):
        assert pop.hyper(2) == {k: _f32(v) for k, v in pairs[0][2].items()}
        assert pop.hyper(1) == {k: _f32(v) for k, v in dict(pairs[1][2], noise_clip=cfg_a[1].noise_clip).items()}
        assert pop.agents[2].td3 == TD3Config(2, 0.15, 0.35) and pop.learner.learners[2].cfg == pop.agents[2].td3
        assert [fl.seed for fl in pop.learner.learners] == HYP_A["seeds"] == [fl.noise_seed for fl in pop.learner.learners]
    _assert_equal(_loaded_and_continued(path, HYP_B, OTHER, six_values, td3=cfg_b), want)


def test_resume_is_bitwise_n_step(gpu_device, tmp_path):
    """Case 4.  Per-agent n, one of them moved by an exploit before the save: n_step_of(a) reads the file's table back from the
    device, and the continuation is bitwise."""
    from ddpg_trucktrailer_amd.fused_learn import nstep_discount
    path = str(tmp_path / "nstep.pt")
    pairs = [(0, 2, dict(EXPLOIT[0][2], n_step=3)), (1, 1, EXPLOIT[1][2])]       # (agent 0: n 1 -> 3, not its src's 2)
    want = _saved_and_continued(path, HYP_A, pairs, n_step=[1, 3, 2], n_step_max=3)

    def table(pop):
        assert pop.n_steps == [3, 3, 2] and [lp.ring.n_step for lp in pop.loops] == [3, 3, 2]
        gammas = [pairs[0][2]["gamma"], pairs[1][2]["gamma"], HYP_A["gammas"][2]]
        for a, (n, g) in enumerate(zip([3, 3, 2], gammas)):
            assert pop.n_step_of(a) == (n, _f32(g), _f32(nstep_discount(g, n)))
    _assert_equal(_loaded_and_continued(path, HYP_B, OTHER, table, n_step=[2, 1, 1], n_step_max=3), want)


def test_refusals_write_nothing(ddpg_file):
    """A population of another shape refuses the file with the pure check's message, and nothing of it changed."""
    import torch
    from ddpg_trucktrailer_amd.checkpoint import load_population_checkpoint
    path, _ = ddpg_file
    pop = _pop(dict(HYP_B, seeds=HYP_B["seeds"][:2], alphas=1e-4, betas=1e-3, taus=1e-3, gammas=0.99))
    before = [p.detach().clone() for ag in pop.agents for p in ag.actor.parameters()]
    with pytest.raises(ValueError, match="K: the checkpoint holds 3 agents"):
        load_population_checkpoint(path, pop)
    assert pop.vector_steps == 0 and pop.seeds == HYP_B["seeds"][:2]
    assert all(torch.equal(x, p) for x, p in zip(before, (p for ag in pop.agents for p in ag.actor.parameters())))


def test_resume_under_pbt(gpu_device, tmp_path):
    """Case 5.  A controller takes PBT.step after every block of 5 steps, two blocks before the save and two after.  A fresh
    population with a fresh controller (another seed) loads the file: the same history, decision for decision, and the same bits.
    ready = 5, window = 4, min_episodes = 1: a round needs two agents with one finished episode each.  Untrained agents finish no
    episode within 20 steps (measured: none at 64, 128, 256, 512 or 1024 lanes per agent, so more lanes do not help), so population
    A's lanes get step caps of 3 + lane % 16 before the first step: their first episodes end at steps 3 .. 18, some in every
    block, on both sides of the save.  The caps are env state: they reach B through the file."""
    from ddpg_trucktrailer_amd.checkpoint import load_population_checkpoint, save_population_checkpoint
    from ddpg_trucktrailer_amd.pbt import PBT
    path = str(tmp_path / "pbt.pt")
    kw = dict(ready=5, window=4, min_episodes=1, quantile=0.34)

    def blocks(pop, pbt, n):
        for _ in range(n):
            pop.run(5)
            pbt.step(pop, pop.drain_episodes())
    a, pbt_a = _pop(HYP_A), PBT(K, seed=1, **kw)
    for lp in a.loops:
        lp.env.set_max_steps([3 + lane % 16 for lane in range(N)])
    blocks(a, pbt_a, 2)
    at_save = len(pbt_a.history)
    save_population_checkpoint(path, a, pbt_a, {"blocks": 2})
    blocks(a, pbt_a, 2)
    print(f"PBT decisions: {at_save} before the save, {len(pbt_a.history) - at_save} after; "
          f"windows {[len(w) for w in pbt_a.windows]}")
    assert at_save >= 1 and len(pbt_a.history) > at_save, "the case needs a round on each side of the save"
    b, pbt_b = _pop(HYP_B), PBT(K, seed=77, **kw)
    assert load_population_checkpoint(path, b, pbt_b) == {"blocks": 2}
    assert pbt_b.history == pbt_a.history[:at_save]
    blocks(b, pbt_b, 2)
    assert pbt_b.history == pbt_a.history and [list(w) for w in pbt_b.windows] == [list(w) for w in pbt_a.windows]
    _assert_equal(_snapshot(b), _snapshot(a))


def test_one_agent_continues_in_a_lone_loop(ddpg_file, gpu_device, monkeypatch):
    """Case 6.  sd["agents"][1] through DDPGRollout.load_state_dict on a lone serial-order loop built with seed 99 and the exploited
    hyperparameters (tests/test_gpu_population.py's lone loops: pipeline=False, TT_ACTOR_TAIL=1): 9 steps later it holds agent 1's
    bits."""
    import torch
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    path, want = ddpg_file
    sd = torch.load(path, map_location="cpu", weights_only=True)["population"]["agents"][1]
    assert sd["hyper"] == EXPLOIT[1][2] and sd["n_step"] == 1
    monkeypatch.setenv("TT_ACTOR_TAIL", "1")
    env = TruckTrailerVecEnv(N, device=gpu_device)
    env.reset(seed=99)
    h = sd["hyper"]
    lp = DDPGRollout(env, seed=99, alpha=h["alpha"], beta=h["beta"], tau=h["tau"], gamma=h["gamma"], pipeline=False, batch_size=B,
                     replay_slots=SLOTS, updates_per_step=UPS, graph_steps=G, episode_log=1 << 12)
    assert lp.learner.fuse_tail and not lp.pipeline
    lp.load_state_dict(sd)
    lp.run(AFTER)
    torch.cuda.synchronize()
    got = _agent_snapshot(lp.agent, lp.learner, lp.ring, lp.noise, lp.env, lp.drain_episodes())
    mine = {k: v for k, v in want["agents"][1].items() if k != "hyper"}
    _assert_agent_equal(got, mine, "the lone loop against agent 1")
    assert lp.vector_steps == want["vector_steps"] and lp.seed == HYP_A["seeds"][1]


def test_learn_log_is_empty_after_a_load_and_continues(ddpg_file):
    """Case 7.  learn_log=64: records of the 6 steps before the load are gone after it, and the next records' step values go on
    from the loaded step counts.  (The log's launch changes no bit: the population still equals A.)"""
    import torch
    from ddpg_trucktrailer_amd.checkpoint import load_population_checkpoint
    path, want = ddpg_file
    steps = [st["fused_adam"]["step"] for st in torch.load(path, weights_only=True)["population"]["agents"]]
    assert steps == [(BEFORE - 1) * UPS] * K
    pop = _pop(HYP_B, learn_log=64)
    pop.run(OTHER)
    load_population_checkpoint(path, pop)
    for rec in pop.drain_learn_log():
        assert len(rec["step"]) == 0 and rec["dropped"] == 0
    pop.run(AFTER)
    for a, rec in enumerate(pop.drain_learn_log()):
        assert rec["step"].tolist() == list(range(steps[a] + 1, steps[a] + 1 + AFTER * UPS)) and rec["dropped"] == 0
    _assert_equal(_snapshot(pop), want)
    fresh = _pop(HYP_B, learn_log=64)                      # (and on a population without a handle: no log yet, then the same)
    load_population_checkpoint(path, fresh)
    assert all(len(rec["step"]) == 0 for rec in fresh.drain_learn_log())
    fresh.run(1)
    assert [rec["step"].tolist() for rec in fresh.drain_learn_log()] == [[s + 1, s + 2] for s in steps]


def _tool(cwd, *args):
    """One fresh child process of tools/train_population.py, K = 2 x 64 lanes, blocks of 5 steps, with the learn log (every
    per-agent line then ends with the latest update's number, losses, Q mean, |TD| and gradient norms) and an evaluation every
    third block; its per-agent progress lines and evaluation lines, in their order."""
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_population.py"), "--pbt", "5", "--learn-log", "1", "--eval-every", "3",
           "--eval-lanes", "16", *args[:-1], "2", str(N), str(SLOTS), str(UPS), str(B), args[-1], "5", "27", str(G)]
    out = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout, [ln for ln in out.stdout.splitlines() if re.match(r"(evaluation  )?agent \d+ seed ", ln)]


def test_the_tool_resumes_with_the_lines_of_the_uninterrupted_run(gpu_device, tmp_path):
    """Case 8.  Three child processes, one after the other: 4 blocks uninterrupted; 2 blocks with --checkpoint / --save-every 1;
    2 more blocks with --resume.  The per-agent lines of blocks 3 and 4 are identical (the timing line is not compared).  Untrained
    agents finish no episode in 20 steps, so the lines' episode columns say nothing; what makes them depend on the restored
    state is the learn log's record at their end -- the update number and the losses, Q mean and gradient norms of the latest update,
    which move with any bit of the networks, Adam state, rings, seeds or hyperparameters -- and the evaluation after block 3, which
    is due there only when the block counter came back (every third block) and reads the restored actors."""
    ck = str(tmp_path / "run.pt")
    _, whole = _tool(tmp_path, "20")
    assert len(whole) == 10 and [ln.startswith("evaluation") for ln in whole] == [False] * 6 + [True] * 2 + [False] * 2
    records = [re.search(r"  update (\d+): critic loss (\S+)  actor loss (\S+)  Q mean (\S+)", ln) for ln in whole if ln.startswith("agent")]
    assert all(records), whole
    # block b ends at vector step 5 b: its latest update is number (5 b - 1) * UPS, since learn() starts at the second step
    assert [int(m.group(1)) for m in records] == [(5 * b - 1) * UPS for b in (1, 2, 3, 4) for _ in range(2)]
    assert len({m.groups()[1:] for m in records}) == 8            # (every line's losses are its own: agents and blocks differ)
    _, first = _tool(tmp_path, "--checkpoint", ck, "--save-every", "1", "10")
    assert first == whole[:4] and os.path.exists(ck) and [f for f in os.listdir(tmp_path) if f.startswith("run.pt")] == ["run.pt"]
    text, second = _tool(tmp_path, "--resume", ck, "20")
    assert f"resumed from {ck}: continuing from vector step 10 (block 2)" in text
    assert second == whole[4:]
