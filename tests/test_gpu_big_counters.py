"""GPU (-m gpu): the kernels at counter values past 2^24, 2^31 and 2^32 (tests/big_counters.py: EDGES; DESIGN.md, "Counter widths")
against the host model (tests/loop_ref.py, tests/learn_ref.py, tests/td3_ref.py: 64-bit clean, held to that by
tests/test_big_counters_cpu.py).  Every random stream and every hand-over between launches is keyed by a 64-bit device counter
that some kernel narrows -- the two Philox words, k % slots, the 32-bit epochs of the waits, the bias-correction stamp, the tail
words -- and the rest of the suite drives those counters through small values only.  Counters are set directly: an explicit k_dev,
step_dev.fill_, an edited state_dict / checkpoint.  No bound is new: each check names the test whose bound it takes.

  1  replay draws at every edge: tt_ring_sample, the seed-stride form, tt_ring_sample_nstep, a draw with 7 side tuples
  2  tt_mlp_split_pack's cursor and image epoch at every edge
  3  OU noise of fused.actor_act (exact-f32 and split kernel) with step + *step_dev at every edge, split both ways
  4  one learn() at incoming step 2^24, 2^31 - 2, 2^31 - 1, 2^32 - 1, 2^40 + 5 against f64, two launches == tail in one launch
  5  one full TD3 update with the critic step 2^32 - 1 and the actor step 2^31 - 1
  6  save_training_checkpoint / load_training_checkpoint keep the step counts exactly (2^24 + 1, 2^31 + 3)
  7  the loop in lock step across an edge: tests/test_gpu_loop_lockstep.py's new configurations
  8  graphs == eager steps, resume, a population against its lone loops, and the peer-to-peer learner, across an edge

What these tests found.  (i) TrajectoryRing.load_state_dict raised from k = 2^31 (an int32 word was given k) and left zeroed image
epochs, which count as published for k in [2^31 - 1, 2^32 - 2].  (ii) The signed `have - want >= 0` of the waits was compiled to
`have >= want` (v_cmp_ge_i32 on the two words, no subtraction) in await_image, await_progress and k_adam_soft_p2p: at the sign
change that comparison makes a pipelined learn() wait its 0.25 s out and mark a give-up although the step chain is AHEAD of it
(progress = INT_MIN, want = INT_MAX), and lets a policy launch pass a stale image epoch; epoch_reached (csrc/ttnet_common.h) forms the difference unsigned.  (iii) save / load_training_checkpoint rounded
the learn step through an f32 tensor past 2^24.  (iv) The tail words' fill of -1 matches the epoch at step 2^32 - 2.

Do these tests bite?  Value changes only, in a scratch copy of the library, never an index or a slot computation:
  * Philox of the replay draw without its `k >> 32` word (ring_sample_index): caught by test 1 at 2^32 .. 2^32 + 2 and 2^40 + 5, by
    the 2^32 - 5 configurations of test 7 (check g) and by test 8's population -- predicted from the host model, whose draws at k
    and k - 2^32 differ (tests/test_big_counters_cpu.py asserts that); not run.
  * the epoch stored as (int)k instead of (int)(k + 1) (publish_image): caught by test 2 at every edge (the epoch word), and test
    8's graphs would give up -- predicted from the code; not run.
  Neither mutant was run: the second makes every policy launch wait out its 0.25 s and give up, which is not something to do to a
  shared device on purpose, and the first is decided by the host model alone.  Finding (ii) above is the compiler's own mutant of
  the wait; it was read in the library's instructions, and the run that would show its give-up mark was not made either.

Measured on MI355X (each figure from one run; worst error / bound over the run):
  1  draws                    idx exact at all 16 edges, both windows; n-step R 0.13 of nstep_ref's bound; 61 / 100 side rows drawn
  2  cursor and epochs        exact
  3  OU noise                 0.046 (n = 200, exact-f32 kernel), 0.048 (n = 1079, split kernel); both splits of the counter equal
  4  one learn step           the same at all five step counts and in both forms (the bias corrections are 1.0 at each):
                              pre-ReLU 0.30, y 0.012, q 0.015, q_pi 0.030, dq_da 0.0006, grad critic 0.014, grad actor 0.0035,
                              adam m 0.51 / 0.67, v 0.47 / 0.67, p 0.49 / 0.50, target 0.56 / 0.27 (critic / actor)
  5  TD3                      eps 0.015; pre-ReLU 0.33, y 0.016, q 0.023, q2 0.026, q1t 0.019, q2t 0.016, q_pi 0.010, dq_da 0.0007,
                              grad 0.011 / 0.012 / 0.005, adam m 0.43, v 0.63, p 0.48, target 0.37 / 0.41 (the cancelling elements
                              apart: the test's docstring)
  6, 8                        exact
  7  lock step at the edges   policy 0.0076, noise 0.040, env 0.38, pose 0.5; 146 episodes ended at 8 different steps in each of the
                              five configurations (tests/test_gpu_loop_lockstep.py)
The 19 tests here take 6 s together, the slowest 2 s (the first, which also loads the library); the five lock-step configurations
0.1 s each."""
import functools
import math
import os

import numpy as np
import pytest

import learn_checks as K
import learn_ref as R
import loop_ref as M
import td3_ref as T
from big_counters import EDGES, start_at, wrap32

pytestmark = pytest.mark.gpu

N = 200


# ---- 1: replay draws ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reserve,lag", [(0, 0), (2, 1)])
def test_ring_draws_at_every_edge(gpu_device, reserve, lag):
    """tests/test_gpu_loop_lockstep.py::test_ring_draws_are_the_documented_rows with its counters 0 .. 14 replaced by EDGES (n_envs
    200, B 513; tt_ring_sample on 6 slots, the seed-stride form with three draws, tt_ring_sample_nstep with n = 3 on 8 slots): idx is
    draw / draw_nstep exactly, the batches are the host's gather, R within nstep_ref's bound.  Then one draw per edge from a ring
    with 7 side tuples: idx is draw_side exactly (side rows as (-1, j)), the batch the host's gather over ring and side buffer."""
    import torch
    import test_gpu_loop_lockstep as LS
    dev, rows = gpu_device, 513
    worst = LS.check_ring_draws(dev, reserve, lag, EDGES)
    ring, host = LS._filled_ring(dev, 6)
    g = torch.Generator().manual_seed(99)
    side = dict(obs=torch.rand((7, 23), generator=g), act=torch.rand(7, generator=g) * 2 - 1, rew=torch.randn(7, generator=g),
                obs2=torch.rand((7, 23), generator=g), done=(torch.rand(7, generator=g) < 0.5).to(torch.uint8))
    ring.load_side(side["obs"], side["act"], side["rew"], side["obs2"], side["done"])
    side_np = {k: v.numpy() for k, v in side.items()}
    kd = torch.zeros((), dtype=torch.int64, device=dev)
    side_rows = 0
    for k in EDGES:
        kd.fill_(k)
        seed = 2 ** 40 + 7 * (k % 1000)
        out = ring.sample_fused(rows, seed=seed, return_index=True, done_as_bool=False, k_dev=kd, reserve=reserve, lag=lag)
        idx = M.draw_side(seed, k, rows, N, 6, 7, reserve, lag)
        assert np.array_equal(out[5].cpu().numpy(), idx), k
        LS._same_batch(out[:5], M.gather_side(host, side_np, idx), ("side", k))
        side_rows += int((idx[:, 0] < 0).sum())
    assert side_rows >= 16, side_rows          # (7 of 1007 or 607 transitions: about 4 to 6 rows of a draw)
    print(f"RATIOS big counters draws reserve {reserve} lag {lag}: idx exact at {len(EDGES)} edges, worst |R - R64| / bound "
          f"{worst:.3g}, {side_rows} side rows")


# ---- 2: cursor and epochs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [6, 8])
def test_pack_cursor_and_epoch_at_every_edge(gpu_device, slots):
    """tt_mlp_split_pack with a cursor whose counter holds each edge k: the four numbers of the step's parity are {k % s,
    (k + 1) % s, (k - 1) % s, 1} (the kernel takes its 64-bit modulo path from 2^32 on), the epoch word of that parity is
    wrap32(k + 1), the other parity's numbers and epoch, the running step's copy [0..3] and the progress word keep what they held,
    the arrival count is back at 0 and nothing gave up."""
    import torch
    from ddpg_trucktrailer_amd import fused
    from ddpg_trucktrailer_amd.agent import Agent
    from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing
    dev = gpu_device
    ring = TrajectoryRing(N, slots, 23, dev)
    actor = Agent(1e-4, 1e-3, (23,), 1e-3, 1, batch_size=8, device=dev, replay=False).actor
    fused.packed_weights_of(actor, 0, two_images=True)
    kd = torch.zeros((), dtype=torch.int64, device=dev)
    marks = torch.arange(1000, 1017, dtype=torch.int32)
    marks[14] = marks[15] = 0              # (the arrival count must start at 0; a give-up mark must be the launch's own)
    for k in EDGES:
        ring.cursor_dev[:17] = marks.to(dev)
        kd.fill_(k)
        fused.pack(actor, 0, cursor=ring.cursor(kd))
        torch.cuda.synchronize()
        cw, p = ring.cursor_dev.cpu().tolist(), k & 1
        assert cw[4 + 4 * p: 8 + 4 * p] == [k % slots, (k + 1) % slots, (k - 1) % slots, 1], (k, cw[:17])
        assert cw[12 + p] == wrap32(k + 1), (k, cw[12:14])
        q = 1 - p
        assert cw[4 + 4 * q: 8 + 4 * q] == marks[4 + 4 * q: 8 + 4 * q].tolist() and cw[12 + q] == int(marks[12 + q]), (k, cw[:17])
        assert cw[:4] == marks[:4].tolist() and cw[16] == int(marks[16]) and cw[14] == 0 and cw[15] == 0, (k, cw[:17])
        assert int(kd.item()) == k


# ---- 3: OU noise --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kernel", [(200, "exact_f32"), (1079, "split")])
def test_ou_noise_at_every_edge(gpu_device, n, kernel):
    """fused.actor_act at n = 200 on the exact-f32 kernel and at n = 1079 on the split kernel with a kept image, step + *step_dev
    equal to each edge, given all in `step` and half in each: the OU state equals ou_next(x before, done flags, ou_normal(seed,
    edge, n)) within check b's bound of tests/test_gpu_loop_lockstep.py, 1e-5 scale max(1, |N|) + ulp32(x), a finished lane
    restarts from 0, both splits give the same bits, and the stored action is mu + x."""
    import contextlib
    import torch
    from ddpg_trucktrailer_amd import fused
    from ddpg_trucktrailer_amd.agent import Agent
    dev, seed = gpu_device, 2 ** 35 + 31
    g = torch.Generator().manual_seed(n)
    actor = Agent(1e-4, 1e-3, (23,), 1e-3, 1, batch_size=8, device=dev, replay=False).actor
    obs = (torch.rand((n, 23), generator=g) * 2 - 1).to(dev)
    x0 = (torch.randn(n, generator=g) * 0.05).to(dev)
    done = (torch.rand(n, generator=g) < 0.25).to(torch.uint8).to(dev)
    raw, scaled, mu = (torch.empty(n, device=dev) for _ in range(3))
    high = float(np.float32(math.pi / 4))
    if kernel == "split":
        fused.pack(actor, 0)
        w, ctx = fused.packed_weights_of(actor, 0), contextlib.nullcontext()
    else:
        w, ctx = None, fused.exact_f32(actor)
    step_dev = torch.zeros((), dtype=torch.int64, device=dev)
    worst = 0.0
    with ctx:
        for st in EDGES:
            got = []
            for host_part in (st, st // 2):
                x = x0.clone()
                step_dev.fill_(st - host_part)
                fused.actor_act(actor, obs, x, raw, scaled, seed=seed, step=host_part, step_dev=step_dev, done_prev=done, mu_out=mu,
                                high=high, weights=w)
                got.append(x.cpu().numpy())
                assert torch.allclose(raw, mu + x, atol=1e-7) and torch.equal(scaled, torch.clamp(raw, -1, 1) * high), st
            assert np.array_equal(got[0], got[1]), (st, "step + *step_dev is the counter")
            nrm = M.ou_normal(seed, st, n)
            restart = done.cpu().numpy() != 0
            x_want = M.ou_next(x0.cpu().numpy(), restart, nrm)
            tol = 1e-5 * M.OU_SCALE * np.maximum(1.0, np.abs(nrm)) + np.spacing(np.abs(x_want).astype(np.float32)).astype(np.float64)
            err = np.abs(got[0].astype(np.float64) - x_want) / tol
            worst = max(worst, float(err.max()))
            assert err.max() <= 1.0, (st, err.max(), int(err.argmax()))
            assert (np.abs(got[0].astype(np.float64) - M.OU_SCALE * nrm)[restart] <= tol[restart]).all(), (st, "restart")
    assert restart.sum() >= 10
    print(f"RATIOS big counters noise n {n} {kernel}: worst |x - ou_next| / bound {worst:.3g} over {len(EDGES)} edges")


# ---- 4: one learn step at a large step count ----------------------------------------------------------------------------
LEARN_CASE = (257, 20.0, 3, 999, "trained", 7)
LEARN_STEPS = [2 ** 24, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 32 - 1, 2 ** 40 + 5]


@functools.lru_cache(maxsize=None)
def _learn_case_at(t0):
    """learn_ref's trained case B = 257 with the incoming step t0: the same state and batch (the forwards that decide a unit's side do
    not see the step), and the f64 reference step made again with that count.  Shared; do not write to it."""
    assert LEARN_CASE in R.ALL_CASES
    state, hyper, batch, _, _ = R.case(*LEARN_CASE)
    state = dict(state, step=t0)
    return state, hyper, batch, R.ref_step(state, batch, hyper)


@pytest.mark.parametrize("t0", LEARN_STEPS)
def test_one_learn_step_at_a_large_step_count(gpu_device, t0):
    """learn_checks.against_f64 with its bounds as they are (tests/test_gpu_learn_shapes.py::test_one_learn_step_against_f64), images
    on, at the incoming step t0, as two launches and with the actor tail in one launch: the two forms agree bit for bit and no tail
    consumer gave up; step_dev is the int64 t0 + 1; bias_corr[0] holds the bits of wrap32(t0 + 1), bias_corr[1:3] the critic's
    betas and bias_corr[3:5] the f32 roundings of 1 - beta^(t0 + 1) -- 1.0 here, both: 0.9^(2^24) and 0.999^(2^24) are below
    2^-25 --; the learn log's record of the update carries step == t0 + 1 exactly; with the tail, the producers' hint words and
    every row's word hold wrap32(t0 + 1)."""
    import torch
    dev = gpu_device
    state, hyper, batch, ref = _learn_case_at(t0)
    assert ref["step"] == t0 + 1
    runs, worst = {}, {}
    for tail in (False, True):
        tag = f"big counters learn step {t0} {'tail' if tail else 'two launches'}"
        worst[tail], fl, _, _ = K.against_f64(dev, state, hyper, batch, ref, images=True, tag=tag, tail=tail,
                                              prepare=lambda f: f.enable_learn_log(4))
        assert fl.fuse_tail is tail and fl.tail_gave_up() == 0
        assert fl.step_dev.dtype == torch.int64 and int(fl.step_dev.item()) == t0 + 1
        bc = fl.bias_corr.cpu()
        assert int(bc[:1].view(torch.int32).item()) == wrap32(t0 + 1)
        b1, b2 = (np.float32(x) for x in hyper["critic"]["betas"])
        want = [b1, b2, np.float32(1.0 - float(b1) ** (t0 + 1)), np.float32(1.0 - float(b2) ** (t0 + 1))]
        assert bc[1:5].tolist() == [float(x) for x in want] and bc[3:5].tolist() == [1.0, 1.0]
        rec = fl.drain_learn_log()
        assert rec["step"].dtype == np.int64 and rec["step"].tolist() == [t0 + 1] and rec["nonfinite"].tolist() == [0]
        if tail:
            producers, B = math.ceil(257 / 16), 257
            hints = fl.tail_words[:64].cpu()
            assert hints[:producers].tolist() == [wrap32(t0 + 1)] * producers
            rows = fl.tail_words[64:64 + 2 * B].cpu().view(B, 2)
            assert rows[:, 1].eq(wrap32(t0 + 1)).all() and torch.equal(rows[:, 0].contiguous().view(torch.float32), fl.dq_da.cpu())
        runs[tail] = K.results(fl)
    K.same(runs[True], runs[False], ("tail in one launch against two launches", t0))
    print(f"RATIOS big counters learn step {t0}: worst of both forms " +
          ", ".join(f"{k} {max(worst[False][k], worst[True][k]):.3g}" for k in worst[False]))


# ---- 5: TD3 -------------------------------------------------------------------------------------------------------------
def test_td3_full_update_at_large_step_counts(gpu_device):
    """td3_ref's case B = 257 with the critic step t = 2^32 - 1 and the actor step 2^31 - 1, images on: one full update through the
    body of tests/test_gpu_td3.py::test_one_full_update_against_f64 (td3_ref.td3_step, its bounds unchanged); eps equals
    td3_ref.noise_eps at that t under test_noise's criterion, 1e-5 sigma max(1, |N|), and differs from the noise at t - 2^32 (the
    high Philox word counts); both step counts advance as int64; the actor's bias-correction stamp holds wrap32 of the ACTOR step,
    and the tail words carry it.

    One check of that body is given in its format-derived form (test_gpu_td3._adam_checks, cancelling_targets).  The case's moments
    are zero, and with both bias corrections 1 -- any step count from a few thousand on -- Adam's first step from zero moments is
    lr 0.1 / sqrt(0.001) = 3.16 lr instead of lr: critic parameters move 3.16e-3, and for a few elements of fc2.weight tau (p -
    target0) cancels target0 (critic_2: target0 -4.2616e-06, p 4.2604e-03, new target 3.09e-09).  The new target is then hundreds
    of its own ulps from f64 through the ONE rounding of p - target0, whatever the kernel does: measured on MI355X 4.05 (critic)
    and 262 (critic_2) times the 2 ulp, with every element of all three nets bit-identical to the correctly rounded f32 fma of its
    inputs; at step 0 the same elements give 0.40 and 0.42.  Those elements are held to the f32 fma's bits, all others to 2 ulp."""
    import torch
    import test_gpu_td3 as G
    dev = gpu_device
    case = [c for c in T.F64_CASES if c[0] == 257][0]
    state, hyper, batch, _ = T.case(*case)
    t, ta = 2 ** 32 - 1, 2 ** 31 - 1
    state = dict(state, step=t, actor_step=ta)
    worst, fl = G.full_update_against_f64(dev, state, hyper, batch, True, cancelling_targets=True)
    cfg = T.default_cfg()
    eps = fl.eps.double().cpu().numpy()
    host, nrm = T.noise_eps(77, t, 257, cfg.target_noise, cfg.noise_clip)
    ratio = (np.abs(eps - host) / (1e-5 * cfg.target_noise * np.maximum(1.0, np.abs(nrm)))).max()
    assert ratio <= 1.0, ratio
    low, _ = T.noise_eps(77, t - 2 ** 32, 257, cfg.target_noise, cfg.noise_clip)
    assert np.abs(eps - low).max() > 1e-3
    assert fl.step_dev.dtype == fl.actor_step_dev.dtype == torch.int64
    assert int(fl.step_dev.item()) == t + 1 == 2 ** 32 and int(fl.actor_step_dev.item()) == ta + 1 == 2 ** 31
    assert int(fl.actor_bias_corr.cpu()[:1].view(torch.int32).item()) == wrap32(ta + 1) == -2 ** 31
    assert int(fl.bias_corr.cpu()[:1].view(torch.int32).item()) == wrap32(t + 1) == 0
    rows = fl.tail_words[64:64 + 2 * 257].cpu().view(257, 2)
    assert rows[:, 1].eq(wrap32(ta + 1)).all() and fl.tail_gave_up() == 0
    print(f"RATIOS big counters td3: eps {ratio:.3g}, " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---- 6: checkpoint round trip of the step -------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [2 ** 24 + 1, 2 ** 31 + 3])
def test_training_checkpoint_keeps_the_learn_step(gpu_device, tmp_path, step):
    """A FusedLearner at learn step `step` (learn_ref's trained case B = 257): save_training_checkpoint, load_training_checkpoint
    into a fresh agent and learner whose moments and step are zero: the step count is equal exactly, and one further update equals
    the same update of the learner that made no round trip, bit for bit (step_dev is among the results).  (Before the checkpoint
    carried the integer the step came back as float32(step): 2^24 and 2^31.)"""
    import torch
    from ddpg_trucktrailer_amd import checkpoint
    dev = gpu_device
    state, hyper, batch, _, _ = R.case(*LEARN_CASE)
    state = dict(state, step=step)
    agent, fl, on_dev = K.learner(dev, state, hyper, batch, step)
    agent.fused_learner = fl
    path = checkpoint.save_training_checkpoint(str(tmp_path / "ck.pt"), agent)
    zeros = lambda tree: {n: {k: torch.zeros_like(v) for k, v in d.items()} for n, d in tree.items()}
    fresh = dict(state, step=0, m=zeros(state["m"]), v=zeros(state["v"]))
    agent2, fl2, _ = K.learner(dev, fresh, hyper, batch, 0)
    agent2.fused_learner = fl2
    checkpoint.load_training_checkpoint(path, agent2)
    fl2.refresh_images()
    assert int(fl2.step_dev.item()) == int(fl.step_dev.item()) == step
    assert fl2.step_counts() == fl.step_counts() == {"step": step}
    assert torch.equal(fl2.critic.m, fl.critic.m) and torch.equal(fl2.actor.v, fl.actor.v)
    for f in (fl, fl2):
        f.learn_batch(*on_dev)
    torch.cuda.synchronize()
    assert int(fl2.step_dev.item()) == step + 1
    K.same(K.results(fl2), K.results(fl), ("after the round trip", step))
    # a file written before the counts were kept (no "learn_steps") still loads: the optimizers' f32 step
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck.pop("learn_steps") == {"step": step}
    torch.save(ck, path)
    checkpoint.load_training_checkpoint(path, agent2)
    assert int(fl2.step_dev.item()) == int(np.float32(step))


@pytest.mark.parametrize("step,actor_step", [(2 ** 24 + 1, 2 ** 23 + 1), (2 ** 31 + 3, 2 ** 24 + 1)])
def test_training_checkpoint_keeps_the_td3_steps(gpu_device, tmp_path, step, actor_step):
    """The same with a TD3Learner (td3_ref's case B = 257): both counts come back exactly, and one further full update -- whose
    smoothing noise is keyed by the critic step -- equals the update made without the round trip: eps, y, all six nets, the three
    moment pairs and both counts, bit for bit."""
    import torch
    import test_gpu_td3 as G
    from ddpg_trucktrailer_amd import checkpoint
    dev = gpu_device
    case = [c for c in T.F64_CASES if c[0] == 257][0]
    state, hyper, batch, _ = T.case(*case)
    state = dict(state, step=step, actor_step=actor_step)
    cfg = T.default_cfg()
    agent, fl, _, _ = G._td3_learner(dev, state, hyper, cfg, batch, True, noise_seed=77)
    agent.fused_learner = fl
    path = checkpoint.save_training_checkpoint(str(tmp_path / "ck.pt"), agent)
    zeros = lambda tree: {n: {k: torch.zeros_like(v) for k, v in d.items()} for n, d in tree.items()}
    fresh = dict(state, step=0, actor_step=0, m=zeros(state["m"]), v=zeros(state["v"]))
    agent2, fl2, _, _ = G._td3_learner(dev, fresh, hyper, cfg, batch, True, noise_seed=77)
    agent2.fused_learner = fl2
    checkpoint.load_training_checkpoint(path, agent2)
    assert (int(fl2.step_dev.item()), int(fl2.actor_step_dev.item())) == (step, actor_step)
    assert fl2.step_counts() == fl.step_counts() == {"step": step, "actor_step": actor_step}

    def results(f):
        ag = f.agent
        out = [p.detach().clone() for n in f._nets() for p in n.parameters()]
        return out + [t.clone() for st in (f.actor, f.critic, f.critic_2) for t in (st.m, st.v)] + \
            [f.eps.clone(), f.y.clone(), f.q_pi.clone(), f.dq_da.clone(), f.step_dev.clone(), f.actor_step_dev.clone()]
    for f in (fl, fl2):
        f.learn_batch(u=0, full=True)
    torch.cuda.synchronize()
    assert fl.tail_gave_up() == 0 and fl2.tail_gave_up() == 0
    assert int(fl2.step_dev.item()) == step + 1 and int(fl2.actor_step_dev.item()) == actor_step + 1
    K.same(results(fl2), results(fl), ("after the round trip", step))


# ---- 8: graphs, resume, populations and the peer-to-peer learner across the edge ---------------------------------------
def _loop_state(lp, fl=None):
    fl, ag = fl if fl is not None else lp.learner, lp.agent
    out = [p.detach().clone() for n in (ag.actor, ag.critic, ag.target_actor, ag.target_critic) for p in n.parameters()]
    return out + [t.clone() for t in (lp.ring.obs, lp.ring.act, lp.ring.rew, lp.ring.done, lp.ring.k_dev, lp.noise.x, lp.env.state,
                                      fl.actor.m, fl.actor.v, fl.critic.m, fl.critic.v, fl.step_dev)]


def _lone(dev, seed, graph_steps, **kw):
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    env = TruckTrailerVecEnv(256, device=dev)
    env.reset(seed=seed)
    return DDPGRollout(env, batch_size=64, replay_slots=8, seed=seed, alpha=1e-4, beta=1e-3, tau=1e-3, gamma=0.99,
                       graph_steps=graph_steps, **kw)


def test_graphs_and_resume_across_2_pow_31(gpu_device, tmp_path):
    """DDPGRollout with N = 256, batch 64, 8 slots, pipelined, graphs of 4 steps, loaded at k0 = 2^31 - 6 with u0 = 2^31 - 9 learn
    steps made (the loops have captured their graphs at small counters before they load): run(12) in graphs -- which crosses
    (int)k's sign change with both chains of the pipelined step waiting for each other in device memory -- equals 12 eager steps
    bit for bit, policy_gave_up() is 0 in both and no tail gave up; a save at k0 + 6 loaded into a third loop that runs the last 6
    steps equals the uninterrupted run.  (The load raised "value cannot be converted to type int without overflow" from k = 2^31
    before the ring wrote its words relative to k.)"""
    import torch
    from ddpg_trucktrailer_amd import checkpoint
    dev = gpu_device
    k0, u0 = 2 ** 31 - 6, 2 ** 31 - 9
    graphs, eager, resumed = _lone(dev, 21, 4, pipeline=True), _lone(dev, 21, 0, pipeline=True), _lone(dev, 5, 4, pipeline=True)
    assert graphs.pipeline and eager.pipeline and graphs.graph_steps == 4 and eager.graph_steps == 0
    sd = start_at(graphs.state_dict(), k0, u0, 8, fill_seed=8)
    for lp in (graphs, resumed):
        lp.run(6)                              # warm: four eager steps, the captures, two replays
        assert lp.graph1 is not None
    for lp in (graphs, eager):
        lp.load_state_dict(sd)
        assert lp.ring.k == k0 and int(lp.k_pipe_dev.item()) == k0 and int(lp.learner.step_dev.item()) == u0
    graphs.run(6)
    path = checkpoint.save_loop_checkpoint(str(tmp_path / "loop.pt"), graphs)
    graphs.run(6)
    for _ in range(12):
        eager.step()
    torch.cuda.synchronize()
    assert graphs.graph1 is not None and graphs.ring.k == eager.ring.k == k0 + 12 > 2 ** 31
    assert int(graphs.ring.k_dev.item()) == k0 + 12 and int(graphs.learner.step_dev.item()) == u0 + 12
    for lp in (graphs, eager):
        assert lp.ring.policy_gave_up() == 0 and lp.learner.tail_gave_up() == 0 and not lp.handover_gave_up
    K.same(_loop_state(graphs), _loop_state(eager), "graphs against eager steps")
    checkpoint.load_loop_checkpoint(path, resumed)
    assert resumed.ring.k == k0 + 6 and resumed.vector_steps == k0 + 6
    resumed.run(6)
    torch.cuda.synchronize()
    assert resumed.ring.policy_gave_up() == 0 and resumed.learner.tail_gave_up() == 0
    K.same(_loop_state(resumed), _loop_state(graphs), "resumed at k0 + 6 against the uninterrupted run")
    for lp in (graphs, eager, resumed):
        lp.env.close()


def test_population_across_2_pow_32(gpu_device):
    """PopulationRollout with K = 2 agents x 256 lanes, batch 64, 8 slots, graphs of 4 steps, loaded at k0 = 2^32 - 4 with u0 =
    2^31 - 3 learn steps made, for 8 steps: each agent equals its lone serial loop (tail in one launch, as the population's learn())
    loaded with the agent's part of the same state, bit for bit; nothing gave up."""
    import torch
    from ddpg_trucktrailer_amd.population import PopulationRollout
    dev = gpu_device
    k0, u0, seeds = 2 ** 32 - 4, 2 ** 31 - 3, [21, 22]
    pop = PopulationRollout(256, seeds, batch_size=64, replay_slots=8, graph_steps=4)
    pop.run(6)
    assert pop.graph1 is not None
    sd = pop.state_dict()
    for a, st in enumerate(sd["agents"]):
        start_at(st, k0, u0, 8, fill_seed=80 + a)
    sd["vector_steps"] = k0
    pop.load_state_dict(sd)
    assert pop.k == k0 and pop.vector_steps == k0
    pop.run(8)
    torch.cuda.synchronize()
    assert pop.graph1 is not None and pop.k == k0 + 8 > 2 ** 32 and pop.learner.tail_gave_up() == [0, 0]
    old = os.environ.get("TT_ACTOR_TAIL")
    os.environ["TT_ACTOR_TAIL"] = "1"
    try:
        for a, seed in enumerate(seeds):
            lone = _lone(dev, seed, 4, pipeline=False)
            assert lone.learner.fuse_tail and not lone.pipeline
            lone.run(5)                        # (warm, its graphs captured at small counters)
            lone.load_state_dict(sd["agents"][a])
            lone.run(8)
            torch.cuda.synchronize()
            assert lone.ring.policy_gave_up() == 0 and pop.loops[a].ring.policy_gave_up() == 0
            lp, fl = pop.loops[a], pop.learner.learners[a]
            assert int(fl.step_dev.item()) == u0 + 8 and int(lp.ring.k_dev.item()) == k0 + 8
            K.same(_loop_state(lp, fl), _loop_state(lone), f"agent {a} of the population against its lone loop")
            lone.env.close()
    finally:
        if old is None:
            os.environ.pop("TT_ACTOR_TAIL")
        else:
            os.environ["TT_ACTOR_TAIL"] = old


def test_p2p_learner_across_2_pow_31(gpu_device):
    """A FusedLearner with enable_p2p() at world size 1, started at learn step 2^31 - 2 (learn_ref's trained case B = 257): 4 updates
    -- epochs 2^31 - 1, then INT_MIN and on -- equal the learner with the optimizer in launches of its own and no exchange, bit
    for bit, and p2p_gave_up() is 0."""
    import torch
    dev, t0 = gpu_device, 2 ** 31 - 2
    state, hyper, batch, _, _ = R.case(*LEARN_CASE)
    state = dict(state, step=t0)
    runs = {}
    for how in ("separate", "p2p"):
        _, fl, on_dev = K.learner(dev, state, hyper, batch, t0)
        if how == "p2p":
            fl.enable_p2p()
            on_dev = [t.clone() for t in on_dev]
        else:
            fl.grad_sync_critic = fl.grad_sync_actor = lambda: None
        for _ in range(4):
            fl.learn_batch(*on_dev)
        torch.cuda.synchronize()
        assert int(fl.step_dev.item()) == t0 + 4 and fl.p2p_gave_up() == 0 and fl.tail_gave_up() == 0
        runs[how] = K.results(fl)
    K.same(runs["p2p"], runs["separate"], "the exchange at world size 1 against separate optimizer launches")
