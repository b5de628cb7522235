"""CPU: the 64-bit device counters at the values where something narrows them (tests/big_counters.py: EDGES), with no kernel:

  a  the host model of the replay draw (tests/loop_ref.py) agrees with itself at every edge -- what tests/test_gpu_big_counters.py
     holds the kernels to;
  b  a TrajectoryRing loaded with k at every edge keeps k and leaves its hand-over words BEHIND the epochs the next launches wait
     for, in the kernels' wrapped 32-bit comparison (before the ring wrote them relative to k this failed from k = 2^31 - 1: the
     int32 cursor refused the progress word with "value cannot be converted to type int without overflow", and zeroed epoch words
     count as published for every k in [2^31 - 1, 2^32 - 2]);
  c  after FusedLearner / TD3Learner.load_state_dict no tail word can match the epoch of the next actor-tail launch."""
import types

import numpy as np
import pytest

import loop_ref as M
from big_counters import EDGES, behind, wrap32


def test_edges_and_wrapped_arithmetic():
    assert len(EDGES) == 16 and EDGES[-1] == 2 ** 40 + 5 and 2 ** 31 - 1 in EDGES and 2 ** 32 in EDGES and 2 ** 24 + 1 in EDGES
    assert [wrap32(x) for x in (0, 5, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5, -1)] == \
        [0, 5, 2 ** 31 - 1, -2 ** 31, -1, 0, 5, -1]
    for k in EDGES:
        assert behind(k, k + 1) and behind(k, k + 2) and not behind(k + 1, k + 1) and not behind(k + 2, k + 1)
        assert behind(wrap32(k), wrap32(k + 1)) and not behind(wrap32(k + 1), wrap32(k))
    # the plain comparison, which a signed `have - want >= 0` may be folded to, is wrong exactly at the sign change
    assert wrap32(2 ** 31) < wrap32(2 ** 31 - 1) and not behind(2 ** 31, 2 ** 31 - 1)
    assert not behind(0, 2 ** 31 + 5)          # a zeroed word is NOT behind an epoch of the upper half: it counts as published


# ---- a: the host model at every edge ----------------------------------------------------------------------------------
@pytest.mark.parametrize("reserve,lag", [(0, 0), (2, 1)])
@pytest.mark.parametrize("slots", [6, 8])
@pytest.mark.parametrize("n_step", [1, 3])
def test_the_host_model_agrees_with_itself_at_every_edge(reserve, lag, slots, n_step):
    """Every row of draw / draw_nstep maps through step_of_slot into window: the drawn step lies in the window, lives in the drawn
    slot, and with n steps the base step's last step is still inside the one-step window; the env index is in range, and the draw
    is a function of the whole 64-bit counter (the neighbouring edge and the counter minus 2^32 draw other rows)."""
    n_envs, batch = 200, 513
    for k in EDGES:
        seed = 2 ** 40 + 7 * (k % 1000)
        win = M.window(k, slots, reserve, lag, n_step)
        if n_step == 1:
            idx = M.draw(seed, k, batch, n_envs, slots, reserve, lag)
        else:
            idx = M.draw_nstep(seed, k, batch, n_envs, slots, n_step, reserve, lag)
        assert idx.dtype == np.int64 and idx.shape == (batch, 2)
        assert idx[:, 0].min() >= 0 and idx[:, 0].max() < slots and idx[:, 1].min() >= 0 and idx[:, 1].max() < n_envs
        if not len(win):               # (6 slots under a reserve of 2 hold no window for n = 3: the rows are in bounds, no more)
            assert (slots, reserve, n_step) == (6, 2, 3)
            continue
        assert len(win) == slots - 1 - reserve - (n_step - 1) and win[-1] == k - lag - 1 - (n_step - 1)
        steps = M.step_of_slot(idx[:, 0], k, slots, lag)
        assert steps.min() >= win[0] and steps.max() <= win[-1], (k, steps.min(), steps.max(), win)
        assert np.array_equal(steps % slots, idx[:, 0])
        assert set(steps.tolist()) == set(win), k                      # 513 rows over at most 7 steps: every one is drawn
        assert (steps + n_step - 1).max() <= M.window(k, slots, reserve, lag, 1)[-1]
        other = M.draw(seed, k + 1, batch, n_envs, slots, reserve, lag) if n_step == 1 else \
            M.draw_nstep(seed, k + 1, batch, n_envs, slots, n_step, reserve, lag)
        assert not np.array_equal(other[:, 1], idx[:, 1]), k
        if k - lag >= 2 ** 32:         # the high Philox word counts
            low = M.draw(seed, k - 2 ** 32, batch, n_envs, slots, reserve, lag) if n_step == 1 else \
                M.draw_nstep(seed, k - 2 ** 32, batch, n_envs, slots, n_step, reserve, lag)
            assert not np.array_equal(low[:, 1], idx[:, 1]), k


def test_the_noise_and_action_streams_take_the_whole_counter():
    """ou_normal and random_action at an edge differ from the same stream at the counter minus 2^32 (k >> 32 is a Philox word of its
    own) and from the neighbouring counter; a scalar and an array counter give the same numbers."""
    for k in EDGES:
        a = M.ou_normal(31, k, 64)
        assert np.isfinite(a).all() and not np.array_equal(a, M.ou_normal(31, k + 1, 64))
        assert np.array_equal(M.ou_normal(31, np.array([k, k + 1]), 64)[0], a)
        r = M.random_action(9, np.arange(64), k)
        assert r.dtype == np.float32 and (np.abs(r) <= np.float32(np.pi / 4)).all()
        if k >= 2 ** 32:
            assert not np.array_equal(a, M.ou_normal(31, k - 2 ** 32, 64))
            assert not np.array_equal(r, M.random_action(9, np.arange(64), k - 2 ** 32))


def test_loop_ref_counts_from_a_start_offset():
    """LoopRef(k0, u0): updates_after in closed form is the sum it replaces, and the draws of a loop loaded at k0 are those of the
    absolute step."""
    for pipelined, n_step, ups in ((False, 1, 1), (True, 1, 2), (True, 3, 1), (False, 1, 2)):
        ref = M.LoopRef(31, 17, 200, 8, 33, pipelined, ups, n_step)
        for t in range(12):
            assert ref.updates_after(t) == ups * sum(1 for s in range(t + 1) if ref.learns(s)), (pipelined, n_step, t)
        for k0, u0 in ((2 ** 31 - 5, 2 ** 31 - 7), (2 ** 32 - 5, 2 ** 31 - 7), (2 ** 24 - 5, 2 ** 24 - 6), (1, 0), (3, 5)):
            off = M.LoopRef(31, 17, 200, 8, 33, pipelined, ups, n_step, k0=k0, u0=u0)
            for t in range(k0, k0 + 10):
                assert off.learns(t) is ref.learns(t)
                assert off.updates_after(t) == u0 + ups * sum(1 for s in range(k0, t + 1) if off.learns(s)), (k0, t)
                assert off.draw_window(t) == ref.draw_window(t)
                if off.learns(t):
                    assert all(np.array_equal(a, b) for a, b in zip(off.draws(t), ref.draws(t)))
                    steps = off.steps_of(t, off.draws(t)[0])
                    assert steps.min() >= off.window(t)[0] and steps.max() <= off.window(t)[-1]


# ---- b: the ring's hand-over words after a load -----------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 7] + EDGES)
def test_a_loaded_ring_leaves_its_hand_over_words_behind_the_next_epochs(k):
    """TrajectoryRing.load_state_dict on the CPU with k at every edge (and small values: a fresh ring keeps its zeros): k and k_dev
    come back; BOTH epoch words e are behind k + 1 and k + 2 -- the epochs the policy launches of the next two steps wait for, one
    per parity -- so no launch can take an image that the pack launch of its step has not published; the progress word is
    wrap32(k), what the policy launch of step k - 1 left and what a pipelined learn() with the window counter k waits for."""
    import torch
    from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing
    ring = TrajectoryRing(4, 6, 23, torch.device("cpu"))
    assert not ring.cursor_dev.any()
    ring.cursor_dev[12:17] = torch.tensor([2 ** 31 - 1, -5, 3, 9, 77], dtype=torch.int32)       # what an earlier run left
    sd = ring.state_dict()
    sd["k"] = k
    ring.load_state_dict(sd)
    assert ring.k == k and ring.k_dev.dtype == torch.int64 and int(ring.k_dev.item()) == k
    cur = ring.cursor_dev.tolist()
    for e in cur[12:14]:
        assert behind(e, k + 1) and behind(e, k + 2), (k, e)
    assert cur[16] == wrap32(k)
    assert cur[14] == 0 and cur[15] == 0, "arrival count and give-up mark start clean"
    if k == 0:
        assert not ring.cursor_dev.any()


# ---- c: the tail words after a load -----------------------------------------------------------------------------------
def _bare(cls, step_names):
    """A learner with exactly what load_state_dict touches (the style of tests/test_expert_labels_cpu.py's bare learner)."""
    import torch
    fl = cls.__new__(cls)
    fl.loss_shape = fl.demo_loss = fl.p2p = fl.learn_log = None
    for name in ("actor", "critic", "critic_2"):
        setattr(fl, name, types.SimpleNamespace(m=torch.zeros(3), v=torch.zeros(3)))
    for name in step_names:
        setattr(fl, name, torch.zeros((), dtype=torch.int64))
    fl.tail_words = torch.full((64 + 2 * 1024,), -1, dtype=torch.int32)
    fl.updates = 0
    return fl


@pytest.mark.parametrize("step", [0, 5] + EDGES)
def test_loaded_tail_words_cannot_match_the_next_epoch(step):
    """tail_row and tail_wait_hints (csrc/ttlearn_bodies.h) compare a word's upper half with (int)epoch for EQUALITY, epoch = the
    step count the launch finds = the loaded count + 1 (FusedLearner: the learn step; TD3Learner: the actor step).  So the stale
    value that can never match is any value but wrap32(step + 1) -- and the fill of a fresh learner, -1, DOES match at
    step = 2^32 - 2.  Whatever an earlier run left (here: -1, 0 and the very value that would match), after the load no word
    equals wrap32(step + 1), and the step counts are the int64 values loaded."""
    import torch
    from ddpg_trucktrailer_amd.fused_learn import FusedLearner
    from ddpg_trucktrailer_amd.td3 import TD3Learner
    moments = {"m": torch.zeros(3), "v": torch.zeros(3)}
    for stale in (-1, 0, wrap32(step + 1)):
        fl = _bare(FusedLearner, ("step_dev",))
        fl.tail_words.fill_(stale)
        fl.load_state_dict({"step": step, "actor": moments, "critic": moments})
        assert fl.step_dev.dtype == torch.int64 and int(fl.step_dev.item()) == step
        assert not (fl.tail_words == wrap32(step + 1)).any(), (step, stale)
        assert fl.step_counts() == {"step": step}
        # TD3: the critics' count is somewhere else, and the tail is keyed by the ACTOR step
        t3 = _bare(TD3Learner, ("step_dev", "actor_step_dev"))
        t3.tail_words.fill_(stale)
        critic_step = 2 ** 32 - 1 if step != 2 ** 32 - 1 else 2 ** 31 - 1
        t3.load_state_dict({"step": critic_step, "actor_step": step, "updates": 4, "actor": moments, "critic": moments,
                            "critic_2": moments})
        assert t3.step_counts() == {"step": critic_step, "actor_step": step} and t3.updates == 4
        assert not (t3.tail_words == wrap32(step + 1)).any(), (step, stale)
        t3.set_step_counts({"step": 7, "actor_step": step + 1})
        assert t3.step_counts() == {"step": 7, "actor_step": step + 1} and not (t3.tail_words == wrap32(step + 2)).any()
