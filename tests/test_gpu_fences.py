"""GPU (-m gpu): no entry point of include/ttenv.h reads or writes outside the extents the header states per argument.

Every array handed to the C ABI here is a fenced buffer (tests/fenced.py): a payload of exactly the stated size between two
fences of a recognisable pattern, so that a store past a ragged last row lands in a fence instead of in some other block of torch's
pool, and a load past it returns a fill the test chooses.  Every case asserts

  1. fences intact, and no prefill left in an output the header says is filled;
  2. independence: the same bits for the three fills of the inputs' surroundings (the NaN pattern, 3e38, zeros), all finite;
  3. the same bits as the same calls on ordinary, separately allocated tensors -- the accuracy tests then vouch for the values.

Sizes are the smallest that reach each kernel's ragged paths: one row, one less / one more than a wave or a 16-row group, one
more than a workgroup, a last tile with 1 and with 127 rows.  Nothing here can fault: an overrun of a whole workgroup tile stays
inside the buffer's own allocation."""
import ctypes as C
import math

import pytest

pytestmark = pytest.mark.gpu

ENV_NS = (1, 63, 65, 257, 1000)         # 257: one more than the step kernel's workgroup (TT_BLOCK = 256 in csrc/ttenv_state.h)
_FIELDS = ("w1", "b1", "g1", "be1", "w2", "b2", "g2", "be2", "w3", "b3", "wa", "ba")


def _bits(t):
    import torch
    return t.detach().contiguous().view(-1).view(torch.uint8)


def _three_ways(dev, run):
    """run(alloc) -> None makes the calls on buffers from `alloc` (fenced.Arena or fenced.Plain) and leaves every result in them.
    Runs it on plain tensors and under the three surroundings; asserts the three conditions of the module docstring for every
    buffer (names that start with "~" may keep prefill elements and are exempt from the finite check).  Returns the plain run's
    buffers."""
    import torch
    from fenced import SURROUNDS, Arena, Plain
    plain = Plain(dev)
    run(plain)
    torch.cuda.synchronize()
    ref = {k: v.clone() for k, v in plain.items()}
    for surround in SURROUNDS:
        arena = Arena(dev, surround)
        run(arena)
        torch.cuda.synchronize()
        arena.assert_clean(f"surroundings = {surround}")
        got = dict(arena.items())
        assert got.keys() == ref.keys()
        for k, v in got.items():
            assert torch.equal(_bits(v), _bits(ref[k])), f"{k}: differs from the unfenced run with surroundings = {surround}"
            if surround == "nan" and v.is_floating_point() and not k.startswith("~"):
                assert torch.isfinite(v).all(), f"{k}: not finite"
    return ref


def _stream(dev):
    from ddpg_trucktrailer_amd import _lib as L
    return L.stream(dev)


# ======================================================================================================= policy forward
def _policy_run(c, n, split, max_wg, keep):
    import torch
    from ddpg_trucktrailer_amd import _lib as L, fused

    def run(alloc):
        dev = alloc.device
        lib, st, p = L.load(), _stream(dev), L.ptr
        T = dict(tile_rows=128)            # rows of one workgroup tile of both policy kernels
        g = torch.Generator(device=dev).manual_seed(7 * n + 1)
        obs = alloc.inp("obs", c["obs"], **T)
        action = alloc.inp("action", c["act"].reshape(-1), **T)
        ou = alloc.inp("ou_state", torch.randn(n, device=dev, generator=g) * 0.1, **T)
        done_prev = alloc.inp("done_prev", (torch.rand(n, device=dev, generator=g) < 0.3).to(torch.uint8), **T)
        step_dev = alloc.inp("step_dev", torch.tensor(5, dtype=torch.int64, device=dev))
        ws = []
        for net, critic in ((c["actor"], 0), (c["critic"], 1)):
            w = fused._fill_weights(net, L.TTMlpWeights())
            if split:      # a caller-kept image, fenced directly after tt_mlp_split_ws_bytes()
                img = alloc.out(f"~split_ws.{critic}", (int(lib.tt_mlp_split_ws_bytes()),), torch.uint8, full=False,
                                tile_bytes=1 << 16, also_input=True)
                w.split_ws = img.data_ptr()
                L.check(lib.tt_mlp_split_pack(C.byref(w), critic, p(img), None, None, st))
                w.ws_packed, w.max_workgroups = 1, max_wg
            ws.append(w)
        keep.append(ws)
        mu, q, mu2, raw, scaled = (alloc.out(k, (n,), **T) for k in ("fwd.mu", "fwd.q", "act.mu", "act.raw", "act.scaled"))
        L.check(lib.tt_actor_forward(n, p(obs), C.byref(ws[0]), p(mu), st))
        L.check(lib.tt_critic_forward(n, p(obs), p(action), C.byref(ws[1]), p(q), st))
        high = float(torch.tensor(math.pi / 4, dtype=torch.float32))
        L.check(lib.tt_actor_act(n, p(obs), C.byref(ws[0]), p(ou), p(done_prev), 27, 3, p(step_dev), 0.2 * 1e-2, 0.15 * 0.1, high,
                                 p(mu2), p(raw), p(scaled), st))
    return run


@pytest.mark.parametrize("n", [1, 63, 65, 1000])
def test_exact_f32_policy_kernel_stays_inside_its_rows(gpu_device, n):
    import torch
    from test_gpu_policy_tile_chain import _case
    keep = []
    c = _case(gpu_device, n)
    ref = _three_ways(gpu_device, _policy_run(c, n, False, 0, keep))
    assert torch.equal(ref["obs"], c["obs"])                             # (the inputs came through untouched)


@pytest.mark.parametrize("max_wg", [0, 2])
@pytest.mark.parametrize("n", [1025, 1151])
def test_split_f16_policy_kernel_stays_inside_its_rows(gpu_device, n, max_wg):
    """Nine tiles, the last with 1 row / with 127 rows; max_workgroups = 2: a workgroup's last tile requests a "next tile" that
    does not exist.  mu and Q also against the f64 modules, with the bound of tests/test_gpu_policy_tile_chain.py."""
    from test_gpu_policy_tile_chain import _case
    c = _case(gpu_device, n)
    keep = []
    ref = _three_ways(gpu_device, _policy_run(c, n, True, max_wg, keep))
    for name, want, bound in (("fwd.mu", c["mu64"], c["bound_mu"]), ("act.mu", c["mu64"], c["bound_mu"]), ("fwd.q", c["q64"], c["bound_q"])):
        e = (ref[name] - want).abs().max().item()
        print(f"n={n} max_workgroups={max_wg} {name}: error {e:.3e}, bound {bound:.3e}")
        assert e <= bound, (name, e, bound)


# ================================================================================================================= env
def _env_run(N, compare_log_blob):
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv

    def run(alloc):
        dev = alloc.device
        env = TruckTrailerVecEnv(N, device=dev)
        h, lib, st, p = env._h, env.lib, _stream(dev), L.ptr
        chk = lambda rc: L.check(rc, h)
        T = dict(tile_rows=256)                                          # one workgroup of every env kernel: 256 lanes
        soa = lambda rows, width=8: dict(tile_bytes=rows * 256 * width)   # [rows, N] arrays: a workgroup's lanes of every row
        f64, i32, i64, u8 = torch.float64, torch.int32, torch.int64, torch.uint8
        lanes = torch.arange(N, device=dev)
        g = torch.Generator(device=dev).manual_seed(N)
        some_end = torch.where(lanes % 3 == 0, 1, 60).to(i32)            # every third lane's episode ends at its next step

        chk(lib.tt_env_reset(h, None, 11, p(alloc.out("reset.obs", (N, 23), **T)), st))
        mask = alloc.inp("mask", (lanes % 3 == 0).to(u8), **T)
        chk(lib.tt_env_reset(h, p(mask), 12, p(alloc.out("~reset_masked.obs", (N, 23), full=False, **T)), st))
        env.set_max_steps(some_end)
        action = alloc.inp("action", (torch.rand(N, device=dev, generator=g) * 2 - 1) * 0.9, **T)

        def step(tag, auto):
            o = dict(obs=alloc.out(f"{tag}.obs", (N, 23), **T), rew=alloc.out(f"{tag}.reward", (N,), **T),
                     done=alloc.out(f"{tag}.done", (N,), u8, **T), comp=alloc.out(f"{tag}.comp", (L.NINFO, N), f64, **soa(L.NINFO)),
                     viol=alloc.out(f"{tag}.violation", (N,), u8, **T), flags=alloc.out(f"{tag}.flags", (N,), u8, **T))
            info = L.TTInfo(o["comp"].data_ptr(), o["viol"].data_ptr(), o["flags"].data_ptr())
            chk(lib.tt_env_step(h, p(action), p(o["obs"]), p(o["rew"]), p(o["done"]), C.byref(info), auto, st))
        step("step", 0)
        step("step_reset", 1)
        chk(lib.tt_env_step_random(h, 99, p(alloc.out("random.action", (N,), **T)), p(alloc.out("random.obs", (N, 23), **T)),
                                   p(alloc.out("random.reward", (N,), **T)), p(alloc.out("random.done", (N,), u8, **T)), None, 1, st))
        steer = alloc.inp("steering", (torch.rand(N, device=dev, generator=g) * 2 - 1) * 0.7, **T)
        chk(lib.tt_env_observe(h, p(steer), p(alloc.out("observe.obs", (N, 23), **T)), st))
        chk(lib.tt_env_get_state(h, p(alloc.out("state", (6, N), f64, **soa(6))), st))
        chk(lib.tt_env_get_episode(h, p(alloc.out("episode.steps", (N,), i32, **T)), p(alloc.out("episode.max_steps", (N,), i32, **T)),
                                   p(alloc.out("episode.start", (3, N), f64, **soa(3))), p(alloc.out("episode.goal", (3, N), f64, **soa(3))),
                                   p(alloc.out("episode.L2", (N,), f64, **T)), st))
        L.check(lib.tt_random_actions(N, 5, 9, p(alloc.out("random_actions", (N,), **T)), st))
        chk(lib.tt_env_rollout_random(h, 3, 77, p(alloc.out("rollout.obs", (N, 23), **T)), p(alloc.out("rollout.reward_sum", (N,), **T)),
                                      p(alloc.out("rollout.episodes_done", (N,), i32, **T)), st))
        # checkpoint blob, fenced directly after tt_env_state_bytes()
        blob = alloc.out("~env_blob", (int(lib.tt_env_state_bytes(h)),), u8, full=False, tile_bytes=1 << 16)
        meta = (C.c_uint64 * 4)()
        chk(lib.tt_env_export(h, p(blob), C.byref(meta), st))
        assert int(meta[2]) == N

        # held lanes
        chk(lib.tt_env_set_hold(h, 1, st))
        chk(lib.tt_env_reset(h, None, 13, None, st))
        env.set_max_steps(some_end)
        chk(lib.tt_env_hold_begin(h, st))
        mu = alloc.inp("hold.mu", torch.rand(N, device=dev, generator=g) * 2 - 1, **T)
        chk(lib.tt_env_step_hold(h, p(mu), 0.7, p(alloc.out("hold.obs", (N, 23), **T)), st))            # every lane live: all rows
        chk(lib.tt_env_step_hold(h, p(mu), 0.7, p(alloc.out("~hold.obs2", (N, 23), full=False, **T)), st))   # finished lanes hold still
        chk(lib.tt_env_hold_read(h, p(alloc.out("hold.ret", (N,), f64, **T)), p(alloc.out("hold.len", (N,), i32, **T)),
                                 p(alloc.out("hold.flags", (N,), u8, **T)), p(alloc.out("hold.success", (N,), u8, **T)),
                                 p(alloc.out("hold.end", (3, N), f64, **soa(3))), p(alloc.out("hold.live", (1,), i64)), st))
        torch.cuda.synchronize()
        assert int(alloc["hold.live"].item()) <= N - (N + 2) // 3          # every third lane finished at its first held step
        chk(lib.tt_env_set_hold(h, 0, st))

        # episode log: 2 N episodes end, the caller's arrays hold exactly `capacity` = N records
        chk(lib.tt_env_set_episode_log2(h, N, L.LOG_DETAIL, st))
        for rep in range(2):
            env.set_max_steps(torch.ones(N, dtype=i32, device=dev))
            step(f"log{rep}", 1)
        # the log's checkpoint blob, fenced directly after tt_env_episode_log_bytes()
        lblob = alloc.out("~log_blob", (int(lib.tt_env_episode_log_bytes(h)),), u8, full=False, tile_bytes=1 << 16)
        meta2 = (C.c_uint64 * 2)()
        chk(lib.tt_env_export_episode_log(h, p(lblob), C.byref(meta2), st))
        rec = dict(ret=alloc.out("drain.ret", (N,), f64, **T), len=alloc.out("drain.len", (N,), i32, **T),
                   flags=alloc.out("drain.flags", (N,), u8, **T), success=alloc.out("drain.success", (N,), u8, **T),
                   lane=alloc.out("drain.lane", (N,), i32, **T), end_step=alloc.out("drain.end_step", (N,), i64, **T),
                   comp=alloc.out("drain.comp", (len(L.LOG_COMPONENTS), N), f64, **soa(9)),
                   start=alloc.out("drain.start", (3, N), f64, **soa(3)))
        n_out, counts = alloc.out("drain.n", (1,), i64), alloc.out("drain.counts", (len(L.LOG_COUNTS),), i64)
        chk(lib.tt_env_drain_episode_log2(h, *(p(rec[k]) for k in ("ret", "len", "flags", "success", "lane", "end_step", "comp", "start")),
                                          p(n_out), p(counts), st))
        torch.cuda.synchronize()
        alloc.assert_clean("before the records are put in lane order")
        assert int(n_out.item()) == 2 * N and int(counts[0].item()) == 2 * N
        assert int(meta2[0]) == N and int(meta2[1]) == N
        header = lblob[:8 * 64].view(i64)                  # the block's 64 header words: written records, then the counters at word 48
        assert int(header[0].item()) == 2 * N and int(header[48].item()) == 2 * N
        if not compare_log_blob:
            # The records of one launch sit in the order of its atomics: fixed for one wave, not for several.  The blob's fences
            # are checked at every N (above); its CONTENTS take part in the comparison between runs only where they are fixed.
            lblob.zero_()
        # the first launch's N finishers fill the arrays, in an order that follows its atomics: lane order for the comparison
        order = torch.argsort(rec["lane"].long())
        assert torch.equal(rec["lane"][order].long(), lanes) and rec["end_step"].eq(0).all()
        for k, v in rec.items():
            v.copy_(v[:, order] if v.dim() == 2 else v[order])
        env.close()
    return run


@pytest.mark.parametrize("N", ENV_NS)
def test_env_entry_points_stay_inside_their_lanes(gpu_device, N):
    """reset (full, masked), step with a full tt_info with and without auto-reset, step_random with action_out, observe, the
    getters, random_actions, the K-step rollout, export, the held step and its read-back, and the episode log's drain into arrays
    of exactly `capacity` entries after 2 N episodes ended; tt_env_export_episode_log into a blob fenced at every N (its contents
    are compared between the runs at N = 1 and 63, where one wave fixes the record order, and only its header elsewhere)."""
    import torch
    ref = _three_ways(gpu_device, _env_run(N, compare_log_blob=N <= 64))
    assert ref["step.done"].sum().item() >= (N + 2) // 3                # the lanes whose episodes were made to end
    assert torch.isnan(ref["~reset_masked.obs"][1::3]).all() and torch.isfinite(ref["~reset_masked.obs"][0::3]).all()


def _packed_actor(alloc, net, name="~split_ws"):
    """A tt_mlp_weights of `net` with a caller-kept image buffer from `alloc` (not packed yet)."""
    import torch
    from ddpg_trucktrailer_amd import _lib as L, fused
    w = fused._fill_weights(net, L.TTMlpWeights())
    img = alloc.out(name, (int(L.load().tt_mlp_split_ws_bytes()),), torch.uint8, full=False, tile_bytes=1 << 16, also_input=True)
    w.split_ws, w.ws_packed = img.data_ptr(), 1
    return w, img


def _ring_run(N, actor, keep):
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    from ddpg_trucktrailer_amd.vec_env import TruckTrailerVecEnv
    from fenced import pattern_bytes
    SLOTS, K = 4, 5
    t, t1, tm = K % SLOTS, (K + 1) % SLOTS, (K - 1) % SLOTS

    def run(alloc):
        dev = alloc.device
        env = TruckTrailerVecEnv(N, device=dev)
        h, lib, st, p = env._h, env.lib, _stream(dev), L.ptr
        R = dict(full=False, tile_bytes=256 * 23 * 4, also_input=True)     # a slot is [N, 23] / [N]: one workgroup's rows past the end
        ring = dict(obs=alloc.out("~ring.obs", (SLOTS, N, 23), **R), act=alloc.out("~ring.act", (SLOTS, N), **R),
                    rew=alloc.out("~ring.rew", (SLOTS, N), **R), done=alloc.out("~ring.done", (SLOTS, N), torch.uint8, **R))
        # what the step reads is valid: slot t's observations, slot t-1's done flags; everything else keeps the pattern
        obs0 = torch.empty((N, 23), device=dev)
        L.check(lib.tt_env_reset(h, None, 21, p(obs0), st), h)
        ring["obs"][t].copy_(obs0)
        ring["done"][tm].copy_((torch.arange(N, device=dev) % 5 == 0).to(torch.uint8))
        before = {k: v.clone() for k, v in ring.items()}
        cursor = alloc.inp("cursor", torch.zeros(32, dtype=torch.int32, device=dev))
        k_dev = alloc.inp("k_dev", torch.tensor(K, dtype=torch.int64, device=dev))
        ou = alloc.inp("ou_state", torch.full((N,), 0.05, device=dev), tile_rows=128)
        scaled = alloc.out("act_scaled", (N,), tile_rows=128)
        w, img = _packed_actor(alloc, actor)
        keep.append(w)
        cur = L.TTRingCursor(k_dev.data_ptr(), SLOTS, 0, cursor.data_ptr())
        view = L.TTRingView(cursor.data_ptr(), ring["obs"].data_ptr(), ring["act"].data_ptr(), ring["rew"].data_ptr(),
                            ring["done"].data_ptr(), N, SLOTS)
        L.check(lib.tt_mlp_split_pack(C.byref(w), 0, p(img), None, C.byref(cur), st))
        high = float(torch.tensor(math.pi / 4, dtype=torch.float32))
        L.check(lib.tt_actor_act_ring(N, C.byref(view), C.byref(w), p(ou), 27, 0, p(k_dev), 0.2 * 1e-2, 0.15 * 0.1, high, p(scaled), st))
        env.set_step_counter(k_dev)
        L.check(lib.tt_env_step_ring(h, p(scaled), C.byref(view), 1, st), h)
        torch.cuda.synchronize()
        assert int(k_dev.item()) == K + 1 and cursor[:4].tolist() == [t, t1, tm, 1] and int(cursor[15]) == 0
        # only row t + 1 of obs and row t of act, rew and done may differ from before -- and those are written whole
        for k, row in (("obs", t1), ("act", t), ("rew", t), ("done", t)):
            for slot in range(SLOTS):
                if slot != row:
                    assert torch.equal(_bits(ring[k][slot]), _bits(before[k][slot])), (k, slot)
            width = ring[k].element_size()
            pat = pattern_bytes(ring[k].dtype).to(dev)
            words = _bits(ring[k][row]).view(-1, width)
            assert not (words == pat).all(dim=1).any(), f"{k}: slot {row} keeps prefill"
            if ring[k].is_floating_point():
                assert torch.isfinite(ring[k][row]).all(), k
        env.close()
    return run


@pytest.mark.parametrize("N", ENV_NS)
def test_ring_step_touches_one_slot_of_each_array(gpu_device, N):
    """tt_actor_act_ring and tt_env_step_ring on a ring of 4 slots prefilled with the pattern."""
    from test_gpu_policy_tile_chain import _case
    keep = []
    _three_ways(gpu_device, _ring_run(N, _case(gpu_device, 65)["actor"], keep))


# ======================================================================================================== replay draw
def _ring_data(alloc, n_envs, slots, k):
    import torch
    dev = alloc.device
    g = torch.Generator(device=dev).manual_seed(3)
    rnd = lambda *s: torch.rand(s, device=dev, generator=g)
    T = dict(tile_bytes=4 * 23 * 4)          # the draw gathers single rows: four sampled rows per workgroup
    return dict(obs=alloc.inp("ring.obs", rnd(slots, n_envs, 23) * 2 - 1, **T), act=alloc.inp("ring.act", rnd(slots, n_envs) * 2 - 1, **T),
                rew=alloc.inp("ring.rew", rnd(slots, n_envs) * 10 - 5, **T),
                done=alloc.inp("ring.done", (rnd(slots, n_envs) < 0.2).to(torch.uint8), **T),
                k_dev=alloc.inp("k_dev", torch.tensor(k, dtype=torch.int64, device=dev)), rnd=rnd)


def _batch_out(alloc, tag, rows):
    import torch
    T = dict(tile_rows=256)
    return dict(s=alloc.out(f"{tag}.s", (rows, 23), **T), a=alloc.out(f"{tag}.a", (rows,), **T), r=alloc.out(f"{tag}.r", (rows,), **T),
                s2=alloc.out(f"{tag}.s2", (rows, 23), **T), d=alloc.out(f"{tag}.d", (rows,), torch.uint8, **T),
                idx=alloc.out(f"{tag}.idx", (rows, 2), torch.int32, **T))


def _sample_args(ring, out, batch, n_envs, slots, seed, draws=1, stride=0):
    from ddpg_trucktrailer_amd import _lib as L
    p = lambda t: t.data_ptr()
    return L.TTSampleArgs(batch, n_envs, slots, 0, p(ring["k_dev"]), p(ring["obs"]), p(ring["act"]), p(ring["rew"]), p(ring["done"]), seed,
                          None, p(out["s"]), p(out["a"]), p(out["r"]), p(out["s2"]), p(out["d"]), p(out["idx"]), 0, draws, stride, None)


N_ENVS, SLOTS, K_STEPS = 37, 8, 23


def _replay_run(batch, side):
    import torch
    from ddpg_trucktrailer_amd import _lib as L

    def run(alloc):
        dev = alloc.device
        lib, st, p = L.load(), _stream(dev), L.ptr
        ring = _ring_data(alloc, N_ENVS, SLOTS, K_STEPS)
        sb = None
        if side:
            rnd, T = ring["rnd"], dict(tile_bytes=4 * 23 * 4)
            sd = dict(obs=alloc.inp("side.obs", rnd(side, 23), **T), act=alloc.inp("side.act", rnd(side), **T),
                      rew=alloc.inp("side.rew", rnd(side), **T), obs2=alloc.inp("side.obs2", rnd(side, 23), **T),
                      done=alloc.inp("side.done", (rnd(side) < 0.3).to(torch.uint8), **T))
            sb = L.TTSideBuffer(*(sd[k].data_ptr() for k in ("obs", "act", "rew", "obs2", "done")), side, 0)
        o = _batch_out(alloc, "draw", batch)
        L.check(lib.tt_ring_sample(batch, N_ENVS, SLOTS, p(ring["k_dev"]), p(ring["obs"]), p(ring["act"]), p(ring["rew"]), p(ring["done"]),
                                   1234, 0, 0, C.byref(sb) if sb is not None else None, p(o["s"]), p(o["a"]), p(o["r"]), p(o["s2"]),
                                   p(o["d"]), p(o["idx"]), st))
        if not side:       # (side tuples are single steps: an n-step draw refuses them)
            o3 = _batch_out(alloc, "nstep", batch)
            args = _sample_args(ring, o3, batch, N_ENVS, SLOTS, 1234)
            L.check(lib.tt_ring_sample_nstep(C.byref(args), 3, 0.99, st))
    return run


@pytest.mark.parametrize("side", [0, 7])
@pytest.mark.parametrize("batch", [1, 3, 5, 250])
def test_replay_draw_stays_inside_its_batch(gpu_device, batch, side):
    """tt_ring_sample with and without a side buffer of 7 tuples, and tt_ring_sample_nstep at n_step = 3; the ring itself is
    fenced and run under the three fills."""
    ref = _three_ways(gpu_device, _replay_run(batch, side))
    idx = ref["draw.idx"]
    assert ((idx[:, 0] >= -1) & (idx[:, 0] < SLOTS)).all() and (idx[:, 1] >= 0).all()
    if side and batch == 250:
        assert (idx[:, 0] == -1).any() and (idx[idx[:, 0] == -1, 1] < side).all()


def test_pack_and_sample_stays_inside_three_draws_of_five_rows(gpu_device):
    """tt_mlp_split_pack_and_sample with draws = 3, batch = 5: outputs of 15 rows, four sampled rows per workgroup; the image is
    fenced directly after tt_mlp_split_ws_bytes().  Draw u is what tt_ring_sample draws with seed + u * seed_stride."""
    import torch
    from ddpg_trucktrailer_amd import _lib as L
    from test_gpu_policy_tile_chain import _case
    actor = _case(gpu_device, 65)["actor"]
    keep = []

    def run(alloc):
        dev = alloc.device
        lib, st, p = L.load(), _stream(dev), L.ptr
        ring = _ring_data(alloc, N_ENVS, SLOTS, K_STEPS)
        o = _batch_out(alloc, "draws", 15)
        w, img = _packed_actor(alloc, actor)
        keep.append(w)
        args = _sample_args(ring, o, 5, N_ENVS, SLOTS, 1234, draws=3, stride=1000)
        L.check(lib.tt_mlp_split_pack_and_sample(C.byref(w), 0, p(img), C.byref(args), None, st))
        ref_img = alloc.out("~split_ws.alone", (img.numel(),), torch.uint8, full=False, tile_bytes=1 << 16)
        L.check(lib.tt_mlp_split_pack(C.byref(w), 0, p(ref_img), None, None, st))
        for u in range(3):
            o1 = _batch_out(alloc, f"draw{u}", 5)
            L.check(lib.tt_ring_sample(5, N_ENVS, SLOTS, p(ring["k_dev"]), p(ring["obs"]), p(ring["act"]), p(ring["rew"]), p(ring["done"]),
                                       1234 + 1000 * u, 0, 0, None, p(o1["s"]), p(o1["a"]), p(o1["r"]), p(o1["s2"]), p(o1["d"]),
                                       p(o1["idx"]), st))
    ref = _three_ways(gpu_device, run)
    assert torch.equal(ref["~split_ws"], ref["~split_ws.alone"])
    for u in range(3):
        for k in ("s", "a", "r", "s2", "d", "idx"):
            assert torch.equal(ref[f"draws.{k}"][5 * u:5 * u + 5], ref[f"draw{u}.{k}"]), (u, k)


# ================================================================================================== lone learn() chain
HYP_CRITIC = (1e-3, 0.9, 0.999, 1e-8, 1e-2)         # lr, beta1, beta2, eps, weight decay
HYP_ACTOR = (1e-4, 0.9, 0.999, 1e-8, 0.0)
TAU = 1e-3


def _learn_run(B, images, shaped, keep):
    import torch
    from ddpg_trucktrailer_amd import _lib as L, fused
    from ddpg_trucktrailer_amd.fused_learn import _NetState, _p
    from test_gpu_fused_learn import _fwd_job
    from test_gpu_policy_tile_chain import _nets

    def run(alloc):
        dev = alloc.device
        lib, st = L.load(), _stream(dev)
        f = dict(dtype=torch.float32, device=dev)
        R = dict(tile_rows=16)                     # rows of one workgroup of the learner's row kernels
        RW = dict(tile_rows=16, also_input=True)   # ... of arrays one launch writes and a later one reads
        actor, critic = _nets(dev, seed=B)
        actor_t, critic_t = _nets(dev, seed=B + 1000)
        nets = dict(actor=actor, critic=critic, actor_t=actor_t, critic_t=critic_t)
        W = {}
        for tag, net in nets.items():              # every parameter and target tensor is a fenced view
            for name, prm in net.named_parameters():
                prm.data = alloc.inp(f"{tag}.{name}", prm.data)
            w = W[tag] = fused.weights_of(net)
            if images:                             # fenced directly after tt_mlp_fc2_image_bytes(); zeroed once, then packed
                img = alloc.inp(f"{tag}.fc2_img", torch.zeros(int(lib.tt_mlp_fc2_image_bytes()), dtype=torch.uint8, device=dev),
                                tile_bytes=1 << 16)
                w.fc2_img = img.data_ptr()
                L.check(lib.tt_mlp_fc2_image_pack(C.byref(w), st))
        keep.append((nets, W))

        def saved(tag):
            t = {k: alloc.out(f"{tag}.{k}", shape, **RW) for k, shape in (("xh1", (B, 400)), ("h1", (B, 400)), ("xh2", (B, 300)),
                                                                          ("h2", (B, 300)), ("rstd1", (B,)), ("rstd2", (B,)))}
            return L.TTMlpSaved(**{k: v.data_ptr() for k, v in t.items()})

        def rows_ws(tag):
            t = {k: alloc.out(f"{tag}.{k}", shape, **RW) for k, shape in (("dpre", (B,)), ("dz", (B, 300)), ("dx2", (B, 300)),
                                                                          ("dy1", (B, 400)), ("dx1", (B, 400)))}
            return L.TTMlpBwdWs(**{k: v.data_ptr() for k, v in t.items()})

        def state(tag, net, target):
            """_NetState over fenced tensors: moments and two sets of gradients at the offsets of its flat buffers."""
            s = _NetState(net, target, B, dev)
            s.g0, s.g1, ms, vs, off = [], [], [], [], 0
            for prm, fld in zip(s.params, _FIELDS):
                k, mis = prm.numel(), (4 * off) % 256
                ms.append(alloc.inp(f"{tag}.exp_avg.{fld}", torch.zeros(k, **f), misalign=mis))
                vs.append(alloc.inp(f"{tag}.exp_avg_sq.{fld}", torch.zeros(k, **f), misalign=mis))
                s.g0.append(alloc.out(f"{tag}.grad0.{fld}", (k,), misalign=mis))
                s.g1.append(alloc.out(f"{tag}.grad.{fld}", (k,), misalign=mis, also_input=True))
                off += k
            arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            s.ms, s.vs, s.a_m, s.a_v, s.a_g = ms, vs, arr(ms), arr(vs), arr(s.g1)
            s.gs = []
            for gl in (s.g0, s.g1):
                gw = L.TTMlpWeights()
                gw.in_dim, gw.fc1_dims, gw.fc2_dims = 23, 400, 300
                for fld, t in zip(_FIELDS, gl):
                    setattr(gw, fld, t.data_ptr())
                s.gs.append(gw)
            s.img = L.TTFc2Images(net=W[tag].fc2_img, target=W[tag + "_t"].fc2_img) if images else None
            return s

        g = torch.Generator(device=dev).manual_seed(B + 1)
        s = alloc.inp("s", torch.rand((B, 23), device=dev, generator=g) * 2 - 1, **R)
        a = alloc.inp("a", torch.rand((B, 1), device=dev, generator=g) * 2.4 - 1.2, **R)
        s2 = alloc.inp("s2", torch.rand((B, 23), device=dev, generator=g) * 2 - 1, **R)
        r = alloc.inp("r", torch.randn(B, generator=g, **f), **R)
        done = alloc.inp("done", (torch.rand(B, device=dev, generator=g) < 0.3).to(torch.uint8), **R)
        st_c, st_a = state("critic", critic, critic_t), state("actor", actor, actor_t)
        keep.append((st_c, st_a))

        # tt_mlp_forward_save, actor and critic, with saved (six arrays) and dq_da
        out_a, out_c, dq0 = alloc.out("save.mu", (B,), **RW), alloc.out("save.q", (B,), **R), alloc.out("save.dq_da", (B,), **RW)
        sv0_a, sv0_c = saved("save.actor"), saved("save.critic")
        L.check(lib.tt_mlp_forward_save(B, 0, _p(s), None, C.byref(W["actor"]), _p(out_a), C.byref(sv0_a), None, st))
        L.check(lib.tt_mlp_forward_save(B, 1, _p(s), _p(a), C.byref(W["critic"]), _p(out_c), C.byref(sv0_c), _p(dq0), st))

        # tt_mlp_forward_multi with the four jobs of learn()
        mu_t, z, q, mu = alloc.out("mu_target", (B,), **RW), alloc.out("z_state", (B, 300), **RW), alloc.out("q", (B,), **RW), alloc.out("mu", (B,), **RW)
        sv_c, sv_a = saved("critic.saved"), saved("actor.saved")
        jobs = (L.TTFwdJob * 4)(_fwd_job(actor_t, 0, s2, out=mu_t), _fwd_job(critic_t, 1, s2, z_state=z),
                                _fwd_job(critic, 1, s, a, out=q, saved=sv_c), _fwd_job(actor, 0, s, out=mu, saved=sv_a))
        L.check(lib.tt_mlp_forward_multi(B, 4, jobs, st))

        # tt_mlp_backward_rows_pair with the TD prologue
        step = alloc.inp("step_dev", torch.zeros((), dtype=torch.int64, device=dev))
        bias = alloc.out("~bias_corr", (8,), full=False, also_input=True)        # TT_BIAS_CORR_FLOATS; [0..4] are written
        y, qt = alloc.out("y", (B,), **RW), alloc.out("q_target", (B,), **R)
        td = L.TTTdInput(z_state=z.data_ptr(), mu_target=mu_t.data_ptr(), target_critic=C.pointer(W["critic_t"]), reward=r.data_ptr(),
                         done=done.data_ptr(), gamma=0.99, y_out=y.data_ptr(), q_out=qt.data_ptr(), step_dev=step.data_ptr(),
                         bias_corr_out=bias.data_ptr(), adam_beta1=HYP_CRITIC[1], adam_beta2=HYP_CRITIC[2])
        ws_c, ws_a = rows_ws("critic.ws"), rows_ws("actor.ws")
        rows = (_p(q), C.byref(W["critic"]), C.byref(sv_c), C.byref(ws_c), C.byref(td), _p(mu), C.byref(W["actor"]), C.byref(sv_a),
                C.byref(ws_a), None)
        if shaped:
            pre = alloc.out("pre", (B,), **RW)
            shape = L.TTLossShape(huber_delta=1.0, pre_scale=2 * 0.01 / B, pre=pre.data_ptr())
            L.check(lib.tt_mlp_backward_rows_pair_shaped(B, 1.0 / B, *rows, C.byref(shape), st))
        else:
            L.check(lib.tt_mlp_backward_rows_pair(B, 2.0 / B, *rows, st))

        # tt_mlp_backward_weights with count = 0, both networks (the actor's rows scaled by the saved pass's dQ/da)
        no_adam = (0, None, None, None, None, None, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, None, None)
        L.check(lib.tt_mlp_backward_weights(B, 1, _p(s), _p(a), C.byref(sv_c), C.byref(ws_c), C.byref(st_c.gs[0]), None, None, 1.0,
                                            *no_adam, st))
        if shaped:
            L.check(lib.tt_mlp_backward_weights_shaped(B, 0, _p(s), None, C.byref(sv_a), C.byref(ws_a), C.byref(st_a.gs[0]), _p(dq0), _p(mu),
                                                       -1.0 / B, *no_adam, C.byref(shape), st))
        else:
            L.check(lib.tt_mlp_backward_weights(B, 0, _p(s), None, C.byref(sv_a), C.byref(ws_a), C.byref(st_a.gs[0]), _p(dq0), _p(mu),
                                                -1.0 / B, *no_adam, st))

        # tt_mlp_backward_weights with the optimizer step (critic)
        adam = lambda sx, hyp: (sx.count, sx.a_p, sx.a_m, sx.a_v, sx.a_t, _p(step), *hyp, TAU,
                                C.byref(sx.img) if sx.img is not None else None, _p(bias))
        L.check(lib.tt_mlp_backward_weights(B, 1, _p(s), _p(a), C.byref(sv_c), C.byref(ws_c), C.byref(st_c.gs[1]), None, None, 1.0,
                                            *adam(st_c, HYP_CRITIC), st))

        # tt_mlp_actor_tail, tail_words fenced directly after 64 + 2 B ints
        q_pi, dq = alloc.out("q_pi", (B,), **R), alloc.out("dq_da", (B,), **R)
        tail = alloc.inp("tail_words", torch.full((64 + 2 * B,), -1, dtype=torch.int32, device=dev), tile_bytes=4 * (64 + 2 * 1024))
        gave_up = torch.zeros(2, dtype=torch.int32).pin_memory()
        head = (B, _p(s), _p(mu), C.byref(W["critic"]), _p(q_pi), _p(dq), C.byref(sv_a), C.byref(ws_a), C.byref(st_a.gs[1]), -1.0 / B)
        if shaped:
            L.check(lib.tt_mlp_actor_tail_shaped(*head, *adam(st_a, HYP_ACTOR), _p(tail), C.c_void_p(gave_up.data_ptr()), C.byref(shape), st))
        else:
            L.check(lib.tt_mlp_actor_tail(*head, *adam(st_a, HYP_ACTOR), _p(tail), C.c_void_p(gave_up.data_ptr()), st))

        # tt_adam_soft_update with the twelve critic tensors (numel 1, 300, 400, 9200, 120000 against 256-thread workgroups)
        L.check(lib.tt_adam_soft_update(st_c.count, st_c.a_p, st_c.a_g, st_c.a_m, st_c.a_v, st_c.a_t, st_c.a_n, _p(step), *HYP_CRITIC, TAU,
                                        C.byref(st_c.img) if st_c.img is not None else None, _p(bias), st))
        torch.cuda.synchronize()
        assert int(gave_up[0]) == 0 and int(step.item()) == 1
    return run


@pytest.mark.parametrize("images", [True, False])
@pytest.mark.parametrize("B", [1, 15, 17, 250])
def test_lone_learn_chain_stays_inside_its_batch(gpu_device, B, images):
    """forward_save, forward_multi, backward_rows_pair with the TD prologue, backward_weights with count = 0 and with the
    optimizer step, actor_tail and adam_soft_update on fenced buffers; every parameter, moment, target and fc2 image included.
    With NaN behind row B - 1 of every saved and per-row gradient array all gradients, parameters and moments come out finite."""
    keep = []
    ref = _three_ways(gpu_device, _learn_run(B, images, False, keep))
    assert ref["tail_words"][64:].view(B, 2)[:, 1].eq(1).all()          # every row's word carries learn step 1


def test_shaped_learn_chain_stays_inside_its_batch(gpu_device):
    """The loss-shape variants of the rows launch, the actor's weight launch and the tail (separate kernels over the same bodies),
    with pre_out [B], once at B = 250."""
    keep = []
    ref = _three_ways(gpu_device, _learn_run(250, True, True, keep))
    assert ref["pre"].abs().max().item() > 0
