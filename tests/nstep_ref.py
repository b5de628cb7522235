"""What tests/test_nstep.py (CPU) and tests/test_gpu_nstep.py (GPU) share: the synthetic trajectory ring of the n-step draw's
tests and the restatement of the walk (include/ttenv.h: tt_ring_sample_nstep) in f64 numpy, from the rows a draw reports."""
import numpy as np

N_ENVS, SLOTS, K, BATCH = 512, 16, 37, 4096


def synthetic_ring(device, seed=5, done_p=0.10):
    """n_envs = 512, slots = 16, k = 37; rewards U(-5, 5), done with probability 0.10, observations and actions U(-1, 1)."""
    import torch
    from ddpg_trucktrailer_amd.replay_buffer import TrajectoryRing
    rng = np.random.RandomState(seed)
    ring = TrajectoryRing(N_ENVS, SLOTS, 23, device)
    ring.obs.copy_(torch.from_numpy(rng.uniform(-1, 1, ring.obs.shape).astype(np.float32)))
    ring.act.copy_(torch.from_numpy(rng.uniform(-1, 1, ring.act.shape).astype(np.float32)))
    ring.rew.copy_(torch.from_numpy(rng.uniform(-5, 5, ring.rew.shape).astype(np.float32)))
    ring.done.copy_(torch.from_numpy((rng.rand(*ring.done.shape) < done_p).astype(np.uint8)))
    ring.k = K
    ring.k_dev.fill_(K)
    return ring


def walk64(ring, idx, n_step, gamma):
    """The n-step rows of base steps idx [B, 2] = (slot, env), in f64: dict of s, a, R, bound, s2, D, m.  gamma enters as the f32
    number the kernel is given.  bound = 4 n 2^-24 sum_j |gamma^j r_j|: n fused multiply-adds and n - 1 roundings in g_j, each
    <= 2^-24 relative, times a margin of 2 (which also covers a separate multiply and add)."""
    obs, act, rew, done = (getattr(ring, k).cpu().numpy() for k in ("obs", "act", "rew", "done"))
    idx = np.asarray(idx.cpu().numpy(), dtype=np.int64)
    t0, e = idx[:, 0], idx[:, 1]
    slots = obs.shape[0]
    g = np.float64(np.float32(gamma))
    B = len(t0)
    R, mag = np.zeros(B), np.zeros(B)
    m, D = np.full(B, n_step), np.zeros(B, dtype=bool)
    for j in range(n_step):
        tj = (t0 + j) % slots
        live = ~D
        R += np.where(live, g ** j * rew[tj, e].astype(np.float64), 0.0)
        mag += np.where(live, np.abs(g ** j * rew[tj, e].astype(np.float64)), 0.0)
        ends = live & (done[tj, e] != 0)
        m = np.where(ends, j + 1, m)
        D |= ends
    return dict(s=obs[t0, e], a=act[t0, e], R=R, bound=4 * n_step * 2.0 ** -24 * mag, s2=obs[(t0 + m) % slots, e], D=D, m=m)


def check_rows(ring, out, n_step, gamma, k, avail):
    """out = (s, a, r, s2, d, idx) of a draw with window `avail` ending at step k - 1: exact fields exact, R within the bound,
    back inside [n - 1, avail), and (n >= 3) at least 10 % truncated and 10 % full rows.  Returns (reference, back)."""
    s, a, r, s2, d, idx = (x.cpu().numpy() for x in out)
    ref = walk64(ring, out[5], n_step, gamma)
    slots = ring.slots
    assert idx[:, 0].min() >= 0 and idx[:, 0].max() < slots and idx[:, 1].min() >= 0 and idx[:, 1].max() < ring.n
    back = (k - 1 - idx[:, 0]) % slots
    assert back.min() >= n_step - 1 and back.max() < avail, (back.min(), back.max())
    assert np.array_equal(s, ref["s"]) and np.array_equal(a.reshape(-1), ref["a"]) and np.array_equal(s2, ref["s2"])
    assert np.array_equal(d.astype(bool), ref["D"])
    err = np.abs(r.astype(np.float64) - ref["R"])
    worst = (err / np.maximum(ref["bound"], 1e-300)).max()
    print(f"n_step {n_step} gamma {gamma}: worst |R - R64| / bound = {worst:.3f}, truncated {np.mean(ref['m'] < n_step):.3f}, "
          f"full {np.mean(~ref['D']):.3f}")
    assert (err <= ref["bound"]).all(), worst
    if n_step >= 3:      # both branches of the walk carry weight
        assert np.mean(ref["m"] < n_step) >= 0.10 and np.mean(~ref["D"]) >= 0.10
    return ref, back
