"""What tests/test_big_counters_cpu.py (CPU) and tests/test_gpu_big_counters.py (GPU) share: the counter values at which a 64-bit device
counter crosses a width some kernel or tensor narrows it to ("Counter widths"), and the wrapped 32-bit arithmetic the
hand-over words are compared in, and the edit that starts a loop at such a counter (start_at).  Nothing is imported here but by
start_at, which takes torch; no HIP."""

# 2^24: the last width at which an f32 holds every integer (f32 step tensors); 2^31: (int)k changes sign; 2^32: (unsigned)k and the
# low Philox word wrap, the high word becomes 1; 2^40 + 5: both Philox words carry bits
EDGES = [base + d for base in (2 ** 24, 2 ** 31, 2 ** 32) for d in (-2, -1, 0, 1, 2)] + [2 ** 40 + 5]


def wrap32(x):
    """x as a signed 32-bit integer: (int)x of the kernels."""
    return ((int(x) + 2 ** 31) & 0xFFFFFFFF) - 2 ** 31


def behind(have, want):
    """A 32-bit word holding `have` has NOT reached `want` in the kernels' wrapped comparison (ttnet_common.h: epoch_reached):
    (have - want) mod 2^32, read as signed, is negative."""
    return wrap32(int(have) - int(want)) < 0


def start_at(sd, k0, u0, slots, fill_seed=None):
    """A loop's state_dict(), edited in place into one of vector step k0 with u0 learn steps made: the ring's counter and
    vector_steps, the learner's step count (TD3: the actor's count u0 // 2 and `updates` = u0, a delay of 2 that has run in step),
    the observation the next policy launch reads moved to slot k0 % slots, and -- with fill_seed -- every other ring row filled with
    a seeded pattern, so that a misdirected draw shows."""
    import torch
    ring = sd["ring"]
    obs0 = ring["obs"][ring["k"] % slots].clone()
    if fill_seed is not None:
        g = torch.Generator().manual_seed(fill_seed)
        ring["obs"].copy_(torch.rand(ring["obs"].shape, generator=g) * 2 - 1)
        ring["act"].copy_(torch.rand(ring["act"].shape, generator=g) * 2 - 1)
        ring["rew"].copy_(torch.rand(ring["rew"].shape, generator=g) * 10 - 5)
        ring["done"].copy_((torch.rand(ring["done"].shape, generator=g) < 0.2).to(torch.uint8))
    ring["obs"][k0 % slots] = obs0
    ring["k"] = k0
    sd["vector_steps"] = k0
    sd["fused_adam"]["step"] = u0
    if "actor_step" in sd["fused_adam"]:
        sd["fused_adam"]["actor_step"] = u0 // 2
        sd["fused_adam"]["updates"] = u0
    return sd
