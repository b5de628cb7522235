"""Replay memory.

ReplayBuffer mirrors DDPG/replay_buffer.py:3-34 (store_transition / sample_buffer, uniform sampling WITH
replacement through numpy's global RNG) with the storage on the device in float32 instead of float64 host
arrays.  TrajectoryRing is the vector form used by the N-env loop: the env kernel writes straight into it."""
import ctypes as C

import numpy as np
import torch

from ddpg_trucktrailer_amd import _lib as L


def check_n_step(n):
    """int(n) when an n-step draw can have that n, 1 .. TT_NSTEP_MAX (include/ttenv.h); a ValueError otherwise."""
    n = int(n)
    if not 1 <= n <= L.NSTEP_MAX:
        raise ValueError(f"n_step = {n} is outside 1 .. {L.NSTEP_MAX}")
    return n


def wrap32(x):
    """The low 32 bits of the integer x as a signed 32-bit number: what a device word holds of a 64-bit counter ((int)k in the
    kernels), and what an int32 tensor takes without an overflow error."""
    return ((int(x) + 2 ** 31) & 0xFFFFFFFF) - 2 ** 31


def slots_needed(n_step, reserve=0):
    """Ring slots an n-step draw needs, as the kernels ask: a base step with all its n steps inside the window, which leaves out
    the slot being written and the `reserve` newest ones (a pipelined draw's)."""
    return 3 + reserve + (n_step - 1)


def learn_start(n_step):
    """(learn_from, warm_steps): learn() starts at the vector step whose window holds a base step with its n steps (n = 1:
    step 2), and whole-step graphs, which always learn, after the eager steps that warm the loop up."""
    return 1 + n_step, max(4, 1 + n_step)


class ReplayBuffer:
    def __init__(self, max_size, input_shape, n_actions, device=None):
        self.mem_size = int(max_size)
        self.mem_cntr = 0
        self.device = torch.device(device) if device is not None else torch.device('cpu')
        f32 = dict(dtype=torch.float32, device=self.device)
        self.state_memory = torch.zeros((self.mem_size, *input_shape), **f32)
        self.new_state_memory = torch.zeros((self.mem_size, *input_shape), **f32)
        self.action_memory = torch.zeros((self.mem_size, n_actions), **f32)
        self.reward_memory = torch.zeros(self.mem_size, **f32)
        self.terminal_memory = torch.zeros(self.mem_size, dtype=torch.bool, device=self.device)

    def store_transition(self, state, action, reward, state_, done):
        index = self.mem_cntr % self.mem_size
        self.state_memory[index] = torch.as_tensor(np.asarray(state), dtype=torch.float32)
        self.action_memory[index] = torch.as_tensor(np.asarray(action), dtype=torch.float32)
        self.reward_memory[index] = float(reward)
        self.new_state_memory[index] = torch.as_tensor(np.asarray(state_), dtype=torch.float32)
        self.terminal_memory[index] = bool(done)
        self.mem_cntr += 1

    def store_batch(self, states, actions, rewards, states_, dones):
        """Bulk insert (expert transitions, trainv2.py:457-466): k transitions at once, wrapping around."""
        k = len(rewards)
        idx = (torch.arange(k, device=self.device) + self.mem_cntr) % self.mem_size
        self.state_memory[idx] = torch.as_tensor(states, dtype=torch.float32, device=self.device)
        self.action_memory[idx] = torch.as_tensor(actions, dtype=torch.float32, device=self.device).reshape(k, -1)
        self.reward_memory[idx] = torch.as_tensor(rewards, dtype=torch.float32, device=self.device)
        self.new_state_memory[idx] = torch.as_tensor(states_, dtype=torch.float32, device=self.device)
        self.terminal_memory[idx] = torch.as_tensor(dones, dtype=torch.bool, device=self.device)
        self.mem_cntr += k

    def sample_buffer(self, batch_size):
        max_mem = min(self.mem_cntr, self.mem_size)
        batch = torch.as_tensor(np.random.choice(max_mem, batch_size), device=self.device)
        return (self.state_memory[batch], self.action_memory[batch], self.reward_memory[batch],
                self.new_state_memory[batch], self.terminal_memory[batch])


class TrajectoryRing:
    """Time-major ring of the last T vector steps of N envs, all on the device, f32.

    obs[t] is the observation the policy saw at vector step t and obs[t+1] the one the env returned, so a
    transition (t, n) is (obs[t][n], act[t][n], rew[t][n], obs[t+1][n], done[t][n]) and each observation is
    stored ONCE (101 B per transition instead of 193 B).  For a finished env obs[t+1][n] is the first
    observation of its next episode; DDPG zeroes Q' for done transitions (DDPG_agent.py:89), so that row is
    never used.  The env kernel writes obs[t+1], rew[t], done[t] in place: inserting costs no copy."""

    def __init__(self, n_envs, slots, obs_dim, device):
        assert slots >= 3
        self.n, self.slots, self.device = n_envs, slots, device
        self.obs = torch.zeros((slots, n_envs, obs_dim), dtype=torch.float32, device=device)
        self.act = torch.zeros((slots, n_envs), dtype=torch.float32, device=device)
        self.rew = torch.zeros((slots, n_envs), dtype=torch.float32, device=device)
        self.done = torch.zeros((slots, n_envs), dtype=torch.uint8, device=device)
        self.k = 0                                                          # vector steps completed (host)
        self.k_dev = torch.zeros((), dtype=torch.int64, device=device)      # same, on the device (graph-safe)
        self._env_counts = False                                            # True: the env's step kernel advances k_dev
        self.label = None            # enable_labels(): [slots, n_envs] f32, the expert's decision on the state of (t, n)
        # stand-alone transitions (expert tuples, trainv2.py:457-466) that take part in every uniform draw.  Fixed
        # capacity and fixed addresses (a captured sampling launch keeps pointing at them); only `count` moves, and a
        # launch bakes it by value: holders of captured graphs re-capture when side_epoch moves
        self.side = None
        self.side_count = 0
        self.side_epoch = 0
        # success replay (enable_success_replay): the side rows [base, base + capacity) are the harvest's region,
        # `state` its device words (L.HARVEST_STATE), `work` the plan launch's scratch; None: off
        self.harvest = None
        self.n_step = 1              # > 1: the loop that owns the ring draws n-step tuples (DDPGRollout(n_step=...)): no side tuples
        # {t, t+1, t-1, t > 0}: ring slots of the running vector step, written on the device by the step's opening launch
        # (include/ttenv.h: tt_ring_view / tt_ring_cursor) so that captured launches need no per-position pointers
        # [4..7] / [8..11]: the cursors {t, t+1, t-1, t > 0} of even / odd steps, [0..3]: the running step's (include/ttenv.h)
        # ring cursors [0..11] + the image hand-over words [12..15] (include/ttenv.h: TT_CURSOR_INTS)
        # [16]: the step chain's progress (k + 1 once the policy launch of step k has begun): what a pipelined learn() waits for
        # [18..19]: address of the host word below (TT_CURSOR_GAVE_UP_MIRROR)
        self.cursor_dev = torch.zeros(32, dtype=torch.int32, device=device)
        # a launch that gives up waiting for the other chain marks cursor[15] AND this word of pinned (device-visible) host
        # memory: the host sees a give-up by reading its own memory, with no copy or synchronize in the loop
        self.gave_up_host = None
        if torch.device(device).type == "cuda":
            self.gave_up_host = torch.zeros(2, dtype=torch.int32).pin_memory()
            self._gave_up_np = self.gave_up_host.numpy()
            self._write_mirror_address()

    def _write_mirror_address(self):
        if self.gave_up_host is not None:
            self.cursor_dev[18:20] = torch.tensor([self.gave_up_host.data_ptr()], dtype=torch.int64).view(torch.int32).to(self.device)

    def attach(self, env):
        """Let the env's step kernel advance k_dev (tt_env_set_step_counter): one launch less per vector step.  From
        then on every env.step()/step_random() of that env counts as one stored vector step."""
        env.set_step_counter(self.k_dev)
        self._env_counts = True

    def enable_labels(self):
        """Allocate the label array [slots, n_envs] f32, zeroed: label[t][n] is the MPC expert's decision on
        the state obs[t][n] the policy acted in, written for the loop's labelled lanes (include/ttenv.h: tt_env_mpc_label_ring);
        lanes that are not labelled keep zeros.  Checkpoints carry the array only once it is enabled.  Before anything is
        captured: its address is a launch argument."""
        if self.label is None:
            self.label = torch.zeros((self.slots, self.n), dtype=torch.float32, device=self.device)
        return self.label

    @property
    def capacity(self):
        return (self.slots - 1) * self.n

    def __len__(self):
        return min(self.k, self.slots - 1) * self.n

    def slot(self, k=None):
        return (self.k if k is None else k) % self.slots

    def advance(self, steps=1):
        self.k += steps                         # host mirror
        if not self._env_counts:                # (else the env's step kernels advanced k_dev, under graph replays too)
            self.k_dev += steps

    # ---- expert / stand-alone transitions ---------------------------------------------------------------
    def load_side(self, obs, act, rew, obs2, done, capacity=None):
        """Append k stand-alone transitions (obs [k,23], act [k] or [k,1], rew [k], obs2 [k,23], done [k]) to the side
        buffer the sampler mixes into its uniform draw: the bulk form of the reference's `agent.remember` loop over
        stored expert transitions (trainv2.py:457-466).  The first call fixes the capacity (default: k)."""
        if self.n_step > 1:
            raise ValueError(f"side tuples in a ring that is drawn with n_step = {self.n_step} are not supported: they are single "
                             "steps, and their rows would need a discount of their own in the TD launch")
        if self.harvest is not None:
            raise ValueError("load_side after enable_success_replay is not supported: the harvest's region lies behind the rows "
                             "loaded before it (load the demonstrations first)")
        f = dict(dtype=torch.float32, device=self.device)
        obs = torch.as_tensor(obs, **f).reshape(-1, self.obs.shape[2])
        k = obs.shape[0]
        if self.side is None:
            cap = int(capacity) if capacity is not None else k
            d = self.obs.shape[2]
            self.side = dict(obs=torch.zeros((cap, d), **f), act=torch.zeros(cap, **f), rew=torch.zeros(cap, **f),
                             obs2=torch.zeros((cap, d), **f), done=torch.zeros(cap, dtype=torch.uint8, device=self.device))
        cap = self.side["act"].shape[0]
        if self.side_count + k > cap:
            raise ValueError(f"side buffer holds {cap} transitions, {self.side_count} used, {k} more do not fit")
        a, b = self.side_count, self.side_count + k
        self.side["obs"][a:b] = obs
        self.side["act"][a:b] = torch.as_tensor(act, **f).reshape(-1)
        self.side["rew"][a:b] = torch.as_tensor(rew, **f).reshape(-1)
        self.side["obs2"][a:b] = torch.as_tensor(obs2, **f).reshape(-1, self.obs.shape[2])
        self.side["done"][a:b] = torch.as_tensor(np.asarray(done).astype(np.uint8) if not torch.is_tensor(done) else done,
                                                 device=self.device).to(torch.uint8).reshape(-1)
        self.side_count = b
        self.side_epoch += 1
        return k

    # ---- success replay: the agent's own successful episodes, harvested into a region of the side buffer -------------------
    def enable_success_replay(self, capacity):
        """Give the side buffer a region of `capacity` rows for harvested transitions, behind the rows loaded
        so far: the side arrays are allocated, or extended by `capacity` rows (new addresses: before anything is captured).  The
        region starts empty; harvest() fills it on the device, first in first out, and expose_successes() moves side_count --
        which the samplers take by value -- up to the rows it holds.  load_side is refused from here on."""
        if self.harvest is not None:
            raise ValueError("success replay is already enabled on this ring")
        if self.n_step > 1:
            raise ValueError(f"success replay in a ring that is drawn with n_step = {self.n_step} is not supported: side tuples are single steps")
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError(f"capacity = {capacity} is not a whole number >= 1")
        f = dict(dtype=torch.float32, device=self.device)
        d, base = self.obs.shape[2], int(self.side_count)
        new = dict(obs=torch.zeros((base + capacity, d), **f), act=torch.zeros(base + capacity, **f), rew=torch.zeros(base + capacity, **f),
                   obs2=torch.zeros((base + capacity, d), **f), done=torch.zeros(base + capacity, dtype=torch.uint8, device=self.device))
        if self.side is not None:
            for k, v in new.items():
                v[:base] = self.side[k][:base]
        self.side = new
        self.side_epoch += 1
        self.harvest = dict(base=base, capacity=capacity, state=torch.zeros(8, dtype=torch.int64, device=self.device), work=None)
        self._harvest_host = torch.zeros(8, dtype=torch.int64)
        if torch.device(self.device).type == "cuda":
            self._harvest_host = self._harvest_host.pin_memory()
        return self.harvest

    def harvest_struct(self, record_capacity, tail=0, step_base=0):
        """tt_harvest over the region (include/ttenv.h), with a work array for a log of `record_capacity` records; keeps what it
        points at alive."""
        hv, sd = self.harvest, self.side
        if hv["work"] is None or hv["work"].numel() < int(record_capacity):
            hv["work"] = torch.zeros(int(record_capacity), dtype=torch.int32, device=self.device)
        a, d = hv["base"], self.obs.shape[2]
        at = lambda t, width: t.data_ptr() + a * width * t.element_size()
        return L.TTHarvest(hv["state"].data_ptr(), at(sd["obs"], d), at(sd["act"], 1), at(sd["rew"], 1), at(sd["obs2"], d),
                           at(sd["done"], 1), hv["capacity"], int(tail), int(step_base), hv["work"].data_ptr())

    def harvest_state_async(self):
        """Queue a copy of the harvest's device words to pinned host memory on the current stream; read_harvest_state() after the
        stream's next synchronize."""
        self._harvest_host.copy_(self.harvest["state"], non_blocking=True)

    def read_harvest_state(self):
        return dict(zip(L.HARVEST_STATE, (int(x) for x in self._harvest_host[:len(L.HARVEST_STATE)].tolist())))

    def expose_successes(self, written_rows):
        """side_count = base + min(written_rows, capacity): the samplers draw the region's filled rows from the next launch on.  The
        count moves only while the region fills, so holders of captured graphs (side_epoch) re-capture until then and never after."""
        hv = self.harvest
        count = hv["base"] + min(int(written_rows), hv["capacity"])
        if count != self.side_count:
            self.side_count = count
            self.side_epoch += 1
        return count - hv["base"]

    def _side_struct(self):
        if self.side is None or self.side_count == 0:
            return None
        sd = self.side
        return L.TTSideBuffer(sd["obs"].data_ptr(), sd["act"].data_ptr(), sd["rew"].data_ptr(), sd["obs2"].data_ptr(),
                              sd["done"].data_ptr(), int(self.side_count), 0)

    # ---- checkpoint ----------------------------------------------------------------------------------------
    def state_dict(self, with_replay=True):
        sd = {"k": int(self.k), "slots": int(self.slots), "n": int(self.n), "side_count": int(self.side_count)}
        if with_replay:
            sd.update(obs=self.obs.cpu(), act=self.act.cpu(), rew=self.rew.cpu(), done=self.done.cpu())
            if self.label is not None:
                sd["label"] = self.label.cpu()
            if self.side is not None:
                sd["side"] = {k: v.cpu() for k, v in self.side.items()}
        if self.harvest is not None:      # the region's base and size, the device words, and (side_count above) the exposed count
            sd["harvest"] = {"base": int(self.harvest["base"]), "capacity": int(self.harvest["capacity"]),
                             "state": self.harvest["state"].cpu(), "exposed": int(self.side_count) - int(self.harvest["base"])}
        return sd

    def load_state_dict(self, sd):
        assert (int(sd["slots"]), int(sd["n"])) == (self.slots, self.n), "replay ring geometry differs"
        mine = (self.harvest["base"], self.harvest["capacity"]) if self.harvest is not None else None
        theirs = (int(sd["harvest"]["base"]), int(sd["harvest"]["capacity"])) if "harvest" in sd else None
        if mine != theirs:
            raise ValueError(f"the ring's success-replay region (base, capacity) is {mine} and the checkpoint's ring has {theirs}")
        if self.harvest is not None:
            self.harvest["state"].copy_(sd["harvest"]["state"])
        if "obs" in sd:
            if (self.label is not None) != ("label" in sd):
                raise ValueError("the ring's label array is " + ("enabled" if self.label is not None else "off") +
                                 " and the checkpoint's ring has " + ("one" if "label" in sd else "none"))
            self.obs.copy_(sd["obs"]); self.act.copy_(sd["act"]); self.rew.copy_(sd["rew"]); self.done.copy_(sd["done"])
            if self.label is not None:
                self.label.copy_(sd["label"])
            if "side" in sd:
                cap = sd["side"]["act"].shape[0]
                if self.side is None or self.side["act"].shape[0] != cap:
                    self.side = {k: v.to(self.device).clone() for k, v in sd["side"].items()}
                else:
                    for k, v in sd["side"].items():
                        self.side[k].copy_(v)
        # the side buffer's count always follows the checkpoint: a file without side tuples (or saved with_replay=False)
        # must not leave this ring's older tuples in the draw; captured launches bake the count, so the epoch moves with it
        count = int(sd.get("side_count", 0)) if ("obs" in sd and "side" in sd) else 0
        if count != self.side_count:
            self.side_count = count
            self.side_epoch += 1
        self.k = int(sd["k"])               # the counters come back whether or not the contents did
        self.k_dev.fill_(self.k)
        # The hand-over words hold the low 32 bits of 64-bit step numbers and are compared in wrapped arithmetic (ttnet_common.h:
        # epoch_reached), so they are written RELATIVE to k ("Counter widths"): both image epochs become wrap32(k), which
        # is behind k + 1 and k + 2, what the policy launches of the next two steps wait for -- a zero is "already published" for
        # every k in [2^31 - 1, 2^32 - 2] -- and the step chain is where the counters say (TT_CURSOR_PROGRESS).  k = 0 keeps zeros.
        self.cursor_dev.zero_()
        self.cursor_dev[12:14] = wrap32(self.k)
        self.cursor_dev[16] = wrap32(self.k)
        self._write_mirror_address()
        if self.gave_up_host is not None:
            self._gave_up_np[0] = 0

    def policy_gave_up(self):
        """The mark of a launch that stopped waiting for the other chain -- a policy launch for its image, or learn()'s first launch
        for the step chain's progress (include/ttenv.h: TT_CURSOR_GAVE_UP, TT_CURSOR_PROGRESS) --, 0 = never.  The mark is the low
        32 bits of (vector step number + 1) as a signed int32: the step number + 1 itself below 2^31, negative from there to
        2^32, and 0 -- indistinguishable from "never" -- for the one step in every 2^32 with step + 1 = 0 mod 2^32 (DESIGN.md,
        "Counter widths").  Synchronises."""
        return int(self.cursor_dev[15].item()) or self.gave_up_seen()

    def gave_up_seen(self):
        """The same mark as the host sees it WITHOUT touching the GPU (the launch that gives up also sets a word of pinned host
        memory: TT_CURSOR_GAVE_UP_MIRROR): what a loop looks at between graph replays.  A mark not yet visible here is seen
        by the next look; policy_gave_up() is the exact, synchronising form."""
        return int(self._gave_up_np[0]) if self.gave_up_host is not None else 0

    def mark_gave_up_for_test(self, step):
        """What a launch of vector step `step` that gives up leaves behind (device word and host mirror): tests of the fallback."""
        self.cursor_dev[15] = wrap32(int(step) + 1)
        torch.cuda.current_stream(self.device).synchronize()
        if self.gave_up_host is not None:
            self._gave_up_np[0] = wrap32(int(step) + 1)

    def clear_gave_up(self):
        self.cursor_dev[15] = 0
        if self.gave_up_host is not None:
            torch.cuda.current_stream(self.device).synchronize()
            self._gave_up_np[0] = 0

    def view(self):
        return L.TTRingView(self.cursor_dev.data_ptr(), self.obs.data_ptr(), self.act.data_ptr(), self.rew.data_ptr(),
                            self.done.data_ptr(), self.n, self.slots)

    def cursor(self, counter=None):
        """tt_ring_cursor for a step's opening launch; counter: the device step counter to take the step number from (default:
        the ring's own; a loop whose opening launch may run before the previous env step has advanced that one passes its
        own count of opened steps)."""
        return L.TTRingCursor((self.k_dev if counter is None else counter).data_ptr(), self.slots, 0, self.cursor_dev.data_ptr())

    def _batch_bufs(self, batch_size):
        # one set per batch size, kept for the ring's lifetime: captured graphs hold these addresses, so a draw of another
        # size must not free (and hand to someone else) the buffers a graph still writes
        cache = self.__dict__.setdefault("_buf_cache", {})
        if batch_size not in cache:
            f = dict(dtype=torch.float32, device=self.device)
            d = self.obs.shape[2]
            cache[batch_size] = (torch.empty((batch_size, d), **f), torch.empty((batch_size, 1), **f), torch.empty(batch_size, **f),
                                 torch.empty((batch_size, d), **f), torch.empty(batch_size, dtype=torch.uint8, device=self.device),
                                 torch.empty((batch_size, 2), dtype=torch.int32, device=self.device))
        self._bufs = cache[batch_size]          # (the set of the latest draw)
        return self._bufs

    def sample_args(self, batch_size, seed=0, k_dev=None, reserve=0, lag=0, draws=1, seed_stride=0, wait_for_steps=False):
        """tt_sample_args for one draw into the ring's batch buffers (include/ttenv.h); keeps what it points at alive.
        draws > 1 (tt_mlp_split_pack_and_sample only): that many draws of batch_size rows, draw u with seed + u * seed_stride
        into rows [u * batch_size, (u + 1) * batch_size) of the buffers _batch_bufs(draws * batch_size).
        wait_for_steps (tt_mlp_forward_multi_sampled only): the launch first waits, in device memory, until the step chain has
        reached step *k_dev - 1 (cursor word 16, written by every ring-addressed policy launch): tt_sample_args.step_progress."""
        s, a, r, s2, dn, idx = self._batch_bufs(batch_size * max(1, int(draws)))
        p = lambda t: t.data_ptr()
        side = self._side_struct()
        self._side_keep = side
        return L.TTSampleArgs(batch_size, self.n, self.slots, int(reserve), p(self.k_dev if k_dev is None else k_dev),
                              p(self.obs), p(self.act), p(self.rew), p(self.done), int(seed) & (2 ** 64 - 1),
                              C.pointer(side) if side is not None else None, p(s), p(a), p(r), p(s2), p(dn), p(idx), int(lag),
                              max(1, int(draws)), int(seed_stride) & (2 ** 64 - 1),
                              self.cursor_dev.data_ptr() + 4 * 16 if wait_for_steps else None)

    @staticmethod
    def _check_n_step(n_step, gamma):
        n_step = check_n_step(n_step)
        if n_step > 1 and (gamma is None or not 0.0 < float(gamma) < 1.0):
            raise ValueError(f"n_step = {n_step} needs gamma in (0, 1), not {gamma}")
        return n_step

    def sample_fused(self, batch_size, seed=0, return_index=False, done_as_bool=True, k_dev=None, reserve=0, lag=0, n_step=1,
                     gamma=None):
        """sample() as ONE HIP launch (tt_ring_sample): Philox indices keyed by (seed, k_dev) + gather.
        done_as_bool=False returns the raw uint8 flags (no conversion launch; what the fused learner takes).
        k_dev / reserve / lag: another device step counter, the number of newest slots to keep out of the window and the
        number of counted steps that may still be under way (a pipelined loop samples BESIDE the env steps of the running
        and of the previous vector step: include/ttenv.h, tt_ring_sample).
        n_step > 1 (with gamma): n-step tuples (tt_ring_sample_nstep) -- r is the discounted sum of up to n rewards from a base
        step that has its n steps inside the window, s2 the observation where the sum stops and done whether an episode's end
        stopped it; the TD target then discounts q' by gamma ** n_step."""
        if self._check_n_step(n_step, gamma) > 1:
            args = self.sample_args(batch_size, seed=seed, k_dev=k_dev, reserve=reserve, lag=lag)
            s, a, r, s2, dn, idx = self._bufs
            L.check(L.load().tt_ring_sample_nstep(C.byref(args), int(n_step), float(gamma),
                                                  L.stream(self.device)))
            out = (s, a, r, s2, dn.bool() if done_as_bool else dn)
            return out + (idx,) if return_index else out
        s, a, r, s2, dn, idx = self._batch_bufs(batch_size)
        p = L.ptr
        side = self._side_struct()
        L.check(L.load().tt_ring_sample(batch_size, self.n, self.slots, p(self.k_dev if k_dev is None else k_dev), p(self.obs),
                                        p(self.act), p(self.rew), p(self.done), int(seed) & (2 ** 64 - 1), int(reserve), int(lag),
                                        C.byref(side) if side is not None else None,
                                        p(s), p(a), p(r), p(s2), p(dn), p(idx),
                                        L.stream(self.device)))
        out = (s, a, r, s2, dn.bool() if done_as_bool else dn)
        return out + (idx,) if return_index else out

    def sample(self, batch_size, generator=None, n_step=1, gamma=None, return_index=False):
        """Uniform with replacement over the stored transitions; index math on the device (k_dev), so the call
        can sit inside a captured hipGraph.
        n_step > 1 (with gamma): the torch twin of tt_ring_sample_nstep -- the same window and the same walk in f32 (a multiply
        and an add where the kernel has one fused multiply-add), with torch's random numbers for the step and the env.
        return_index: also the (slot, env) of every row's base step, [batch, 2] int64 (side rows: (-1, j))."""
        dev = self.device
        if self._check_n_step(n_step, gamma) > 1:
            return self._sample_nstep(batch_size, generator, int(n_step), float(gamma), return_index)
        u = torch.rand((2, batch_size), device=dev, generator=generator)
        avail = torch.clamp(self.k_dev, max=self.slots - 1)                          # complete transitions, in steps
        back = (u[0] * avail).long().clamp_(max=self.slots - 2)                      # 0 = newest
        t = torch.remainder(self.k_dev - 1 - back, self.slots)
        n = (u[1] * self.n).long().clamp_(max=self.n - 1)
        t1 = torch.remainder(t + 1, self.slots)
        out = [self.obs[t, n], self.act[t, n].unsqueeze(1), self.rew[t, n], self.obs[t1, n], self.done[t, n].bool()]
        if self.side is not None and self.side_count > 0:      # the same mixed uniform draw as tt_ring_sample
            m = self.side_count
            in_ring = (avail * self.n).to(torch.float64)
            pick = torch.rand(batch_size, device=dev, generator=generator, dtype=torch.float64) * (in_ring + m) < m
            j = (torch.rand(batch_size, device=dev, generator=generator) * m).long().clamp_(max=m - 1)
            sd = self.side
            for i, src in enumerate((sd["obs"][j], sd["act"][j].unsqueeze(1), sd["rew"][j], sd["obs2"][j], sd["done"][j].bool())):
                sel = pick.view(-1, *([1] * (src.dim() - 1)))
                out[i] = torch.where(sel, src, out[i])
            if return_index:
                return tuple(out) + (torch.where(pick.unsqueeze(1), torch.stack((torch.full_like(j, -1), j), 1), torch.stack((t, n), 1)),)
        if return_index:
            return tuple(out) + (torch.stack((t, n), 1),)
        return tuple(out)

    def _sample_nstep(self, batch_size, generator, n_step, gamma, return_index):
        if self.side is not None and self.side_count > 0:
            raise ValueError("an n-step draw (n_step > 1) from a ring with side tuples is not supported")
        if self.slots < slots_needed(n_step):
            raise ValueError(f"a ring of {self.slots} slots has no window for n_step = {n_step}")
        dev = self.device
        u = torch.rand((2, batch_size), device=dev, generator=generator)
        avail = torch.clamp(self.k_dev, max=self.slots - 1)
        avail_n = torch.clamp(avail - (n_step - 1), min=1)             # base steps with their n steps in the window
        back = (n_step - 1) + torch.minimum((u[0] * avail_n).long(), avail_n - 1)
        t0 = self.k_dev - 1 - back
        e = (u[1] * self.n).long().clamp_(max=self.n - 1)
        ret = torch.zeros(batch_size, dtype=torch.float32, device=dev)
        g = torch.ones((), dtype=torch.float32, device=dev)
        gam = torch.tensor(gamma, dtype=torch.float32, device=dev)
        open_ = torch.ones(batch_size, dtype=torch.bool, device=dev)   # no done met yet
        m = torch.full((batch_size,), n_step, dtype=torch.int64, device=dev)
        for j in range(n_step):
            tj = torch.remainder(t0 + j, self.slots)
            ret = torch.where(open_, ret + g * self.rew[tj, e], ret)
            ends = open_ & (self.done[tj, e] != 0)
            m = torch.where(ends, torch.full_like(m, j + 1), m)
            open_ = open_ & ~ends
            g = g * gam
        t = torch.remainder(t0, self.slots)
        t2 = torch.remainder(t0 + m, self.slots)
        out = (self.obs[t, e], self.act[t, e].unsqueeze(1), ret, self.obs[t2, e], ~open_)
        return out + (torch.stack((t, e), 1),) if return_index else out
