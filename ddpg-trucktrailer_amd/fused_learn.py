"""FusedLearner: Agent.learn() (DDPG/DDPG_agent.py:72-106) as five hand-written HIP launches after the sampling one
(csrc/ttlearn.hip) instead of ~140 autograd kernels, for the reference-shaped networks (23-400-300-1, LayerNorm) on a
GPU; with data-parallel ranks, eight launches and the two gradient all-reduces.

Same order of operations as the reference: TD target from the target nets -> critic MSE step -> actor step through
the ALREADY UPDATED critic -> soft update of both targets.  Same optimizer arithmetic (torch.optim.Adam with the
critic's weight decay folded into the gradient).  Parity with the torch path / the reference's fixture F5 is tested
in tests/test_gpu_fused_learn.py."""
import ctypes as C

import torch

from ddpg_trucktrailer_amd import _lib as L
from ddpg_trucktrailer_amd import fused
from ddpg_trucktrailer_amd.options import compare_options, refuse, write_options
from ddpg_trucktrailer_amd.replay_buffer import check_n_step, wrap32

_p = L.ptr        # (the name this module's callers import)

_ORDER = ("fc1.weight", "fc1.bias", "bn1.weight", "bn1.bias", "fc2.weight", "fc2.bias", "bn2.weight", "bn2.bias")
_FIELDS = ("w1", "b1", "g1", "be1", "w2", "b2", "g2", "be2", "w3", "b3", "wa", "ba")


def _named(net):
    d = dict(net.named_parameters())
    head = "mu" if hasattr(net, "mu") else "q"
    names = list(_ORDER) + [head + ".weight", head + ".bias"]
    if hasattr(net, "action_value"):
        names += ["action_value.weight", "action_value.bias"]
    return [d[n] for n in names]


def _no_sync():
    return None


class _DeviceMemory:
    """numel f32 of device memory owned by someone else, for torch.as_tensor (the CUDA array interface, version 2)."""

    def __init__(self, ptr, numel):
        self.__cuda_array_interface__ = {"shape": (int(numel),), "typestr": "<f4", "data": (int(ptr), False), "version": 2}


def _device_view(ptr, numel, dev, owner=None):
    if not ptr:
        raise RuntimeError("the peer-to-peer exchange returned no gradient buffer")
    t = torch.as_tensor(_DeviceMemory(ptr, numel), device=dev)
    assert t.data_ptr() == int(ptr) and t.numel() == numel and t.dtype == torch.float32, "torch copied the external buffer"
    t._tt_owner = owner                   # (the memory lives as long as the exchange handle does)
    return t


class _NetState:
    """Per-network device buffers: flat gradient (views per parameter, in tt_mlp_weights order), Adam moments."""

    def __init__(self, net, target, batch, dev):
        self.net, self.target = net, target
        self.params = _named(net)
        self.targets = _named(target) if target is not None else None
        self.critic = hasattr(net, "action_value")
        n = sum(p.numel() for p in self.params)
        f = dict(dtype=torch.float32, device=dev)
        self.m, self.v = torch.zeros(n, **f), torch.zeros(n, **f)
        self.ms, self.vs, off = [], [], 0
        for p in self.params:
            k = p.numel()
            self.ms.append(self.m[off:off + k]); self.vs.append(self.v[off:off + k])
            off += k
        self.gstruct = L.TTMlpWeights()
        self.gstruct.in_dim, self.gstruct.fc1_dims, self.gstruct.fc2_dims = 23, 400, 300
        self.bind_flat_grad(torch.zeros(n, **f))
        self.saved_t = dict(xh1=torch.empty((batch, 400), **f), h1=torch.empty((batch, 400), **f),
                            xh2=torch.empty((batch, 300), **f), h2=torch.empty((batch, 300), **f),
                            rstd1=torch.empty(batch, **f), rstd2=torch.empty(batch, **f))
        self.saved = L.TTMlpSaved(**{k: v.data_ptr() for k, v in self.saved_t.items()})
        cnt = len(self.params)
        arr = lambda ts: (C.c_void_p * cnt)(*[t.data_ptr() for t in ts])
        self.a_p, self.a_m, self.a_v = arr(self.params), arr(self.ms), arr(self.vs)
        self.a_t = arr(self.targets) if self.targets is not None else None
        self.a_n = (C.c_int32 * cnt)(*[p.numel() for p in self.params])
        self.count = cnt
        self.images = None              # a tt_fc2_images of net and target, set by the learner when it keeps fc2 images

    def images_ref(self, on=True):
        """The tt_fc2_images argument of an optimizer step: a reference, or None without images (or with `on` false)."""
        return C.byref(self.images) if (on and self.images is not None) else None

    def bind_flat_grad(self, flat):
        """The flat gradient buffer (tt_mlp_weights order) the backward launches write and the optimizer launch / the gradient
        exchange read: a torch allocation, or a view of a site's buffer of the peer-to-peer exchange (FusedLearner.enable_p2p).
        Launches captured before a re-bind keep the old addresses: bind before capturing."""
        assert flat.numel() == sum(p.numel() for p in self.params) and flat.dtype == torch.float32
        self.flat_grad = flat
        self.grads, off = [], 0
        for p in self.params:
            k = p.numel()
            self.grads.append(flat[off:off + k].view_as(p))
            off += k
        for name, g in zip(_FIELDS, self.grads):
            setattr(self.gstruct, name, g.data_ptr())
        self.a_g = (C.c_void_p * len(self.params))(*[t.data_ptr() for t in self.grads])


def nstep_discount(gamma, n_step):
    """The TD discount of n-step tuples, gamma ** n_step, in f64 (the C structs round it to f32): the one expression behind the lone
    learner's tt_td_input.gamma and a population's tt_pop_nstep.discount, so both hold the same bits."""
    return float(gamma) if n_step == 1 else float(gamma) ** int(n_step)


def check_learn_log(capacity, every=1):
    """The (capacity, every) of a learn log, or ValueError: what every constructor that takes learn_log= / learn_log_every= refuses."""
    capacity, every = int(capacity), int(every)
    if not 1 <= capacity <= L.LEARN_LOG_MAX_CAPACITY:
        raise ValueError(f"learn_log = {capacity} records is not in [1, {L.LEARN_LOG_MAX_CAPACITY}]")
    if every < 1:
        raise ValueError(f"learn_log_every = {every} is not >= 1")
    return capacity, every


class LearnLog:
    """The learn log of one or more FusedLearners that take their updates together (include/ttenv.h: tt_learn_log_*): one record
    per update and agent with the losses, the Q / TD-target / dQ/da / mu statistics, both gradient norms and a non-finite count,
    reduced on the device by one capturable launch behind the update.  A ring of the latest `capacity` records per agent; an update
    whose step count is no multiple of `every` leaves none.  Not part of any checkpoint."""

    def __init__(self, learners, capacity, every=1):
        import numpy as np
        self._np = np
        self.capacity, self.every = check_learn_log(capacity, every)
        self.learners = list(learners)
        self.lib = L.load()
        jobs = (L.TTLearnLogJob * len(self.learners))()
        for j, fl in zip(jobs, self.learners):
            if fl.grad_sync_critic is not None or fl.p2p is not None:
                raise ValueError("a learn log with data-parallel ranks is not supported: a rank's own gradient buffer is not what "
                                 "its optimizer applies")
            j.y, j.q, j.q_pi, j.dq_da, j.mu = (t.data_ptr() for t in (fl.y, fl.q, fl.q_pi, fl.dq_da, fl.mu))
            j.grad_critic, j.grad_actor = fl.critic.flat_grad.data_ptr(), fl.actor.flat_grad.data_ptr()
            j.numel_critic, j.numel_actor = fl.critic.flat_grad.numel(), fl.actor.flat_grad.numel()
            j.step_dev = fl.step_dev.data_ptr()
        h = C.c_void_p()
        L.check(self.lib.tt_learn_log_create(len(self.learners), self.learners[0].B, jobs, self.capacity, self.every, C.byref(h)))
        self._h = h
        self.reset_cursors()

    def __del__(self):
        if getattr(self, "_h", None) is not None and L._lib is not None:
            torch.cuda.synchronize()
            L._lib.tt_learn_log_destroy(self._h)
            self._h = None

    def _stream(self):
        return L.stream(self.learners[0].dev)

    def append(self):
        """The one launch, on the current stream (capturable): a record of what the update before it on this stream left."""
        L.check(self.lib.tt_learn_log_append(self._h, self._stream()))

    def reset_cursors(self):
        """Each agent's drain cursor to its step count now (synchronises)."""
        self.cursor = [int(fl.step_dev.item()) for fl in self.learners]

    def clear(self):
        """Every slot empty and every drain cursor at its agent's step count now: after a step counter was set back."""
        L.check(self.lib.tt_learn_log_clear(self._h, self._stream()))
        self.reset_cursors()

    def drain(self, a=0):
        """Agent a's records newer than its last drain, oldest first: {"step": int64[n], "nonfinite": int32[n], one float64[n] per
        name of _lib.LEARN_LOG_VALUES, "dropped": int} -- dropped = the updates since the last drain that should have left a record
        (steps divisible by `every`) minus the records found: overwritten in the ring before anyone drained them.  Synchronises."""
        np = self._np
        cap, after = self.capacity, self.cursor[a]
        step, bad = np.empty(cap, np.int64), np.empty(cap, np.int32)
        vals = np.empty((len(L.LEARN_LOG_VALUES), cap), np.float64)
        n = C.c_int64(0)
        L.check(self.lib.tt_learn_log_drain(self._h, int(a), after, cap, step.ctypes.data, vals.ctypes.data, bad.ctypes.data, C.byref(n)))
        n = int(n.value)
        now = int(self.learners[a].step_dev.item())         # (the drain waited for the device: every update up to `now` is in)
        out = {"step": step[:n].copy(), "nonfinite": bad[:n].copy()}
        for name, col in zip(L.LEARN_LOG_VALUES, vals):
            out[name] = col[:n].copy()
        out["dropped"] = max(0, now // self.every - after // self.every) - n
        self.cursor[a] = max(now, after)
        return out


class FusedLearner:
    grad_clip, _clip = None, {}        # (without a clip: set_grad_clip gives an instance its own)

    def __init__(self, agent, batch_size, fc2_images=None, loss_shape=None, demo_loss=None, expert_lanes=None, labels=None,
                 grad_clip=None):
        """fc2_images (None = on unless TT_LEARN_F32=1): the 400 x 300 products of learn() on the f16 MFMA from pre-split
        images of the four networks' fc2 (include/ttenv.h: tt_mlp_weights.fc2_img) that the optimizer launches keep current;
        off = every product on the exact-f32 MFMA straight from the weights.
        loss_shape (None = the MSE critic loss and the plain actor loss, every launch the one it was): a loss_shape.LossShape --
        the rows launch, the actor's weight launch and the tail then go through the shaped entry points (include/ttenv.h:
        tt_loss_shape), the same number of launches.  Not with data-parallel ranks.
        demo_loss (None = no row of the batch is treated as a demonstration): a demo_loss.DemoLoss -- learn_batch then takes the
        draw's index buffer (demo_index=) and the actor's step through the demonstration entry points (include/ttenv.h:
        tt_demo_loss), the same number of launches.  Composes with loss_shape.  Not with data-parallel ranks.
        expert_lanes (with demo_loss; None = the entry points above): a whole number >= 0 -- the ring rows of lanes < expert_lanes
        are demonstration rows as well (the loop's mpc.ExpertLanes) and the actor's step goes through the
        _lanes entry points, which with 0 leave the bits of the entry points above.
        labels (with demo_loss; None = the entry points above): (first, count) -- the ring rows of lanes [first, first + count) are
        LABELLED rows (the loop's mpc.ExpertLabels): their cloning target is the ring's label array, handed
        over as a third entry or with set_label_array() before the first update, the filter does not apply to them and the actor's step goes through
        the _labels entry points.  first >= expert_lanes (None counts as 0).
        grad_clip (None = every launch the one it was): a grad_clip.GradClip -- learn_batch then runs the separate-optimizer order
        inside itself (weight gradients with no optimizer step, then the optimizer launch, at both sites; fuse_tail does not apply), and
        a network with a max_norm takes its step through tt_adam_soft_update_clipped (include/ttenv.h: tt_grad_clip; DESIGN.md section
        34).  Not with data-parallel ranks, demo_loss, expert_lanes or labels."""
        import os
        if expert_lanes is not None and not (isinstance(expert_lanes, int) and not isinstance(expert_lanes, bool) and expert_lanes >= 0):
            raise ValueError(f"expert_lanes = {expert_lanes!r} is not None or a whole number >= 0")
        if expert_lanes is not None and demo_loss is None:
            raise ValueError(f"expert_lanes = {expert_lanes} without demo_loss: the learner has nothing to do with the lanes")
        label_array = None
        if isinstance(labels, (tuple, list)) and len(labels) == 3:      # (first, count, the ring's label array)
            labels, label_array = tuple(labels[:2]), labels[2]
        if labels is not None:
            ok = isinstance(labels, (tuple, list)) and len(labels) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in labels)
            if not ok or labels[0] < 0 or labels[1] < 1:
                raise ValueError(f"labels = {labels!r} is not None or (first >= 0, count >= 1) in whole numbers")
            if demo_loss is None:
                raise ValueError(f"labels = {tuple(labels)} without demo_loss: the learner has nothing to do with the labels")
            if labels[0] < (expert_lanes or 0):
                raise ValueError(f"labels = {tuple(labels)}: first = {labels[0]} overlaps the {expert_lanes} expert lanes")
            labels = (int(labels[0]), int(labels[1]))
        assert fused.supported(agent.actor) and fused.supported(agent.critic)
        self.agent, self.B = agent, int(batch_size)
        dev = self.dev = agent.actor.fc1.weight.device
        self.lib = L.load()
        self.critic = _NetState(agent.critic, agent.target_critic, self.B, dev)
        self.actor = _NetState(agent.actor, agent.target_actor, self.B, dev)
        self.use_images = (os.environ.get("TT_LEARN_F32") != "1") if fc2_images is None else bool(fc2_images)
        # this learner's own weight structs of the four networks (the module-level ones of fused.weights_of serve inference)
        self._wstruct, self._img, self._img_seen = {}, {}, {}
        for net in self._nets():
            self._make_weights(net)
        for st in (self.actor, self.critic):
            st.images = L.TTFc2Images(net=self._img_ptr(st.net), target=self._img_ptr(st.target)) if self.use_images else None
        f = dict(dtype=torch.float32, device=dev)
        B = self.B
        self.ws_t = dict(dpre=torch.empty(B, **f), dz=torch.empty((B, 300), **f), dx2=torch.empty((B, 300), **f),
                         dy1=torch.empty((B, 400), **f), dx1=torch.empty((B, 400), **f))
        self.ws = L.TTMlpBwdWs(**{k: v.data_ptr() for k, v in self.ws_t.items()})
        # the actor's per-row gradients have a workspace of their own: its (unit) backward runs beside the critic's
        self.ws_actor_t = {k: torch.empty_like(v) for k, v in self.ws_t.items()}
        self.ws_actor = L.TTMlpBwdWs(**{k: v.data_ptr() for k, v in self.ws_actor_t.items()})
        self.mu_t, self.q_t, self.y, self.q, self.mu, self.q_pi, self.dq_da = (torch.empty(B, **f) for _ in range(7))
        self.step_dev = torch.zeros((), dtype=torch.int64, device=dev)      # learn() calls done (Adam's step count)
        # Adam's bias corrections of the running step, left by the launch that advances step_dev (tt_td_input.bias_corr_out)
        self.bias_corr = torch.zeros(8, dtype=torch.float32, device=dev)
        self.z_t = torch.empty((B, 300), **f)          # the target critic's state branch on s' (before the action enters)
        self.grad_sync_critic = self.grad_sync_actor = None
        self.p2p = None                    # the peer-to-peer gradient exchange (enable_p2p), a tt_p2p handle
        self.learn_log = None              # the learn log (enable_learn_log), a LearnLog of this one learner
        # learn()'s last two launches in ONE grid (tt_mlp_actor_tail): dQ/da is handed to the actor's weight-gradient workgroups in
        # device memory.  For the configurations learn() bounds (a small policy launch, several updates per step): its 200 waiting
        # workgroups would crowd a policy launch that owns 171 CUs.  Set by the loop (DDPGRollout), off by default.
        self.fuse_tail = False
        self.tail_words = torch.full((64 + 2 * 1024,), -1, dtype=torch.int32, device=dev)      # hints + one {step, dQ/da} word per row
        self.tail_gave_up_host = torch.zeros(2, dtype=torch.int32).pin_memory() if dev.type == "cuda" else None
        ga, gc = agent.actor.optimizer.param_groups[0], agent.critic.optimizer.param_groups[0]
        self.hyp_actor = (ga["lr"], ga["betas"][0], ga["betas"][1], ga["eps"], ga["weight_decay"])
        self.hyp_critic = (gc["lr"], gc["betas"][0], gc["betas"][1], gc["eps"], gc["weight_decay"])
        self.loss_shape, self.pre, self._shape = None, None, None
        if loss_shape is not None:
            self.set_loss_shape(loss_shape)
        self.demo_loss, self.dq_eff, self.code, self._demo_actions = None, None, None, None
        self.expert_lanes = expert_lanes
        self.labels, self.label_array, self._labels_struct, self._demo_index = labels, None, None, None
        if label_array is not None:
            self.set_label_array(label_array)
        if demo_loss is not None:
            self.set_demo_loss(demo_loss)
        if grad_clip is not None:
            self.set_grad_clip(grad_clip)

    def set_loss_shape(self, loss_shape):
        """Turn a LossShape on (before anything is captured: the constants travel by value in the launches' arguments).  The learner
        owns pre [B], the actor head's pre-activations of the batch as the rows launch recomputes them."""
        from ddpg_trucktrailer_amd.loss_shape import check_loss_shape
        check_loss_shape(loss_shape, td3=getattr(self.agent, "td3", None),
                         data_parallel=self.grad_sync_critic is not None or self.p2p is not None)
        self.loss_shape = loss_shape
        self.pre = torch.zeros(self.B, dtype=torch.float32, device=self.dev)
        self._shape = L.TTLossShape(huber_delta=loss_shape.delta_arg(), pre_scale=loss_shape.pre_scale(self.B),
                                    pre=self.pre.data_ptr())

    def _refuse_ranks_with_loss_shape(self):
        for name in ("loss_shape", "demo_loss", "grad_clip"):
            if getattr(self, name) is not None:
                refuse(name, data_parallel=True)

    def set_demo_loss(self, demo_loss):
        """Turn a DemoLoss on (before anything is captured: the constants travel by value in the launches' arguments).  The learner
        owns dq_eff [B], the derivative the actor's rows are scaled by (dQ/da with the cloning term folded in; dq_da keeps the true
        one), and code [B] int32: 0 a ring row, 1 a demonstration row the filter left out, 2 a demonstration row applied."""
        from ddpg_trucktrailer_amd.demo_loss import check_demo_loss
        check_demo_loss(demo_loss, td3=getattr(self.agent, "td3", None),
                        data_parallel=self.grad_sync_critic is not None or self.p2p is not None)
        self.demo_loss = demo_loss
        self.dq_eff = torch.zeros(self.B, dtype=torch.float32, device=self.dev)
        self.code = torch.zeros(self.B, dtype=torch.int32, device=self.dev)

    def set_grad_clip(self, grad_clip):
        """Turn a GradClip on (before anything is captured: max_norm travels by value, the buffers by address).  Per clipped network
        the learner owns the norm's partial sums (f64), out = (norm, coef) of the last update and counts = (updates, clipped updates)."""
        from ddpg_trucktrailer_amd.grad_clip import check_grad_clip
        check_grad_clip(grad_clip, td3=getattr(self.agent, "td3", None),
                        data_parallel=self.grad_sync_critic is not None or self.p2p is not None, demo_loss=self.demo_loss,
                        expert=self.expert_lanes, labels=self.labels)
        self.grad_clip, self._clip = grad_clip, {}
        for name in ("critic", "actor"):
            max_norm = getattr(grad_clip, name)
            if max_norm is None:
                continue
            partials = torch.zeros(L.GRAD_CLIP_PARTIALS, dtype=torch.float64, device=self.dev)
            out = torch.zeros(2, dtype=torch.float32, device=self.dev)
            counts = torch.zeros(2, dtype=torch.int64, device=self.dev)
            struct = L.TTGradClip(max_norm=max_norm, partials=partials.data_ptr(), out=out.data_ptr(), counts=counts.data_ptr())
            self._clip[name] = dict(partials=partials, out=out, counts=counts, struct=struct)

    def clip_stats(self):
        """Per clipped network {"norm", "coef"} of its last update -- the norm of the unclipped gradient and the coefficient applied to
        it -- and {"updates", "clipped"}, its updates so far and those with coef < 1 (counted from this learner's creation: a checkpoint
        does not carry them).  Synchronises."""
        if self.grad_clip is None:
            raise ValueError("grad_clip is off (FusedLearner(grad_clip=...))")
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)
        stats = {}
        for name, c in self._clip.items():
            (norm, coef), (updates, clipped) = c["out"].tolist(), c["counts"].tolist()
            stats[name] = {"norm": norm, "coef": coef, "updates": updates, "clipped": clipped}
        return stats

    def _demo_struct(self, actions, demo_index):
        """tt_demo_loss of one update: the batch's stored actions, the draw's index buffer, q of the first launch."""
        dl = self.demo_loss
        return L.TTDemoLoss(a=actions.data_ptr(), idx=demo_index.data_ptr(), q=self.q.data_ptr(), k=dl.k(), q_filter=int(dl.q_filter),
                            dq_eff=self.dq_eff.data_ptr(), code=self.code.data_ptr())

    def set_label_array(self, label):
        """The ring's label array [slots, N] f32 (TrajectoryRing.enable_labels) that labelled rows take their target from; before
        anything is captured (its address is a launch argument)."""
        if self.labels is None:
            raise ValueError("labels is off (FusedLearner(labels=(first, count)))")
        first, count = self.labels
        ok = torch.is_tensor(label) and label.dtype == torch.float32 and label.dim() == 2 and label.is_contiguous() and label.device == self.dev
        if not ok:
            raise ValueError("labels: the label array is not a contiguous [slots, N] f32 tensor on the learner's device")
        if first + count > label.shape[1]:
            raise ValueError(f"labels: lanes [{first}, {first + count}) leave the label array's {label.shape[1]} lanes")
        self.label_array = label
        self._labels_struct = L.TTDemoLabels(label=label.data_ptr(), n_envs=int(label.shape[1]), slots=int(label.shape[0]),
                                             first=first, count=count)

    def demo_stats(self):
        """Of the last update (synchronises): {"demo_rows": rows that came from the side buffer or, with expert_lanes, from an
        expert lane of the ring, "applied": those the filter let
        through, "bc_loss": lambda (1/B) sum over the applied rows of (mu - a)^2, formed on the host in f64 from code, mu and the
        batch's stored actions}.  With labels also "labelled": the labelled rows (code 3) -- they count as applied (not as
        demo_rows) and enter bc_loss with their label as a."""
        if self.demo_loss is None:
            raise ValueError("demo_loss is off (FusedLearner(demo_loss=...))")
        lab = {} if self.labels is None else {"labelled": 0}
        if self._demo_actions is None:
            return {"demo_rows": 0, "applied": 0, "bc_loss": 0.0, **lab}
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)
        code = self.code.cpu()
        a = self._demo_actions.double().cpu().view(-1)
        if self.labels is not None:
            from ddpg_trucktrailer_amd.mpc import gather_labels
            three = code == 3
            # (the labelled rows alone are gathered: a side row's second index counts side tuples and may be >= N)
            _, values = gather_labels(self.label_array.cpu(), self._demo_index.cpu(), *self.labels)
            a = torch.where(three, values.double(), a)
            lab = {"labelled": int(three.sum().item())}
        on = code >= 2
        d = (self.mu.double().cpu() - a)[on]
        return {"demo_rows": int(((code == 1) | (code == 2)).sum().item()), "applied": int(on.sum().item()),
                "bc_loss": float(self.demo_loss.bc_weight * (d * d).sum().item() / self.B), **lab}

    def _nets(self):
        """The networks this learner keeps weight structs and fc2 images of (a subclass with more networks overrides this)."""
        ag = self.agent
        return (ag.actor, ag.critic, ag.target_actor, ag.target_critic)

    def _states(self):
        """The trained networks' _NetStates (a subclass with more networks overrides this)."""
        return (self.actor, self.critic)

    # ------------------------------------------------------------------------------------------------- fc2 images
    def _make_weights(self, net):
        w = fused._fill_weights(net, L.TTMlpWeights())
        if self.use_images:
            img = torch.zeros(int(self.lib.tt_mlp_fc2_image_bytes()), dtype=torch.uint8, device=self.dev)   # padding stays zero
            self._img[id(net)] = img
            w.fc2_img = img.data_ptr()
        self._wstruct[id(net)] = (tuple(p.data_ptr() for p in net.parameters()), w)
        self._img_seen[id(net)] = None

    def _img_ptr(self, net):
        t = self._img.get(id(net))
        return None if t is None else t.data_ptr()

    def w(self, net):
        """The learner's tt_mlp_weights of one of its four networks (with the fc2 image when images are on)."""
        key, w = self._wstruct[id(net)]
        if key != tuple(p.data_ptr() for p in net.parameters()):      # parameter storage replaced: rebuild
            self._make_weights(net)
            for st in self._states():
                if self.use_images:
                    st.images = L.TTFc2Images(net=self._img_ptr(st.net), target=self._img_ptr(st.target))
            w = self._wstruct[id(net)][1]
        return w

    def images_current(self):
        """Have the four fc2 tensors been left alone by everything but this learner's own launches since their images were
        made?  (torch counts in-place writes per tensor; the learner's kernels update weights AND images together.)"""
        if not self.use_images:
            return True
        return all(self._img_seen[id(n)] == (n.fc2.weight._version, n.fc2.weight.data_ptr()) for n in self._nets())

    def refresh_images(self, force=False):
        """(Re)make the image of every network whose fc2 was written by anyone else -- load_state_dict, a torch optimizer,
        the hard target copy -- since the last look.  Called at the top of every eager learn step; a loop that replays
        captured graphs calls it before it replays (DDPGRollout.run)."""
        if not self.use_images:
            return
        for n in self._nets():
            seen = (n.fc2.weight._version, n.fc2.weight.data_ptr())
            if force or self._img_seen[id(n)] != seen:
                L.check(self.lib.tt_mlp_fc2_image_pack(C.byref(self.w(n)), self._stream()))
                self._img_seen[id(n)] = seen

    # -------------------------------------------------------------------------------------------------
    def _stream(self):
        return L.stream(self.dev)

    def _fresh(self):
        if self.use_images and not torch.cuda.is_current_stream_capturing():
            self.refresh_images()          # (a capture holds launches only: its owner looks before it replays)

    def _labels_ref(self):
        if self._labels_struct is None:
            raise ValueError("labels is set: the learner needs the ring's label array first (set_label_array)")
        return C.byref(self._labels_struct)

    def _fwd(self, net, obs, action, out, saved=None, dq_da=None, demo=None):
        self._fresh()
        if demo is not None:       # the critic on (s, mu(s)) with the demonstration term in dq_eff (csrc/ttdemo.hip)
            args = (self.B, 1, L.ptr(obs), L.ptr(action), C.byref(self.w(net)), L.ptr(out), C.byref(saved) if saved else None,
                    L.ptr(dq_da), C.byref(demo))
            if self.labels is not None:
                L.check(self.lib.tt_mlp_forward_save_demo_labels(*args, self.expert_lanes or 0, self._labels_ref(), self._stream()))
            elif self.expert_lanes is not None:
                L.check(self.lib.tt_mlp_forward_save_demo_lanes(*args, self.expert_lanes, self._stream()))
            else:
                L.check(self.lib.tt_mlp_forward_save_demo(*args, self._stream()))
            return
        L.check(self.lib.tt_mlp_forward_save(self.B, 1 if action is not None else 0, L.ptr(obs), L.ptr(action),
                                             C.byref(self.w(net)), L.ptr(out), C.byref(saved) if saved else None,
                                             L.ptr(dq_da), self._stream()))

    def _adam(self, st, hyp, tau):
        lr, b1, b2, eps, wd = hyp
        if self.p2p is not None:       # the mean of the ranks' gradients is formed INSIDE this launch (include/ttenv.h: tt_p2p_*)
            L.check_p2p(self.lib.tt_adam_soft_update_p2p(self.p2p, 0 if st.critic else 1, st.count, st.a_p, st.a_m, st.a_v, st.a_t, st.a_n,
                                                         L.ptr(self.step_dev), lr, b1, b2, eps, wd, tau, st.images_ref(),
                                                         L.ptr(self.bias_corr), self._stream()), self.p2p)
            return
        args = (st.count, st.a_p, st.a_g, st.a_m, st.a_v, st.a_t, st.a_n, L.ptr(self.step_dev), lr, b1, b2, eps, wd, tau, st.images_ref(),
                L.ptr(self.bias_corr))
        clip = self._clip.get("critic" if st.critic else "actor")
        if clip is not None:           # the norm's launch, then the optimizer step on coef * grad (csrc/ttclip.hip)
            L.check(self.lib.tt_adam_soft_update_clipped(*args, C.byref(clip["struct"]), self._stream()))
        else:
            L.check(self.lib.tt_adam_soft_update(*args, self._stream()))

    def enable_data_parallel(self, group=None):
        """Mean of the flat gradient buffers over the ranks at the reference's two optimizer sites (RCCL: one AVG
        all-reduce per site, straight on the flat buffer; other backends: SUM, then a divide)."""
        import torch.distributed as dist
        self._refuse_ranks_with_learn_log()
        self._refuse_ranks_with_loss_shape()
        world = dist.get_world_size(group)
        avg = dist.get_backend(group) == "nccl"

        def sync(flat):
            if avg:
                dist.all_reduce(flat, op=dist.ReduceOp.AVG, group=group)
            else:
                dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
                flat.div_(world)
        self.grad_sync_critic = lambda: sync(self.critic.flat_grad)
        self.grad_sync_actor = lambda: sync(self.actor.flat_grad)

    # ---- peer-to-peer gradient exchange ---------------------------------------------------------------------------
    def enable_p2p(self, group=None, timeout_s=None):
        """Data-parallel ranks WITHOUT collective launches on learn()'s chain (include/ttenv.h: tt_p2p_*): both flat gradient
        buffers move into a block of fine-grained device memory that the peers open through an IPC handle, and each rank's Adam
        launch reads every rank's gradients itself (sum in rank order / world: the same bits on every rank), behind a flag
        barrier in device memory.  The process group -- any backend -- only carries the handles (128 bytes per rank), once.  World size 1
        (no process group needed) runs the same launches against this rank's own block.  Call before anything is captured."""
        import os
        import torch.distributed as dist
        self._refuse_ranks_with_learn_log()
        self._refuse_ranks_with_loss_shape()
        if timeout_s is None:      # (default here: 10 s -- the first launches of a process load its kernels, and the ranks do that at
            timeout_s = float(os.environ.get("TT_P2P_TIMEOUT_S", "10"))      # their own pace; the library's own default is 2 s)
        have = dist.is_available() and dist.is_initialized()
        world, rank = (dist.get_world_size(group), dist.get_rank(group)) if have else (1, 0)
        if world > L.P2P_MAX_RANKS:
            raise ValueError(f"the peer-to-peer exchange serves up to {L.P2P_MAX_RANKS} ranks (one node), not {world}")
        numel = (C.c_int32 * 2)(self.critic.flat_grad.numel(), self.actor.flat_grad.numel())
        h = C.c_void_p()
        index = self.dev.index if self.dev.index is not None else torch.cuda.current_device()
        L.check_p2p(self.lib.tt_p2p_create(index, rank, world, 2, numel, C.byref(h)))
        if timeout_s is not None:
            L.check_p2p(self.lib.tt_p2p_set_timeout(h, float(timeout_s)), h)
        mine = C.create_string_buffer(L.P2P_HANDLE_BYTES)
        L.check_p2p(self.lib.tt_p2p_export(h, mine), h)
        if world > 1:
            handles = [None] * world
            dist.all_gather_object(handles, bytes(mine.raw), group=group)
            for r, hb in enumerate(handles):
                if r != rank:
                    L.check_p2p(self.lib.tt_p2p_attach(h, r, C.create_string_buffer(hb, L.P2P_HANDLE_BYTES)), h)
            dist.barrier(group)            # every rank has opened every block before anyone launches into it
        self.p2p, self._p2p_group, self._p2p_world = h, group, world
        for site, st in enumerate((self.critic, self.actor)):
            st.bind_flat_grad(_device_view(self.lib.tt_p2p_grad(h, site), st.flat_grad.numel(), self.dev, owner=self))
        self.grad_sync_critic = self.grad_sync_actor = _no_sync       # (learn_batch's data-parallel order: separate Adam launches)
        self.p2p_reset()                   # (the fresh block's zeros are behind the next epoch only below 2^31 - 1 learn steps)

    # ---- learn log -----------------------------------------------------------------------------------------------
    def _refuse_ranks_with_learn_log(self):
        if self.learn_log is not None:
            raise ValueError("data-parallel ranks with a learn log are not supported: a rank's own gradient buffer is not what its "
                             "optimizer applies")

    def enable_learn_log(self, capacity, every=1):
        """Turn the learn log on (LearnLog; include/ttenv.h: tt_learn_log_*): from now on learn_batch ends with one more launch
        that leaves a record of the update -- critic and actor loss, Q / TD-target / |TD| / |dQ/da| / mu statistics, both gradient
        norms, a non-finite count -- in a ring of the latest `capacity` records in device memory, for every update whose step
        count is a multiple of `every`.  Capturable: call it before anything is captured.  drain_learn_log() collects the records.
        The log is NOT part of a checkpoint (state_dict): load_state_dict empties it.  Not with data-parallel ranks."""
        if self.learn_log is not None:
            raise ValueError("the learn log is already on")
        self.learn_log = LearnLog([self], capacity, every)

    def append_learn_log(self):
        """The learn log's launch alone, on the current stream: a record of whatever the learner's buffers hold now."""
        if self.learn_log is None:
            raise ValueError("the learn log is off (enable_learn_log)")
        self.learn_log.append()

    def drain_learn_log(self):
        """The records newer than the last drain as a dict of numpy columns, and "dropped" (LearnLog.drain).  Synchronises."""
        if self.learn_log is None:
            raise ValueError("the learn log is off (enable_learn_log)")
        return self.learn_log.drain(0)

    def tail_gave_up(self):
        """0, or the learn step at which a weight-gradient workgroup of tt_mlp_actor_tail stopped waiting for dQ/da (that learn() is
        garbage).  Reads host memory only."""
        return int(self.tail_gave_up_host[0]) if self.tail_gave_up_host is not None else 0

    def p2p_gave_up(self):
        """0, or the learn step at which this rank's Adam launch stopped waiting for a peer's gradients (it then used whatever the
        buffers held: the ranks have diverged).  Reads host memory only."""
        return int(self.lib.tt_p2p_gave_up(self.p2p)) if self.p2p is not None else 0

    def p2p_reset(self):
        """After the learn-step counter was set (a resume): arrival words of earlier runs must not satisfy new waits.  The words
        become the low 32 bits of the step count as it stands, which is behind the next update's epoch in the kernel's wrapped
        comparison wherever the count is (tt_p2p_reset_at); zeros are behind it only while the count is below 2^31 - 1."""
        if self.p2p is None:
            return
        import torch.distributed as dist
        multi = self._p2p_world > 1
        torch.cuda.synchronize(self.dev)
        if multi:
            dist.barrier(self._p2p_group)
        L.check_p2p(self.lib.tt_p2p_reset_at(self.p2p, int(self.step_dev.item()), self._stream()), self.p2p)
        if multi:
            dist.barrier(self._p2p_group)

    # learn() in the three pieces the two gradient all-reduces cut it into (each piece is pure kernel launches on the
    # current stream, so a data-parallel loop can capture each as a hipGraph and keep only the collectives eager)
    def phase_a(self, states, actions, rewards, states_, done_u8, fuse_adam, window_dev=None, sample=None, image=None, n_step=1):
        """Forwards, TD target, critic backward (+ the critic's Adam/soft update in the same launch when fuse_adam).
        sample: a tt_sample_args (TrajectoryRing.sample_args) whose batch buffers ARE the five tensors given -- the forward
        launch then makes the replay draw itself (tt_mlp_forward_multi_sampled) instead of reading a batch drawn before.
        image: (packed actor weights struct, tt_ring_cursor whose k_dev is a snapshot word, that word's tensor) -- the critic's
        backward launch then also packs the vector step's policy image (tt_image_job; needs `sample`: the forward launch leaves
        the step number in the snapshot word).
        n_step > 1: n-step returns (include/ttenv.h: tt_ring_sample_nstep).  With `sample` the forward launch makes the n-step
        draw (tt_mlp_forward_multi_sampled_nstep); without it the five tensors must hold a batch drawn with the same n_step
        (TrajectoryRing.sample_fused).  Either way the TD target discounts q' by gamma ** n_step."""
        ag, B = self.agent, self.B
        n_step = check_n_step(n_step)
        self._fresh()
        # DDPG_agent.py:85-93 and :87, :101.  Only the target critic's LAST step needs the target actor's action (it enters
        # after LayerNorm2, networks.py:62-66), so four passes run side by side -- target actor on s', the target critic's
        # state branch on s', Q(s,a), mu(s), each filling 16 of the 256 CUs -- and the critic's backward then finishes
        # q'(s', mu'(s')) and the TD target.  The four are ONE launch (tt_mlp_forward_multi): a stream fork/join inside
        # a captured graph costs more than the kernel it would hide
        jobs = self.fwd_jobs(states, actions, states_)
        if sample is not None:
            assert (sample.s_out, sample.a_out, sample.s2_out) == (states.data_ptr(), actions.data_ptr(), states_.data_ptr())
            snap = L.ptr(image[2]) if image is not None else None
            if n_step > 1:
                L.check(self.lib.tt_mlp_forward_multi_sampled_nstep(B, 4, jobs, C.byref(sample), n_step, float(ag.gamma), snap,
                                                                    self._stream()))
            else:
                L.check(self.lib.tt_mlp_forward_multi_sampled(B, 4, jobs, C.byref(sample), snap, self._stream()))
        else:
            L.check(self.lib.tt_mlp_forward_multi(B, 4, jobs, self._stream()))
        self._rows(rewards, done_u8, window_dev, image, n_step)
        self._weights(self.critic, self.hyp_critic, ag.tau, states, actions, self.ws, adam=fuse_adam)

    def fwd_jobs(self, states, actions, states_):
        """learn()'s four forwards (tt_fwd_job[4]) on a batch, in their order: the target actor and the target critic's state
        branch on s', Q(s, a) and mu(s) with what their backward needs.  (Also a population's: PopulationLearner.)"""
        ag = self.agent
        jobs = (L.TTFwdJob * 4)()
        for j, (net, crit, obs, act, out, saved, zst) in enumerate((
                (ag.target_actor, 0, states_, None, self.mu_t, None, None),
                (ag.target_critic, 1, states_, None, None, None, self.z_t),
                (ag.critic, 1, states, actions, self.q, self.critic.saved, None),
                (ag.actor, 0, states, None, self.mu, self.actor.saved, None))):
            jobs[j].critic, jobs[j].obs, jobs[j].action = crit, L.ptr(obs), L.ptr(act)
            jobs[j].w, jobs[j].out = C.pointer(self.w(net)), L.ptr(out)
            jobs[j].saved = C.pointer(saved) if saved is not None else None
            jobs[j].dq_da, jobs[j].z_state = None, L.ptr(zst)
        return jobs

    def td_input(self, rewards, done_u8, window_dev=None, n_step=1):
        """The input of the TD prologue of the critic's per-row backward (tt_td_input).  (Also a population's: PopulationLearner.)
        n_step > 1: the rows are n-step tuples, and every row that the prologue discounts has the discount gamma ** n_step."""
        ag = self.agent
        gamma = nstep_discount(ag.gamma, n_step)         # (f64; the struct member rounds it to f32)
        return L.TTTdInput(z_state=self.z_t.data_ptr(), mu_target=self.mu_t.data_ptr(),
                           target_critic=C.pointer(self.w(ag.target_critic)), reward=rewards.data_ptr(),
                           done=done_u8.data_ptr(), gamma=gamma, y_out=self.y.data_ptr(),
                           q_out=self.q_t.data_ptr(), step_dev=self.step_dev.data_ptr(), window_dev=L.ptr(window_dev),
                           bias_corr_out=self.bias_corr.data_ptr(), adam_beta1=self.hyp_critic[1], adam_beta2=self.hyp_critic[2])

    def pop_net(self, st, ws, hyp):
        """One trained network's tt_pop_net from its _NetState, per-row workspace and optimizer hyperparameters: what a
        population's descriptors (PopulationLearner) and TD3's (td3.TD3Learner) hold per network."""
        lr, b1, b2, eps, wd = hyp
        return L.TTPopNet(C.pointer(ws), C.pointer(st.gstruct), st.count, 0, C.cast(st.a_p, C.c_void_p), C.cast(st.a_m, C.c_void_p),
                          C.cast(st.a_v, C.c_void_p), C.cast(st.a_t, C.c_void_p), lr, b1, b2, eps, wd, self.agent.tau,
                          C.pointer(st.images) if st.images is not None else None)

    def _rows(self, rewards, done_u8, window_dev=None, image=None, n_step=1):
        """learn()'s per-row backward launch (tt_mlp_backward_rows_pair) after the forwards of phase_a."""
        ag, B = self.agent, self.B
        # critic step (DDPG_agent.py:95-98); its backward launch first finishes q'(s', mu'(s')) and the TD target for its
        # rows (tt_td_input)
        td = self.td_input(rewards, done_u8, window_dev, n_step)
        # ... and, on other workgroups of the same launch, the ACTOR's per-row backward for a unit gradient: it is linear in
        # the row's d(loss)/d(pre-tanh), which needs the updated critic and is applied in phase_b (include/ttenv.h)
        job = C.byref(L.TTImageJob(C.pointer(image[0]), C.pointer(image[1]))) if image is not None else None
        shape = self.loss_shape       # with one: the same grid with the Huber clamp and the actor's pre-activations (csrc/ttshape.hip)
        args = [B, 2.0 / B if shape is None else shape.critic_scale(B), L.ptr(self.q), C.byref(self.w(ag.critic)), C.byref(self.critic.saved),
                C.byref(self.ws), C.byref(td), L.ptr(self.mu), C.byref(self.w(ag.actor)), C.byref(self.actor.saved), C.byref(self.ws_actor), job]
        if shape is None:
            L.check(self.lib.tt_mlp_backward_rows_pair(*args, self._stream()))
        else:
            L.check(self.lib.tt_mlp_backward_rows_pair_shaped(*args, C.byref(self._shape), self._stream()))

    def _weights(self, st, hyp, tau, obs, action, ws, adam, row=None):
        """The weight-gradient launch (tt_mlp_backward_weights), with Adam + soft update in it when `adam`."""
        lr, b1, b2, eps, wd = hyp
        dq, mu, sc = row if row is not None else (None, None, 1.0)
        shaped = self.loss_shape is not None and not st.critic and row is not None      # the actor's rows also carry the penalty's term
        args = [self.B, 1 if st.critic else 0, L.ptr(obs), L.ptr(action), C.byref(st.saved), C.byref(ws), C.byref(st.gstruct),
                L.ptr(dq), L.ptr(mu), float(sc), st.count if adam else 0, st.a_p, st.a_m, st.a_v, st.a_t, L.ptr(self.step_dev),
                lr, b1, b2, eps, wd, tau, st.images_ref(adam), L.ptr(self.bias_corr)]      # (the shaped form ignores the action)
        if shaped:
            L.check(self.lib.tt_mlp_backward_weights_shaped(*args, C.byref(self._shape), self._stream()))
        else:
            L.check(self.lib.tt_mlp_backward_weights(*args, self._stream()))

    def phase_b(self, states, separate_adam, demo=None):
        """[critic Adam/soft update when not already applied,] then the actor step through the UPDATED critic
        (DDPG_agent.py:100-104): Q(s, mu(s)) with dQ/da (a critic forward), and the actor's weight gradients from its unit
        per-row backward scaled by -(1/B) dQ/da (1 - mu^2) per row (+ its Adam unless separate_adam).
        demo: a tt_demo_loss (_demo_struct) -- the same launches through the demonstration entry points, the rows scaled by dq_eff."""
        ag, B = self.agent, self.B
        if separate_adam:
            self._adam(self.critic, self.hyp_critic, ag.tau)
        elif self.fuse_tail:
            self._fresh()
            st = self.actor
            lr, b1, b2, eps, wd = self.hyp_actor
            args = [B, L.ptr(states), L.ptr(self.mu), C.byref(self.w(ag.critic)), L.ptr(self.q_pi), L.ptr(self.dq_da), C.byref(st.saved),
                    C.byref(self.ws_actor), C.byref(st.gstruct), -1.0 / B, st.count, st.a_p, st.a_m, st.a_v, st.a_t, L.ptr(self.step_dev),
                    lr, b1, b2, eps, wd, ag.tau, st.images_ref(), L.ptr(self.bias_corr), L.ptr(self.tail_words),
                    C.c_void_p(self.tail_gave_up_host.data_ptr())]
            shape = C.byref(self._shape) if self.loss_shape is not None else None
            if demo is not None and self.labels is not None:
                L.check(self.lib.tt_mlp_actor_tail_demo_labels(*args, shape, C.byref(demo), self.expert_lanes or 0, self._labels_ref(),
                                                               self._stream()))
            elif demo is not None and self.expert_lanes is not None:
                L.check(self.lib.tt_mlp_actor_tail_demo_lanes(*args, shape, C.byref(demo), self.expert_lanes, self._stream()))
            elif demo is not None:            # (the demonstration form takes the shape as well, NULL without one)
                L.check(self.lib.tt_mlp_actor_tail_demo(*args, shape, C.byref(demo), self._stream()))
            elif shape is not None:
                L.check(self.lib.tt_mlp_actor_tail_shaped(*args, shape, self._stream()))
            else:
                L.check(self.lib.tt_mlp_actor_tail(*args, self._stream()))
            return
        self._fwd(ag.critic, states, self.mu, self.q_pi, dq_da=self.dq_da, demo=demo)
        self._weights(self.actor, self.hyp_actor, ag.tau, states, None, self.ws_actor, adam=not separate_adam,
                      row=(self.dq_eff if demo is not None else self.dq_da, self.mu, -1.0 / B))

    def phase_c(self):
        self._adam(self.actor, self.hyp_actor, self.agent.tau)

    def learn_batch(self, states, actions, rewards, states_, done_u8, window_dev=None, sample=None, image=None, n_step=1,
                    demo_index=None):
        """states, states_ [B,23] f32; actions [B,1] f32; rewards [B] f32; done_u8 [B] uint8 -- all contiguous.
        window_dev: device int64 advanced by the critic's backward launch (a pipelined loop's sampling window).
        sample: see phase_a (the five tensors are then the draw's batch buffers, filled by learn()'s first launch).
        n_step: see phase_a (n-step returns; 1 = the one-step learn(), launch for launch).
        demo_index (with demo_loss; else it must be None): the draw's [B, 2] int32 index buffer of this batch (TrajectoryRing: the
        sixth of its batch buffers) -- row b is a demonstration row where demo_index[b, 0] < 0, or, with expert_lanes, where
        demo_index[b, 1] < expert_lanes; with labels, a ring row of a labelled lane is a labelled row."""
        assert states.shape[0] == self.B and done_u8.dtype == torch.uint8
        demo = None
        if self.demo_loss is not None:
            from ddpg_trucktrailer_amd.demo_loss import check_demo_loss
            if demo_index is None:
                raise ValueError("demo_loss is set: learn_batch needs demo_index, the draw's [B, 2] int32 index buffer")
            check_demo_loss(self.demo_loss, n_step=n_step)
            assert demo_index.dtype == torch.int32 and tuple(demo_index.shape) == (self.B, 2) and demo_index.is_contiguous()
            assert actions.is_contiguous() and actions.numel() == self.B
            demo = self._demo_struct(actions, demo_index)
            self._demo_actions, self._demo_index = actions, demo_index
        elif demo_index is not None:
            raise ValueError("demo_index without demo_loss (FusedLearner(demo_loss=...))")
        dp = self.grad_sync_critic is not None
        if dp:
            self._refuse_ranks_with_learn_log()
            self._refuse_ranks_with_loss_shape()
        separate = dp or self.grad_clip is not None      # a clip needs the whole gradient before the optimizer: the ranks' order, no collective
        assert image is None or sample is not None
        self.phase_a(states, actions, rewards, states_, done_u8, fuse_adam=not separate, window_dev=window_dev, sample=sample, image=image,
                     n_step=n_step)
        if dp:
            self.grad_sync_critic()
        self.phase_b(states, separate_adam=separate, demo=demo)
        if dp:
            self.grad_sync_actor()
        if separate:
            self.phase_c()
        if self.learn_log is not None:
            self.learn_log.append()

    # ---- checkpoint ---------------------------------------------------------------------------------------------
    def state_dict(self):
        """Adam moments of both networks (flat, tt_mlp_weights order), the learn-step count and the loss shape when one is set,
        the demonstration loss and the gradient clip likewise.  (The learn log is not in it.)"""
        sd = {"step": int(self.step_dev.item()),
              "actor": {"m": self.actor.m.cpu(), "v": self.actor.v.cpu()},
              "critic": {"m": self.critic.m.cpu(), "v": self.critic.v.cpu()}}
        write_options(sd, loss_shape=self.loss_shape, demo_loss=self.demo_loss, grad_clip=self.grad_clip)
        return sd

    def load_state_dict(self, sd):
        compare_options(sd, "learner", loss_shape=self.loss_shape, demo_loss=self.demo_loss, grad_clip=self.grad_clip)
        for name in ("actor", "critic"):
            st = getattr(self, name)
            st.m.copy_(sd[name]["m"]); st.v.copy_(sd[name]["v"])
        self.step_dev.fill_(int(sd["step"]))
        self.reset_tail_words(int(sd["step"]))
        self.p2p_reset()
        if self.learn_log is not None:     # (a step counter set back must not meet records from its future)
            self.learn_log.clear()

    def reset_tail_words(self, step):
        """After the count the actor tail keys its words by was set to `step` (FusedLearner: the learn step; TD3Learner: the actor
        step): no word of an earlier run may match the epoch of the next tail launch.  tail_row and tail_wait_hints
        (csrc/ttlearn_bodies.h) compare a word's upper half with (int)(step + 1) for EQUALITY, so a stale word is harmless exactly
        when it differs from wrap32(step + 1).  The fill is -1, a fresh learner's, which differs from every epoch but that of
        step = 2^32 - 2 mod 2^32; there it is -2.  Every later launch finds the words of the launch before it, one step behind
        its own epoch."""
        self.tail_words.fill_(-1 if wrap32(step + 1) != -1 else -2)

    def step_counts(self):
        """The learner's step counts as exact integers (a checkpoint keeps them beside the torch optimizers' f32 `step` tensors,
        which hold integers exactly only up to 2^24).  Synchronises."""
        return {"step": int(self.step_dev.item())}

    def set_step_counts(self, counts):
        """step_counts() back, after import_from_optimizers (whose f32 step may be rounded)."""
        self.step_dev.fill_(int(counts["step"]))
        self.reset_tail_words(int(counts["step"]))
        self.p2p_reset()

    # ---- checkpoint interoperability with the torch optimizers ------------------------------------------
    # (the optimizers' own `step` stays an f32 tensor, as torch.optim.Adam makes it -- its fused form reads it as such --, so past
    # 2^24 it is the learn step ROUNDED: checkpoint.py carries step_counts() beside the optimizer state)
    def export_to_optimizers(self):
        step = self.step_dev.to(torch.float32).clone()
        for st, opt in ((self.actor, self.agent.actor.optimizer), (self.critic, self.agent.critic.optimizer)):
            for p, m, v in zip(st.params, st.ms, st.vs):
                opt.state[p] = {"step": step.clone(), "exp_avg": m.view_as(p).clone(), "exp_avg_sq": v.view_as(p).clone()}

    def import_from_optimizers(self):
        for st, opt in ((self.actor, self.agent.actor.optimizer), (self.critic, self.agent.critic.optimizer)):
            for p, m, v in zip(st.params, st.ms, st.vs):
                s = opt.state.get(p)
                if s:
                    m.copy_(s["exp_avg"].reshape(-1)); v.copy_(s["exp_avg_sq"].reshape(-1))
                    self.step_dev.fill_(int(float(s["step"])))
        if self.learn_log is not None:
            self.learn_log.clear()
