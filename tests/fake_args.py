"""Plausible arguments of the lone learner's entry points -- plain (csrc/ttlearn.hip), with a tt_loss_shape (csrc/ttshape.hip) and with a
tt_demo_loss (csrc/ttdemo.hip) -- over made-up device addresses, and one spoiled argument at a time: the library checks them on the
host, and with one bad argument nothing reaches the GPU.  For the CPU tests of those refusals."""
import ctypes as C

_BASE = dict(rows="tt_mlp_backward_rows_pair", weights="tt_mlp_backward_weights", tail_="tt_mlp_actor_tail", fwd="tt_mlp_forward_save")
_SUFFIX = dict(plain="", shaped="_shaped", demo="_demo")


def entry_name(entry, form):
    return _BASE[entry] + _SUFFIX[form]


class Fake:
    """form: "plain", "shaped" or "demo" -- which entry point rows / weights / tail_ / fwd call.  with_shape / with_demo false: the
    struct's argument is NULL."""

    def __init__(self, L, B, form):
        addr = iter(range(0x10000, 0x10000 + 0x1000 * 400, 0x1000))
        nxt = self.nxt = lambda: next(addr)
        self.L, self.B, self.form = L, B, form
        self.actor, self.critic, self.target_critic, self.grads = (L.TTMlpWeights(*[nxt() for _ in range(12)], 23, 400, 300) for _ in range(4))
        self.saved_c, self.saved_a = (L.TTMlpSaved(*[nxt() for _ in range(6)]) for _ in range(2))
        self.ws_c, self.ws_a = (L.TTMlpBwdWs(*[nxt() for _ in range(5)]) for _ in range(2))
        self.td = L.TTTdInput(z_state=nxt(), mu_target=nxt(), target_critic=C.pointer(self.target_critic), reward=nxt(), done=nxt(),
                              gamma=0.99, y_out=nxt(), q_out=nxt(), step_dev=nxt(), window_dev=None, bias_corr_out=nxt(),
                              adam_beta1=0.9, adam_beta2=0.999)
        self.q, self.mu, self.obs, self.q_pi, self.dq_da, self.step, self.bias_corr, self.tail = (nxt() for _ in range(8))
        self.tables = [(C.c_void_p * 12)(*[nxt() for _ in range(12)]) for _ in range(4)]      # (the actor's launches read ten of them)
        self.shape = L.TTLossShape(1.5, 0.01, nxt())
        self.demo = L.TTDemoLoss(a=nxt(), idx=nxt(), q=nxt(), k=0.2, q_filter=1, dq_eff=nxt(), code=nxt())
        self.with_shape = self.with_demo = True
        self.count = 10
        self.critic_flag, self.action = 0, None          # of the weight launch
        self.fwd_critic = 1                              # of the forward
        self.scale = 1.0 / max(1, B)

    def _call(self, entry, args):
        """The entry point of this form with the common arguments, then the form's own structs, then a NULL stream."""
        if self.form != "plain" and (self.form == "shaped" or entry == "tail_"):
            args.append(C.byref(self.shape) if self.with_shape else None)
        if self.form == "demo":
            args.append(C.byref(self.demo) if self.with_demo else None)
        return getattr(self.L.load(), entry_name(entry, self.form))(*args, None)

    def rows(self):
        return self._call("rows", [self.B, self.scale, self.q, C.byref(self.critic), C.byref(self.saved_c), C.byref(self.ws_c), C.byref(self.td),
                                   self.mu, C.byref(self.actor), C.byref(self.saved_a), C.byref(self.ws_a), None])

    def _optimizer(self):
        return [self.count, *self.tables, self.step, 1e-4, 0.9, 0.999, 1e-8, 0.0, 1e-3, None, self.bias_corr]

    def weights(self):
        return self._call("weights", [self.B, self.critic_flag, self.obs, self.action, C.byref(self.saved_a), C.byref(self.ws_a),
                                      C.byref(self.grads), self.dq_da, self.mu, -self.scale, *self._optimizer()])

    def tail_(self):
        return self._call("tail_", [self.B, self.obs, self.mu, C.byref(self.critic), self.q_pi, self.dq_da, C.byref(self.saved_a),
                                    C.byref(self.ws_a), C.byref(self.grads), -self.scale, *self._optimizer(), self.tail, None])

    def fwd(self):
        return self._call("fwd", [self.B, self.fwd_critic, self.obs, self.mu, C.byref(self.critic), self.q_pi, None, self.dq_da])

    def last_error(self):
        return self.L.load().tt_last_error(None).decode()


def set_field(obj, field, value):
    return lambda f: setattr(getattr(f, obj), field, value)


# (word the message must hold, what spoils one argument) of the launches that have a plain and a shaped form
ROWS = [("n = 0", lambda f: setattr(f, "B", 0)), ("q_out", lambda f: setattr(f, "q", None)),
        ("mu_out", lambda f: setattr(f, "mu", None)), ("weights", set_field("critic", "wa", None)),
        ("weights", set_field("actor", "w3", None)), ("weights", set_field("actor", "fc1_dims", 401)),
        ("saved", set_field("saved_c", "h2", None)), ("saved", set_field("saved_a", "rstd2", None)),
        ("workspace", set_field("ws_c", "dz", None)), ("workspace", set_field("ws_a", "dx1", None)),
        ("same workspace", lambda f: setattr(f.ws_a, "dx2", f.ws_c.dx2)),
        ("TD input", set_field("td", "y_out", None)), ("TD input", set_field("td", "reward", None)),
        ("TD input", set_field("target_critic", "ba", None))]
WEIGHTS = [("critic", lambda f: setattr(f, "critic_flag", 1)), ("row_dq_da", lambda f: setattr(f, "dq_da", None)),
           ("row_mu", lambda f: setattr(f, "mu", None)), ("n = 0", lambda f: setattr(f, "B", 0)),
           ("n = 1025", lambda f: setattr(f, "B", 1025)), ("obs", lambda f: setattr(f, "obs", None)),
           ("saved", set_field("saved_a", "xh1", None)), ("workspace", set_field("ws_a", "dpre", None)),
           ("grads", set_field("grads", "b3", None)), ("count = 12", lambda f: setattr(f, "count", 12)),
           ("count = 5", lambda f: setattr(f, "count", 5)), ("optimizer step", lambda f: f.tables[1].__setitem__(3, None)),
           ("optimizer step", lambda f: setattr(f, "step", None))]
TAIL = [("n = 0", lambda f: setattr(f, "B", 0)), ("n = 1025", lambda f: setattr(f, "B", 1025)),
        ("obs", lambda f: setattr(f, "obs", None)), ("mu", lambda f: setattr(f, "mu", None)),
        ("q_out", lambda f: setattr(f, "q_pi", None)), ("dq_da", lambda f: setattr(f, "dq_da", None)),
        ("critic", set_field("critic", "wa", None)), ("saved", set_field("saved_a", "h1", None)),
        ("workspace", set_field("ws_a", "dy1", None)), ("grads", set_field("grads", "w1", None)),
        ("count = 0", lambda f: setattr(f, "count", 0)), ("optimizer step", lambda f: f.tables[0].__setitem__(9, None)),
        ("tail_words", lambda f: setattr(f, "tail", None))]
