"""The loss shape of learn(): a Huber critic loss and a pre-activation penalty on the actor (include/ttenv.h: tt_loss_shape;
csrc/ttshape.hip).

    LossShape          huber_delta (None = the MSE critic loss) and pre_penalty c >= 0
    check_loss_shape   every combination a loop or a learner refuses with a loss shape, as one pure function

    critic   huber_delta = None: loss = mse_loss(y, q), d(loss)/dq = (2/B)(q - y).
             huber_delta = d > 0: loss = torch.nn.functional.huber_loss(q, y, delta=d), mean over the rows, so
             d(loss)/dq[b] = (1/B) clamp(q[b] - y[b], -d, d).  Inside the quadratic zone that is HALF the MSE gradient: torch's
             Huber loss is 0.5 e^2 there.  The option keeps torch's definition; a learning rate tuned for MSE sees half the step.
    actor    loss = -mean Q(s, mu(s)) + c mean(pre(s)^2), pre = the head's value before tanh (rlkit's
             policy_pre_activation_weight).  Its gradient 2 c pre / B does not vanish where tanh saturates.

The torch form is Agent(loss_shape=).learn_batch (agent.py): the CPU path, and the twin the kernels are tested against."""
from ddpg_trucktrailer_amd.options import Option, finite_number, refuse


class LossShape(Option):
    """huber_delta: None, or a finite number > 0.  pre_penalty: a finite number >= 0.  LossShape() changes nothing."""
    FIELDS = ("huber_delta", "pre_penalty")

    def __init__(self, huber_delta=None, pre_penalty=0.0):
        finite_number("huber_delta", huber_delta, "> 0", or_none=True)
        finite_number("pre_penalty", pre_penalty, ">= 0")
        self.huber_delta = None if huber_delta is None else float(huber_delta)
        self.pre_penalty = float(pre_penalty)

    # what the launches take (include/ttenv.h: tt_loss_shape and the caller's scale_critic), for a batch of B rows
    def critic_scale(self, batch):
        """scale_critic of the rows launch: 2/B for the MSE loss, 1/B for the Huber loss."""
        return (2.0 if self.huber_delta is None else 1.0) / int(batch)

    def delta_arg(self):
        return 0.0 if self.huber_delta is None else self.huber_delta

    def pre_scale(self, batch):
        """k = 2c/B, formed in f64 (the struct member rounds it to f32)."""
        return 2.0 * self.pre_penalty / int(batch)


def check_loss_shape(shape, td3=None, population=False, data_parallel=False, force_dp=False):
    """What is refused with a loss shape, each a ValueError that names loss_shape.  Those paths have kernels of their own (TD3,
    populations) or cannot be tested on one GPU (data-parallel ranks, the p2p exchange, the TT_FORCE_DP launch structure)."""
    LossShape.expect("loss_shape", shape)
    return refuse("loss_shape", shape, td3=td3, population=population, data_parallel=data_parallel, force_dp=force_dp)
