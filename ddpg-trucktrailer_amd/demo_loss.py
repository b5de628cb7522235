"""The demonstration loss of learn(): behaviour cloning on the batch rows that came from the replay side buffer, gated by a Q-filter
(Nair et al. 2018, "Overcoming Exploration in RL with Demonstrations"; include/ttenv.h: tt_demo_loss; csrc/ttdemo.hip; DESIGN.md
section 25).

    DemoLoss          bc_weight lambda > 0 and q_filter
    check_demo_loss   every combination a loop or a learner refuses with a demonstration loss, as one pure function

    actor    loss = -mean_b Q(s_b, mu(s_b)) + lambda (1/B) sum_b m_b (mu_b - a_b)^2
             a_b = the row's stored action; demo_b = the row came from the side buffer (TrajectoryRing.load_side; the draw's index
             buffer holds idx[b, 0] < 0 for such a row); m_b = demo_b and, with q_filter, q_b > q_pi_b (strict; a NaN on either side
             leaves m_b = 0).
    filter   THE TWO SIDES ARE ONE CRITIC ADAM STEP APART.  q_b = Q(s_b, a_b) from the critic forward that precedes the critic step
             of this update (the q of the TD error); q_pi_b = Q(s_b, mu(s_b)) through the UPDATED critic (the forward the actor loss
             is built from).  Both numbers exist anyway; a second critic forward on (s, a) would lengthen the launch the learn
             chain waits on longest.
    critic   unchanged: a demonstration row feeds the TD error like any other row.

The torch form is Agent(demo_loss=).learn_batch(..., demo_rows=) (agent.py): the CPU path, and the twin the kernels are tested
against."""
from ddpg_trucktrailer_amd.options import Option, finite_number, refuse


class DemoLoss(Option):
    """bc_weight: a finite number > 0.  q_filter: apply the term only where the critic rates the stored action above the policy's."""
    FIELDS = ("bc_weight", "q_filter")

    def __init__(self, bc_weight, q_filter=True):
        finite_number("demo_loss: bc_weight", bc_weight, "> 0")
        if not isinstance(q_filter, (bool, int)) or q_filter not in (0, 1):
            raise ValueError(f"demo_loss: q_filter = {q_filter!r} is not a bool")
        self.bc_weight = float(bc_weight)
        self.q_filter = bool(q_filter)

    def k(self):
        """k = 2 lambda of tt_demo_loss, formed in f64 (the struct member rounds it to f32)."""
        return 2.0 * self.bc_weight


def check_demo_loss(demo, td3=None, population=False, data_parallel=False, force_dp=False, n_step=1):
    """What is refused with a demonstration loss, each a ValueError that names demo_loss.  Those paths have kernels of their own
    (TD3, populations), cannot be tested on one GPU (data-parallel ranks, the p2p exchange, the TT_FORCE_DP launch structure) or
    cannot hold demonstration rows at all (n_step > 1: the ring refuses side tuples there)."""
    DemoLoss.expect("demo_loss", demo)
    return refuse("demo_loss", demo, td3=td3, population=population, data_parallel=data_parallel, force_dp=force_dp, n_step=n_step)
