"""The cases of tests/learn_ref.py's f64 learn() step with a loss shape (ddpg_trucktrailer_amd/loss_shape.py): a Huber critic loss
with delta and the actor's pre-activation penalty c mean(pre^2), both arguments of learn_ref.ref_step and learn_ref.actor_half.  What
tests/test_loss_shape_cpu.py (CPU) and tests/test_gpu_loss_shape.py (GPU) share.  States, batches and their MAX_DISCARD cap are learn_ref's, unchanged: neither option moves a pre-ReLU value of critic(s, a)
or actor(s), so a batch that learn_ref.make_batch found clean stays clean.

    delta_of(ref)       the delta of a case: the median of |q - y| of the f64 reference on the batch
    shaped(case, ..)    a learn_ref case with a shape, and learn_ref.ref_step's result on it
    saturated_state     a state whose actor head is scaled and biased so that mu is exactly +-1.0f on some rows of a batch"""
import torch

import learn_ref as R

SEED = R.SEED
# (B, scale, warm_steps, incoming step, hyperparameters, seed): fresh states at the batch sizes of the f64 test, and learn_ref's
# trained-scale cases (scale 20, step 999) that the bitwise tests run
F64_CASES = [(B, 1.0, 0, 0, "default", SEED) for B in (1, 33, 257)]
OFF_CASES = [(B, 20.0, 3, 999, "trained", SEED) for B in (1, 257)]
PATH_CASE = (33, 20.0, 3, 999, "trained", SEED)
# (huber on, c): delta on, c on (small, and large enough that the penalty dominates the actor's gradient), both together
SHAPES = [(True, 0.0), (False, 0.01), (False, 1.0), (True, 0.01), (True, 1.0)]


def delta_of(ref):
    """The case's delta: the median of |q - y| of the f64 reference (torch.median: the lower of the two middle rows of an even
    batch)."""
    return float((ref["q"] - ref["y"]).abs().median().item())


def sides(ref, delta):
    """(rows with |q - y| < delta, rows with |q - y| > delta) of the f64 reference."""
    e = (ref["q"] - ref["y"]).abs()
    return int((e < delta).sum().item()), int((e > delta).sum().item())


def shaped(case, huber, c):
    """(state, hyper, batch, delta or None, learn_ref.ref_step's result) of a learn_ref case tuple with a shape; the batch is
    learn_ref.case's own (do not write to it)."""
    state, hyper, batch, ref, _ = R.case(*case)
    delta = delta_of(ref) if huber else None
    return state, hyper, batch, delta, R.ref_step(state, batch, hyper, delta=delta, c=c)


def saturated_state(state, batch, gain=13.0, bias=-18.5):
    """`state` with the actor's head weights times `gain` and its bias set to `bias` (the target actor's head likewise).  For the B = 33
    case of F64_CASES the head's pre-activation then lies beyond +-9.3 on eleven rows, with both signs -- tanh is exactly +-1.0f in
    f32 from 9.02 on -- and within 8.7 on the others (tests/test_loss_shape_cpu.py checks that on the f64 reference).  The head comes
    after both ReLUs: no pre-ReLU value of actor(s) or critic(s, a) moves, so the batch stays clean."""
    nets = {n: {k: v.clone() for k, v in sd.items()} for n, sd in state["nets"].items()}
    for n in ("actor", "target_actor"):
        nets[n]["mu.weight"] = nets[n]["mu.weight"] * gain
        nets[n]["mu.bias"] = torch.full_like(nets[n]["mu.bias"], bias)
    return dict(state, nets=nets)
