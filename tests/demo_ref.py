"""The cases of tests/learn_ref.py's f64 learn() step with a demonstration loss (ddpg_trucktrailer_amd/demo_loss.py): a behaviour-cloning
term lambda (1/B) sum_b m_b (mu_b - a_b)^2 on the demonstration rows of the batch, m_b gated by the Q-filter q_b > q_pi_b; lam, the
filter and the rows' mask are arguments of learn_ref.ref_step, the applied mask one of learn_ref.actor_half.  What
tests/test_demo_loss_cpu.py (CPU) and tests/test_gpu_demo_loss.py (GPU) share.  States and batches are learn_ref.case's, unchanged:
the option moves no pre-ReLU value of critic(s, a) or actor(s), so a batch that learn_ref.make_batch found clean stays clean.

    demo_mask(B)        THE RULE that names the demonstration rows of a batch: rows b with b % 3 == 0 (row 0 alone at B = 1)
    filter_of           the f64 filter of a step: q (the critic BEFORE the update) > q_pi (the UPDATED critic), the margin below
                        which a row is undecided, and the rows on each side
    ref_step            learn_ref.ref_step on the rows of demo_mask; also returns code
    zero_action_case    a state and batch (action_value weights zero, stored actions zero) with dQ/da exactly 0 on every row

The two sides of the filter are one critic Adam step apart, by definition (demo_loss.py): q is the first forward's, q_pi the third's.
A row whose |q - q_pi| is below FILTER_MARGIN -- the sum of the two 2e-5 max(1, max |.|) bounds tests/test_gpu_learn_shapes.py puts on
q and q_pi -- can fall on either side in f32: it is "undecided", a test accepts either code for it and forms the reference gradient
with the mask the code under test chose (learn_ref's rule for dQ/da near a ReLU boundary).  Undecided rows may be at most
learn_ref.MAX_DISCARD of the demonstration rows, and at B >= 33 each side of the filter must hold at least MIN_SIDE of them."""
import functools

import torch

import learn_ref as R
import shape_ref as S

MIN_SIDE = 1.0 / 8.0
MAX_UNDECIDED = R.MAX_DISCARD
F64_CASES = S.F64_CASES
OFF_CASES = S.OFF_CASES
PATH_CASE = S.PATH_CASE
# (lambda, q_filter): small and large (where the cloning term dominates the actor's gradient), with and without the filter
DEMOS = [(0.1, True), (10.0, True), (0.1, False), (10.0, False)]


def demo_mask(B):
    """[B] bool: the demonstration rows of a batch of B rows -- b % 3 == 0."""
    return torch.arange(B) % 3 == 0


def demo_index(B, device="cpu"):
    """The draw's [B, 2] int32 index buffer that marks demo_mask(B): (-1, j) for the j-th demonstration row, (0, b) for a ring row."""
    m = demo_mask(B)
    idx = torch.stack((torch.zeros(B, dtype=torch.int32), torch.arange(B, dtype=torch.int32)), 1)
    idx[m, 0] = -1
    idx[m, 1] = torch.arange(int(m.sum()), dtype=torch.int32)
    return idx.to(device).contiguous()


def filter_margin(q, q_pi):
    return 4e-5 * max(1.0, q.abs().max().item(), q_pi.abs().max().item())


def filter_of(q, q_pi, mask):
    """dict(above = demonstration rows with q > q_pi, undecided = those with |q - q_pi| < margin, margin) of f64 q and q_pi."""
    q, q_pi = q.double().view(-1), q_pi.double().view(-1)
    margin = filter_margin(q, q_pi)
    return dict(above=mask & (q > q_pi), undecided=mask & ((q - q_pi).abs() < margin), margin=margin)


def check_inputs(q, q_pi, mask):
    """The conditions on a case's inputs: undecided rows at most MAX_UNDECIDED of the demonstration rows, and from 33 rows on at least
    MIN_SIDE of them on each side of the filter.  Returns (rows above, rows not above, undecided rows, demonstration rows)."""
    f = filter_of(q, q_pi, mask)
    n, above, und = int(mask.sum()), int(f["above"].sum()), int(f["undecided"].sum())
    assert und <= MAX_UNDECIDED * n, f"{und} of {n} demonstration rows are within {f['margin']:.3g} of the filter's boundary"
    if mask.numel() >= 33:
        assert above >= MIN_SIDE * n and n - above >= MIN_SIDE * n, f"{above} of {n} demonstration rows have q > q_pi"
    return above, n - above, und, n


def codes(mask, applied):
    """code [B] int: 0 a ring row, 1 a demonstration row left out, 2 a demonstration row applied."""
    return mask.to(torch.int32) + (mask & applied).to(torch.int32)


def ref_step(state, batch, hyper, delta=None, c=0.0, lam=0.0, q_filter=True, mask=None):
    """learn_ref.ref_step with demo_mask(B) for the demonstration rows where `mask` is None; also returns code."""
    out = R.ref_step(state, batch, hyper, delta, c, lam, q_filter, demo_mask(len(batch[0])) if mask is None else mask)
    return dict(out, code=codes(out["demo"], out["applied"]))


def demo_case(case, lam, q_filter, huber=False, c=0.0):
    """(state, hyper, batch, delta or None, ref_step's result) of a learn_ref case tuple with a demonstration loss [and a shape]; the
    batch is learn_ref.case's own (do not write to it)."""
    state, hyper, batch, ref, _ = R.case(*case)
    delta = S.delta_of(ref) if huber else None
    return state, hyper, batch, delta, ref_step(state, batch, hyper, delta=delta, c=c, lam=lam, q_filter=q_filter)


@functools.lru_cache(maxsize=None)
def zero_action_case(case):
    """(state, hyper, batch) of a FRESH learn_ref case (step 0, zero Adam moments) made so that dQ/da is exactly 0 on every row, in
    every precision, THROUGH THE UPDATED CRITIC: the action_value weights of the critic and the target critic are zero, and so is every
    stored action of the batch.  dQ/da = sum_j w3_j [z2_j > 0] wa_j, and the critic's step must leave wa at zero for it to stay 0
    in the third forward: wa's gradient is sum_b dz2[b][j] a_b + weight_decay wa = 0 with a = 0, and Adam from zero moments moves a
    zero gradient nowhere.  Everything else of the critic moves, so q (before the step) and q_pi (after it) differ and the filter has
    rows on both sides.  Made once per process and shared: do not write to it."""
    state, hyper, batch, _, _ = R.case(*case)
    assert state["step"] == 0 and all(float(v.abs().max()) == 0.0 for k in ("m", "v") for v in state[k]["critic"].values())
    nets = {n: {k: v.clone() for k, v in sd.items()} for n, sd in state["nets"].items()}
    for n in ("critic", "target_critic"):
        nets[n]["action_value.weight"] = torch.zeros_like(nets[n]["action_value.weight"])
    state = dict(state, nets=nets)
    batch = [t.clone() for t in batch]
    batch[1].zero_()
    # the critic's pre-ReLU values moved with wa: rows with a unit within learn_ref.MARGIN of zero are replaced, as make_batch does
    g = torch.Generator().manual_seed(case[5] + case[0] + 5000)
    for _ in range(R.MAX_PASSES):
        bad = (ref_step(state, batch, hyper)["margin"] < R.MARGIN).nonzero().view(-1)
        if bad.numel() == 0:
            return state, hyper, batch
        assert bad.numel() <= R.MAX_DISCARD * case[0], f"{bad.numel()} of {case[0]} rows within {R.MARGIN} of a ReLU boundary"
        for t, f in zip(batch, R._candidates(bad.numel(), g)):
            t[bad] = f
        batch[1].zero_()
    raise AssertionError(f"rows within {R.MARGIN} of a ReLU boundary are left after {R.MAX_PASSES} passes")
