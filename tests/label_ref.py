"""One learn() step in f64 with LABELLED rows (include/ttenv.h: tt_demo_labels): rows whose cloning target is the
expert's label instead of the stored action and which the Q-filter never leaves out.  Built ON learn_ref: the critic half and the filter
of the other demonstration rows are learn_ref.ref_step's, the actor half is learn_ref.actor_half with the per-row TARGET vector for
`a` and the computed mask for `applied` -- there is no second actor half here.  What tests/test_expert_labels_cpu.py (CPU) and
tests/test_gpu_expert_labels.py (GPU) share.

    FIRST, COUNT, EXPERT    the lanes of the planted index: expert lanes [0, 2), labelled lanes [2, 5)
    planted_index(B)        a draw's [B, 2] index buffer that mixes side rows, ring rows of lanes 0-1, ring rows of lanes 2-4 and other
                            ring rows so that demonstration and labelled rows TOGETHER are demo_ref.demo_mask(B) (b % 3 == 0)
    planted_labels()        a label array [ARRAY_SLOTS, LANES] f32 whose entries differ from every stored action of learn_ref's batches
    row_targets / row_mask  the target vector and the applied mask learn_ref.actor_half takes
    codes                   0 / 1 / 2 as demo_ref.codes, 3 on a labelled row
    actor_half, ref_step    learn_ref's, with labelled rows"""
import torch

import demo_ref as D
import learn_ref as R

EXPERT, FIRST, COUNT = 2, 2, 3
_actor_half = R.actor_half          # (bound here: a test may put actor_half below in learn_ref.actor_half's place)
SLOTS, LANES = 5, 64          # the planted index draws slots [0, SLOTS) and lanes [0, LANES)
ARRAY_SLOTS = SLOTS + 2        # the label array's slots: the last two are never drawn


def planted_index(B, device="cpu"):
    """Rows b % 3 == 0 in turn: a side row (-1, j), a ring row of an expert lane (slot, lane < 2), a ring row of a labelled lane (slot,
    2 <= lane < 5) -- b % 9 == 0, 3, 6 --; every other row a ring row of a lane >= 5."""
    b = torch.arange(B, dtype=torch.int32)
    idx = torch.stack((b % SLOTS, FIRST + COUNT + b % (LANES - FIRST - COUNT)), 1)
    side, ring, lab = b % 9 == 0, b % 9 == 3, b % 9 == 6
    idx[side, 0], idx[side, 1] = -1, torch.arange(int(side.sum()), dtype=torch.int32)
    idx[ring, 1] = (b[ring] // 9) % EXPERT
    idx[lab, 1] = FIRST + (b[lab] // 9) % COUNT
    return idx.to(device).contiguous()


def label_rows(index, first=FIRST, count=COUNT):
    """mpc.label_mask's rule, written out (the tests compare the two)."""
    index = index.cpu()
    return (index[:, 0] >= 0) & (index[:, 1] >= first) & (index[:, 1] < first + count)


def planted_labels(device="cpu"):
    """[ARRAY_SLOTS, LANES] f32 in [-0.9, 0.9], every entry different; the stored actions of learn_ref's batches are U(-1.2, 1.2) draws, so a
    labelled row's label differs from its stored action (the tests assert it)."""
    n = ARRAY_SLOTS * LANES
    return (torch.arange(n, dtype=torch.float32).mul(1.8 / (n - 1)).sub(0.9).view(ARRAY_SLOTS, LANES)).to(device).contiguous()


def labels_of(index, array):
    """[B] the label of each row's (slot, lane) -- read for every ring row, used on the labelled ones."""
    idx = index.cpu().long()
    return array.cpu()[idx[:, 0].clamp(min=0), idx[:, 1].clamp(max=array.shape[1] - 1)]


def row_targets(a, labels, lab):
    return torch.where(lab, labels.to(a.dtype).view(-1), a.view(-1))


def row_mask(applied, lab):
    return lab.clone() if applied is None else applied | lab


def codes(mask, applied, lab):
    return torch.where(lab, torch.full((lab.numel(),), 3, dtype=torch.int32), D.codes(mask & ~lab, applied & ~lab))


def actor_half(critic, actor, s, a, labels, lab, dq_da=None, c=0.0, lam=0.0, applied=None):
    """learn_ref.actor_half with labelled rows: the label is the target and the row is applied whatever `applied` says."""
    return _actor_half(critic, actor, s, row_targets(a.to(s), labels.to(s), lab.to(s.device)), dq_da=dq_da, c=c, lam=lam,
                        applied=row_mask(None if applied is None else applied.to(s.device), lab.to(s.device)))


def ref_step(state, batch, hyper, labels, lab, delta=None, c=0.0, lam=0.0, q_filter=True, mask=None):
    """One learn() in f64 with the demonstration rows `mask` (filtered as learn_ref.ref_step filters them) and the labelled rows `lab`
    (disjoint from mask) cloning `labels` [B].  learn_ref.ref_step gives the critic half, q, q_pi and the filter; the actor's step is
    made again from the updated critic with actor_half above.  Returns learn_ref.ref_step's dict with the actor's gradients, nets and
    moments, dq_eff, applied (labelled rows included), bc_loss and actor_loss of this form, and labelled, code."""
    mask = torch.zeros(lab.numel(), dtype=torch.bool) if mask is None else mask.cpu().bool().view(-1)
    lab = lab.cpu().bool().view(-1)
    assert not bool((mask & lab).any())
    base = R.ref_step(state, batch, hyper, delta, c, lam, q_filter, mask)
    s, a = batch[0].detach().cpu().double(), batch[1].detach().cpu().double().view(-1)
    agent = R.load_agent(dict(state, nets=dict(state["nets"], critic=base["nets"]["critic"])), hyper, torch.device("cpu"), torch.float64)
    half = actor_half(agent.critic, agent.actor, s, a, labels.cpu().double(), lab, c=c, lam=lam, applied=base["applied"])
    assert torch.equal(half["q_pi"], base["q_pi"]) and torch.equal(half["dq_da"], base["dq_da"])
    for k, p in agent.actor.named_parameters():
        p.grad = half["grads"][k]
    agent.actor.optimizer.step()
    agent.update_network_parameters()
    nets = dict(base["nets"])
    for n in ("actor", "target_actor"):
        nets[n] = {k: v.detach().clone() for k, v in getattr(agent, n).state_dict().items()}
    applied = row_mask(base["applied"], lab)
    return dict(base, grads=dict(base["grads"], actor=half["grads"]), nets=nets,
                m=dict(base["m"], actor=R._moments(agent.actor, "exp_avg")), v=dict(base["v"], actor=R._moments(agent.actor, "exp_avg_sq")),
                actor_loss=half["q_part"] + half["pen_part"] + half["bc_part"], applied=applied, dq_eff=half["dq_eff"],
                bc_loss=half["bc_part"], labelled=lab, code=codes(mask, base["applied"], lab))
