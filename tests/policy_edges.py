"""Host side of the policy forward's edge tests (tests/test_policy_edges_cpu.py, tests/test_gpu_policy_edges.py): nets,
rows and references.  numpy and torch on the CPU only -- nothing here touches a kernel.

What the two forward kernels (csrc/ttnet_split.hip from 1024 rows, csrc/ttnet.hip) are otherwise fed is uniform [-1, 1]
observations on init-scale weights.  Here: rows at the edge of the split's stated range (|activation| < 4094, |weight| < 1023;
a piece really becomes inf at 16 |x| >= 65520 and 64 |w| >= 65520, i.e. 4095 and 1023.75 -- the values below keep clear of
those), rows where LayerNorm's eps carries the result, rows beyond the range and rows that are not finite, PLANTED at chosen
positions among ordinary rows so that a test can also ask what they do to their neighbours.

Three references of one forward:
  ref64        the torch modules in f64 (the yardstick's zero);
  numpy_f32    a plain f32 evaluation: f32 matmul, two-pass LayerNorm (what "f32 accuracy" means; no kernel under test);
  split_model  the two-piece scheme of csrc/ttnet_split.hip in numpy -- operands scaled by 16 / 64, rn16 twice, the three
               products h*h' + h*m' + m*h' accumulated in f64, rounded to f32, scaled back by 2^-10: the SCHEME's error without
               the accumulation order of any kernel.

Left out on purpose: a layer-1 bias that is the same in every neuron but NOT a power of two (0.37) under zero or near-zero
observations.  The pre-activations then differ only by the rounding of 0.37 + (tiny), LayerNorm divides by that rounding noise
(variance ~1e-16 against eps 1e-5 keeps it finite, but the mean's own rounding is of the size of the deviations), numpy-f32 and
the split model both miss f64 by 1.2e-4, and by how much depends on the summation order: no fixed yardstick fits it.  With 0.5
every pre-activation is the same exact number in every arithmetic, which is the case kept (CASES["const"])."""
import numpy as np
import torch

IN, H1, H2 = 23, 400, 300
EPS = 1e-5
SX, SW = 16.0, 64.0                       # csrc/ttnet_pack.h
F16_MAX = 65504.0                         # largest finite f16; rn16 gives inf from 65520
SPLIT_POSITIONS = lambda n: (0, 31, 32, 63, 64, 127, 128, 129, 1023, 1024, n - 1)      # noqa: E731  (n = 1024 + 55)
F32_POSITIONS = (0, 15, 16, 63, 64, 191, 192, 199)                                    # (n = 200)
N_SPLIT, N_F32 = 1024 + 55, 200

VARIANTS = ("base", "b1_zero", "b1_half", "dead", "w_near", "w_beyond")
# planted single weights: (layer, row, col, value); |w| <= 1023.5 keeps 64 |w| <= 65504
NEAR_WEIGHTS = (("fc1", 7, 3, 1020.0), ("fc1", 200, 11, -1020.0), ("fc2", 5, 17, 1020.0), ("fc2", 250, 399, -1020.0),
                ("fc2", 100, 200, -1022.0))
BEYOND_WEIGHT = ("fc2", 5, 17, 1030.0)


def nets(variant="base", seed=0):
    """(actor, critic) on the CPU in f32: the seeded affines and heads of tests/test_gpu_fused_net.py::_nets, then the variant."""
    from ddpg_trucktrailer_amd.networks import ActorNetwork, CriticNetwork
    assert variant in VARIANTS
    torch.manual_seed(seed)
    a = ActorNetwork(1e-4, (IN,), H1, H2, 1, name="actor", device="cpu")
    c = CriticNetwork(1e-3, (IN,), H1, H2, 1, name="critic", device="cpu")
    with torch.no_grad():
        for net in (a, c):
            net.bn1.weight.uniform_(0.5, 1.5); net.bn1.bias.uniform_(-0.3, 0.3)
            net.bn2.weight.uniform_(0.5, 1.5); net.bn2.bias.uniform_(-0.3, 0.3)
        a.mu.weight.uniform_(-0.2, 0.2); c.q.weight.uniform_(-0.2, 0.2)
        for net in (a, c):
            if variant == "b1_zero":
                net.fc1.bias.zero_()
            elif variant == "b1_half":
                net.fc1.bias.fill_(0.5)
            elif variant == "dead":           # |LayerNorm's normalised value| <= sqrt(399) < 20 and gamma <= 1.5: always below 40
                net.bn1.bias.fill_(-40.0)
            elif variant == "w_near":
                for layer, i, j, v in NEAR_WEIGHTS:
                    getattr(net, layer).weight[i, j] = v
            elif variant == "w_beyond":
                layer, i, j, v = BEYOND_WEIGHT
                getattr(net, layer).weight[i, j] = v
    return a, c


def to_device(net, dev):
    """A copy of `net` on `dev` (a fresh module of the same class with the same parameters)."""
    from ddpg_trucktrailer_amd.networks import ActorNetwork, CriticNetwork
    cls, lr = (ActorNetwork, 1e-4) if hasattr(net, "mu") else (CriticNetwork, 1e-3)
    out = cls(lr, (IN,), H1, H2, 1, name=net.name, device=dev)
    out.load_state_dict(net.state_dict())
    return out


# ---- rows: each builder returns [k, 23] f32 observations ------------------------------------------------------------------
def _rng(seed):
    return np.random.RandomState(seed)


def rows_ordinary(k, seed=1):
    return _rng(seed).uniform(-1, 1, (k, IN)).astype(np.float32)


def rows_large(k, seed=2):
    return _rng(seed).uniform(-4000, 4000, (k, IN)).astype(np.float32)


def rows_one_component(k, value, seed=3):
    """Ordinary rows with ONE component (another one in every row) set to `value`."""
    x = rows_ordinary(k, seed)
    x[np.arange(k), (7 * np.arange(k) + 2) % IN] = value
    return x


def rows_mixed(k, seed=4):
    r = _rng(seed)
    return (r.choice([-1.0, 1.0], (k, IN)) * 10.0 ** r.uniform(-6, 3, (k, IN))).astype(np.float32)


def rows_tiny(k, seed=5):
    return _rng(seed).uniform(-1e-6, 1e-6, (k, IN)).astype(np.float32)


def rows_zero(k):
    return np.zeros((k, IN), np.float32)


def rows_eps(k, seed=6):
    """+-1e-3: on the b1 = 0 net the layer-1 variance is ~1e-8, far below eps."""
    return _rng(seed).uniform(-1e-3, 1e-3, (k, IN)).astype(np.float32)


def rows_nonfinite(k, seed=7):
    """One component NaN, +inf, -inf in turn."""
    x = rows_ordinary(k, seed)
    x[np.arange(k), (7 * np.arange(k) + 2) % IN] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(k) % 3]
    return x


def actions_ordinary(k, seed=8):
    return _rng(seed).uniform(-1.2, 1.2, (k, 1)).astype(np.float32)


def actions_edge(k):
    return np.array([1.2, -1.2, 0.0, 1e4, -1e4], np.float32)[np.arange(k) % 5].reshape(k, 1)


def actions_nan(k):
    return np.full((k, 1), np.nan, np.float32)


# kind: "finite" (inside the split's range), "outside" (finite, beyond the split's range: the split kernel answers NaN, the
# exact-f32 kernel and torch a finite number), "nonfinite" (torch answers NaN).  act: the critic's actions on the planted rows
# (None: ordinary ones).  nan_for: which module's planted rows torch answers NaN on.
CASES = {
    "ordinary":  dict(variant="base", kind="finite", rows=lambda k: rows_ordinary(k, 11)),
    "large4000": dict(variant="base", kind="finite", rows=rows_large),
    "one4090":   dict(variant="base", kind="finite", rows=lambda k: rows_one_component(k, 4090.0)),
    "mixed":     dict(variant="base", kind="finite", rows=rows_mixed),
    "tiny":      dict(variant="base", kind="finite", rows=rows_tiny),
    "zero":      dict(variant="base", kind="finite", rows=rows_zero),
    "eps":       dict(variant="b1_zero", kind="finite", rows=rows_eps),
    "const":     dict(variant="b1_half", kind="finite", rows=rows_zero),
    "dead":      dict(variant="dead", kind="finite", rows=rows_mixed),
    "w_near":    dict(variant="w_near", kind="finite", rows=lambda k: rows_ordinary(k, 12)),
    "act_edge":  dict(variant="base", kind="finite", rows=lambda k: rows_ordinary(k, 13), act=actions_edge),
    "out4096":   dict(variant="base", kind="outside", rows=lambda k: rows_one_component(k, 4096.0)),
    "out1e6":    dict(variant="base", kind="outside", rows=lambda k: rows_one_component(k, -1e6)),
    "w_beyond":  dict(variant="w_beyond", kind="outside", rows=lambda k: rows_ordinary(k, 14)),      # EVERY row is outside
    "nan":       dict(variant="base", kind="nonfinite", rows=lambda k: rows_one_component(k, np.nan), nan_for=("actor", "critic")),
    "pinf":      dict(variant="base", kind="nonfinite", rows=lambda k: rows_one_component(k, np.inf), nan_for=("actor", "critic")),
    "ninf":      dict(variant="base", kind="nonfinite", rows=lambda k: rows_one_component(k, -np.inf), nan_for=("actor", "critic")),
    "act_nan":   dict(variant="base", kind="nonfinite", rows=lambda k: rows_ordinary(k, 15), act=actions_nan, nan_for=("critic",)),
}


def plant(base, rows, positions):
    """Overwrite rows `positions` of `base` (in place) with `rows`; returns the boolean mask of the planted rows."""
    positions = np.asarray(positions)
    assert len(rows) == len(positions) == len(set(positions.tolist())) and positions.min() >= 0 and positions.max() < len(base)
    base[positions] = rows
    mask = np.zeros(len(base), bool)
    mask[positions] = True
    return mask


def build_case(name, n, positions):
    """(obs [n,23], act [n,1], mask [n]) of case `name` and (obs, act) of its CLEAN twin: the same ordinary rows everywhere,
    with other ordinary rows where the case's are planted."""
    case = CASES[name]
    k = len(positions)
    clean_obs, clean_act = rows_ordinary(n, 100 + n), actions_ordinary(n, 200 + n)
    obs, act = clean_obs.copy(), clean_act.copy()
    mask = plant(obs, case["rows"](k), positions)
    if case.get("act"):
        plant(act, case["act"](k), positions)
    return obs, act, mask, clean_obs, clean_act


# ---- references ------------------------------------------------------------------------------------------------------
def ref64(net, obs, act=None):
    """The module in f64 -> (out [n] f64, layer-1 pre-activations [n,400], hidden layer after ReLU [n,400])."""
    d = lambda t: t.detach().double()      # noqa: E731
    with torch.no_grad():
        x = torch.from_numpy(np.asarray(obs)).double()
        pre1 = x @ d(net.fc1.weight).T + d(net.fc1.bias)
        h1 = torch.relu(torch.nn.functional.layer_norm(pre1, (H1,), d(net.bn1.weight), d(net.bn1.bias), EPS))
        y = torch.nn.functional.layer_norm(h1 @ d(net.fc2.weight).T + d(net.fc2.bias), (H2,), d(net.bn2.weight), d(net.bn2.bias), EPS)
        if hasattr(net, "mu"):
            out = torch.tanh(torch.relu(y) @ d(net.mu.weight).T + d(net.mu.bias))
        else:
            a = torch.from_numpy(np.asarray(act)).double()
            out = torch.relu(y + a @ d(net.action_value.weight).T + d(net.action_value.bias)) @ d(net.q.weight).T + d(net.q.bias)
    return out.view(-1).numpy(), pre1.numpy(), h1.numpy()


def torch_f32(net, obs, act=None):
    with torch.no_grad():
        x = torch.from_numpy(np.asarray(obs))
        return (net(x) if hasattr(net, "mu") else net(x, torch.from_numpy(np.asarray(act)))).view(-1).numpy()


def _params(net):
    p = {k: v.detach().numpy().astype(np.float32) for k, v in net.state_dict().items()}
    head = "mu" if hasattr(net, "mu") else "q"
    return p, head


def _ln_f32(x, g, b):
    f = np.float32
    mean = x.mean(axis=1, keepdims=True, dtype=f)
    d = x - mean
    var = (d * d).mean(axis=1, keepdims=True, dtype=f)
    return d / np.sqrt(var + f(EPS)) * g + b


def _tail_f32(p, head, y, act):
    if head == "q":
        y = y + np.asarray(act, np.float32) @ p["action_value.weight"].T + p["action_value.bias"]
    v = np.maximum(y, np.float32(0)) @ p[head + ".weight"].T + p[head + ".bias"]
    return (np.tanh(v) if head == "mu" else v).reshape(-1).astype(np.float32)


def numpy_f32(net, obs, act=None):
    """Plain f32: f32 matmuls, two-pass LayerNorm, np.maximum for ReLU (which, like F.relu, hands a NaN on)."""
    p, head = _params(net)
    with np.errstate(all="ignore"):
        x = np.asarray(obs, np.float32)
        h1 = np.maximum(_ln_f32(x @ p["fc1.weight"].T + p["fc1.bias"], p["bn1.weight"], p["bn1.bias"]), np.float32(0))
        y = _ln_f32(h1 @ p["fc2.weight"].T + p["fc2.bias"], p["bn2.weight"], p["bn2.bias"])
        return _tail_f32(p, head, y, act)


def split_pieces(x, scale):
    """The two f16 pieces (h, m) of scale * x, both conversions round-to-nearest-even (csrc/ttnet_pack.h: split2).  Beyond the
    range h is inf (and m = -inf)."""
    with np.errstate(all="ignore"):
        xs = np.asarray(x, np.float32) * np.float32(scale)
        h = xs.astype(np.float16)
        m = (xs - h.astype(np.float32)).astype(np.float16)
    return h, m


def _split_matmul(x, w):
    """x [n,k] (scaled by 16) times w [m,k]^T (scaled by 64) from their pieces: three products in f64 -> f32 -> * 2^-10."""
    xh, xm = (t.astype(np.float64) for t in split_pieces(x, SX))
    wh, wm = (t.astype(np.float64) for t in split_pieces(w, SW))
    with np.errstate(all="ignore"):
        acc = xm @ wh.T + xh @ wm.T + xh @ wh.T
        return acc.astype(np.float32) * np.float32(1.0 / (SX * SW))


def split_model(net, obs, act=None):
    """The split-f16 scheme in numpy.  Layer 1 carries its bias as a 24th input that is 1 (as the kernel's image does); layer 2's
    bias is added in f32.  Everything else is numpy_f32's arithmetic."""
    p, head = _params(net)
    with np.errstate(all="ignore"):
        x = np.asarray(obs, np.float32)
        x1 = np.concatenate([x, np.ones((len(x), 1), np.float32)], axis=1)
        w1 = np.concatenate([p["fc1.weight"], p["fc1.bias"][:, None]], axis=1)
        h1 = np.maximum(_ln_f32(_split_matmul(x1, w1), p["bn1.weight"], p["bn1.bias"]), np.float32(0))
        y = _ln_f32(_split_matmul(h1, p["fc2.weight"]) + p["fc2.bias"], p["bn2.weight"], p["bn2.bias"])
        return _tail_f32(p, head, y, act)


def split_operands(net, obs):
    """What the split kernel splits, for range checks: (observations [n,23], hidden layer [n,400] from f64, weights incl. fc1's
    bias as one flat array)."""
    _, _, h1 = ref64(net, obs, np.zeros((len(obs), 1), np.float32))
    p, _ = _params(net)
    return np.asarray(obs, np.float32), h1, np.concatenate([p["fc1.weight"].ravel(), p["fc1.bias"], p["fc2.weight"].ravel()])


def q_floor(q64):
    """The absolute part of Q's bound: 1e-6 x max(1, max |q|) over the rows compared."""
    q64 = q64[np.isfinite(q64)]
    return 1e-6 * max(1.0, float(np.abs(q64).max()) if len(q64) else 0.0)
