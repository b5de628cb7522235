"""The four per-episode objectives of DDPG/viz_how_agent_learn.py (compute_metrics, :13-33; pareto_analysis.py:26-49 groups the
terms the same way), from a drained detailed episode log (TruckTrailerVecEnv.enable_episode_log(detail=True)), on the device:

    efficiency = progress + staged + exploration + final bonus + backward
    smoothness = smoothness
    precision  = heading + orientation
    safety     = safety

and their running averages over the last 100 episodes, as plot_running_average draws them (:35-60: a deque of maxlen 100 per
objective, averaged after each episode)."""
import torch

from ddpg_trucktrailer_amd import _lib as L

OBJECTIVES = ("efficiency", "smoothness", "precision", "safety")
_GROUPS = {
    "efficiency": ("progress_reward", "staged_success", "exploration_bonus", "final_success_bonus", "backward_penalty"),
    "smoothness": ("smoothness_penalty",),
    "precision": ("heading_reward", "orientation_reward"),
    "safety": ("safety_penalty",),
}


def objectives(records):
    """{objective: [m] f64} from a drained detailed log's `components` [m, 9] (columns L.LOG_COMPONENTS), each summed in the
    order compute_metrics adds its terms."""
    comp = records["components"] if isinstance(records, dict) else records
    if comp.dim() != 2 or comp.shape[1] != len(L.LOG_COMPONENTS):
        raise ValueError(f"components must be [m, {len(L.LOG_COMPONENTS)}] (a detailed episode log), got {tuple(comp.shape)}")
    out = {}
    for name, terms in _GROUPS.items():
        acc = comp[:, L.LOG_COMPONENTS.index(terms[0])].clone()
        for t in terms[1:]:
            acc = acc + comp[:, L.LOG_COMPONENTS.index(t)]
        out[name] = acc
    return out


class RunningObjectives:
    """The last `window` episodes' objectives across drains; update() returns, per objective, the running average after each of
    the new episodes ([m] f64, the mean of up to `window` most recent values, as a deque(maxlen=window) gives)."""

    def __init__(self, window=100):
        self.window = int(window)
        self.hist = None

    def update(self, records):
        obj = objectives(records)
        if self.hist is None:
            self.hist = {k: v.new_zeros(0) for k, v in obj.items()}
        out = {}
        for k, v in obj.items():
            h = torch.cat([self.hist[k], v])
            m, p = v.shape[0], h.shape[0] - v.shape[0]          # p: episodes before these
            # trailing window sums by a cumulative sum over [history | new], differences of prefix sums
            cs = torch.cat([h.new_zeros(1), torch.cumsum(h, 0)])
            end = torch.arange(p + 1, p + m + 1, device=h.device)
            lo = torch.clamp(end - self.window, min=0)
            out[k] = (cs[end] - cs[lo]) / (end - lo).to(h.dtype)
            self.hist[k] = h[-self.window:]
        return out

    def last(self):
        """{objective: the current running average (float) or None before the first episode}."""
        if self.hist is None or self.hist["safety"].numel() == 0:
            return {k: None for k in OBJECTIVES}
        return {k: float(v.mean().item()) for k, v in self.hist.items()}
