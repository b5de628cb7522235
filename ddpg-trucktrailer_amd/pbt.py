"""Population-based training (PBT; Jaderberg et al., 2017) for a PopulationRollout: a host-side controller that, every `ready`
vector steps, ranks the agents by their recent episodes, lets the worst take a copy of a better agent's networks and optimizer
state ("exploit") and perturbs the hyperparameters they inherit ("explore").  The copy is one launch on the device
(PopulationRollout.exploit, include/ttenv.h: tt_pop_exploit); everything here is host logic on drained episode records.

    pbt = PBT(K, ready=200)
    ...
    pop.run(k)
    decisions = pbt.step(pop, pop.drain_episodes())

Rules:
  - per agent, the last `window` episodes that ENDED since that agent's last exploit (or since the start) count;
  - a round is due once `ready` vector steps have passed since the last round; it needs two or more eligible agents (>= min_episodes
    such episodes, default `window`) -- otherwise it is tried again at the next call;
  - step(..., evaluation=records) ranks a round on the records of a greedy evaluation (evaluation.Evaluator: every agent from the same
    start poses, no noise) instead: every agent with >= min_episodes records is eligible, the windows are not consulted, and
    the rest of the round -- truncation, the draws and their order, exploit -- is the same;
  - ranking: "return" = mean return; "success" = success rate, then mean return (checkpoint.BestModelTracker's order); ties go to
    the lower agent index;
  - truncation selection: m = min(max(1, floor(quantile * E)), E // 2) of the E eligible agents; each of the bottom m (worst
    first) takes a src drawn uniformly from the top m with the controller's own np.random.RandomState(seed);
  - explore: each hyperparameter in `explore` takes a factor drawn from `factors` (in the order alpha, beta, tau, gamma): alpha,
    beta and tau are multiplied by it, gamma is perturbed in 1 - gamma space (1 - gamma' = f (1 - gamma)); each value is clamped
    to `bounds`; the others are src's unchanged.  dst's window is cleared;
  - n_step_choices (e.g. (1, 3, 5, 8); None: n is not PBT's business, and every decision and draw is as without the option): dst also
    inherits src's n-step horizon, and explore moves it to a neighbour in the sorted choices or keeps it -- one more draw of the
    same RNG (0, 1, 2: down, keep, up; clamped at the ends), taken after the pair's src and factor draws: the first pair of a
    run takes the same src, alpha, beta, tau and gamma with the option as without, and every later draw comes one per pair later;
  - clip_factors (e.g. (0.8, 1.2); None: the gradient clip is not PBT's business, and every decision and draw is as without the
    option): dst inherits src's two max_norm values ("clip_critic", "clip_actor": the clip travels with the weights it was tuned
    on), and explore multiplies each by a factor drawn from clip_factors as alpha's is from `factors` -- two more draws of the same
    RNG per pair, the critic's then the actor's, after the pair's other draws -- and clamps it to bounds["clip"].  A 0 (that
    network is not clipped) stays 0, whatever its draw."""
import collections
import math

import numpy as np

HYPERS = ("alpha", "beta", "tau", "gamma")
BOUNDS = {"alpha": (1e-6, 1e-2), "beta": (1e-6, 1e-1), "tau": (1e-5, 1e-1), "gamma": (0.9, 0.9999), "clip": (1e-3, 1e6)}
CLIPS = ("clip_critic", "clip_actor")
METRICS = ("return", "success")


class PBT:
    def __init__(self, K, ready, seed=0, quantile=0.25, metric="return", window=100, min_episodes=None, explore=HYPERS,
                 factors=(0.8, 1.2), bounds=None, n_step_choices=None, clip_factors=None):
        self.K, self.ready = int(K), int(ready)
        if self.K < 1 or self.ready < 1:
            raise ValueError(f"PBT: K = {K} and ready = {ready} must be >= 1")
        if metric not in METRICS:
            raise ValueError(f"PBT: metric {metric!r} is not one of {METRICS}")
        if not 0.0 < float(quantile) <= 0.5:
            raise ValueError(f"PBT: quantile = {quantile} is not in (0, 0.5]")
        bad = [h for h in explore if h not in HYPERS]
        if bad:
            raise ValueError(f"PBT: cannot explore {bad} (only {HYPERS})")
        self.quantile, self.metric, self.window = float(quantile), metric, int(window)
        self.min_episodes = self.window if min_episodes is None else int(min_episodes)
        if self.window < 1 or not 1 <= self.min_episodes <= self.window:
            raise ValueError(f"PBT: window = {window}, min_episodes = {min_episodes}: need 1 <= min_episodes <= window")
        self.explore = tuple(h for h in HYPERS if h in explore)
        self.factors = tuple(float(f) for f in factors)
        if not self.factors or any(not f > 0.0 for f in self.factors):
            raise ValueError(f"PBT: factors {factors} must be positive")
        self.n_step_choices = None
        if n_step_choices is not None:
            self.n_step_choices = tuple(sorted({int(n) for n in n_step_choices}))
            if not self.n_step_choices or self.n_step_choices[0] < 1:
                raise ValueError(f"PBT: n_step_choices {n_step_choices} must be positive step counts")
        self.clip_factors = None
        if clip_factors is not None:
            self.clip_factors = tuple(float(f) for f in clip_factors)
            if not self.clip_factors or any(not (f > 0.0 and math.isfinite(f)) for f in self.clip_factors):
                raise ValueError(f"PBT: clip_factors {clip_factors} must be positive")
        self.bounds = dict(BOUNDS)
        self.bounds.update(bounds or {})
        self.rng = np.random.RandomState(seed)
        self.windows = [collections.deque(maxlen=self.window) for _ in range(self.K)]
        self.last_round = 0
        self.history = []

    # ------------------------------------------------------------------------------------------------- episodes
    def observe(self, drained):
        """drained: PopulationRollout.drain_episodes() -- per agent a dict with "ret" and "success" tensors (or sequences)."""
        if len(drained) != self.K:
            raise ValueError(f"PBT.observe: {len(drained)} records for {self.K} agents")
        for w, r in zip(self.windows, drained):
            ret, ok = _host(r["ret"]), _host(r["success"])
            if len(ret) != len(ok):
                raise ValueError("PBT.observe: ret and success differ in length")
            w.extend((float(x), bool(s)) for x, s in zip(ret, ok))

    def score(self, a):
        """Agent a's ranking key over its window (larger is better), or None while it has fewer than min_episodes episodes."""
        return self._score_of(self.windows[a])

    def evaluation_scores(self, evaluation):
        """Per agent, the ranking key over ALL the records of an evaluation (evaluation.Evaluator.run: per agent a dict with "ret"
        and "success"), or None for an agent with fewer than min_episodes of them.  The windows are not read."""
        if len(evaluation) != self.K:
            raise ValueError(f"PBT: {len(evaluation)} evaluation records for {self.K} agents")
        out = []
        for r in evaluation:
            ret, ok = _host(r["ret"]), _host(r["success"])
            if len(ret) != len(ok):
                raise ValueError("PBT: an evaluation's ret and success differ in length")
            out.append(self._score_of([(float(x), bool(s)) for x, s in zip(ret, ok)]))
        return out

    def _score_of(self, w):
        if len(w) < self.min_episodes:
            return None
        mean = sum(x for x, _ in w) / len(w)
        if self.metric == "return":
            return (mean,)
        return (sum(1 for _, s in w if s) / len(w), mean)

    # ------------------------------------------------------------------------------------------------- a round
    def decide(self, vector_step, hypers, evaluation=None):
        """hypers: per agent {"alpha", "beta", "tau", "gamma"} (and "n_step" with n_step_choices, "clip_critic" and "clip_actor" with
        clip_factors) as they are now.  Returns the
        round's decisions (possibly none): [{"step", "dst", "src", "dst_score", "src_score", "old", "new"}] -- "new" is what dst
        takes.  evaluation: the K record dicts of an evaluation -- the round then ranks on those records alone
        (evaluation_scores), everything after the ranking is the same."""
        if len(hypers) != self.K:
            raise ValueError(f"PBT.decide: {len(hypers)} hyperparameter sets for {self.K} agents")
        if vector_step - self.last_round < self.ready:
            return []
        every = [self.score(a) for a in range(self.K)] if evaluation is None else self.evaluation_scores(evaluation)
        scores = {a: s for a, s in enumerate(every) if s is not None}
        E = len(scores)
        if E < 2:
            return []                  # (tried again at the next call)
        # best first; ties: the lower index ranks higher
        ranked = sorted(scores, key=lambda a: tuple(-x for x in scores[a]) + (a,))
        m = min(max(1, int(math.floor(self.quantile * E))), E // 2)
        top, bottom = ranked[:m], ranked[E - m:][::-1]
        out = []
        for dst in bottom:
            src = top[self.rng.randint(m)]
            new = {k: float(hypers[src][k]) for k in HYPERS}
            for k in self.explore:
                f = self.factors[self.rng.randint(len(self.factors))]
                x = 1.0 - (1.0 - new[k]) * f if k == "gamma" else new[k] * f
                lo, hi = self.bounds[k]
                new[k] = min(max(x, lo), hi)
            old = {k: float(hypers[dst][k]) for k in HYPERS}
            if self.n_step_choices is not None:
                old["n_step"] = int(hypers[dst]["n_step"])
                new["n_step"] = self._explore_n(int(hypers[src]["n_step"]))
            if self.clip_factors is not None:
                lo, hi = self.bounds["clip"]
                for k in CLIPS:
                    f = self.clip_factors[self.rng.randint(len(self.clip_factors))]
                    x = float(hypers[src][k])
                    old[k] = float(hypers[dst][k])
                    new[k] = min(max(x * f, lo), hi) if x > 0.0 else 0.0
            out.append({"step": int(vector_step), "dst": dst, "src": src, "dst_score": scores[dst], "src_score": scores[src],
                        "old": old, "new": new})
            self.windows[dst].clear()
        self.last_round = int(vector_step)
        self.history.extend(out)
        return out

    def _explore_n(self, n):
        """A neighbour of n in the sorted choices, or n itself (one draw).  An n that is no choice moves from the nearest one."""
        c = self.n_step_choices
        i = min(range(len(c)), key=lambda j: (abs(c[j] - n), j))
        move = int(self.rng.randint(3)) - 1
        if move == 0:
            return n
        return c[min(max(i + move, 0), len(c) - 1)]

    def step(self, pop, drained, evaluation=None):
        """observe(drained), decide at pop.vector_steps, and apply the decisions with one pop.exploit launch.  evaluation: None, or
        what evaluation.Evaluator.run returned for pop's actors (the same start poses for every agent, no noise): the round
        ranks on it instead of on the training windows."""
        self.observe(drained)
        hypers = [{k: float(getattr(ag, k)) for k in HYPERS} for ag in pop.agents]
        if self.n_step_choices is not None:
            for h, n in zip(hypers, pop.n_steps):
                h["n_step"] = int(n)
        if self.clip_factors is not None:
            if not getattr(pop, "clip_table", False):
                raise ValueError("PBT: clip_factors needs a population built with a gradient clip (PopulationRollout(grad_clip=...))")
            for h, (c, a) in zip(hypers, pop.grad_clips):
                h["clip_critic"], h["clip_actor"] = float(c), float(a)
        out = self.decide(pop.vector_steps, hypers, evaluation)
        if out:
            pop.exploit([(d["dst"], d["src"], d["new"]) for d in out])
        return out

    # ------------------------------------------------------------------------------------------------- checkpoint
    def state_dict(self):
        sd = {"rng": self.rng.get_state(), "windows": [list(w) for w in self.windows], "last_round": self.last_round,
              "history": [dict(d) for d in self.history]}
        if self.clip_factors is not None:          # (only with the option: a state written without it is what it was)
            sd["clip_factors"] = list(self.clip_factors)
        return sd

    def load_state_dict(self, sd):
        if len(sd["windows"]) != self.K:
            raise ValueError(f"PBT.load_state_dict: {len(sd['windows'])} windows for {self.K} agents")
        have = None if sd.get("clip_factors") is None else tuple(float(f) for f in sd["clip_factors"])
        if have != self.clip_factors:
            raise ValueError(f"PBT.load_state_dict: the state was written with clip_factors = {have}, this controller has {self.clip_factors}")
        self.rng.set_state(sd["rng"])
        self.windows = [collections.deque(w, maxlen=self.window) for w in sd["windows"]]
        self.last_round = int(sd["last_round"])
        self.history = [dict(d) for d in sd["history"]]


def _host(x):
    if hasattr(x, "detach"):
        return x.detach().cpu().tolist()
    return list(x)
