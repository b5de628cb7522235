"""CPU: the episode log's host side and its kernels' budgets.

* BestModelTracker.update_many feeds drained episode-log records through trainv2.py's "save when best" rule
  (DDPG/trainv2.py:538-572), restated plainly here;
* the k_step_log variants the loop launches keep k_step's occupancy (four waves per SIMD, no scratch, no spills), and every
  kernel of the golden table (tests/golden/kernel_resources_main.json: the library's kernels before the log was added, less
  those retired since) still exists with the register / LDS / scratch row the table gives it."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN


def trainv2_best_rule(scores, successes, start_episode):
    """trainv2.py:488-572 written out: per episode i, the 100-episode means and the is_best test."""
    score_history, success_history, fired = [], [], []
    best_score, best_success_rate = -float("inf"), 0.0
    for j, (score, success) in enumerate(zip(scores, successes)):
        i = start_episode + j
        score_history.append(score)
        avg_score = np.mean(score_history[-100:])
        success_history.append(1 if success else 0)
        success_rate = np.mean(success_history[-100:])
        is_better_success = success_rate > best_success_rate
        is_equal_success_better_score = success_rate == best_success_rate and avg_score > best_score
        is_best = (is_better_success or is_equal_success_better_score) and i > (start_episode + 100)
        if is_best:
            fired.append(j)
            best_success_rate = success_rate
            best_score = avg_score
    return fired, float(avg_score), float(success_rate)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_update_many_follows_the_trainv2_rule(seed):
    from ddpg_trucktrailer_amd.checkpoint import BestModelTracker
    rng = np.random.RandomState(seed)
    n = 700
    # a learning curve: returns drift up, success gets likelier, with plateaus so that ties in success rate occur
    ret = np.cumsum(rng.normal(0.5, 20.0, n)) - 300.0
    success = rng.uniform(size=n) < np.clip(np.linspace(-0.1, 0.6, n), 0.0, 1.0)
    length = rng.randint(5, 300, n).astype(np.int32)
    records = {"ret": ret, "success": success, "len": length}
    want, avg, rate = trainv2_best_rule(ret.tolist(), success.tolist(), 0)
    assert want, "the synthetic curve never set a best: the test would show nothing"

    tr = BestModelTracker(start_episode=0)
    got, g_avg, g_rate = tr.update_many(records, first_episode=0)
    assert got == want and g_avg == avg and g_rate == rate
    assert tr.total_steps == int(length.sum()) and tr.score_history == ret.tolist()

    # the same records drained in several pieces give the same decisions
    tr2 = BestModelTracker(start_episode=0)
    fired, k = [], 0
    for cut in (37, 250, 251, 600, n):
        part = {key: v[k:cut] for key, v in records.items()}
        b, g_avg2, g_rate2 = tr2.update_many(part, first_episode=k)
        fired += [k + j for j in b]
        k = cut
    assert fired == want and (g_avg2, g_rate2) == (avg, rate)


def test_update_many_of_nothing():
    from ddpg_trucktrailer_amd.checkpoint import BestModelTracker
    tr = BestModelTracker()
    assert tr.update_many({"ret": [], "success": [], "len": []}, 5) == ([], None, None)


@pytest.fixture(scope="module")
def ks():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import kernel_resources as kr
    return kr.kernels()


def test_logging_step_kernels_keep_four_waves_per_simd(ks):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    log = kr.find(ks, "10k_step_log")
    assert len(log) == 16, sorted(log)
    for n, v in log.items():
        assert v["vgpr_spills"] == 0, (n, v)
    # k_step_log<PER_ENV = false, INFO = false, AUTO_RESET, RANDOM_POLICY>: the variants the DDPG loop and bench.py launch
    # with the log on -- the budget tests/test_kernel_resources.py holds k_step's same variants to: no scratch, no vector spill
    # (SGPRs spilled into VGPR lanes, as k_step's own do, cost no memory traffic)
    loop = kr.find(ks, "10k_step_logILb0ELb0E")
    assert len(loop) == 4
    for n, v in loop.items():
        assert kr.waves_per_simd(v["vgpr"]) >= 4 and v["scratch"] == 0 and v["vgpr_spills"] == 0, (n, v)


def test_kernels_of_the_golden_table_are_unchanged(ks):
    before = json.load(open(os.path.join(GOLDEN, "kernel_resources_main.json")))
    assert len(before) >= 40
    changed = {n: (v, ks.get(n)) for n, v in before.items() if ks.get(n) != v}
    assert not changed, changed
