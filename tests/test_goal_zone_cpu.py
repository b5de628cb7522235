"""CPU: the goal-zone scenarios of tests/goal_zone_cases.py are what they claim to be, and the oracle they are judged by agrees
with the real reference there.

 1  Census as a condition on the inputs: the C oracle alone, stepped through scenarios A and B, visits every branch the GPU
    tests (tests/test_gpu_goal_zone.py) are there for, at least MINIMA_A / MINIMA_B times.  The minima sit far below what the
    recipe gives (goal_zone_cases' docstring); a generator that misses one is wrong, not the minimum.
 2  Fixture F8 (tests/golden/f8_goal_zone.npz, the real reference on 24 lanes of A and 2 of B): the scipy twin, the fixed-step
    twin and the C oracle replay it free-running under the very checks and tolerances test_oracle_golden.py applies to F1-F3.
 3  Scenario C winds the headings without changing the motion: the oracle's own drift between the k = 0 copy and each wound
    copy stays far inside the project's 1e-5, flags identical, so that tolerance applies to the wound lanes unchanged."""
import numpy as np
import pytest

import goal_zone_cases as Z
from conftest import load_group
from test_oracle_golden import test_c_oracle_within_tolerance as check_c_oracle
from test_oracle_golden import test_fixed_step_twin_within_tolerance as check_fixed_step_twin
from test_oracle_golden import test_scipy_twin_reproduces_reference as check_scipy_twin


def _f8():
    return [pytest.param(t, id=f"f8-{n}") for n, t in load_group("f8_goal_zone.npz").items()]


def test_scenario_a_census():
    sc = Z.scenario_a()
    assert sc.start.shape == (1000, 3) and sc.actions.dtype == np.float32 and sc.term_mask is None
    assert (sc.kind[13 * 64:14 * 64] == 6).all() and (sc.kind[14 * 64:15 * 64] != 6).sum() == 1
    c = Z.census(sc)
    print("CENSUS A", c)
    assert c["all_done"] and c["finite"]
    Z.check_minima(c, Z.MINIMA_A)
    assert c["final_bonus"] >= 50 and c["goal_reached"] == c["success"]


def test_scenario_b_census():
    sc = Z.scenario_b()
    assert sc.start.shape == (549, 3) and sc.term_mask == Z.c_oracle.F_MAX_STEPS
    c = Z.census(sc)
    print("CENSUS B", c)
    assert c["all_done"] and c["finite"] and c["max_steps"] == 549
    Z.check_minima(c, Z.MINIMA_B)
    assert 0x37 in c["flag_bytes"] and 0x58 in c["flag_bytes"] and c["overrides_5_7"] > 0


def test_scenario_c_winding_leaves_the_oracle_where_it_was():
    """Per |k|: worst difference between the k = 0 copy and the copy wound k turns over 30 steps (obs, state less the 2*pi*k,
    reward terms).  Measured: obs 6.0e-8, state 4.3e-9, reward terms 9.0e-7 at k = 100000; 3.0e-8 / 2.1e-10 / 1.2e-9 at |k| = 10000."""
    sc = Z.scenario_c()
    nb = sc.n_base
    assert sc.state0.shape == (832, 6) and np.abs(sc.state0[:, :2]).max() > 6e5
    ora, obs0 = Z.make_oracle(sc)
    base = slice(0, nb)
    worst = {}
    alive = np.ones(nb, bool)
    for a in sc.actions:
        obs, rew, done, info = ora.step(a, nthreads=4)
        st, fl, vi = ora.state(), ora.flags(), ora.violation()
        for r, k in enumerate(Z.WINDS[1:], start=1):
            sl = slice(r * nb, (r + 1) * nb)
            assert np.array_equal(fl[sl][alive], fl[base][alive]) and np.array_equal(vi[sl][alive], vi[base][alive]), k
            s = st[sl].copy()
            s[:, :2] -= 2 * np.pi * k
            w = worst.setdefault(abs(k), [0.0, 0.0, 0.0])
            w[0] = max(w[0], np.abs(obs[sl][alive] - obs[base][alive]).max())
            w[1] = max(w[1], np.abs(s[alive] - st[base][alive]).max())
            w[2] = max(w[2], np.abs(info[sl][alive] - info[base][alive]).max())
        alive &= ~done[base]
    print("WINDING DRIFT (obs, state, reward terms) per |k|:", {k: [f"{x:.1e}" for x in v] for k, v in worst.items()})
    for k, (o, s, r) in worst.items():
        assert o <= 1e-6 and s <= 1e-7 and r <= 2e-6, (k, o, s, r)      # a fifth of TOL = 1e-5 at the most


def test_fixture_f8_holds_what_it_was_made_for():
    g = load_group("f8_goal_zone.npz")
    a = {n: t for n, t in g.items() if n.startswith("a")}
    b = {n: t for n, t in g.items() if n.startswith("b")}
    assert len(a) == 24 and all(sum(n.endswith(f"kind{k}") for n in a) == 3 for k in range(8))
    assert all(t["done"][-1] and not t["done"][:-1].any() for t in a.values())
    staged = lambda t: set(t["info"][:, 5].tolist())
    assert sum(bool(t["success"][-1]) and t["info"][-1, 8] == 200.0 and t["flags"][-1][3] for t in a.values()) >= 4
    assert sum(35.0 in staged(t) and not staged(t) & {110.0, 135.0} for t in a.values()) >= 2
    assert any(t["flags"][-1].sum() >= 2 for t in a.values())                      # several flags at once
    sc = Z.scenario_a()
    for n, t in a.items():
        lane = int(n[1:4])
        assert np.array_equal(t["actions"], sc.actions[:len(t["actions"]), lane]) and np.array_equal(t["start"], sc.start[lane])
        assert np.array_equal(t["goal"], sc.goal[lane]) and float(t["L2"]) == sc.L2[lane]
    for t in b.values():      # on past done to the step limit; at the goal again with the 100 latched: bonus paid, stage not
        latched = np.cumsum(t["info"][:, 5] >= 110.0) > 0
        assert ((t["info"][:, 8] == 200.0) & (t["info"][:, 5] < 110.0) & latched).any()
        assert len(t["actions"]) == int(t["max_episode_steps"]) and t["flags"][-1][2] and t["done"][:-1].any()
        assert (t["info"][:, 5] >= 110.0).sum() == 1 and np.isfinite(t["reward"]).all()
    assert len(b) == 2


@pytest.mark.parametrize("t", _f8())
def test_scipy_twin_reproduces_f8(t):
    check_scipy_twin(t)


@pytest.mark.parametrize("t", _f8())
def test_fixed_step_twin_within_tolerance_on_f8(t):
    check_fixed_step_twin(t)


@pytest.mark.parametrize("t", _f8())
def test_c_oracle_within_tolerance_on_f8(t):
    check_c_oracle(t)
