"""tools/option_cost.py: report() -- the lines every option-cost tool prints and the timing gate of DESIGN.md section 13 -- against
the reports recorded under profiles/ (fed the legs they print, it returns their lines character for character) and the gate's
verdict at its limit.  No GPU: report() is a pure function of the legs."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("option_cost", os.path.join(ROOT, "tools", "option_cost.py"))
option_cost = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(option_cost)

# (the recorded file, the names its tool forms from the arguments of that run, the width of its name column)
RECORDED = {
    "grad_clip": ("grad_clip_cost.txt", dict(off="the loop without a clip", on="GradClip(10000.0, 1.0)"), 28),
    "loss_shape": ("loss_shape_cost.txt", dict(off="the loop without a shape", on="LossShape(1.0, 0.01)"), 28),
    "demo": ("demo_cost.txt", dict(off="the loop without demo_loss", on="DemoLoss(1.0, True), 65536 side tuples"), 40),
}


def recorded(name):
    """The six lines of a recorded report, and the legs its three variant lines print."""
    text = open(os.path.join(ROOT, "profiles", name)).read().splitlines()
    at = next(i for i, ln in enumerate(text) if ln.startswith("# DDPGRollout, N = 4096"))
    lines = text[at:at + 6]
    legs = [[float(x) for x in re.findall(r"leg \d+ +([0-9.]+)", ln)] for ln in lines[1:4]]
    return lines, dict(zip(("off", "on", "parent"), legs))


@pytest.mark.parametrize("which", sorted(RECORDED))
def test_report_reproduces_the_recorded_lines(which):
    name, names, width = RECORDED[which]
    lines, res = recorded(name)
    if which == "grad_clip":
        assert res == {"off": [3.91274, 3.92422, 3.93414], "on": [5.43059, 5.43977, 5.45680], "parent": [3.90320, 3.92490, 3.91997]}
    got = option_cost.report(res, names, width, steps=400, warmup=60, legs=3)
    assert got == lines
    assert got[-1].endswith(": within") and got[0].startswith("# DDPGRollout, N = 4096, 64 updates per vector step, B = 256")


def test_gate_verdict_at_the_limit():
    # every value is a binary fraction, so that the limit is exact: the parent's median 0.75 + (1.0 - 0.5) = 1.25
    parent = [0.5, 0.75, 1.0]
    names = dict(off="off", on="on")
    at = option_cost.report({"off": [1.25, 1.25, 1.25], "on": [2.0, 2.0, 2.0], "parent": parent}, names, 28, 400, 60, 3)
    assert at[-1] == "# gate: off median 1.25000 ms against the parent's median + its legs' max - min = 1.25000 ms: within"
    above = option_cost.report({"off": [1.25001, 1.25001, 1.25001], "on": [2.0, 2.0, 2.0], "parent": parent}, names, 28, 400, 60, 3)
    assert above[-1] == "# gate: off median 1.25001 ms against the parent's median + its legs' max - min = 1.25000 ms: NOT within"
    none = option_cost.report({"off": [1.25, 1.25, 1.25], "on": [2.0, 2.0, 2.0]}, names, 28, 400, 60, 3)
    assert none[-1] == "# no --parent-tree: the gate against the parent commit was not evaluated"
    assert len(none) == 5 and len(at) == 6 and at[:3] == none[:3] and at[4] == none[3]      # (at[3]: the parent's line)


def test_records_form_has_a_line_per_variant_with_the_option():
    res = {"parent": [1.0, 1.0], "off": [1.0, 1.0], "expert": [1.5, 1.5], "expert+bc": [2.0, 2.0]}
    names = {"off": "the loop without expert", "expert": "E", "expert+bc": "E + D"}
    lines = option_cost.report(res, names, 55, 100, 30, 2, records=True)
    assert [ln.split(":")[0].strip() for ln in lines[1:5]] == ["the parent commit's loop", "the loop without expert", "E", "E + D"]
    assert lines[5] == ("# expert - off = +500.00 us per vector step (+50.00 %); the off legs' own max - min is 0.00 us per vector step "
                        "(a record, not a gate)")
    assert lines[6].startswith("# expert+bc - off = +1000.00 us per vector step (+100.00 %)")
    assert lines[7] == "# gate: off median 1.00000 ms against the parent's median + its legs' max - min = 1.00000 ms: within" and len(lines) == 8
