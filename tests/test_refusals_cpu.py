"""CPU: what the library refuses before any HIP call, pinned to the text.  tests/golden/refusals.json is a table of bad calls with
the return code and the full message (tt_last_error(NULL)) each of them left, written once by tests/golden/make_golden_refusals.py
from the library as it stood before the host side's refusals were moved onto one function (csrc/tthost.h: tthost::fail).  The
table is replayed here and code and text are compared exactly; entry points with several checks come with inputs that fail
different ones, which pins the order of the checks too.

An argument of the table is a JSON value: null (NULL), a number, {"ptr": n} (a pointer that is never dereferenced: every call
here is refused first), {"out": ctype} (the address of a fresh value of that type), {"struct": name, "fields": {...}} (the
address of a _lib structure; a field may itself be an argument) or {"array": name, "items": [fields, ...]}."""
import ctypes as C
import json
import os

import pytest

from conftest import GOLDEN

TABLE = os.path.join(GOLDEN, "refusals.json")


def _struct(L, keep, name, fields):
    s = getattr(L, name)()
    for k, v in fields.items():
        setattr(s, k, _arg(L, keep, v, field=True))
    keep.append(s)
    return s


def _arg(L, keep, v, field=False):
    if not isinstance(v, dict):
        return v
    if "ptr" in v:
        return v["ptr"] if field else C.c_void_p(v["ptr"])
    if "out" in v:
        t = {"ptr": C.c_void_p, "i64": C.c_int64, "f32x4": C.c_float * 4, "nstep": L.TTPopNstep}[v["out"]]
        keep.append(t())
        return C.byref(keep[-1])
    if "struct" in v:
        return C.pointer(_struct(L, keep, v["struct"], v["fields"]))
    t = getattr(L, v["array"])
    keep.append((t * len(v["items"]))(*[_struct(L, keep, v["array"], f) for f in v["items"]]))
    return C.cast(keep[-1], C.POINTER(t))


def call(L, case):
    """Makes the call of one table entry; returns (return code, tt_last_error(NULL))."""
    dll, keep = L.load(), []
    fn = getattr(dll, case["fn"])
    args = [_arg(L, keep, a) for a in case["args"]]
    rc = fn(*[C.cast(a, t) if isinstance(a, C.c_void_p) else a for a, t in zip(args, fn.argtypes)])      # ({"ptr": n} for a typed pointer)
    return int(rc), dll.tt_last_error(None).decode()


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib
    return _lib


def test_every_refusal_of_the_table_keeps_its_code_and_its_text(L):
    table = json.load(open(TABLE))
    assert len(table) >= 100 and len({c["fn"] for c in table}) >= 35
    wrong = []
    for case in table:
        assert case["code"] != L.TT_OK and case["message"].startswith(case["fn"]), case      # the table holds refusals only
        got = call(L, case)
        if got != (case["code"], case["message"]):
            wrong.append((case["fn"], case["args"], got, (case["code"], case["message"])))
    assert not wrong, wrong
