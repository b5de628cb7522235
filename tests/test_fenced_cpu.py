"""The fenced-buffer harness (tests/fenced.py) on CPU tensors: it is trusted by tests/test_gpu_fences.py because a write one element
or one byte past either end of a payload, and an element left unwritten, are each reported here with the right buffer and side."""
import pytest
import torch

from fenced import ALIGN, MIN_FENCE, SURROUNDS, Arena, pattern_bytes

DTYPES = (torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8)


def _arena(surround="nan"):
    a = Arena("cpu", surround)
    a.out("obs", (5, 23), torch.float32, tile_rows=128)
    a.out("done", (7,), torch.uint8, tile_rows=256)
    a.out("comp", (12, 3), torch.float64, tile_rows=1)
    a.out("idx", (5, 2), torch.int32, tile_rows=4)
    a.out("n", (1,), torch.int64)
    a.inp("act", torch.arange(7, dtype=torch.float32), tile_rows=256)
    a.inp("flags", torch.arange(7, dtype=torch.uint8), tile_rows=256)
    return a


def _fill(a):
    """What a correct kernel does: every output element written, nothing else touched."""
    for name in ("obs", "done", "comp", "idx", "n"):
        a[name].zero_()


def _bytes_around(a, name):
    """(the whole allocation as bytes, index of the payload's first byte, index one past its last)"""
    b = a.bufs[name]
    return b.raw, b.start, b.start + b.nbytes


def test_a_clean_operation_reports_nothing():
    for surround in SURROUNDS:
        a = _arena(surround)
        _fill(a)
        assert a.check() == []
        a.assert_clean()
        assert torch.equal(a["act"], torch.arange(7, dtype=torch.float32))      # inputs hold their data, not the fill


def test_payloads_are_aligned_and_fences_are_large_enough():
    a = _arena()
    for name, b in a.bufs.items():
        assert b.tensor.data_ptr() % ALIGN == 0, name
        assert b.start >= b.back >= MIN_FENCE, name            # the front fence is as large as the back fence
    assert a.bufs["obs"].back >= 128 * 23 * 4          # one policy tile of observation rows
    assert a.bufs["done"].back >= MIN_FENCE
    g = Arena("cpu")
    t = g.out("grad_b1", (400,), torch.float32, tile_rows=256, misalign=36800 % ALIGN)      # a view of a flat gradient buffer
    assert t.data_ptr() % ALIGN == 36800 % ALIGN and t.is_contiguous() and t.shape == (400,)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_one_element_past_either_end_is_reported_with_name_and_side(dtype):
    for where, side in ((-1, "front"), (0, "back")):
        a = Arena("cpu")
        a.out("other", (9,), dtype)
        t = a.out("victim", (3, 5), dtype, tile_rows=16)
        a["other"].zero_(); t.zero_()
        raw, first, end = _bytes_around(a, "victim")
        w = t.element_size()
        pos = first - w if where < 0 else end
        raw[pos:pos + w].view(dtype).fill_(1)           # one element of the payload's type, next to the payload
        found = a.check()
        assert len(found) == 1, found
        f = found[0]
        assert (f.name, f.kind, f.side) == ("victim", "fence", side)
        # the first changed byte (little endian: the element's low byte; 1.0 as f32 / f64 changes only the high bytes)
        assert (-w <= f.offset < 0) if where < 0 else (0 <= f.offset < w), f
        assert "victim" in str(f) and side in str(f)
        with pytest.raises(AssertionError, match="victim"):
            a.assert_clean("case")


def test_one_byte_next_to_a_u8_buffer_is_reported():
    """A u8 array written in 4-byte words spills at most 3 bytes: fences are compared as bytes, so even one is seen -- also a byte
    that happens to be written with a plausible value, 0 or 1."""
    for value in (0, 1, 0xA4):
        for where, side, offset in ((-1, "front", -1), (0, "back", 0), (2, "back", 2)):
            a = _arena()
            _fill(a)
            raw, first, end = _bytes_around(a, "done")
            raw[first - 1 if where < 0 else end + where] = value
            found = a.check()
            assert found == [("done", "fence", side, offset)], (value, where, found)
    # the 7-byte array written as two 4-byte words
    a = _arena()
    _fill(a)
    raw, first, end = _bytes_around(a, "done")
    raw[first:first + 8].zero_()
    assert a.check() == [("done", "fence", "back", 0)]


def test_an_element_left_unwritten_is_reported():
    for name, index in (("obs", 5 * 23 - 1), ("done", 3), ("comp", 0), ("idx", 9), ("n", 0)):
        a = _arena()
        _fill(a)
        flat = a[name].view(-1)
        flat[index:index + 1].copy_(pattern_bytes(a[name].dtype).view(a[name].dtype))      # as if never written
        assert a.check() == [(name, "unwritten", "payload", index)], name
    # a buffer that is not declared fully written may keep its prefill
    a = Arena("cpu")
    a.out("ring", (4, 8), torch.float32, full=False)
    assert a.check() == []


def test_input_fences_carry_the_chosen_fill_on_the_payloads_element_grid():
    """A load one element past an input returns one whole element of the chosen fill: the NaN pattern, 3e38 or zero."""
    import math
    for surround in SURROUNDS:
        a = _arena(surround)
        for name in ("act", "flags"):
            raw, first, end = _bytes_around(a, name)
            dt = a[name].dtype
            w = a[name].element_size()
            lo = first - (first // w) * w                    # the element grid of the payload, from the allocation's start
            before, after = raw[lo:first].view(dt), raw[end:end + ((len(raw) - end) // w) * w].view(dt)
            for x in (before[-1], after[0], after[-1]):
                if dt == torch.uint8:
                    assert int(x) == {"nan": 0xA5, "huge": 0xFF, "zero": 0}[surround]
                elif surround == "nan":
                    assert math.isnan(float(x))
                else:
                    assert float(x) == (0.0 if surround == "zero" else float(torch.tensor(3e38, dtype=dt)))
    # outputs are surrounded by the pattern whatever the inputs' fill
    a = _arena("zero")
    raw, first, end = _bytes_around(a, "obs")
    assert torch.isnan(raw[end:end + 4].view(torch.float32)).all() and torch.isnan(a["obs"]).all()
