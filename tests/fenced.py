"""Fenced buffers: the instrument of tests/test_gpu_fences.py (plain torch; works on CPU tensors, tests/test_fenced_cpu.py).

Every array of the C ABI (include/ttenv.h) is a caller-owned device pointer of a stated extent.  An Arena hands out named buffers
whose payload has exactly that extent and sits between a front fence and a back fence of a recognisable bit pattern, inside one
larger allocation of its own:

    | slack | front fence (as large as the back fence) | payload (256-byte aligned [+ misalign]) | back fence (>= one workgroup tile, >= 4 KiB) |

A store past either end of the payload lands in a fence and is found by Arena.check(), byte by byte (a u8 array written in 4-byte
words is caught); it never leaves the allocation, so nothing here can fault.  A load past the end returns the fence's fill, which
the caller chooses for INPUT buffers (`surround`): the NaN pattern, a huge finite value or zeros -- a result that depends on it
depends on memory the kernel must not read.  Output payloads are prefilled with the pattern, so an element the kernel was to
write and did not is found too.

Patterns per element width: f32 0x7FC5A5A5 and f64 0x7FF8A5A5A5A5A5A5 (quiet NaNs with a fixed payload), i32 0x5A5A5A5A, i64
0x5A5A5A5A5A5A5A5A, u8 0xA5.  The fill is laid out on the payload's own element grid, so an element read just past the payload is
one whole pattern element."""
import collections

import torch

ALIGN = 256
MIN_FENCE = 4096
SURROUNDS = ("nan", "huge", "zero")

_INT_VIEW = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
_PATTERN = {torch.float32: 0x7FC5A5A5, torch.float64: 0x7FF8A5A5A5A5A5A5, torch.int32: 0x5A5A5A5A,
            torch.int64: 0x5A5A5A5A5A5A5A5A, torch.uint8: 0xA5}
# a value far outside anything valid: 3e38 for floats, near the type's maximum for integers
_HUGE = {torch.float32: 3e38, torch.float64: 3e38, torch.int32: 0x7FFFFFF0, torch.int64: 0x7FFFFFFFFFFFFFF0, torch.uint8: 0xFF}

Finding = collections.namedtuple("Finding", "name kind side offset")
Finding.__str__ = lambda f: (f"{f.name}: {f.side} fence changed at byte {f.offset}" if f.kind == "fence" else
                             f"{f.name}: payload element {f.offset} still holds the prefill")


def pattern_bytes(dtype, fill="nan"):
    """The little-endian bytes of one fill element of `dtype` (a CPU uint8 tensor of the element's width)."""
    if fill == "zero":
        return torch.zeros(torch.empty((), dtype=dtype).element_size(), dtype=torch.uint8)
    if fill == "huge":
        return torch.tensor([_HUGE[dtype]], dtype=dtype).view(torch.uint8).clone()
    assert fill == "nan", fill
    width = torch.empty((), dtype=dtype).element_size()
    return torch.tensor([_PATTERN[dtype]], dtype=torch.int64).view(torch.uint8)[:width].clone()


def _tiled(pat, phase, nbytes):
    """nbytes bytes whose byte i is pat[(i - phase) mod width]: the pattern on an element grid that passes through `phase`."""
    w = pat.numel()
    return pat.repeat(nbytes // w + 3)[(w - phase % w) % w:][:nbytes]


class _Buf:
    __slots__ = ("name", "raw", "start", "nbytes", "back", "dtype", "shape", "full", "expected", "tensor")


class Arena:
    def __init__(self, device, surround="nan"):
        assert surround in SURROUNDS, surround
        self.device, self.surround = torch.device(device), surround
        self.bufs = {}

    # ------------------------------------------------------------------------------------------------- making buffers
    def _make(self, name, shape, dtype, tile_rows, misalign, fence_fill, full, tile_bytes=0):
        assert name not in self.bufs, name
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        width = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * width
        row_bytes = nbytes // shape[0] if shape and shape[0] else width
        assert 0 <= misalign < ALIGN and misalign % width == 0
        back = -(-max(MIN_FENCE, tile_rows * row_bytes, tile_bytes) // ALIGN) * ALIGN
        front = back                                       # (an underrun of a whole tile stays inside the allocation too)
        raw = torch.empty(ALIGN + front + misalign + nbytes + back, dtype=torch.uint8, device=self.device)
        start = (-raw.data_ptr()) % ALIGN + front + misalign
        total = start + nbytes + back
        raw = raw[:total]
        pat = pattern_bytes(dtype, fence_fill)
        image = _tiled(pat, start, total).clone()
        image[start:start + nbytes] = _tiled(pattern_bytes(dtype, "nan"), 0, nbytes)      # the payload's prefill
        raw.copy_(image)
        b = _Buf()
        b.name, b.raw, b.start, b.nbytes, b.back, b.dtype, b.shape, b.full = name, raw, start, nbytes, back, dtype, shape, full
        b.expected = raw.clone()
        b.tensor = raw[start:start + nbytes].view(dtype).view(shape)
        assert b.tensor.data_ptr() % ALIGN == misalign
        self.bufs[name] = b
        return b.tensor

    def out(self, name, shape, dtype=torch.float32, tile_rows=1, full=True, misalign=0, tile_bytes=0, also_input=False):
        """An output of exactly `shape`, prefilled with the pattern.  full: the entry point fills every element (check() then
        reports any that still holds the prefill).  tile_rows: rows (of shape[1:] elements) one workgroup of the kernel under
        test covers -- the back fence holds at least that many (or tile_bytes bytes, for layouts that are not row-major by
        workgroup), so a whole tile past the end stays inside the allocation.  misalign: the payload's address modulo 256
        (bytes), for pointers the library's own callers pass less aligned.  also_input: a later launch reads the buffer, so its
        fences take the arena's `surround` fill like an input's."""
        return self._make(name, shape, dtype, tile_rows, misalign, self.surround if also_input else "nan", full, tile_bytes)

    def inp(self, name, data, tile_rows=1, misalign=0, tile_bytes=0):
        """An input (or an in/out array): a copy of `data` between fences of the arena's `surround` fill."""
        t = self._make(name, data.shape if data.dim() else (1,), data.dtype, tile_rows, misalign, self.surround, False, tile_bytes)
        t.copy_(data.reshape(t.shape))
        return t.view(data.shape) if data.dim() else t.view(())

    def __getitem__(self, name):
        return self.bufs[name].tensor

    def items(self):
        return [(name, b.tensor) for name, b in self.bufs.items()]

    # ------------------------------------------------------------------------------------------------------- checking
    def check(self):
        """A list of Findings (empty = clean): per buffer (a) the first changed byte of either fence -- side "front": offset < 0,
        bytes before the payload's first byte; side "back": offset >= 0, bytes past its end -- and (b) for fully written
        buffers the first payload element that still holds the prefill bits."""
        found = []
        for b in self.bufs.values():
            end = b.start + b.nbytes
            for side, lo, hi, origin in (("front", 0, b.start, b.start), ("back", end, end + b.back, end)):
                bad = (b.raw[lo:hi] != b.expected[lo:hi]).nonzero()
                if bad.numel():
                    found.append(Finding(b.name, "fence", side, int(bad[0, 0]) + lo - origin))
            if b.full and b.nbytes:
                width = b.nbytes // max(1, b.tensor.numel())
                same = (b.raw[b.start:end].view(_INT_VIEW[width]) == b.expected[b.start:end].view(_INT_VIEW[width])).nonzero()
                if same.numel():
                    found.append(Finding(b.name, "unwritten", "payload", int(same[0, 0])))
        return found

    def assert_clean(self, what=""):
        found = self.check()
        assert not found, f"{what}: " + "; ".join(str(f) for f in found)


class Plain:
    """The same interface on ordinary, separately allocated tensors of exactly the stated size (what the library's callers pass):
    the run a fenced run is compared with, bit for bit.  Outputs get the same prefill, so that elements an entry point leaves
    alone compare equal."""
    surround = None

    def __init__(self, device):
        self.device, self.tensors = torch.device(device), {}

    def out(self, name, shape, dtype=torch.float32, **_):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        t = torch.empty(shape, dtype=dtype, device=self.device)
        nbytes = t.numel() * t.element_size()
        t.view(-1).view(torch.uint8).copy_(_tiled(pattern_bytes(dtype, "nan"), 0, nbytes))
        self.tensors[name] = t
        return t

    def inp(self, name, data, **_):
        self.tensors[name] = t = data.clone()
        return t

    def __getitem__(self, name):
        return self.tensors[name]

    def items(self):
        return list(self.tensors.items())

    def check(self):
        return []

    def assert_clean(self, what=""):
        pass
