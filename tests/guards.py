"""A guarded arena: buffers whose surroundings are known, so that a kernel's write OUTSIDE the buffer its ABI declares is seen.

Every GPU test takes its outputs and workspaces from ``torch.empty``; the caching allocator rounds each request up and carves it from
a segment of several megabytes, so a kernel that writes one row past its output, one head stride too far, into the slack rows of the
compacted cache or past a workspace whose size function is a little too small corrupts a neighbouring tensor and every value test
still passes.  ``Arena.carve`` hands out a buffer from the MIDDLE of a larger ``uint8`` allocation instead:

* the buffer starts 256-byte aligned and is EXACTLY as large as asked for - the byte behind its last declared byte is guard;
* the guard on each side is at least 64 KiB and at least one unit of the buffer's outermost stride (one head, one layer's rows, one
  1024-row tile, one workspace sub-buffer - ``guard=`` names it in bytes where the shape does not), so an off-by-one row / head / tile /
  split lands in it;
* guards hold a position-dependent byte pattern, a fixed integer hash of the byte's offset in the allocation that ``check`` generates
  again instead of keeping a copy.  A kernel that writes zeros, NaNs, counters or copies of its input there changes a byte with
  probability 255/256;
* a strided buffer (``strides=``) also gets a GAP MASK: the bytes inside its extent that belong to no declared element hold the pattern
  too and are checked (an ``out_head_stride`` larger than m, the o_stride_* of the dense forward, ...).  ``declare`` narrows the
  declared elements further (only rows ``fill .. fill+t`` of a dense cache, only row ``tail_len[b]`` of a tail, no slack row).

What it sees: writes within the guard of a declared buffer, writes into stride gaps and undeclared rows, and - with ``interior`` - a
dependence on what a workspace held before the call.  What it does NOT see: a wild write further away than the guard, and a write
of the very byte the pattern holds at that place (``pattern_byte`` says which; tests/test_guards.py asserts it is the only blind spot).

Plain module: no fixture, no pytest setting.  Works on CPU tensors (the self-test) and on device tensors; the comparison runs where
the arena lives and only the verdict - counts and first offsets - crosses to the host."""
from __future__ import annotations

import contextlib
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple, Union

import torch

MIN_GUARD = 64 * 1024
ALIGN = 256
_CHUNK = 1 << 22       # pattern bytes generated at a time (the hash runs in int64: 32 MiB of temporaries per chunk)


def pattern(lo: int, hi: int, device, seed: int = 0) -> torch.Tensor:
    """The guard pattern of allocation offsets lo .. hi as uint8: the low byte of a 32-bit integer hash of the offset."""
    out = torch.empty(max(hi - lo, 0), dtype=torch.uint8, device=device)
    for a in range(lo, hi, _CHUNK):
        b = min(a + _CHUNK, hi)
        x = torch.arange(a, b, dtype=torch.int64, device=device) + (seed * 0x9E3779B1 & 0xFFFFFFFF)
        x = (x * 0x9E3779B1) & 0xFFFFFFFF
        x = x ^ (x >> 15)
        x = (x * 0x85EBCA6B) & 0xFFFFFFFF
        x = x ^ (x >> 13)
        x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        x = x ^ (x >> 16)
        out[a - lo:b - lo] = (x & 0xFF).to(torch.uint8)
    return out


def pattern_byte(offset: int, seed: int = 0) -> int:
    """The same hash for one offset, in plain Python (what a guard byte at `offset` of its allocation holds)."""
    x = (offset + (seed * 0x9E3779B1 & 0xFFFFFFFF))
    x = (x * 0x9E3779B1) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x & 0xFF


def _round_up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


@dataclass
class Violation:
    name: str
    where: str          # "before" | "after" | "gap"
    first: int          # first changed byte, relative to the buffer's first byte (negative: in the guard before it)
    count: int          # changed bytes in that region
    at: str             # `first` in the buffer's own units

    def __str__(self):
        place = {"before": "before the buffer", "after": "after the buffer", "gap": "in a gap of the buffer"}[self.where]
        return f"{self.name}: {self.count} byte(s) changed {place}, first at byte {self.first} = {self.at}"


@dataclass
class _Buf:
    name: str
    slab: int
    start: int                  # offset of the first byte in the slab
    nbytes: int                 # extent: exactly what was asked for
    guard: int
    shape: Tuple[int, ...]
    strides: Tuple[int, ...]    # elements
    itemsize: int
    names: Tuple[str, ...]
    tensor: torch.Tensor = field(repr=False, default=None)
    gap: Optional[torch.Tensor] = field(repr=False, default=None)   # bool per extent byte: True = belongs to no declared element

    def locate(self, off: int) -> str:
        """Byte offset relative to the buffer -> its own units, outermost stride first ("head 4 of 4, row 0, +0 B")."""
        dims = sorted((d for d in range(len(self.shape)) if self.strides[d] > 0), key=lambda d: -self.strides[d])
        rest, parts = off, []
        for d in dims:
            sb = self.strides[d] * self.itemsize
            idx = rest // sb            # (floors: a byte in the guard before the buffer is "head -1")
            rest -= idx * sb
            parts.append(f"{self.names[d]} {idx} of {self.shape[d]}")
        parts.append(f"+{rest} B")
        return ", ".join(parts)


class Arena:
    """Hands out guarded buffers on `device`.  Slabs of `slab_bytes` (or as large as one buffer with its guards needs) are allocated on
    demand; a buffer never touches a slab's edge."""

    def __init__(self, device, slab_bytes: int = 8 << 20, seed: int = 0):
        self.device = torch.device(device)
        self.slab_bytes = slab_bytes
        self.seed = seed
        self.slabs: List[torch.Tensor] = []
        self.cursor: List[int] = []
        self.bufs: List[_Buf] = []

    # ---- carving -----------------------------------------------------------------------------------------------------------------
    def carve(self, name: str, spec: Union[int, Tuple[Sequence[int], torch.dtype]], guard: Optional[int] = None, align: int = ALIGN,
              strides: Optional[Sequence[int]] = None, names: Optional[Sequence[str]] = None) -> torch.Tensor:
        """A buffer of `spec` = nbytes (-> uint8 [nbytes]) or (shape, dtype), with element `strides` (default: contiguous).
        `guard`: bytes of one outermost unit where the shape does not say it (a workspace sub-buffer, a 1024-row tile); the guard on
        each side is max(guard, one outermost stride, 64 KiB), rounded up to `align`.  `names`: what the dims are called in a report."""
        if isinstance(spec, int):
            shape, dtype = (spec,), torch.uint8
        else:
            shape, dtype = tuple(int(s) for s in spec[0]), spec[1]
        itemsize = torch.empty((), dtype=dtype).element_size()
        if strides is None:
            strides, acc = [], 1
            for s in reversed(shape):
                strides.append(acc)
                acc *= max(s, 1)
            strides = tuple(reversed(strides))
        strides = tuple(int(s) for s in strides)
        assert len(strides) == len(shape) and all(s >= 0 for s in strides) and align % itemsize == 0
        numel = 1
        for s in shape:
            numel *= s
        extent = 0 if numel == 0 else (1 + sum((n - 1) * st for n, st in zip(shape, strides))) * itemsize
        unit = max(strides) * itemsize if len(shape) > 1 else 0
        g = _round_up(max(MIN_GUARD, unit, guard or 0), align)
        need = g + _round_up(extent, align) + g
        si = None
        for i, slab in enumerate(self.slabs):
            if _round_up(self.cursor[i], align) + need <= slab.numel():
                si = i
                break
        if si is None:
            self.slabs.append(torch.empty(max(self.slab_bytes, need + align), dtype=torch.uint8, device=self.device))
            self.cursor.append(0)
            si = len(self.slabs) - 1
        slab = self.slabs[si]
        # (the slab's own base is aligned by the allocator; keep the buffer's ADDRESS aligned whatever it is)
        base = slab.data_ptr()
        lo = _round_up(base + self.cursor[si], align) - base
        start = lo + g
        end = start + extent
        self.cursor[si] = _round_up(end, align) + g
        slab[lo:self.cursor[si]] = pattern(lo, self.cursor[si], self.device, self.seed + si)
        if extent:
            t = slab[start:end].view(dtype).as_strided(shape, strides)
        else:
            t = slab[start:start].view(dtype).view(shape)
        assert extent == 0 or t.data_ptr() % align == 0
        names = tuple(names) if names is not None else tuple(f"dim{d}" for d in range(len(shape)))
        if dtype == torch.uint8 and len(shape) == 1:
            names = ("byte",)
        b = _Buf(name, si, start, extent, g, shape, strides, itemsize, names, t)
        self.bufs.append(b)
        self._set_declared(b, None)
        return t

    def _find(self, t: Union[str, torch.Tensor]) -> _Buf:
        for b in self.bufs:
            if (isinstance(t, str) and b.name == t) or (isinstance(t, torch.Tensor) and b.tensor is t):
                return b
        raise KeyError(t if isinstance(t, str) else "not a tensor carved from this arena")

    def _set_declared(self, b: _Buf, mask: Optional[torch.Tensor]) -> None:
        if b.nbytes == 0:
            b.gap = None
            return
        covered = torch.zeros(b.nbytes // b.itemsize, dtype=torch.bool, device=self.device)
        view = covered.as_strided(b.shape, b.strides)
        if mask is None:
            view.fill_(True)
        else:
            view.copy_(mask.to(self.device).expand(b.shape))
        b.gap = None if bool(covered.all()) else (~covered).repeat_interleave(b.itemsize)

    def declare(self, t: Union[str, torch.Tensor], writable: torch.Tensor) -> None:
        """Narrow what a kernel may write in a carved buffer to the elements where `writable` (bool, broadcastable to the buffer's shape)
        is True, and where the caller has put data of its own.  Every other byte of the extent is gap: it must still hold the
        pattern at check time - so call this AFTER filling the rows the kernel reads, with those rows included in `writable`, or
        leave them holding the pattern where the kernel only moves bytes."""
        self._set_declared(self._find(t), writable)

    # ---- checking ----------------------------------------------------------------------------------------------------------------
    def _diff(self, b: _Buf, lo: int, hi: int) -> torch.Tensor:
        return self.slabs[b.slab][lo:hi] != pattern(lo, hi, self.device, self.seed + b.slab)

    def check(self) -> List[Violation]:
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        out: List[Violation] = []
        for b in self.bufs:
            regions = [("before", b.start - b.guard, b.start, None), ("after", b.start + b.nbytes, b.start + b.nbytes + b.guard, None)]
            if b.gap is not None:
                regions.append(("gap", b.start, b.start + b.nbytes, b.gap))
            diffs = []
            for _, lo, hi, gap in regions:
                d = self._diff(b, lo, hi)
                diffs.append(d & gap if gap is not None else d)
            counts = torch.stack([d.sum() for d in diffs]).tolist()          # (the verdict: one small copy per buffer)
            for (where, lo, _, _), d, n in zip(regions, diffs, counts):
                if n:
                    first = lo + int(d.to(torch.uint8).argmax()) - b.start
                    out.append(Violation(b.name, where, first, int(n), b.locate(first)))
        return out

    def assert_clean(self) -> None:
        v = self.check()
        assert not v, "guard violations:\n  " + "\n  ".join(str(x) for x in v)

    def blind_spot(self, t: Union[str, torch.Tensor], off: int) -> int:
        """The one byte value whose write at `off` (relative to the buffer) `check` cannot see: the pattern's own."""
        b = self._find(t)
        return pattern_byte(b.start + off, self.seed + b.slab)

    def raw(self, t: Union[str, torch.Tensor]) -> Tuple[torch.Tensor, int]:
        """(the slab's bytes, the buffer's offset in it): for a self-test that plays the faulty kernel."""
        b = self._find(t)
        return self.slabs[b.slab], b.start


def interior(buf: torch.Tensor, fill: int) -> torch.Tensor:
    """Pre-fill a workspace's INSIDE with 0x00 or 0xFF bytes (NaN as fp16 / fp32, 4 G as a counter): a kernel whose workspace "needs no
    initialisation" returns the same bits after either."""
    assert fill in (0x00, 0xFF) and buf.dtype == torch.uint8 and buf.is_contiguous()
    buf.fill_(fill)
    return buf


@contextlib.contextmanager
def frozen(*tensors: Optional[torch.Tensor]):
    """Snapshot read-only inputs (q, k, v, masks, metadata, pointer tables, a fork's shared cache, row statistics) and assert on exit
    that each is bit-identical.  None entries are skipped."""
    live = [t for t in tensors if t is not None]
    snaps = [t.detach().clone() for t in live]
    yield
    for i, (t, s) in enumerate(zip(live, snaps)):
        if t.is_cuda:
            torch.cuda.synchronize(t.device)
        a = t.contiguous().view(-1).view(torch.uint8) if t.numel() else t
        b = s.contiguous().view(-1).view(torch.uint8) if s.numel() else s
        assert torch.equal(a, b), f"read-only input {i} (shape {tuple(t.shape)}, {t.dtype}) was written: " \
                                  f"{int((a != b).sum())} byte(s) differ, first at byte {int((a != b).to(torch.uint8).argmax())}"
