"""CPU self-test of tests/guards.py: a tool that cannot see the fault it was built for fails here, before anyone needs a GPU.

On CPU tensors, for a contiguous and a strided buffer: a clean run, a one-byte write immediately before and immediately after the
buffer, a write one outer-stride unit past the end, a write into a stride gap - each detected and named - and a write of the very byte
the pattern holds, the one blind spot.  Then a fault model of the real thing in plain torch: an order-preserving gather that is off by
one row from the second 1024-row tile on lands in a slack row and is caught by the gap mask."""
import pytest
import torch

import guards
from guards import Arena, frozen, interior

Hkv, ROWS, D = 3, 40, 64                                # a [Hkv, ROWS, D] fp16 output
CONTIG = dict(spec=((Hkv, ROWS, D), torch.float16), strides=None)
STRIDED = dict(spec=((Hkv, ROWS, D), torch.float16), strides=((ROWS + 24) * D, D, 1))   # head stride 24 rows wider than the rows
NAMES = ("head", "row", "elem")


def _carve(kind):
    a = Arena("cpu", slab_bytes=1 << 20)
    a.carve("neighbour_before", 1000)
    t = a.carve("out", kind["spec"], strides=kind["strides"], names=NAMES)
    a.carve("neighbour_after", 77)
    return a, t


def _poke(a, t, off, value=None):
    """what a faulty kernel does: one byte at `off` relative to the buffer's first byte"""
    slab, start = a.raw(t)
    old = int(slab[start + off])
    slab[start + off] = (old + 1) & 0xFF if value is None else value
    return old


def _extent(t):
    return (1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))) * t.element_size()


@pytest.mark.parametrize("kind", [CONTIG, STRIDED], ids=["contiguous", "strided"])
def test_clean_run_and_exact_size(kind):
    a, t = _carve(kind)
    assert t.data_ptr() % 256 == 0 and t.shape == (Hkv, ROWS, D) and t.dtype == torch.float16
    t.copy_(torch.randn(Hkv, ROWS, D).half())           # every declared element written: still clean
    assert a.check() == []
    a.assert_clean()
    b = a._find(t)
    assert b.nbytes == _extent(t), "the size is exactly what was asked for, not rounded"
    assert b.guard >= guards.MIN_GUARD and b.guard >= t.stride(0) * 2, "at least 64 KiB and one outermost stride"
    assert (b.gap is None) == (kind is CONTIG)


def test_guard_is_one_outer_unit_when_that_is_larger_than_64k():
    a = Arena("cpu", slab_bytes=1 << 20)
    t = a.carve("big_heads", ((2, 300, 128), torch.float16))
    assert a._find(t).guard >= 300 * 128 * 2 > guards.MIN_GUARD
    w = a.carve("ws", 5000, guard=200_000)               # a workspace: the caller names its sub-buffer
    assert a._find(w).guard >= 200_000 and w.numel() == 5000 and w.dtype == torch.uint8
    a.assert_clean()


@pytest.mark.parametrize("kind", [CONTIG, STRIDED], ids=["contiguous", "strided"])
def test_one_byte_before_and_after(kind):
    a, t = _carve(kind)
    _poke(a, t, -1)
    (v,) = a.check()
    assert (v.name, v.where, v.first, v.count) == ("out", "before", -1, 1) and v.at.startswith("head -1 of 3")
    a, t = _carve(kind)
    n = _extent(t)
    _poke(a, t, n)
    (v,) = a.check()
    assert (v.name, v.where, v.first, v.count) == ("out", "after", n, 1)
    if kind is CONTIG:
        assert v.at == "head 3 of 3, row 0 of 40, elem 0 of 64, +0 B", v.at
    else:
        assert v.at == "head 2 of 3, row 40 of 40, elem 0 of 64, +0 B", v.at
    with pytest.raises(AssertionError, match=r"out: 1 byte\(s\) changed after the buffer"):
        a.assert_clean()


@pytest.mark.parametrize("kind", [CONTIG, STRIDED], ids=["contiguous", "strided"])
def test_write_one_outer_unit_past_the_end(kind):
    """A head stride too far: row 5 of head Hkv.  It lies inside the guard because the guard is at least one outermost stride."""
    a, t = _carve(kind)
    off = (Hkv * t.stride(0) + 5 * D) * 2
    slab, start = a.raw(t)
    slab[start + off:start + off + 2 * D] = 0            # one row of zeros
    (v,) = a.check()
    assert v.name == "out" and v.where == "after" and v.first >= off and v.count >= 2 * D - 4
    assert v.at.startswith("head 3 of 3, row 5 of 40"), v.at
    assert [x.name for x in a.check()] == ["out"], "the neighbours are clean: their guards do not overlap this one"


def test_write_into_a_stride_gap():
    a, t = _carve(STRIDED)
    off = (1 * t.stride(0) + ROWS * D) * 2               # the first byte behind head 1's rows: "row 40" of head 1
    _poke(a, t, off)
    (v,) = a.check()
    assert (v.where, v.first, v.count) == ("gap", off, 1) and v.at == "head 1 of 3, row 40 of 40, elem 0 of 64, +0 B", v.at


def test_declare_narrows_the_writable_rows():
    """Only rows 7 .. 10 of every head are declared (a dense append): a write to row 10 is a gap violation, a write to row 9 is not."""
    a, t = _carve(CONTIG)
    rows = torch.zeros(1, ROWS, 1, dtype=torch.bool)
    rows[0, 7:10] = True
    a.declare(t, rows)
    t[:, 7:10] = 1.0
    a.assert_clean()
    t[2, 10, 3] = 1.0
    (v,) = a.check()
    assert v.where == "gap" and v.at == "head 2 of 3, row 10 of 40, elem 3 of 64, +0 B", v.at


@pytest.mark.parametrize("kind", [CONTIG, STRIDED], ids=["contiguous", "strided"])
def test_the_blind_spot_is_the_patterns_own_byte_and_nothing_else(kind):
    a, t = _carve(kind)
    n = _extent(t)
    for off in (-1, n, n + 12345, -guards.MIN_GUARD):
        same = a.blind_spot(t, off)
        for value in range(256):
            old = _poke(a, t, off, value)
            assert old == same, "the guard holds the documented hash of its offset"
            seen = bool(a.check())
            assert seen == (value != same), (off, value)
            _poke(a, t, off, old)
    a.assert_clean()
    # position-dependent: a copied run of guard bytes does not match somewhere else
    p = guards.pattern(0, 4096, "cpu")
    assert len(set(p.tolist())) == 256 and not torch.equal(p[:2048], p[2048:])
    assert [guards.pattern_byte(i) for i in range(64)] == p[:64].tolist()


def test_interior_and_frozen():
    a = Arena("cpu", slab_bytes=1 << 20)
    ws = a.carve("ws", 1001)
    assert interior(ws, 0xFF).view(-1)[1000] == 255 and interior(ws, 0x00).sum() == 0
    a.assert_clean()
    x, y = torch.arange(10.0), torch.arange(6, dtype=torch.int32).view(2, 3)[:, :2]
    with frozen(x, None, y):
        pass
    with pytest.raises(AssertionError, match=r"read-only input 1 .* was written"):
        with frozen(x, y):
            y[1, 1] = 9


# ---- the fault model of the real thing: the compaction gather --------------------------------------------------------------------
TILE = 1024


def _gather(k, masks, seg, out, tile_fault=0):
    """Order-preserving gather in plain torch, walked tile by tile like the kernel: the j-th kept row of head h goes to row seg[h] + j.
    `tile_fault`: added to the base of every tile but the first (a tile_base that counts one row too many)."""
    for h in range(k.shape[0]):
        base = 0
        for t0 in range(0, k.shape[1], TILE):
            m = masks[h, t0:t0 + TILE]
            rows = k[h, t0:t0 + TILE][m]
            at = seg[h] + base + (tile_fault if t0 else 0)
            out[at:at + rows.shape[0]] = rows
            base += int(m.sum())


@pytest.mark.parametrize("slack", [1, 37])
def test_gather_off_by_one_at_a_tile_edge_lands_in_a_slack_row(slack):
    Hk, klen, Dd = 3, 2 * TILE + 100, 32
    g = torch.Generator().manual_seed(slack)
    k = torch.randn(Hk, klen, Dd, generator=g).half()
    masks = torch.rand(Hk, klen, generator=g) < 0.4
    masks[1] = False                                     # an all-evicted head: its only rows are slack
    lens = masks.sum(-1).tolist()
    seg = [sum(lens[:h]) + h * slack for h in range(Hk)]
    total = sum(lens) + Hk * slack
    for fault in (0, 1):
        a = Arena("cpu", slab_bytes=4 << 20)
        out = a.carve("k_out", ((total, Dd), torch.float16), guard=TILE * Dd * 2, names=("row", "elem"))
        assert a._find(out).guard >= TILE * Dd * 2
        declared = torch.zeros(total, 1, dtype=torch.bool)
        for h in range(Hk):
            declared[seg[h]:seg[h] + lens[h]] = True
        a.declare(out, declared)
        _gather(k, masks, seg, out, tile_fault=fault)
        want = torch.cat([k[h][masks[h]] for h in range(Hk)])
        got = torch.cat([out[seg[h]:seg[h] + lens[h]] for h in range(Hk)])
        v = a.check()
        if not fault:
            assert v == [] and torch.equal(got, want)
            continue
        # the last kept row of head 0 went one row too far: the first slack row behind head 0
        assert v and v[0].name == "k_out" and v[0].where == "gap", v
        assert v[0].at.startswith(f"row {lens[0]} of {total}"), v[0].at
        assert v[0].count >= Dd * 2 - 8                  # (a row of fp16 noise: nearly every byte differs from the pattern)
