"""GPU: attention over a dense cache through an index of kept positions (kvz_retain_attn / kvz_retain_attn_append,
include/kvzip_hip_retain.h).  Exact probes scattered into a dense store under four mask kinds (tests/retain_probes.py; the index is built
on the host), bit equality with kvz_varlen_attn on the compacted copy and oracle parity on random data, the append form against
kvz_dense_append + kvz_retain_attn with guard bands around everything it may not write, and an index that points outside the rows in
use."""
import contextlib

import pytest
import torch

import attn_probes as ap
import kvzip_oracle as orc
import retain_probes as rp
from conftest import check_attn
from guards import Arena, frozen, interior

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}       # (the bounds of tests/test_gpu_spec_attn.py)
SINK, N = 5, 1500
TAILS = (1, 40)            # rows behind the context before the query positions
ITEMS = (0, 3, 16)         # attn_items: the default, fewer items than heads (every head one range), ranges of 256 keys
GEOMS = [(G, D, q_len) for G in (1, 4, 7) for D in (64, 128) for q_len in (1, 3, 9)]
DTYPES = [torch.float16, torch.bfloat16]


def _ops():
    from kvzip_amd import ops
    return ops


@contextlib.contextmanager
def knob(name, val):
    lib = _ops()._lib.load()
    prev = lib.kvz_debug_set_tunable(name.encode(), int(val))
    try:
        yield
    finally:
        lib.kvz_debug_set_tunable(name.encode(), prev)


def _eff_items(items, Hkv=4):
    return items if items > 0 else torch.cuda.get_device_properties(0).multi_processor_count - Hkv


def _attend(d, p, idx=None):
    """kvz_retain_attn of probe p's queries over the dense store d -> [Hkv*q_len, G, D] (CPU)."""
    ops = _ops()
    out = ops.retain_attn(p.q.to(DEV), d.k.to(DEV).unsqueeze(0), d.v.to(DEV).unsqueeze(0), (d.idx if idx is None else idx).to(DEV), d.meta,
                          d.ctx_end, d.fill, p.q_len, causal=p.causal, softmax_scale=p.scale)
    torch.cuda.synchronize()
    return out.cpu()


def _append(d, p):
    """kvz_retain_attn_append: the store without its last row + that row -> (out, k, v) as the device holds them afterwards."""
    ops = _ops()
    before, k_new, v_new = rp.split_last(d)
    k, v = before.k.to(DEV).unsqueeze(0), before.v.to(DEV).unsqueeze(0)
    out = ops.retain_attn_append(p.q.to(DEV), k, v, k_new.to(DEV), v_new.to(DEV), d.idx.to(DEV), d.meta, d.ctx_end, before.fill,
                                 softmax_scale=p.scale)
    torch.cuda.synchronize()
    return out.cpu(), k[0].cpu(), v[0].cpu()


def _same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(-1).view(torch.int16), b.view(-1).view(torch.int16))


def _exact(name, make, G, D, q_len, dtype, causal=True):
    """Every tail x attn_items: the plain form, and at q_len = 1 the append form, give the bits of the exact expectation."""
    masks = rp.make_masks(N, seed=G + D + q_len)
    for tail0 in TAILS:
        tail = tail0 + q_len
        lens = rp.head_lens(masks, SINK, tail)
        for items in ITEMS:
            p = make(lens, q_len, G, D, dtype, causal, _eff_items(items))
            want = ap.expected(p, "div")
            d = rp.scatter(p, masks, SINK, tail)
            with knob("attn_items", items):
                got = _attend(d, p)
                same, n = ap.bits_equal(got, want)
                assert not torch.isnan(got.float()).any(), (name, tail0, items, "an evicted or unfilled row was read")
                assert same, (name, tail0, items, n, int(ap.steps(got, want).max()))
                if q_len == 1:
                    got, k, v = _append(d, p)
                    assert ap.bits_equal(got, want)[0], (name, tail0, items, "append form")
                    assert _same_bits(k, d.k) and _same_bits(v, d.v), (name, "append form: the store afterwards")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("G,D,q_len", GEOMS)
def test_uniform_probe_exact(G, D, q_len, dtype):
    _exact(f"uniform G{G} D{D} q{q_len} {dtype}",
           lambda lens, q, g, dd, dt, causal, it: ap.uniform_probe(lens, q, g, dd, dt, causal=causal, items=(it,), slack=0, seed=q),
           G, D, q_len, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("G,D,q_len", GEOMS)
def test_weighted_probe_exact(G, D, q_len, dtype):
    _exact(f"weighted G{G} D{D} q{q_len} {dtype}",
           lambda lens, q, g, dd, dt, causal, it: ap.weighted_probe(lens, q, g, dd, dt, causal=causal, slack=0, seed=q),
           G, D, q_len, dtype)


@pytest.mark.parametrize("kind", ["uniform", "weighted"])
def test_probes_without_causal_mask(kind):
    for G, D, q_len in ((7, 128, 3), (4, 64, 9)):
        if kind == "uniform":
            make = lambda lens, q, g, dd, dt, causal, it: ap.uniform_probe(lens, q, g, dd, dt, causal=causal, items=(it,), slack=0, seed=1)
        else:
            make = lambda lens, q, g, dd, dt, causal, it: ap.weighted_probe(lens, q, g, dd, dt, causal=causal, slack=0, seed=1)
        _exact(f"{kind} non-causal G{G} D{D} q{q_len}", make, G, D, q_len, torch.float16, causal=False)


def test_range_edge_at_the_end_of_the_index():
    """With 16 items the ranges are 256 keys long; a head with exactly 256 indexed positions (sink 5 + 251 kept) has a range edge at
    n_h: one block reads only indexed rows and the next starts with the first computed one."""
    G, D, dtype = 7, 128, torch.float16
    masks = rp.make_masks(N, seed=3, random_kept=251)
    for q_len in (1, 3):
        for tail0 in TAILS:
            tail = tail0 + q_len
            lens = rp.head_lens(masks, SINK, tail)
            assert ap.decode_chunk(lens, 16) == 256 == SINK + int(masks[2].sum())
            for p in (ap.uniform_probe(lens, q_len, G, D, dtype, items=(16,), slack=0, seed=2),
                      ap.weighted_probe(lens, q_len, G, D, dtype, slack=0, seed=2)):
                d = rp.scatter(p, masks, SINK, tail)
                with knob("attn_items", 16):
                    got = _attend(d, p)
                assert ap.bits_equal(got, ap.expected(p, "div"))[0], (p.kind, q_len, tail0)


BOUNDARY_KEYS = {128: (8192, 8193), 64: (16384, 16385)}     # keys of the long head: 8 * 1024 / D key ranges of 128 keys, and one more


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("G,D", [(7, 128), (4, 64)])
def test_combine_at_the_boundary_between_its_two_paths(G, D, dtype):
    """The combine holds up to 8 partials per thread in registers (8 * 1024 / D per row) and takes its general path beyond.  With
    attn_items = 1024 a key range is its 128-key minimum, so a head of 8192 keys (D = 128; 16384 at D = 64) has the last partial count
    of the fast path and a head of one key more the first of the general path.  The heads beside it have one key (the query's own
    row: every head of a dense cache has the tail) and two.  Split edges marked; both probe families, plain and append form."""
    n_ctx = BOUNDARY_KEYS[D][1] + 100
    for n, partials in zip(BOUNDARY_KEYS[D], (8 * 1024 // D, 8 * 1024 // D + 1)):
        one = torch.zeros(n_ctx, dtype=torch.bool)
        one[n_ctx // 2] = True
        masks = [rp.make_masks(n_ctx, seed=n, kinds=("random",), random_kept=n - 1)[0], torch.zeros(n_ctx, dtype=torch.bool), one]
        lens = rp.head_lens(masks, 0, 1)
        assert lens == [n, 1, 2] and ap.decode_chunk(lens, 1024) == 128 and -(-n // 128) == partials
        for p in (ap.uniform_probe(lens, 1, G, D, dtype, items=(1024,), slack=0, seed=n),
                  ap.weighted_probe(lens, 1, G, D, dtype, slack=0, seed=n)):
            want = ap.expected(p, "div")
            d = rp.scatter(p, masks, 0, 1)
            with knob("attn_items", 1024):
                got = _attend(d, p)
                assert ap.bits_equal(got, want)[0], (p.kind, n, int(ap.steps(got, want).max()))
                got, k, v = _append(d, p)
                assert ap.bits_equal(got, want)[0], (p.kind, n, "append form", int(ap.steps(got, want).max()))
                assert _same_bits(k, d.k) and _same_bits(v, d.v), (p.kind, n, "append form: the store afterwards")


def _gather_route(p):
    """kvz_varlen_attn on the compacted copy (the probe's own flat rows, no slack), metadata on the device as RetainCache.prepare
    hands it over."""
    ops = _ops()
    ks = torch.tensor(p.starts, dtype=torch.int32, device=DEV)
    kl = torch.tensor(p.lens, dtype=torch.int32, device=DEV)
    out = ops.varlen_attn(p.q.to(DEV), p.k.to(DEV), p.v.to(DEV), ks, kl, p.q_len, max(p.lens), causal=True, softmax_scale=p.scale)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("G,D,q_len", GEOMS)
def test_random_equals_gather_route_and_oracle(G, D, q_len, dtype):
    masks = rp.make_masks(N, seed=7 * G + q_len)
    Hkv = len(masks)
    for tail0 in TAILS:
        tail = tail0 + q_len
        lens = rp.head_lens(masks, SINK, tail)
        p = rp.random_probe(lens, q_len, G, D, dtype, seed=q_len + tail0)
        d = rp.scatter(p, masks, SINK, tail)
        want = orc.varlen_attn(p.q, p.k, p.v, p.starts, p.lens, q_len, causal=True)
        for items in ITEMS:
            with knob("attn_items", items):
                got = _attend(d, p)
                ref = _gather_route(p)
                assert torch.equal(got, ref), (G, D, q_len, dtype, tail0, items, int((got != ref).sum()))
                if q_len == 1:
                    got_a, k, v = _append(d, p)
                    assert torch.equal(got_a, ref) and _same_bits(k, d.k) and _same_bits(v, d.v), (G, D, dtype, tail0, items, "append form")
        check_attn(f"retain/random/G{G}D{D}q{q_len}t{tail0}/{dtype}", got.reshape(Hkv * q_len, G, D), want, TOL[dtype], ulp_of=dtype)


def _ok(rc, who):
    assert rc == 0, f"{who}: code {rc}: {_ops()._lib.load().kvz_last_error()}"


@pytest.mark.parametrize("items", [3, 16, 0], ids=["items3", "items16", "default"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("G,D", [(7, 128), (4, 64), (1, 128)])
def test_append_form_guarded(G, D, dtype, items):
    """kvz_retain_attn_append through the C ABI on buffers carved from a guarded arena: the stores (only row `fill` of every head is
    declared writable), the index, out and a workspace of exactly kvz_retain_attn_workspace_bytes, dirty (0x00 and 0xFF).  The output
    equals kvz_dense_append followed by kvz_retain_attn, row `fill` holds the new K, V, nothing else changed."""
    ops = _ops()
    lib = ops._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    masks = rp.make_masks(N, seed=G)
    Hkv = len(masks)
    tail = 40 + 1
    lens = rp.head_lens(masks, SINK, tail)
    p = rp.random_probe(lens, 1, G, D, dtype, seed=5)
    full = rp.scatter(p, masks, SINK, tail)
    before, k_new, v_new = rp.split_last(full)
    cap, fill = before.k.shape[1], before.fill
    k_new, v_new = k_new.to(DEV), v_new.to(DEV)
    with knob("attn_items", items):
        # the two-call form on ordinary tensors
        k2, v2 = before.k.to(DEV).unsqueeze(0), before.v.to(DEV).unsqueeze(0)
        _ok(lib.kvz_dense_append(k2.data_ptr(), v2.data_ptr(), k2.stride(1), fill, k_new.data_ptr(), v_new.data_ptr(), k_new.stride(1),
                                 k_new.stride(2), v_new.stride(1), v_new.stride(2), Hkv, 1, D, 2, st), "kvz_dense_append")
        want = ops.retain_attn(p.q.to(DEV), k2, v2, full.idx.to(DEV), full.meta, full.ctx_end, fill + 1, 1, softmax_scale=p.scale)
        torch.cuda.synchronize()
        assert _same_bits(k2[0], full.k) and _same_bits(v2[0], full.v)
        a = Arena(DEV)
        writable = torch.zeros(Hkv, cap, 1, dtype=torch.bool)
        writable[:, fill] = True
        stores = []
        for name, src in (("k_store", before.k), ("v_store", before.v)):
            buf = a.carve(name, ((Hkv, cap, D), dtype), names=("head", "row", "elem"))
            in_use = ~torch.isnan(src.float()).all(-1)                # (every other row keeps the arena's pattern)
            buf[in_use.to(DEV)] = src.to(DEV)[in_use.to(DEV)]
            a.declare(buf, writable | in_use.unsqueeze(-1))
            stores.append(buf)
        k, v = stores
        idx = a.carve("idx", ((full.idx.numel(),), torch.int32))
        idx.copy_(full.idx.to(DEV))
        need = int(lib.kvz_retain_attn_workspace_bytes(Hkv, G, 1, D))
        ws = a.carve("retain_ws", need, guard=need)
        out = a.carve("out", ((Hkv, G, D), dtype), names=("head", "group", "elem"))
        q = p.q.to(DEV)
        meta = full.meta
        meta_before = list(meta)
        snap_k, snap_v = k.clone(), v.clone()
        for dirt in (0x00, 0xFF):
            interior(ws, dirt)
            out.fill_(float("nan"))
            k.copy_(snap_k)
            v.copy_(snap_v)
            with frozen(q, k_new, v_new, idx):
                _ok(lib.kvz_retain_attn_append(q.data_ptr(), k.data_ptr(), v.data_ptr(), k.stride(0), cap, k_new.data_ptr(), v_new.data_ptr(),
                                               k_new.stride(1), v_new.stride(1), idx.data_ptr(), idx.numel(), meta, full.ctx_end, fill, Hkv,
                                               G, D, float(p.scale), ops._dtype_code(dtype), out.data_ptr(), ws.data_ptr(), ws.numel(), st),
                    "kvz_retain_attn_append")
                torch.cuda.synchronize()
            assert list(meta) == meta_before
            assert _same_bits(out, want), (G, D, dtype, items, dirt)
            assert _same_bits(k[:, fill], k_new[0, :, 0]) and _same_bits(v[:, fill], v_new[0, :, 0]), "row `fill` holds the new K, V"
            rest = torch.ones(cap, dtype=torch.bool, device=DEV)
            rest[fill] = False
            assert _same_bits(k[:, rest], snap_k[:, rest]) and _same_bits(v[:, rest], snap_v[:, rest]), "another row of the store was written"
            a.assert_clean()


def test_out_of_range_index_values_are_clamped():
    """Positions at or behind `fill`, far outside the store and negative ones: the call returns and the device is fine afterwards (the
    kernel clamps a position to the rows in use before it becomes an address).  The output is not compared."""
    G, D, dtype = 7, 128, torch.float16
    masks = rp.make_masks(N, seed=1)
    for q_len in (1, 3):
        tail = 1 + q_len
        lens = rp.head_lens(masks, SINK, tail)
        p = rp.random_probe(lens, q_len, G, D, dtype, seed=9)
        d = rp.scatter(p, masks, SINK, tail)
        bad = d.idx.clone()
        bad[0::3] = d.fill
        bad[1::7] = 2 ** 31 - 1
        bad[2::11] = -5
        bad[3::13] = d.fill + 10 ** 6
        for items in (0, 16):
            with knob("attn_items", items):
                out = _attend(d, p, idx=bad)
                assert out.shape == p.q.shape
                if q_len == 1:
                    ops = _ops()
                    before, k_new, v_new = rp.split_last(d)
                    k, v = before.k.to(DEV).unsqueeze(0), before.v.to(DEV).unsqueeze(0)
                    ops.retain_attn_append(p.q.to(DEV), k, v, k_new.to(DEV), v_new.to(DEV), bad.to(DEV), d.meta, d.ctx_end, before.fill,
                                           softmax_scale=p.scale)
                    torch.cuda.synchronize()
    # the device still computes: the same call with the true index gives the gather route's bits
    assert torch.equal(_attend(d, p), _gather_route(p))
