"""Guard bands for the entry points of include/kvzip_hip_tighten.h (the layer tests/test_gpu_guard_bands.py is for kvzip_hip.h):
kvz_recompact_layers and kvz_mask_resurrects called through the C ABI on outputs carved from a guarded arena (tests/guards.py).
The outputs have exactly sum(new_len + slack) rows and only the rows new_len + appended of every head are declared writable, the
counter is 4 bytes; every input - the old flat K,V, both masks, both plans, the appended-row counts, the pointer table - is frozen.
Each call must return KVZ_OK, give the bits of the ordinary ops call and leave guards, slack rows and inputs untouched."""
import pytest
import torch

from guards import Arena, frozen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def _ops():
    from kvzip_amd import ops
    return ops


def _ok(rc, who):
    assert rc == 0, f"{who}: code {rc}: {_ops()._lib.load().kvz_last_error()}"


def _same(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.numel() == b.numel() and torch.equal(a.view(-1).view(torch.uint8), b.view(-1).view(torch.uint8))


def _masks(mode, L, Hkv, N, g):
    """(old, new) CPU bool [L, Hkv, N] with new a subset of old, and the tensors the ops take."""
    def heads(mh):
        return mh.view(L, Hkv, 1).expand(L, Hkv, N).clone(), mh.view(L, 1, Hkv, 1).to(DEV).expand(L, 1, Hkv, N)

    def toks(m):
        return m, m.view(L, 1, Hkv, N).to(DEV)
    nh = torch.rand(L, Hkv, generator=g) < 0.5
    nh[0, 0], nh[-1, -1] = False, True
    if mode == "tok-tok":
        old = torch.rand(L, Hkv, N, generator=g) < 0.6
        new = old & (torch.rand(L, Hkv, N, generator=g) < 0.5)
        new[0, 0] = False                      # an emptied head
        new[0, 1] = old[0, 1]                  # an unchanged head
        old[-1, -1, max(N - 5, 0):] = True     # kept up to the last word before sink + N, by both
        new[-1, -1, max(N - 5, 0):] = True
        return toks(old) + toks(new)
    if mode == "tok-head":
        new, new_t = heads(nh)
        return toks((torch.rand(L, Hkv, N, generator=g) < 0.6) | new) + (new, new_t)
    oh = nh.clone()
    oh[0, 0] = True
    return heads(oh) + heads(nh)


def _recompact(mode, L, Hkv, sink, N, tail, slack, D, eb, seed):
    ops = _ops()
    lib = ops._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    klen = sink + N + tail
    g = torch.Generator().manual_seed(seed)
    it = _INT[eb]
    K = [torch.randint(0, 100, (1, Hkv, klen, D), generator=g).to(it).to(DEV) for _ in range(L)]
    V = [torch.randint(0, 100, (1, Hkv, klen, D), generator=g).to(it).to(DEV) for _ in range(L)]
    old, old_t, new, new_t = _masks(mode, L, Hkv, N, g)
    ones = lambda n: torch.ones(L, Hkv, n, dtype=torch.bool)   # noqa: E731
    old_lens = torch.cat([ones(sink), old, ones(tail)], -1).sum(-1)
    new_lens = torch.cat([ones(sink), new, ones(tail)], -1).sum(-1)
    old_plan = ops.compact_plan(old_t, sink, klen, slack=slack)
    new_plan = ops.compact_plan(new_t, sink, klen, slack=slack)
    ko, vo = ops.compact_layers(K, V, old_plan, [int(old_lens[l].sum()) + Hkv * slack for l in range(L)])
    app = [min(3, slack), min(1, slack)] + [0] * (L - 2)        # rows appended behind every head of a layer since the old prune
    old_seg = old_plan.seg_start.cpu().tolist()
    for l in range(L):
        for h in range(Hkv):
            s = old_seg[l][h] + int(old_lens[l, h])
            ko[l][s:s + app[l]] = 101 + h
            vo[l][s:s + app[l]] = 111 + h
    tail_rows = torch.tensor(app, dtype=torch.int32).to(DEV) if any(app) else None
    totals = [int(new_lens[l].sum()) + Hkv * slack for l in range(L)]
    assert all(t > 0 for t in totals)
    seg_h = [[int(new_lens[l, :h].sum()) + h * slack for h in range(Hkv)] for l in range(L)]
    assert new_plan.seg_start.cpu().tolist() == seg_h
    a = Arena(DEV)
    count = a.carve("count", ((1,), torch.int32))
    outs = []
    for l in range(L):
        pair = []
        for kv in "kv":
            o = a.carve(f"{kv}_out{l}", ((totals[l], D), it), guard=1024 * D * eb, names=("row", "elem"))
            dec = torch.zeros(totals[l], 1, dtype=torch.bool)
            for h in range(Hkv):
                dec[seg_h[l][h]:seg_h[l][h] + int(new_lens[l, h]) + app[l]] = True
            a.declare(o, dec)
            pair.append(o)
        outs.append(pair)
    ov, otok1 = ops._mask_bytes(old_t)
    nv, ntok1 = ops._mask_bytes(new_t)
    assert otok1 == (0 if mode == "head-head" else 1) and ntok1 == (1 if mode == "tok-tok" else 0)
    table = torch.tensor([[t.data_ptr() for t in ko], [t.data_ptr() for t in vo], [o[0].data_ptr() for o in outs],
                          [o[1].data_ptr() for o in outs]], dtype=torch.int64).to(DEV)
    inputs = (ov, nv, old_plan.meta, old_plan.tile_base, new_plan.meta, new_plan.tile_base, tail_rows, table, *ko, *vo)
    with frozen(*inputs):
        _ok(lib.kvz_mask_resurrects(nv.data_ptr(), ntok1, ov.data_ptr(), otok1, L * Hkv, N, count.data_ptr(), st), "kvz_mask_resurrects")
        assert int(count) == 0 == int(ops.mask_resurrects(new_t, old_t))
        _ok(lib.kvz_mask_resurrects(ov.data_ptr(), otok1, nv.data_ptr(), ntok1, L * Hkv, N, count.data_ptr(), st), "kvz_mask_resurrects")
        assert int(count) == int((old & ~new).sum()) == int(ops.mask_resurrects(old_t, new_t)) > 0
        _ok(lib.kvz_recompact_layers(table[0].data_ptr(), table[1].data_ptr(), ov.data_ptr(), otok1, old_plan.tile_base.data_ptr(),
                                     old_plan.seg_start.data_ptr(), old_plan.len_k.data_ptr(), nv.data_ptr(), ntok1,
                                     new_plan.tile_base.data_ptr(), new_plan.seg_start.data_ptr(), new_plan.len_k.data_ptr(),
                                     None if tail_rows is None else tail_rows.data_ptr(), L, Hkv, N, sink, klen, D, eb,
                                     table[2].data_ptr(), table[3].data_ptr(), st), "kvz_recompact_layers")
        torch.cuda.synchronize()
    kr, vr = ops.recompact_layers(ko, vo, old_plan, old_t, new_plan, new_t, totals, tail_rows=app)
    full = torch.cat([ones(sink), new, ones(tail)], -1)
    for l in range(L):
        for h in range(Hkv):
            s, n = seg_h[l][h], int(new_lens[l, h])
            idx = full[l, h].nonzero().view(-1).to(DEV)
            for got, src, ordinary, mark in ((outs[l][0], K[l], kr[l], 101 + h), (outs[l][1], V[l], vr[l], 111 + h)):
                assert _same(got[s:s + n], src[0, h].index_select(0, idx)), (mode, l, h, "moved rows != index_select on the full mask")
                assert _same(got[s:s + n + app[l]], ordinary[s:s + n + app[l]]), (mode, l, h, "guarded call != ordinary call")
                assert bool((got[s + n:s + n + app[l]] == mark).all()), (mode, l, h, "appended rows")
    a.assert_clean()


def _geoms():
    """(sink, N, rows behind the context): klen straddling one and two tiles, every sink % 4"""
    return [(4, 1019, 0), (5, 1019, 0), (6, 1010, 9), (7, 2041, 0), (5, 2 * 1024 + 37, 3)]


@pytest.mark.parametrize("slack", [0, 4])
@pytest.mark.parametrize("mode", ["tok-tok", "tok-head", "head-head"])
def test_recompact_over_mask_geometries(mode, slack):
    for i, (sink, N, tail) in enumerate(_geoms()):
        _recompact(mode, 2, 3, sink, N, tail, slack, 128, 2, seed=i)


@pytest.mark.parametrize("D,eb", [(64, 1), (64, 2), (128, 2), (128, 4), (256, 4)], ids=["64B", "128B", "256B", "512B", "1024B"])
def test_recompact_every_row_size(D, eb):
    """Row bytes 64 .. 1024: the five recompact_gather_kernel<LPR> instantiations (the kernel moves bytes: integer views)."""
    for sink, tail, klen in ((8, 0, 2049), (5, 9, 1025)):
        for slack in (0, 2):
            _recompact("tok-tok", 2, 2, sink, klen - sink - tail, tail, slack, D, eb, seed=D + eb)
