"""Guard bands for the writing entry point of include/kvzip_hip_multi.h (the layer tests/test_gpu_guard_bands.py is for kvzip_hip.h):
kvz_multi_attn_append called through the C ABI on buffers carved from a guarded arena (tests/guards.py) - the flat K and V of every
cache (only the rows a segment holds plus the ONE new row of a live cache's segment are declared: the slack behind them keeps the
pattern), out, and a workspace of exactly kvz_multi_attn_workspace_bytes, dirty (0x00 and 0xFF).  Each call must return KVZ_OK, give the
bits of the exact expectation and of the ordinary ops call, leave guards, slack rows and the rows the segments held untouched, and its
read-only inputs frozen."""
import ctypes as C

import pytest
import torch

import attn_probes as ap
import multi_probes as mp
import test_gpu_multi_attn as tma
from guards import Arena, frozen, interior

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ok(rc, who):
    from kvzip_amd import ops
    assert rc == 0, f"{who}: code {rc}: {ops._lib.load().kvz_last_error()}"


def _same(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.numel() == b.numel() and torch.equal(a.view(-1).view(torch.uint8), b.view(-1).view(torch.uint8))


def _guarded(c, items):
    from kvzip_amd import ops
    lib = ops._lib.load()
    B, Hkv, G, D = c.q.shape
    dtype = c.dtype
    st = torch.cuda.current_stream().cuda_stream
    with tma.knob("attn_items", items):
        want = mp.expected_out(c)
        ordinary = tma._run(c)[0]
        q, kn = c.q.to(DEV), c.k_new.to(DEV)
        vn = c.v_new.to(DEV).transpose(1, 2).contiguous().transpose(1, 2)
        a = Arena(DEV)
        ks, vs, held = [], [], []
        for b in range(B):
            dec = torch.zeros(c.rows[b], 1, dtype=torch.bool)
            for h in range(Hkv):
                s0 = c.starts[b][h]
                dec[s0:s0 + c.seen(b, h) + (1 if c.offset[b] >= 0 else 0)] = True
            pair = []
            for name, arena in (("k", c.arena_k), ("v", c.arena_v)):
                t = a.carve(f"{name}{b}", ((c.rows[b], D), dtype), names=("row", "elem"))
                src = arena[c.row0[b]:c.row0[b] + c.rows[b]].to(DEV)
                t[dec[:, 0].to(DEV)] = src[dec[:, 0].to(DEV)]      # (the rows the segments hold; the slack keeps the arena's pattern)
                a.declare(t, dec)
                pair.append(t)
            ks.append(pair[0]); vs.append(pair[1]); held.append(dec[:, 0].clone())
        need = int(lib.kvz_multi_attn_workspace_bytes(B, Hkv, G, D))
        ws = a.carve("multi_ws", need, guard=need)
        out = a.carve("out", ((B, Hkv, G, D), dtype), names=("cache", "head", "group", "elem"))
        table = ops.MultiTable(ks, vs, c.starts, c.lens, c.slack)
        off = (C.c_int32 * B)(*c.offset)
        snap = [(k.clone(), v.clone()) for k, v in zip(ks, vs)]
        for fill in (0x00, 0xFF):
            interior(ws, fill)
            out.fill_(float("nan"))
            with frozen(q, kn, vn):
                _ok(lib.kvz_multi_attn_append(q.data_ptr(), table.k_ptrs, table.v_ptrs, table.seg, table.lens, table.slack, off, kn.data_ptr(),
                                              vn.data_ptr(), kn.stride(0), kn.stride(1), vn.stride(0), vn.stride(1), B, Hkv, G, D, float(c.scale),
                                              ops._dtype_code(dtype), out.data_ptr(), ws.data_ptr(), ws.numel(), st), "kvz_multi_attn_append")
                torch.cuda.synchronize()
            assert ap.bits_equal(out.cpu(), want)[0] and _same(out, ordinary), (c.kind, fill, items)
            for b in range(B):
                new_rows = torch.zeros(c.rows[b], dtype=torch.bool)
                if c.offset[b] >= 0:
                    for h in range(Hkv):
                        r = c.starts[b][h] + c.seen(b, h)
                        new_rows[r] = True
                        assert _same(ks[b][r], c.k_new[b, h, 0]) and _same(vs[b][r], c.v_new[b, h, 0]), (c.kind, b, h, "new row")
                else:
                    assert bool((out[b] == 0).all())
                old = (held[b] & ~new_rows).to(DEV)
                assert _same(ks[b][old], snap[b][0][old]) and _same(vs[b][old], snap[b][1][old]), (c.kind, b, "a row a segment held was written")
            a.assert_clean()


@pytest.mark.parametrize("items", [3, 16, None], ids=["items3", "items16", "default"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,D", [(7, 128), (20, 64)])
def test_multi_attn_append(G, D, dtype, items):
    """The exact cases of test_gpu_multi_attn (three caches, offsets 0 / 5 / 1) and the same with cache 1 inactive."""
    target = mp.multi_items(items or 0, 6)
    for off in (tma.OFFSETS, [0, -1, 1]):
        _guarded(mp.uniform_case(tma.LENS, off, G, D, dtype, tma.SLACK, items=(target,), seed=G), items)
        _guarded(mp.weighted_case(tma.LENS, off, G, D, dtype, tma.SLACK, seed=G), items)


def test_multi_attn_append_at_the_segment_limit():
    """B * Hkv = 128 segments, lengths <= 200: the largest table; the workspace of that geometry is exact as well."""
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(0, 201, (16, 8), generator=g).tolist()
    offs = torch.randint(-1, 6, (16,), generator=g).tolist()
    for items in (16, None):
        _guarded(mp.weighted_case(lens, offs, 4, 64, torch.float16, slack=8, seed=6), items)
