"""Guard bands for the writing entry point of include/kvzip_hip_multi_prefill.h: kvz_multi_prefill called through the C ABI with EVERY
buffer carved from a guarded arena (tests/guards.py) - q, the flat K and V of every cache (only the rows a segment holds plus the n_b
new rows of a participating cache's segment are declared: the slack behind them keeps the pattern), k_new, v_new, out, and a workspace
of exactly kvz_multi_prefill_workspace_bytes, dirty (0x00 and 0xFF).  Each call must return KVZ_OK, give the bits of the exact
expectation and of the ordinary ops call, leave guards, slack rows and the rows the segments held untouched, and its read-only inputs
frozen."""
import ctypes as C

import pytest
import torch

import attn_probes as ap
import multi_prefill_probes as mpp
import test_gpu_multi_prefill as tmp
from guards import Arena, frozen, interior
from test_gpu_multi_attn import knob

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
    Hkv, T, G, D = c.q.shape
    B, dtype = len(c.lens), c.dtype
    lengths = c.lengths
    st = torch.cuda.current_stream().cuda_stream
    with knob("attn_items", items):
        want = mpp.expected_out(c)
        ordinary = tmp._run(c)[0]
        a = Arena(DEV)
        # q, k_new, v_new as the layer hands them over: [1, T, heads, D] in memory, seen as [1, heads, T, D]
        mq, mk, mv = mpp.as_model_tensors(c)
        q = a.carve("q", ((1, Hkv * G, T, D), dtype), strides=(T * Hkv * G * D, D, Hkv * G * D, 1), names=("batch", "head", "pos", "elem"))
        kn = a.carve("k_new", ((1, Hkv, T, D), dtype), strides=(T * Hkv * D, D, Hkv * D, 1), names=("batch", "head", "pos", "elem"))
        vn = a.carve("v_new", ((1, Hkv, T, D), dtype), strides=(T * Hkv * D, D, Hkv * D, 1), names=("batch", "head", "pos", "elem"))
        q.copy_(mq), kn.copy_(mk), vn.copy_(mv)
        ks, vs, held = [], [], []
        for b in range(B):
            dec = torch.zeros(c.rows[b], 1, dtype=torch.bool)
            for h in range(Hkv):
                s0 = c.starts[b][h]
                dec[s0:s0 + c.old(b, h) + lengths[b]] = True
            pair = []
            for name, arena in (("k", c.arena_k), ("v", c.arena_v)):
                t = a.carve(f"{name}{b}", ((c.rows[b], D), dtype), names=("row", "elem"))
                src = arena[c.row0[b]:c.row0[b] + c.rows[b]].to(DEV)
                t[dec[:, 0].to(DEV)] = src[dec[:, 0].to(DEV)]      # (the rows the segments hold; the slack keeps the arena's pattern)
                a.declare(t, dec)
                pair.append(t)
            ks.append(pair[0]); vs.append(pair[1]); held.append(dec[:, 0].clone())
        need = int(lib.kvz_multi_prefill_workspace_bytes(T, B, Hkv, G, D))
        ws = a.carve("multi_prefill_ws", need, guard=need)
        out = a.carve("out", ((Hkv, T, G, D), dtype), names=("head", "pos", "group", "elem"))
        table = ops.MultiTable(ks, vs, c.starts, c.lens, c.slack)
        cu = (C.c_int32 * (B + 1))(*c.cu_q)
        off = (C.c_int32 * B)(*c.offset)
        snap = [(k.clone(), v.clone()) for k, v in zip(ks, vs)]
        for fill in (0x00, 0xFF):
            interior(ws, fill)
            out.fill_(float("nan"))
            with frozen(q, kn, vn):
                _ok(lib.kvz_multi_prefill(q.data_ptr(), G * q.stride(1), q.stride(1), q.stride(2), cu, table.k_ptrs, table.v_ptrs, table.seg,
                                          table.lens, table.slack, off, kn.data_ptr(), vn.data_ptr(), kn.stride(1), kn.stride(2),
                                          vn.stride(1), vn.stride(2), B, Hkv, G, D, float(c.scale), ops._dtype_code(dtype), out.data_ptr(),
                                          ws.data_ptr(), ws.numel(), st), "kvz_multi_prefill")
                torch.cuda.synchronize()
            assert ap.bits_equal(out.cpu(), want)[0] and _same(out, ordinary), (c.kind, fill, items)
            for b in range(B):
                new_rows = torch.zeros(c.rows[b], dtype=torch.bool)
                for h in range(Hkv):
                    r, n = c.starts[b][h] + c.old(b, h), lengths[b]
                    new_rows[r:r + n] = True
                    sl = slice(c.cu_q[b], c.cu_q[b + 1])
                    assert _same(ks[b][r:r + n], c.k_new[h, sl]) and _same(vs[b][r:r + n], c.v_new[h, sl]), (c.kind, b, h, "new rows")
                assert int(new_rows.sum()) == Hkv * lengths[b]              # the declared 2 * Hkv * n_b rows (K and V), no more
                old = (held[b] & ~new_rows).to(DEV)
                assert _same(ks[b][old], snap[b][0][old]) and _same(vs[b][old], snap[b][1][old]), (c.kind, b, "a row a segment held was written")
            a.assert_clean()


@pytest.mark.parametrize("items", [3, None], ids=["items3", "default"])
@pytest.mark.parametrize("G,D,dtype", [(7, 128, torch.float16), (4, 64, torch.bfloat16)], ids=["f16-G7-D128", "bf16-G4-D64"])
def test_multi_prefill(G, D, dtype, items):
    """The exact cases of test_gpu_multi_prefill (three caches, offsets 0 / 5 / 1) with a cache without positions, and with all
    three taking part."""
    for lengths in ([5, 0, 17], [17, 3, 1]):
        for kind in ("uniform", "weighted"):
            c, _, _ = tmp._probe(kind, tmp._frozen(tmp.LENS), tuple(tmp.OFFSETS), tuple(lengths), G, D, dtype, 10 * G)
            _guarded(c, items)


@pytest.mark.parametrize("items", [3, None], ids=["items3", "default"])
def test_multi_prefill_exactly_at_the_slack(items):
    """offset + n_b == slack for every participating cache: the last new row is the last free row before the next segment (whose
    first row is declared, and must stay what it was)."""
    lens, offsets, lengths = [[300, 37], [0, 129], [64, 255]], [3, 0, 7], [5, 8, 1]
    make = {"uniform": mpp.uniform_case, "weighted": mpp.weighted_case}
    for kind in ("uniform", "weighted"):
        _guarded(make[kind](lens, offsets, lengths, 7, 128, torch.float16, slack=8, seed=3), items)
