"""Guard bands for the verify call of include/kvzip_hip_tree.h (what tests/test_gpu_spec_guards.py is for the chain call):
kvz_tree_attn_append through the C ABI on buffers carved from a guarded arena (tests/guards.py) - the flat K and V (only the rows a
segment holds plus the t node rows behind it are declared: the rest of the slack keeps the pattern), out, and a workspace of exactly
kvz_tree_attn_workspace_bytes, dirty (0x00 and 0xFF).  Each call must return KVZ_OK, give the bits of the exact expectation and of the
ordinary ops call, leave guards, the remaining slack rows and the rows the segments held untouched, and its read-only inputs frozen."""
import ctypes as C

import pytest
import torch

import attn_probes as ap
import spec_probes as sp
import test_gpu_spec_attn as tsa
import test_gpu_tree_attn as tta
import tree_probes as tp
from guards import Arena, frozen, interior

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _same(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.numel() == b.numel() and torch.equal(a.view(-1).view(torch.uint8), b.view(-1).view(torch.uint8))


def _guarded(c, parents, items, meta=True, dev_arrays=True):
    from kvzip_amd import ops
    lib = ops._lib.load()
    Hkv, t, G, D = c.q.shape
    dtype = c.dtype
    st = torch.cuda.current_stream().cuda_stream
    with tsa.knob("attn_items", items):
        want = tp.expected_out(c, parents)
        ordinary = tta._run(c, parents, meta=meta, dev_arrays=dev_arrays)[0]
        q = c.q.to(DEV)
        kn, vn = tsa._new_rows(c)
        rows = c.k.shape[0]
        held = torch.zeros(rows, dtype=torch.bool)
        new_rows = torch.zeros(rows, dtype=torch.bool)
        for h in range(Hkv):
            held[c.starts[h]:c.starts[h] + c.lens[h]] = True
            new_rows[c.starts[h] + c.lens[h]:c.starts[h] + c.lens[h] + t] = True
        a = Arena(DEV)
        kv = []
        for name, src in (("k", c.k), ("v", c.v)):
            buf = a.carve(name, ((rows, D), dtype), names=("row", "elem"))
            buf[held.to(DEV)] = src.to(DEV)[held.to(DEV)]          # (the rows the segments hold; the slack keeps the arena's pattern)
            a.declare(buf, (held | new_rows)[:, None])
            kv.append(buf)
        k, v = kv
        need = int(lib.kvz_tree_attn_workspace_bytes(t, Hkv, G, D))
        ws = a.carve("tree_ws", need, guard=need)
        out = a.carve("out", ((Hkv, t, G, D), dtype), names=("head", "node", "group", "elem"))
        base = [n - c.k_len_offset for n in c.lens]
        ks = torch.tensor(c.starts, dtype=torch.int32, device=DEV) if dev_arrays else None
        kl = torch.tensor(base, dtype=torch.int32, device=DEV) if dev_arrays else None
        mh = ops._meta_host(c.starts, base, Hkv) if meta else None
        mh_before = list(mh) if mh is not None else None
        masks = (C.c_uint64 * t)(*ops.ancestor_masks(parents))
        masks_before = list(masks)
        snap_k, snap_v = k.clone(), v.clone()
        for fill in (0x00, 0xFF):
            interior(ws, fill)
            out.fill_(float("nan"))
            with frozen(q, kn, vn, ks, kl):
                rc = lib.kvz_tree_attn_append(q.data_ptr(), k.data_ptr(), v.data_ptr(), ops._ptr(ks), ops._ptr(kl), c.k_len_offset, mh,
                                              c.k_len_offset + c.slack, kn.data_ptr(), vn.data_ptr(), kn.stride(0), kn.stride(1),
                                              vn.stride(0), vn.stride(1), t, Hkv, G, D, float(c.scale), ops._dtype_code(dtype),
                                              out.data_ptr(), ws.data_ptr(), ws.numel(), masks, st)
                assert rc == 0, f"kvz_tree_attn_append: code {rc}: {lib.kvz_last_error()}"
                torch.cuda.synchronize()
            assert (mh is None or list(mh) == mh_before) and list(masks) == masks_before
            assert ap.bits_equal(out.cpu(), want)[0] and _same(out, ordinary), (c.kind, fill, items)
            for h in range(Hkv):
                r = c.starts[h] + c.lens[h]
                assert _same(k[r:r + t], c.k_new[h]) and _same(v[r:r + t], c.v_new[h]), (c.kind, h, "new rows")
            old = held.to(DEV)
            assert _same(k[old], snap_k[old]) and _same(v[old], snap_v[old]), (c.kind, "a row a segment held was written")
            a.assert_clean()


@pytest.mark.parametrize("items", [3, 16, 0], ids=["items3", "items16", "default"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,t,D", [(7, 4, 128), (7, 9, 128), (2, 16, 64), (1, 64, 128), (64, 1, 64)])
def test_tree_attn_append(G, t, D, dtype, items):
    """Exact cases of test_gpu_tree_attn (one and two row tiles per block, one and two blocks per item, 64 nodes), rows appended before."""
    target = sp.spec_items(items, len(tsa.LENS))
    _guarded(sp.uniform_case(tsa.LENS, t, G, D, dtype, k_len_offset=3, items=(target,), seed=G), tp.parents_of("random", t), items)
    _guarded(sp.weighted_case(tsa.LENS_EMPTY, t, G, D, dtype, seed=G), tp.parents_of("interleaved", t), items)


def test_tree_attn_append_metadata_forms():
    for meta, dev_arrays in ((False, True), (True, False)):
        _guarded(sp.weighted_case(tsa.LENS, 5, 7, 128, torch.float16, k_len_offset=3, seed=2), tp.parents_of("random", 5), 16, meta=meta,
                 dev_arrays=dev_arrays)
