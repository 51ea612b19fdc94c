"""GPU: kvz_tree_keep_path through the C ABI - the rows of the accepted path end up at slots 0 .. n - 1 of the t node slots behind
every (layer, head) segment, K and V, in place; slots whose row stays, the other node slots and everything outside them keep their
bits.  Once on rows tagged with (layer, head, node, K or V), once on buffers carved from a guarded arena (tests/guards.py) that keep
its position-dependent pattern as content, with only the slots that move declared writable."""
import ctypes as C

import pytest
import torch

from guards import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def paths(t):
    """identity, every other node, root and last node, shifted runs whose sources are other entries' destinations, a mix."""
    out = [list(range(t)), list(range(0, t, 2)), [0, t - 1], list(range(1, t)), [1, 2, 3][:max(t - 1, 1)], [0] + list(range(2, t)),
           [t - 1], []]
    if t >= 8:
        out.append([0, 1, 3, 4, 5, t - 2, t - 1])       # a kept prefix, a shifted run, a jump
    return [p for p in out if all(i <= x < t for i, x in enumerate(p))]


def _layout(L, Hkv, t, extra):
    """Per layer: segments of different lengths with t + extra free rows behind each; (rows, row0 [L*Hkv]) with node 0's slot
    `extra` rows into the free rows of (layer, head) - rows appended before the step."""
    rows, row0 = [], []
    for l in range(L):
        acc = 0
        for h in range(Hkv):
            acc += 3 + 5 * h + l                        # the rows the segment holds
            row0.append(acc + extra)
            acc += extra + t + 2                        # appended before, the node slots, slack that stays free
        rows.append(acc)
    return rows, row0


def _call(ks, vs, row0, path, t, Hkv, D, dtype):
    from kvzip_amd import ops
    lib = ops._lib.load()
    L = len(ks)
    kp = (C.c_void_p * L)(*[x.data_ptr() for x in ks])
    vp = (C.c_void_p * L)(*[x.data_ptr() for x in vs])
    r0 = (C.c_int32 * len(row0))(*row0)
    ph = (C.c_int32 * max(len(path), 1))(*path)
    rc = lib.kvz_tree_keep_path(L, kp, vp, r0, ph, len(path), t, Hkv, D, ops._dtype_code(dtype), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.kvz_last_error()


def _bits(x):
    return x.contiguous().view(torch.int16)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("L,Hkv,D", [(1, 1, 64), (3, 4, 128), (1, 4, 64), (3, 1, 128)])
@pytest.mark.parametrize("t", [4, 9, 64])
def test_tagged_rows_end_up_at_the_paths_slots(t, L, Hkv, D, dtype):
    rows, row0 = _layout(L, Hkv, t, extra=2)
    g = torch.Generator().manual_seed(t)
    base_k = [torch.randint(-30000, 30000, (rows[l], D), generator=g, dtype=torch.int16) for l in range(L)]
    base_v = [torch.randint(-30000, 30000, (rows[l], D), generator=g, dtype=torch.int16) for l in range(L)]
    elem = 2048 * (torch.arange(D) % 16)
    for l in range(L):
        for h in range(Hkv):
            for node in range(t):
                for kv, base in enumerate((base_k, base_v)):
                    base[l][row0[l * Hkv + h] + node] = (((l * 4 + h) * 64 + node) * 2 + kv + elem).to(torch.int16)
    for path in paths(t):
        ks = [x.clone().view(dtype).to(DEV) for x in base_k]
        vs = [x.clone().view(dtype).to(DEV) for x in base_v]
        _call(ks, vs, row0, path, t, Hkv, D, dtype)
        for l in range(L):
            for got, base in ((_bits(ks[l]).cpu(), base_k[l]), (_bits(vs[l]).cpu(), base_v[l])):
                want = base.clone()
                for h in range(Hkv):
                    r = row0[l * Hkv + h]
                    for i, p in enumerate(path):
                        want[r + i] = base[r + p]
                assert torch.equal(got, want), (path, l, "rows at the path's slots, every other bit unchanged")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("L,Hkv,D", [(1, 1, 64), (3, 4, 128)])
@pytest.mark.parametrize("t", [5, 64])
def test_only_the_slots_that_move_are_written(t, L, Hkv, D, dtype):
    rows, row0 = _layout(L, Hkv, t, extra=1)
    for path in paths(t):
        a = Arena(DEV)
        ks, vs = [], []
        for l in range(L):
            for name, lst in (("k", ks), ("v", vs)):
                buf = a.carve(f"{name}{l}", ((rows[l], D), dtype), names=("row", "elem"))
                dec = torch.zeros(rows[l], 1, dtype=torch.bool)
                for h in range(Hkv):
                    for i, p in enumerate(path):
                        if p != i:
                            dec[row0[l * Hkv + h] + i] = True
                a.declare(buf, dec)
                lst.append(buf)
        snap = [x.clone() for x in ks + vs]
        _call(ks, vs, row0, path, t, Hkv, D, dtype)
        for l in range(L):
            for buf, s0 in ((ks[l], snap[l]), (vs[l], snap[L + l])):
                for h in range(Hkv):
                    r = row0[l * Hkv + h]
                    for i, p in enumerate(path):
                        assert torch.equal(_bits(buf[r + i]), _bits(s0[r + p])), (path, l, h, i)
        a.assert_clean()
