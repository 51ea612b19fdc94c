"""GPU: kvz_fork_branch_copy through the C ABI.  Tails of three layers with capacities 8 / 40 / 40, B = 5 slots, every element tagged
with its (layer, slot, head, row); after the call every tail equals the host-computed expectation bit for bit - destinations, the
rows >= rows_i behind them, sources and bystanders - and every refusal of the header leaves the tails as they were.

Rows per pair come from {0, 1, 7, 33}.  A run must fit EVERY layer of the call (rows_i > tail_cap_host[l] is KVZ_EINVAL), so the cases
run on all three layers with rows from {0, 1, 7} and on the two layers of capacity 40 with 33 among them; 33 rows against the layer of
capacity 8 is one of the refusals."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAPS = (8, 40, 40)
B = 5
EINVAL, EUNSUPPORTED = -1, -4


def tagged_tails(caps, Hkv, D, dtype, is_v):
    """Per layer [B, Hkv, cap, D]: even columns hold the (layer, slot, head, row) tag, odd columns their own index (K and V differ)."""
    out = []
    for l, cap in enumerate(caps):
        b, h, r = torch.meshgrid(torch.arange(B), torch.arange(Hkv), torch.arange(cap), indexing="ij")
        tag = ((l * 8 + b) * 4 + h) * 64 + r + (8192 if is_v else 0)
        t = tag[..., None].expand(B, Hkv, cap, D).clone()
        t[..., 1::2] = torch.arange(1, D, 2) + 16384 + (8192 if is_v else 0)
        out.append(t.to(torch.int16).view(dtype).to(DEV))
    return out


def expected(tails, pairs, rows):
    out = [t.clone() for t in tails]
    for t, o in zip(tails, out):
        for (s, d), n in zip(pairs, rows):
            o[d, :, :n] = t[s, :, :n]
    return out


def same(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def call(tk, tv, pairs, nrows, **over):
    from kvzip_amd import ops
    lib = ops._lib.load()
    L = len(tk)
    a = dict(k=(C.c_void_p * L)(*[t.data_ptr() for t in tk]), v=(C.c_void_p * L)(*[t.data_ptr() for t in tv]),
             cap=(C.c_int32 * L)(*[t.shape[2] for t in tk]), B=tk[0].shape[0], Hkv=tk[0].shape[1], D=tk[0].shape[3],
             elem=tk[0].element_size())
    n = max(len(pairs), 1)
    a.update(src=(C.c_int32 * n)(*[s for s, _ in pairs]), dst=(C.c_int32 * n)(*[d for _, d in pairs]), rows=(C.c_int32 * n)(*nrows))
    a.update(over)
    rc = lib.kvz_fork_branch_copy(a["k"], a["v"], a["cap"], L, a["B"], a["Hkv"], a["D"], a["elem"], a["src"], a["dst"], a["rows"],
                                  len(pairs), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, lib.kvz_last_error()


CASES = {
    "one source to three destinations": [(2, 0), (2, 4), (2, 1)],
    "two independent pairs": [(4, 1), (0, 3)],
    "no pairs": [],
}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("Hkv,D", [(1, 64), (3, 128), (3, 64), (1, 128)])
def test_copy_is_exact(Hkv, D, dtype):
    for layers, row_sets in (((0, 1, 2), [(7, 0, 1), (1, 7, 7), (0, 0, 0), (7, 7, 7)]), ((1, 2), [(33, 7, 1), (1, 33, 33), (33, 33, 33)])):
        caps = [CAPS[l] for l in layers]
        for name, pairs in CASES.items():
            for rs in row_sets if pairs else [()]:
                rows = list(rs[:len(pairs)])
                tk, tv = tagged_tails(caps, Hkv, D, dtype, False), tagged_tails(caps, Hkv, D, dtype, True)
                wk, wv = expected(tk, pairs, rows), expected(tv, pairs, rows)
                rc, msg = call(tk, tv, pairs, rows)
                assert rc == 0, (name, rows, msg)
                for l in range(len(caps)):
                    assert same(tk[l], wk[l]) and same(tv[l], wv[l]), (name, layers, rows, "layer", l)
                if pairs and max(rows) > 0:           # (the expectation is not the input: something had to move)
                    assert not same(tk[-1], tagged_tails(caps, Hkv, D, dtype, False)[-1])


def test_through_ops_and_more_layers_than_one_launch_takes():
    """ops.fork_branch_copy on 130 layers (one launch carries 128: the entry point issues a second one), capacities alternating."""
    from kvzip_amd import ops
    caps = [8 if l % 3 == 0 else 12 for l in range(130)]
    g = torch.Generator().manual_seed(0)
    tk = [torch.randint(-30000, 30000, (B, 2, c, 64), generator=g, dtype=torch.int16).view(torch.float16).to(DEV) for c in caps]
    tv = [torch.randint(-30000, 30000, (B, 2, c, 64), generator=g, dtype=torch.int16).view(torch.float16).to(DEV) for c in caps]
    pairs, rows = [(1, 0), (1, 4), (3, 2)], [8, 3, 5]
    wk, wv = expected(tk, pairs, rows), expected(tv, pairs, rows)
    ops.fork_branch_copy(tk, tv, pairs, rows)
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(tk, wk)) and all(same(a, b) for a, b in zip(tv, wv))
    assert same(tk[129][0, :, :8], tk[129][1, :, :8]) and same(tk[128][2, :, :5], tk[128][3, :, :5])     # the second launch's layers


def test_refusals_leave_the_tails_untouched():
    Hkv, D, dtype = 3, 128, torch.float16
    tk, tv = tagged_tails(CAPS, Hkv, D, dtype, False), tagged_tails(CAPS, Hkv, D, dtype, True)
    k0, v0 = [t.clone() for t in tk], [t.clone() for t in tv]
    L = len(CAPS)
    ptrs = lambda ts, at=None, val=None: (C.c_void_p * L)(*[val if i == at else t.data_ptr() for i, t in enumerate(ts)])  # noqa: E731
    ok = [(2, 0)]
    refused = [
        ("null table", ok, [1], dict(k=None), EINVAL, b"null pointer"),
        ("null capacities", ok, [1], dict(cap=None), EINVAL, b"null pointer"),
        ("null pair list", ok, [1], dict(rows=None), EINVAL, b"null pointer"),
        ("null tail", ok, [1], dict(v=ptrs(tv, 1, None)), EINVAL, b"layer 1"),
        ("misaligned tail", ok, [1], dict(k=ptrs(tk, 2, tk[2].data_ptr() + 8)), EINVAL, b"aligned"),
        ("src beyond B", [(5, 0)], [1], {}, EINVAL, b"outside [0, 5)"),
        ("src negative", [(-1, 0)], [1], {}, EINVAL, b"outside [0, 5)"),
        ("dst beyond B", [(0, 5)], [1], {}, EINVAL, b"outside [0, 5)"),
        ("src == dst", [(3, 3)], [1], {}, EINVAL, b"onto itself"),
        ("a slot on both sides", [(0, 1), (1, 2)], [1, 1], {}, EINVAL, b"both a source and a destination"),
        ("a slot on both sides, other order", [(1, 2), (0, 1)], [1, 1], {}, EINVAL, b"both a source and a destination"),
        ("repeated dst", [(0, 2), (1, 2)], [1, 1], {}, EINVAL, b"destination twice"),
        ("negative rows", ok, [-1], {}, EINVAL, b"rows[0] = -1"),
        ("rows beyond the smallest capacity", ok, [9], {}, EINVAL, b"capacity 8"),
        ("33 rows against the layer of 8", [(2, 0), (2, 1)], [1, 33], {}, EINVAL, b"rows[1] = 33"),
        ("row bytes not a multiple of 16", ok, [1], dict(D=4), EUNSUPPORTED, b"multiple of 16"),
        ("17 slots", ok, [1], dict(B=17), EUNSUPPORTED, b"B <= 16"),
        ("65 heads", ok, [1], dict(Hkv=65), EUNSUPPORTED, b"Hkv <= 64"),
    ]
    for name, pairs, rows, over, code, text in refused:
        rc, msg = call(tk, tv, pairs, rows, **over)
        assert rc == code and text in msg, (name, rc, msg)
        assert all(same(a, b) for a, b in zip(tk, k0)) and all(same(a, b) for a, b in zip(tv, v0)), name
