"""Attention kernels against inputs whose correct output is known exactly (tests/attn_probes.py): BIT equality, no tolerance.

The random-input attention tests bound the error by 1e-3; at decode magnitudes one key counted wrongly stays under that
(test_attn_probes.py prints by how much).  Here the probes make every weight and every sum of a correct kernel exact, so the only
roundings left are the final normalisation and the 16-bit cast, which attn_probes emulates: an off-by-one at a split edge, a tile
edge, the causal limit, a segment end or the appended row moves an output by several grid steps.  The launch geometry is swept
(attn_items for the decode kernel, flash_min_rows / flash2_* for the multi-row kernels); every knob is restored in `finally`."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import attn_probes as ap

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RAGGED = [0, 1, 15, 16, 17, 127, 128, 129, 1024]


def _ops():
    from kvzip_amd import ops
    return ops


@contextlib.contextmanager
def knobs(**kv):
    lib = _ops()._lib.load()
    prev = []
    try:
        for name, val in kv.items():
            prev.append((name, lib.kvz_debug_set_tunable(name.encode(), int(val))))
        yield
    finally:
        for name, val in reversed(prev):
            lib.kvz_debug_set_tunable(name.encode(), val)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _items_sweep(Hkv):
    # 0: the default (CUs - Hkv)
    return (1, 2, 3, Hkv, 0, 1024)


class _Dev:
    """A probe's tensors on the device."""

    def __init__(self, p):
        self.p = p
        self.q, self.k, self.v = p.q.to(DEV), p.k.to(DEV), p.v.to(DEV)
        self.ks = torch.tensor(p.starts, dtype=torch.int32, device=DEV)


def _attn(d, lens, meta=True):
    """kvz_varlen_attn over `lens` keys per head, workspace allocated under the current knobs."""
    ops = _ops()
    p = d.p
    HQ, G, D = p.q.shape
    Hkv = HQ // p.q_len
    kl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    ws = ops.attn_workspace(Hkv, G, p.q_len, D, DEV)
    mh = ops._meta_host(p.starts, lens, Hkv) if meta else None
    return ops.varlen_attn(d.q, d.k, d.v, d.ks, kl, p.q_len, max(max(lens), 1), causal=p.causal, softmax_scale=p.scale,
                           workspace=ws, meta_host=mh)


def _report(fails, total):
    assert not fails, f"{len(fails)} of {total} calls differ from the exact expectation: {fails[:12]}"


# ------------------------------------------------------------------------------------------------------------------------------
# decode / split kernel + combine
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_decode_uniform_probe_over_geometries(dtype, D, causal):
    """Ragged heads of 0, 1, 15, 16, 17, 127, 128, 129 and 1024 (a multiple of the chunk) keys, every key marked; G in {1, 4, 5, 7, 8},
    q_len in {1, 2, 5, 64 // G}; attn_items in {1, 2, 3, Hkv, default, 1024}; segments by value and from the device arrays."""
    Hkv = len(RAGGED)
    fails, total = [], 0
    for G in (1, 4, 5, 7, 8):
        for q_len in sorted({1, 2, 5, 64 // G}):
            p = ap.uniform_probe(RAGGED, q_len, G, D, dtype, causal=causal, seed=G * 100 + q_len)
            want = ap.expected(p, "div")
            d = _Dev(p)
            for items in _items_sweep(Hkv):
                with knobs(attn_items=items):
                    for meta in (True, False):
                        got = _attn(d, p.lens, meta=meta).cpu()
                        ok, nd = ap.bits_equal(got, want)
                        total += 1
                        if not ok:
                            fails.append((G, q_len, items, meta, nd))
    _report(fails, total)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_decode_weighted_probe_over_geometries(dtype, D):
    """Power-of-two weights with the row maximum at a random key: the running-max rescale inside a split, the merge of the 8 waves
    and the combine of the splits must all be exact."""
    Hkv = len(RAGGED)
    fails, total = [], 0
    for causal in (True, False):
        for G in (1, 7, 8):
            for q_len in sorted({1, 5, 64 // G}):
                p = ap.weighted_probe(RAGGED, q_len, G, D, dtype, causal=causal, spread=8, seed=G + 10 * q_len)
                want = ap.expected(p, "div")
                d = _Dev(p)
                for items in (1, 3, Hkv, 0, 1024):
                    with knobs(attn_items=items):
                        for meta in (True, False):
                            ok, nd = ap.bits_equal(_attn(d, p.lens, meta=meta).cpu(), want)
                            total += 1
                            if not ok:
                                fails.append((causal, G, q_len, items, meta, nd))
    _report(fails, total)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_decode_long_head_split_edges_and_general_combine(dtype, D):
    """A head of 100 000 keys beside short ones: its split edges (for every attn_items value of the sweep), tile edges, ends and causal
    limits marked; with attn_items = 1024 it has ~780 partials, which takes the combine kernel's general path (> 64 partials at
    D = 128, > 128 at D = 64).  Both probe families."""
    lens = [100_000, 129, 0, 4100]
    Hkv = len(lens)
    items_all = [1, 2, 3, Hkv, _cus() - Hkv, 1024]
    fails, total = [], 0
    probes = [ap.uniform_probe(lens, q_len, 7, D, dtype, items=items_all, seed=q_len) for q_len in (1, 5)]
    probes.append(ap.weighted_probe(lens, 1, 7, D, dtype, spread=6, seed=4))
    for p in probes:
        want = ap.expected(p, "div")
        d = _Dev(p)
        for items in _items_sweep(Hkv):
            with knobs(attn_items=items):
                for meta in (True, False):
                    ok, nd = ap.bits_equal(_attn(d, p.lens, meta=meta).cpu(), want)
                    total += 1
                    if not ok:
                        fails.append((p.kind, p.q_len, items, meta, nd))
    assert ap.decode_chunk(lens, 1024) * 128 < lens[0]   # (the general path of the combine is reached)
    _report(fails, total)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_decode_65_heads_device_metadata(dtype):
    """Hkv = 65 > AT_MAXH: the segments always come from the device arrays (a host array handed in anyway is ignored)."""
    ops = _ops()
    g = torch.Generator().manual_seed(65)
    lens = torch.randint(0, 300, (65,), generator=g).tolist()
    lens[3], lens[10], lens[64] = 0, 1, 129
    fails, total = [], 0
    for p in (ap.uniform_probe(lens, 1, 4, 128, dtype, seed=1), ap.uniform_probe(lens, 3, 4, 64, dtype, seed=2),
              ap.weighted_probe(lens, 3, 4, 128, dtype, spread=8, seed=3)):
        want = ap.expected(p, "div")
        d = _Dev(p)
        HQ, G, D = p.q.shape
        for items in _items_sweep(65):
            with knobs(attn_items=items):
                for host in (False, True):
                    kl = torch.tensor(lens, dtype=torch.int32, device=DEV)
                    mh = (C.c_int32 * 130)(*p.starts, *lens) if host else None
                    got = ops.varlen_attn(d.q, d.k, d.v, d.ks, kl, p.q_len, max(lens), causal=p.causal, softmax_scale=p.scale,
                                          workspace=ops.attn_workspace(65, G, p.q_len, D, DEV), meta_host=mh).cpu()
                    ok, nd = ap.bits_equal(got, want)
                    total += 1
                    if not ok:
                        fails.append((p.kind, p.q_len, D, items, host, nd))
    _report(fails, total)


def test_decode_workspace_sized_under_a_smaller_knob_is_refused():
    ops = _ops()
    p = ap.uniform_probe([300, 5, 0], 1, 7, 128, torch.float16, seed=9)
    d = _Dev(p)
    kl = torch.tensor(p.lens, dtype=torch.int32, device=DEV)
    with knobs(attn_items=3):
        small = ops.attn_workspace(3, 7, 1, 128, DEV)
        with knobs(attn_items=1024):
            big = ops.attn_workspace(3, 7, 1, 128, DEV)
            assert big.numel() > small.numel()
            with pytest.raises(ops.KvzError, match=r"code -2"):
                ops.varlen_attn(d.q, d.k, d.v, d.ks, kl, 1, 300, workspace=small)
            with pytest.raises(ops.KvzError, match=r"code -2"):
                ops.varlen_attn_append(d.q, d.k.clone(), d.v.clone(), d.k[:3].view(1, 3, 1, 128), d.v[:3].view(1, 3, 1, 128), d.ks,
                                       kl, 0, 301, workspace=small)
            got = ops.varlen_attn(d.q, d.k, d.v, d.ks, kl, 1, 300, workspace=big, softmax_scale=p.scale).cpu()
            assert ap.bits_equal(got, ap.expected(p, "div"))[0]
        # the larger workspace serves the smaller knob
        got = ops.varlen_attn(d.q, d.k, d.v, d.ks, kl, 1, 300, workspace=big, softmax_scale=p.scale).cpu()
        assert ap.bits_equal(got, ap.expected(p, "div"))[0]


# ------------------------------------------------------------------------------------------------------------------------------
# fused append, device-side offset
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_decode_append_counts_the_new_row_once(dtype):
    """kvz_varlen_attn_append: the appended row is attended exactly once - also where it is the first key of a new split (head 0 has
    256 keys before the append; with attn_items = 2 the chunk is 256) and where the head was empty - and the cache rows written are
    the state rows, byte for byte, with nothing else touched."""
    ops = _ops()
    before = [256, 0, 100, 17]
    after = [n + 1 for n in before]
    Hkv, G, D = 4, 7, 128
    assert ap.decode_chunk(after, 2) == 256
    fails, total = [], 0
    for p in (ap.uniform_probe(after, 1, G, D, dtype, items=(2,), seed=5), ap.weighted_probe(after, 1, G, D, dtype, spread=8, seed=6)):
        want = ap.expected(p, "div")
        d = _Dev(p)
        new_rows = torch.tensor([s + n for s, n in zip(p.starts, before)], device=DEV)
        # the state tensors as a model hands them over: [1, Hkv, 1, D] with a head stride larger than D
        ks_state = torch.zeros(1, Hkv, 3, D, dtype=dtype, device=DEV)[:, :, 1:2]
        vs_state = torch.zeros(1, Hkv, 5, D, dtype=dtype, device=DEV)[:, :, 2:3]
        ks_state[0, :, 0] = d.k[new_rows]
        vs_state[0, :, 0] = d.v[new_rows]
        kl = torch.tensor(before, dtype=torch.int32, device=DEV)
        for items in (2, 1, 0, 1024):
            with knobs(attn_items=items):
                for meta in (True, False):
                    kc, vc = d.k.clone(), d.v.clone()
                    kc[new_rows] = ap.SLACK_VALUE
                    vc[new_rows] = ap.SLACK_VALUE
                    mh = ops._meta_host(p.starts, before, Hkv) if meta else None
                    got = ops.varlen_attn_append(d.q, kc, vc, ks_state, vs_state, d.ks, kl, 0, max(after), softmax_scale=p.scale,
                                                 workspace=ops.attn_workspace(Hkv, G, 1, D, DEV), meta_host=mh).cpu()
                    ok, nd = ap.bits_equal(got, want)
                    cache_ok = torch.equal(kc.view(torch.int16), d.k.view(torch.int16)) and \
                        torch.equal(vc.view(torch.int16), d.v.view(torch.int16))
                    total += 1
                    if not (ok and cache_ok):
                        fails.append((p.kind, items, meta, nd, cache_ok))
    _report(fails, total)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_decode_device_offset_advanced_by_add_i32(dtype):
    """The captured decode step's token counter: offset_dev advanced by kvz_add_i32 on the device.  Every head sees exactly
    k_len + k_len_offset + *offset_dev keys at every step."""
    ops = _ops()
    lib = ops._lib.load()
    base = [0, 15, 128, 300, 1021]
    off, steps = 3, [1, 1, 2, 1]
    full = [n + off + sum(steps) for n in base]
    Hkv, G, D = len(base), 5, 64
    fails, total = [], 0
    for p in (ap.uniform_probe(full, 1, G, D, dtype, seed=7), ap.weighted_probe(full, 1, G, D, dtype, spread=8, seed=8)):
        d = _Dev(p)
        kl = torch.tensor(base, dtype=torch.int32, device=DEV)
        for items in (1, 0, 1024):
            with knobs(attn_items=items):
                dev_off = torch.zeros(1, dtype=torch.int32, device=DEV)
                seen = 0
                for st in [0] + steps:
                    if st:
                        ops.check(lib.kvz_add_i32(dev_off.data_ptr(), st, ops._stream(dev_off)), "kvz_add_i32")
                        seen += st
                    lens = [n + off + seen for n in base]
                    want = ap.expected(p, "div", lens)
                    for meta in (True, False):
                        mh = ops._meta_host(p.starts, base, Hkv) if meta else None
                        got = ops.varlen_attn(d.q, d.k, d.v, d.ks, kl, 1, max(full), softmax_scale=p.scale, k_len_offset=off,
                                              workspace=ops.attn_workspace(Hkv, G, 1, D, DEV), meta_host=mh,
                                              offset_dev=dev_off).cpu()
                        ok, nd = ap.bits_equal(got, want)
                        total += 1
                        if not ok:
                            fails.append((p.kind, items, seen, meta, nd))
                assert int(dev_off.item()) == sum(steps)
    _report(fails, total)


# ------------------------------------------------------------------------------------------------------------------------------
# multi-row kernels (kvz_flash: 16-row, kvz_flash2: 32-row) through kvz_varlen_attn, and the dense forward
# ------------------------------------------------------------------------------------------------------------------------------
MULTI = [  # (lens, q_len, G): heads shorter than q_len leave rows that see no key
    ([0, 5, 130, 2100], 20, 7),
    ([50, 0, 700, 3000], 100, 4),
]


def _multi_configs():
    yield "flash", 64, dict(flash2_min_blocks=1 << 30)
    yield "flash", 128, dict(flash2_min_blocks=1 << 30)
    for split in (0, 1, 2):
        for xcd in (0, 1):
            yield f"flash2/split{split}/xcd{xcd}", 128, dict(flash2_min_blocks=1, flash2_split=split, flash2_xcd=xcd)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_multi_row_kernels_exact(dtype):
    fails, total = [], 0
    for name, D, kn in _multi_configs():
        for lens, q_len, G in MULTI:
            assert q_len * G > 64
            for causal in (True, False):
                for p in (ap.uniform_probe(lens, q_len, G, D, dtype, causal=causal, seed=q_len + D),
                          ap.weighted_probe(lens, q_len, G, D, dtype, causal=causal, spread=6, seed=q_len, headroom=ap.F2_DEFER)):
                    want = ap.expected(p, "rcp")
                    d = _Dev(p)
                    with knobs(flash_min_rows=64, **kn):
                        for meta in (True, False):
                            ok, nd = ap.bits_equal(_attn(d, p.lens, meta=meta).cpu(), want)
                            total += 1
                            if not ok:
                                fails.append((name, q_len, causal, p.kind, meta, nd))
    _report(fails, total)


def _dense_from_probe(p, Hkv, klen, cap):
    """[1, H, q, D] query and [1, Hkv, klen, D] views of a [1, Hkv, cap, D] dense cache built from a probe with Hkv heads of klen keys."""
    HQ, G, D = p.q.shape
    q = p.q.view(Hkv, p.q_len, G, D).permute(0, 2, 1, 3).reshape(1, Hkv * G, p.q_len, D).contiguous()
    kc = torch.full((1, Hkv, cap, D), ap.SLACK_VALUE, dtype=p.dtype)
    vc = torch.full((1, Hkv, cap, D), ap.SLACK_VALUE, dtype=p.dtype)
    for h in range(Hkv):
        kc[0, h, :klen] = p.k[p.starts[h]:p.starts[h] + klen]
        vc[0, h, :klen] = p.v[p.starts[h]:p.starts[h] + klen]
    kc, vc = kc.to(DEV), vc.to(DEV)
    return q.to(DEV), kc[:, :, :klen], vc[:, :, :klen]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_flash_fwd_dense_exact_output_and_lse(dtype):
    """kvz_flash_fwd on the views ops.flash_fwd builds (head stride = the cache capacity): output bits equal, LSE within 4 fp32 ulps of
    the fp64 value of the same exact sums (ulps of the larger of |LSE| and |M| + log2 l, the fp32 sum the kernel forms before it
    scales by ln 2)."""
    ops = _ops()
    fails, total = [], 0
    for (Hkv, G, q_len, klen, D), kn in (((4, 7, 300, 300, 128), {}), ((4, 7, 300, 300, 128), dict(flash2_min_blocks=1)),
                                         ((8, 8, 65, 200, 64), {}), ((2, 7, 1, 77, 128), {})):
        for p in (ap.uniform_probe([klen] * Hkv, q_len, G, D, dtype, seed=klen),
                  ap.weighted_probe([klen] * Hkv, q_len, G, D, dtype, spread=8, seed=klen, headroom=ap.F2_DEFER)):
            want = ap.expected(p, "rcp").view(Hkv, q_len, G, D).permute(1, 0, 2, 3).reshape(1, q_len, Hkv * G, D)
            lse_w, mag = (x.reshape(Hkv, q_len, G).transpose(0, 2, 1).reshape(1, Hkv * G, q_len) for x in ap.expected_lse(p))
            q, kv, vv = _dense_from_probe(p, Hkv, klen, klen + 9)
            with knobs(**kn):
                out, lse = ops.flash_fwd(q, kv, vv, causal=True, softmax_scale=p.scale, return_lse=True)
            ok, nd = ap.bits_equal(out.cpu(), want)
            lse = lse.cpu().double().numpy()
            ulp = np.spacing(np.maximum(np.abs(lse_w), mag).astype(np.float32)).astype(np.float64)
            lse_ok = bool(np.all(np.abs(lse - lse_w) <= 4 * ulp))
            total += 1
            if not (ok and lse_ok):
                fails.append((Hkv, G, q_len, klen, D, kn, p.kind, nd, float(np.max(np.abs(lse - lse_w) / ulp))))
    _report(fails, total)
