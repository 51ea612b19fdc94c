"""GPU: the verify step of speculative decoding (kvz_spec_attn_append) - exact probes (bit equality, tests/spec_probes.py), the cache
after the call, oracle parity on random data, parity with the existing append + multi-row attention path, and two steps with a rewind
between them."""
import contextlib

import pytest
import torch

import attn_probes as ap
import kvzip_oracle as orc
import spec_probes as sp
from conftest import check_attn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}
# ragged lengths: a head with only its sink rows, a head long enough for several key ranges, edges of the 32-key wave tiles
LENS = [5, 3000, 129, 700]
LENS_EMPTY = [5, 0, 129, 700]       # a dropped head of a head-level cache
ITEMS = 16     # attn_items knob of the exact cases: chunks of 256 keys, so the 3000-key head is cut into 12 ranges
# a partial single tile, exactly two tiles (G 4), the step to three tiles (7 x 5 = 35), 63 and 64 rows, rows of one position split
# across two tiles (G 7: position 2 is rows 14 .. 20)
GEOMS = [(7, 1, 128), (7, 2, 128), (7, 4, 128), (7, 5, 128), (7, 9, 128), (4, 8, 128), (4, 16, 128), (2, 3, 64), (2, 16, 64), (64, 1, 64)]


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


def _new_rows(c):
    """The new rows as the model produces them: K contiguous, V a strided view of the projection output ([t, Hkv*D] rows)."""
    kn = c.k_new.to(DEV)
    vn = c.v_new.to(DEV).transpose(0, 1).contiguous().transpose(0, 1)
    assert not vn.is_contiguous() or c.t == 1 or len(c.lens) == 1
    return kn, vn


def _run(c, meta=True, dev_arrays=True, k=None, v=None, offset=None, q=None, kn=None, vn=None):
    """One kvz_spec_attn_append call on the case's tensors -> (out, k, v) as the device holds them afterwards."""
    ops = _ops()
    offset = c.k_len_offset if offset is None else offset
    k = c.k.to(DEV) if k is None else k
    v = c.v.to(DEV) if v is None else v
    Hkv = len(c.lens)
    base = [n - c.k_len_offset for n in c.lens]
    ks = torch.tensor(c.starts, dtype=torch.int32, device=DEV) if dev_arrays else None
    kl = torch.tensor(base, dtype=torch.int32, device=DEV) if dev_arrays else None
    mh = ops._meta_host(c.starts, base, Hkv) if meta else None
    if kn is None:
        kn, vn = _new_rows(c)
    q = c.q.to(DEV) if q is None else q
    out = ops.spec_attn_append(q, k, v, ks, kl, offset, c.k_len_offset + c.slack, kn, vn, softmax_scale=c.scale, meta_host=mh)
    torch.cuda.synchronize()
    return out.cpu(), k.cpu(), v.cpu()


def _check_exact(name, c, **kw):
    out, k, v = _run(c, **kw)
    want = sp.expected_out(c)
    same, n = ap.bits_equal(out, want)
    print(f"\nSPEC {name}: {n} of {want.numel()} outputs differ; worst {int(ap.steps(out, want).max())} steps")
    assert same, (name, n, int(ap.steps(out, want).max()))
    ek, ev = sp.expected_cache(c)
    assert ap.bits_equal(k, ek)[0] and ap.bits_equal(v, ev)[0], (name, "cache: only the t new rows of every head may change")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,t,D", GEOMS)
def test_uniform_probe_exact(G, t, D, dtype):
    with knob("attn_items", ITEMS):
        target = sp.spec_items(ITEMS, len(LENS))
        _check_exact(f"uniform G{G} t{t} D{D} {dtype}", sp.uniform_case(LENS, t, G, D, dtype, items=(target,), seed=t))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,t,D", GEOMS)
def test_weighted_probe_exact(G, t, D, dtype):
    with knob("attn_items", ITEMS):
        _check_exact(f"weighted G{G} t{t} D{D} {dtype}", sp.weighted_case(LENS, t, G, D, dtype, seed=t))


@pytest.mark.parametrize("kind", ["uniform", "weighted"])
def test_offset_metadata_forms_items_and_empty_head(kind):
    """A non-zero k_len_offset (rows appended before the step), head segments by value and / or as device arrays, the default work-item
    count and fewer items than heads, and a head without a row."""
    make = sp.uniform_case if kind == "uniform" else sp.weighted_case
    for meta, dev_arrays in ((True, True), (False, True), (True, False)):
        c = make(LENS, 4, 7, 128, torch.float16, k_len_offset=3, seed=7)
        _check_exact(f"{kind} offset 3 meta {meta} device arrays {dev_arrays}", c, meta=meta, dev_arrays=dev_arrays)
    with knob("attn_items", 3):     # fewer items than heads: every head is one range
        _check_exact(f"{kind} items 3", make(LENS, 5, 7, 128, torch.bfloat16, seed=8))
    for items in (ITEMS, 0):
        with knob("attn_items", items):
            for G, t, D in ((7, 4, 128), (7, 9, 128), (2, 3, 64)):
                _check_exact(f"{kind} empty head items {items} G{G} t{t}", make(LENS_EMPTY, t, G, D, torch.float16, seed=9))


BOUNDARY_KEYS = {128: (8064, 8192), 64: (16256, 16384)}     # old rows of the long head: 8 * 1024 / D - 1 key ranges of 128 keys, and one more


def boundary_cases(G, D, dtype, t=3):
    """(name, case) at the boundary between the two paths of the combine, under attn_items = 1024 (also for the tree form): a head
    whose old rows are 8 * 1024 / D - 1 key ranges of 128 keys, and one range more, beside heads of 1 and 0 rows; with the triangle
    that is the last partial count the combine holds in registers and the first of its general path.  Split edges marked."""
    target = sp.spec_items(1024, 3)
    for n, partials in zip(BOUNDARY_KEYS[D], (8 * 1024 // D, 8 * 1024 // D + 1)):
        lens = [n, 1, 0]
        assert ap.decode_chunk(lens, target) == 128 and n % 128 == 0 and n // 128 + 1 == partials
        yield f"uniform boundary {n} rows D{D} {dtype}", sp.uniform_case(lens, t, G, D, dtype, items=(target,), seed=n)
        yield f"weighted boundary {n} rows D{D} {dtype}", sp.weighted_case(lens, t, G, D, dtype, seed=n)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,D", [(7, 128), (4, 64)])
def test_combine_at_the_boundary_between_its_two_paths(G, D, dtype):
    with knob("attn_items", 1024):
        for name, c in boundary_cases(G, D, dtype):
            _check_exact(name, c)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,t,D", [(7, 2, 128), (7, 5, 128), (7, 9, 128), (4, 16, 128), (2, 3, 64)])
def test_oracle_parity_random(G, t, D, dtype):
    c = sp.random_case([5, 3000, 129, 20000], t, G, D, dtype, k_len_offset=2, seed=t)
    out, k, v = _run(c)
    ek, ev = sp.expected_cache(c)
    assert ap.bits_equal(k, ek)[0] and ap.bits_equal(v, ev)[0]
    Hkv = len(c.lens)
    kk, vv, starts, lens = sp.concat_for_oracle(c)
    want = orc.varlen_attn(c.q.reshape(Hkv * t, G, D), kk, vv, starts, lens, t, causal=True)
    check_attn(f"spec/random/G{G}t{t}D{D}/{dtype}", out.reshape(Hkv * t, G, D), want, TOL[dtype], ulp_of=dtype)


def _existing_path(c, k, v, q, kn, vn, offset):
    """kvz_append_inplace + kvz_varlen_attn(q_len = t, causal) on the given cache -> out [Hkv, t, G, D]."""
    ops = _ops()
    Hkv, t, G, D = q.shape
    base = [n - c.k_len_offset for n in c.lens]
    ks = torch.tensor(c.starts, dtype=torch.int32, device=DEV)
    kl = torch.tensor(base, dtype=torch.int32, device=DEV)
    ops.append_inplace(k, v, kn.unsqueeze(0), vn.unsqueeze(0), ks, kl, offset)
    out = ops.varlen_attn(q.reshape(Hkv * t, G, D), k, v, ks, kl, t, max(base) + offset + t, causal=True, softmax_scale=c.scale,
                          k_len_offset=offset + t)
    torch.cuda.synchronize()
    return out.view(Hkv, t, G, D).cpu()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,t,D", [(7, 2, 128), (7, 4, 128), (7, 9, 128), (4, 16, 128), (2, 3, 64)])
def test_parity_with_append_then_attend(G, t, D, dtype):
    c = sp.random_case([5, 3000, 129, 700], t, G, D, dtype, k_len_offset=2, seed=10 + t)
    out, k, v = _run(c)
    k2, v2 = c.k.to(DEV), c.v.to(DEV)
    kn, vn = _new_rows(c)
    want = _existing_path(c, k2, v2, c.q.to(DEV), kn, vn, c.k_len_offset)
    assert ap.bits_equal(k, k2)[0] and ap.bits_equal(v, v2)[0], "both paths append the same rows"
    check_attn(f"spec/vs-append+attend/G{G}t{t}D{D}/{dtype}", out, want, TOL[dtype], ulp_of=dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,D", [(7, 128), (2, 64)])
def test_one_position_against_the_decode_step(G, D, dtype):
    ops = _ops()
    c = sp.random_case([5, 3000, 129, 700], 1, G, D, dtype, k_len_offset=2, seed=3)
    out, k, v = _run(c)
    Hkv = len(c.lens)
    base = [n - c.k_len_offset for n in c.lens]
    ks = torch.tensor(c.starts, dtype=torch.int32, device=DEV)
    kl = torch.tensor(base, dtype=torch.int32, device=DEV)
    k2, v2 = c.k.to(DEV), c.v.to(DEV)
    kn, vn = _new_rows(c)
    want = ops.varlen_attn_append(c.q.to(DEV).view(Hkv, G, D), k2, v2, kn.view(1, Hkv, 1, D), vn.view(1, Hkv, 1, D), ks, kl,
                                  c.k_len_offset, max(c.lens) + 1, softmax_scale=c.scale)
    torch.cuda.synchronize()
    assert ap.bits_equal(k, k2)[0] and ap.bits_equal(v, v2)[0]
    check_attn(f"spec/t1-vs-varlen_attn_append/G{G}D{D}/{dtype}", out.view(Hkv, G, D), want, TOL[dtype], ulp_of=dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_two_steps_with_a_rewind_between(dtype):
    """Step one: t = 4, of which 2 are kept (the host takes two rows back: the next step starts at offset + 2); step two: t = 3."""
    G, D = 7, 128
    c = sp.random_case([5, 3000, 129, 700], 4, G, D, dtype, k_len_offset=1, seed=21)
    Hkv = len(c.lens)
    gen = torch.Generator().manual_seed(22)
    q2 = torch.randn(Hkv, 3, G, D, generator=gen).to(dtype).to(DEV)
    kn2 = torch.randn(Hkv, 3, D, generator=gen).to(dtype).to(DEV)
    vn2 = torch.randn(3, Hkv, D, generator=gen).to(dtype).to(DEV).transpose(0, 1)
    q1 = c.q.to(DEV)
    kn1, vn1 = _new_rows(c)
    off = c.k_len_offset
    # (a) the verify path: 4 rows, 2 taken back, 3 rows
    ka, va = c.k.to(DEV), c.v.to(DEV)
    out1, _, _ = _run(c, k=ka, v=va)
    out2, ka_c, va_c = _run(c, k=ka, v=va, offset=off + 2, q=q2, kn=kn2, vn=vn2)
    # (b) a cache that never saw the rejected rows
    kb, vb = c.k.to(DEV), c.v.to(DEV)
    _run(c, k=kb, v=vb, q=q1[:, :2].contiguous(), kn=kn1[:, :2], vn=vn1[:, :2])
    out2b, kb_c, vb_c = _run(c, k=kb, v=vb, offset=off + 2, q=q2, kn=kn2, vn=vn2)
    assert ap.bits_equal(out2, out2b)[0], "step two on the rewound cache differs from step two on a cache without the rejected rows"
    # (c) the same accepted runs through the existing path
    kc, vc = c.k.to(DEV), c.v.to(DEV)
    want1 = _existing_path(c, kc, vc, q1[:, :2].contiguous(), kn1[:, :2], vn1[:, :2], off)
    want2 = _existing_path(c, kc, vc, q2, kn2, vn2, off + 2)
    check_attn(f"spec/rewind/step1/{dtype}", out1[:, :2], want1, TOL[dtype], ulp_of=dtype)
    check_attn(f"spec/rewind/step2/{dtype}", out2, want2, TOL[dtype], ulp_of=dtype)
    kc_c, vc_c = kc.cpu(), vc.cpu()
    for h in range(Hkv):
        a, n = c.starts[h], c.lens[h] + 5
        for x, y in ((ka_c, kc_c), (va_c, vc_c), (kb_c, kc_c), (vb_c, vc_c)):
            assert ap.bits_equal(x[a:a + n], y[a:a + n])[0], f"head {h}: the rows of the segment differ between the paths"
