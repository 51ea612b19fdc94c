"""GPU: the tree verify step (kvz_tree_attn_append) - exact probes (bit equality, tests/tree_probes.py) over chains, stars, interleaved
chains and random trees, the cache after the call, bit equality with the chain call on chain parents, and oracle parity on random
data node by node."""
import pytest
import torch

import attn_probes as ap
import kvzip_oracle as orc
import spec_probes as sp
import tree_probes as tp
from conftest import check_attn
from test_gpu_spec_attn import DEV, ITEMS, LENS, LENS_EMPTY, TOL, _new_rows, _ops, boundary_cases, knob
from test_gpu_spec_attn import _run as _run_chain

pytestmark = pytest.mark.gpu
# one row tile (28 rows are two: 7 x 4), the step to three tiles (35 rows) and four (63), a tile group boundary inside a node (G 7: node
# 4 is rows 28 .. 34, tiles 1 and 2), exactly 64 rows, masks that cross bit 31 (t 33) and use bit 63 (t 64), and one node
GEOMS = [(7, 4, 128), (7, 5, 128), (7, 9, 128), (4, 16, 128), (2, 16, 64), (1, 33, 64), (1, 64, 128), (64, 1, 64)]


def _run(c, parents, meta=True, dev_arrays=True):
    """One kvz_tree_attn_append call on the case's tensors -> (out, k, v) as the device holds them afterwards."""
    ops = _ops()
    k, v = c.k.to(DEV), c.v.to(DEV)
    Hkv = len(c.lens)
    base = [n - c.k_len_offset for n in c.lens]
    ks = torch.tensor(c.starts, dtype=torch.int32, device=DEV) if dev_arrays else None
    kl = torch.tensor(base, dtype=torch.int32, device=DEV) if dev_arrays else None
    mh = ops._meta_host(c.starts, base, Hkv) if meta else None
    kn, vn = _new_rows(c)
    out = ops.tree_attn_append(c.q.to(DEV), k, v, ks, kl, c.k_len_offset, c.k_len_offset + c.slack, kn, vn, ops.ancestor_masks(parents),
                               softmax_scale=c.scale, meta_host=mh)
    torch.cuda.synchronize()
    return out.cpu(), k.cpu(), v.cpu()


def _check_exact(name, c, parents, **kw):
    out, k, v = _run(c, parents, **kw)
    want = tp.expected_out(c, parents)
    same, n = ap.bits_equal(out, want)
    print(f"\nTREE {name}: {n} of {want.numel()} outputs differ; worst {int(ap.steps(out, want).max())} steps")
    assert same, (name, n, int(ap.steps(out, want).max()))
    ek, ev = sp.expected_cache(c)
    assert ap.bits_equal(k, ek)[0] and ap.bits_equal(v, ev)[0], (name, "cache: only the t new rows of every head may change")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,t,D", GEOMS)
def test_uniform_probe_exact(G, t, D, dtype):
    """q = 0 and new row j marked on its own V dim: an output shows exactly which new keys its row saw."""
    with knob("attn_items", ITEMS):
        target = sp.spec_items(ITEMS, len(LENS))
        c = sp.uniform_case(LENS, t, G, D, dtype, items=(target,), seed=t)
        for kind in tp.KINDS:
            _check_exact(f"uniform {kind} G{G} t{t} D{D} {dtype}", c, tp.parents_of(kind, t))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,t,D", GEOMS)
def test_weighted_probe_exact(G, t, D, dtype):
    with knob("attn_items", ITEMS):
        c = sp.weighted_case(LENS, t, G, D, dtype, seed=t)
        for kind in tp.KINDS:
            _check_exact(f"weighted {kind} G{G} t{t} D{D} {dtype}", c, tp.parents_of(kind, t))


@pytest.mark.parametrize("kind", ["uniform", "weighted"])
def test_offset_metadata_forms_items_and_empty_head(kind):
    """A non-zero k_len_offset (rows appended before the step), head segments by value and / or as device arrays, the default work-item
    count and fewer items than heads, and a head without a row."""
    make = sp.uniform_case if kind == "uniform" else sp.weighted_case
    for meta, dev_arrays in ((True, True), (False, True), (True, False)):
        c = make(LENS, 4, 7, 128, torch.float16, k_len_offset=3, seed=7)
        _check_exact(f"{kind} offset 3 meta {meta} device arrays {dev_arrays}", c, tp.parents_of("random", 4), meta=meta,
                     dev_arrays=dev_arrays)
    with knob("attn_items", 3):     # fewer items than heads: every head is one range
        _check_exact(f"{kind} items 3", make(LENS, 5, 7, 128, torch.bfloat16, seed=8), tp.parents_of("random", 5))
    for items in (ITEMS, 3, 0):
        with knob("attn_items", items):
            for G, t, D in ((7, 4, 128), (7, 9, 128), (2, 16, 64), (1, 64, 128)):
                for tree in ("star", "random"):
                    _check_exact(f"{kind} empty head items {items} G{G} t{t} {tree}", make(LENS_EMPTY, t, G, D, torch.float16, seed=9),
                                 tp.parents_of(tree, t))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,D", [(7, 128), (4, 64)])
def test_combine_at_the_boundary_between_its_two_paths(G, D, dtype):
    """The cases of the chain form's test of this name (the last partial count of the combine's fast path and the first of its general
    path), on a star and on an interleaved tree of t = 3 nodes."""
    with knob("attn_items", 1024):
        for name, c in boundary_cases(G, D, dtype):
            for kind in ("star", "interleaved"):
                _check_exact(f"{name} {kind}", c, tp.parents_of(kind, 3))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,t,D", GEOMS)
def test_chain_parents_equal_the_chain_call_bit_for_bit(G, t, D, dtype):
    """Random data, every knob value: with parents i - 1 the call is kvz_spec_attn_append - outputs and caches torch.equal."""
    for items in (ITEMS, 3, 0):
        with knob("attn_items", items):
            for lens, off in ((LENS, 2), (LENS_EMPTY, 0)):      # (a head without a row had none appended before the step either)
                c = sp.random_case(lens, t, G, D, dtype, k_len_offset=off, seed=10 + t)
                out, k, v = _run(c, tp.parents_of("chain", t))
                want, k2, v2 = _run_chain(c)
                assert torch.equal(out, want), (items, lens, int(ap.steps(out, want).max()))
                assert ap.bits_equal(k, k2)[0] and ap.bits_equal(v, v2)[0]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,t,D", [(7, 4, 128), (7, 9, 128), (4, 16, 128), (2, 16, 64), (1, 33, 64)])
@pytest.mark.parametrize("kind", ["star", "interleaved", "random"])
def test_oracle_parity_random(kind, G, t, D, dtype):
    """Random data: node p against the oracle over the explicit concatenation of the old rows and p's ancestor rows (q_len = 1)."""
    parents = tp.parents_of(kind, t, seed=1)
    c = sp.random_case(LENS, t, G, D, dtype, k_len_offset=2, seed=t)
    out, k, v = _run(c, parents)
    ek, ev = sp.expected_cache(c)
    assert ap.bits_equal(k, ek)[0] and ap.bits_equal(v, ev)[0]
    Hkv = len(c.lens)
    want = torch.empty_like(out)
    for p in range(t):
        kk, vv, starts, lens = tp.concat_for_oracle(c, parents, p)
        want[:, p] = orc.varlen_attn(c.q[:, p].contiguous(), kk, vv, starts, lens, 1, causal=True, scale=c.scale)
    check_attn(f"tree/random/{kind}/G{G}t{t}D{D}/{dtype}", out.reshape(Hkv * t, G, D), want.reshape(Hkv * t, G, D), TOL[dtype], ulp_of=dtype)
