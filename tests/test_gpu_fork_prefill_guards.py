"""GPU: kvz_fork_prefill_tail writes nothing outside what its ABI declares (tests/guards.py): every buffer carved from a guarded arena
at exactly its declared size, tails with more capacity than used, `out` apart from o_shared and aliased with it."""
import pytest
import torch

import guards
import prefill_probes as pp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _carve_like(arena, name, t, names=None):
    buf = arena.carve(name, (t.shape, t.dtype), names=names)
    buf.copy_(t.to(DEV))
    return buf


@pytest.mark.parametrize("alias", [False, True], ids=["out-apart", "out-is-o_shared"])
@pytest.mark.parametrize("dtype,G,D", [(torch.float16, 7, 128), (torch.bfloat16, 4, 64)], ids=["f16-G7-D128", "bf16-G4-D64"])
def test_writes_stay_inside_the_declared_rows(dtype, G, D, alias):
    from kvzip_amd import ops
    lengths, tail_len, cap, Hkv = [5, 0, 17], [31, 33, 0], 56, 2
    c = pp.with_shared(pp.uniform_case(lengths, tail_len, G, D, dtype, cap, Hkv=Hkv, seed=1), seed=1)
    B, T = len(lengths), c.cu_q[-1]
    arena = guards.Arena(DEV)
    qm, km, vm = pp.as_model_tensors(c)
    # q, k_new, v_new in the layout the model hands over ([1, T, heads, D] storage, transposed views)
    q = _carve_like(arena, "q", qm.transpose(1, 2).contiguous()).transpose(1, 2)
    kn = _carve_like(arena, "k_new", km.transpose(1, 2).contiguous()).transpose(1, 2)
    vn = _carve_like(arena, "v_new", vm.transpose(1, 2).contiguous()).transpose(1, 2)
    tail_names = ("branch", "head", "row", "d")
    tk = arena.carve("tail_k", ((B, Hkv, cap, D), dtype), names=tail_names)
    tv = arena.carve("tail_v", ((B, Hkv, cap, D), dtype), names=tail_names)
    # only rows [t_b, t_b + n_b) of the branches that take part may be written; the rows in use hold the case's data, the rest of the
    # tails - unused rows, and ALL of the branch without positions beyond its rows in use - stays guard pattern
    writable = torch.zeros(B, Hkv, cap, 1, dtype=torch.bool)
    for b, (t, n) in enumerate(zip(tail_len, lengths)):
        tk[b, :, :t] = c.tail_k[b, :, :t].to(DEV)
        tv[b, :, :t] = c.tail_v[b, :, :t].to(DEV)
        writable[b, :, :t + n] = True     # (rows in use: the caller's data, which must come back unchanged - checked below)
    arena.declare(tk, writable)
    arena.declare(tv, writable)
    osh = _carve_like(arena, "o_shared", c.o_shared, names=("head", "pos", "g", "d"))
    lse = _carve_like(arena, "lse_shared", c.lse_shared, names=("head", "pos", "g"))
    out = osh if alias else arena.carve("out", ((Hkv, T, G, D), dtype), names=("head", "pos", "g", "d"))
    need = int(ops._lib.load().kvz_fork_prefill_workspace_bytes(T, B, Hkv, G, D))
    arena.assert_clean()
    old_rows = [(tk[b, :, :t].clone(), tv[b, :, :t].clone()) for b, t in enumerate(tail_len)]
    results = []
    fills = (0x00, 0xFF) if need else (None,)      # (a workspace, should the size function ever return one, must not matter)
    for fill in fills:
        if fill is not None:
            guards.interior(arena.carve(f"ws{fill}", need), fill)
        for b, t in enumerate(tail_len):             # (a second round starts from the same tails)
            tk[b, :, t:t + lengths[b]] = 0
            tv[b, :, t:t + lengths[b]] = 0
        if alias:
            osh.copy_(c.o_shared.to(DEV))
        with guards.frozen(q, kn, vn, lse, None if alias else osh):
            got = ops.fork_prefill_tail(q, c.cu_q, tk, tv, tail_len, kn, vn, osh, lse, softmax_scale=c.scale, out=out)
        arena.assert_clean()
        results.append(got.cpu())
    want = pp.expected_out(c)
    for r in results:
        assert torch.equal(r.view(torch.int16), want.view(torch.int16))
    etk, etv = pp.expected_tails(c)
    for b, (t, n) in enumerate(zip(tail_len, lengths)):
        assert torch.equal(tk[b, :, :t], old_rows[b][0]) and torch.equal(tv[b, :, :t], old_rows[b][1]), (b, "rows in use were written")
        assert torch.equal(tk[b, :, t:t + n].cpu(), etk[b, :, t:t + n]) and torch.equal(tv[b, :, t:t + n].cpu(), etv[b, :, t:t + n])
