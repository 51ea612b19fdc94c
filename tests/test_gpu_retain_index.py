"""GPU: the index of kept positions (kvz_retain_index / kvz_retain_index_heads, include/kvzip_hip_retain.h) against torch.nonzero of
the full mask ones(sink) ++ valid per (layer, head), and a guard-band case: only the index is written."""
import pytest
import torch

from guards import Arena, frozen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, HKV = 2, 3
SHAPES = [(n, sink) for n in (1, 1019, 1024, 2500) for sink in (0, 5, 1030)]


def _ops():
    from kvzip_amd import ops
    return ops


def _mask(kind, N, seed=0):
    """-> valid [L, 1, Hkv, N] bool on the device (head-level: one value per (layer, head) expanded over N, stride 0)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "all":
        m = torch.ones(L, 1, HKV, N, dtype=torch.bool)
    elif kind == "none":
        m = torch.zeros(L, 1, HKV, N, dtype=torch.bool)
    elif kind == "random":
        m = torch.rand(L, 1, HKV, N, generator=g) < 0.3
    elif kind == "heads":
        m = torch.tensor([[True, False, True], [False, False, True]]).view(L, 1, HKV, 1)
        return m.to(DEV).expand(L, 1, HKV, max(N, 2))[..., :N] if N > 1 else m.to(DEV)
    else:
        raise ValueError(kind)
    return m.to(DEV)


def _want(valid, sink):
    """Per (layer, head): the ascending positions of ones(sink) ++ valid."""
    out = []
    v = valid.cpu()
    for l in range(L):
        for h in range(HKV):
            full = torch.cat([torch.ones(sink, dtype=torch.bool), v[l, 0, h]])
            out.append(torch.nonzero(full).flatten().to(torch.int32))
    return out


@pytest.mark.parametrize("kind", ["all", "none", "random", "heads"])
@pytest.mark.parametrize("N,sink", SHAPES)
def test_index_equals_nonzero(N, sink, kind):
    ops = _ops()
    valid = _mask(kind, N, seed=N + sink)
    plan = ops.compact_plan(valid, sink, sink + N, slack=0)
    assert plan.heads == (kind == "heads" and N > 1)
    ix = ops.retain_index(plan)
    torch.cuda.synchronize()
    want = _want(valid, sink)
    idx = ix.idx.cpu()
    assert ix.ctx_end == sink + N and ix.total == sum(w.numel() for w in want) and idx.numel() == max(ix.total, 1)
    o = 0
    for l in range(L):
        for h in range(HKV):
            w = want[l * HKV + h]
            assert ix.starts[l][h] == o and ix.counts[l][h] == w.numel(), (l, h)
            assert torch.equal(idx[o:o + w.numel()], w), (l, h, N, sink, kind)
            o += w.numel()
        assert list(ix.meta_host[l]) == ix.starts[l] + ix.counts[l]
    # the counts the caller already has spare the copy to the host
    again = ops.retain_index(plan, counts_host=ix.counts)
    torch.cuda.synchronize()
    assert torch.equal(again.idx.cpu()[:ix.total], idx[:ix.total])


@pytest.mark.parametrize("kind", ["random", "heads"])
def test_only_the_index_is_written(kind):
    """kvz_retain_index through the C ABI with the index carved from a guarded arena, exactly as long as the kept rows: guards stay
    clean, mask, tile bases and row starts stay frozen; an index declared one entry too short loses that entry and nothing else."""
    ops = _ops()
    lib = ops._lib.load()
    N, sink = 2500, 5
    valid = _mask(kind, N, seed=3)
    plan = ops.compact_plan(valid, sink, sink + N, slack=0)
    ref = ops.retain_index(plan)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    fn = lib.kvz_retain_index_heads if plan.heads else lib.kvz_retain_index
    for short in (0, 1):
        a = Arena(DEV)
        n = ref.total - short
        idx = a.carve("idx", ((n,), torch.int32))
        with frozen(plan.valid, plan.tile_base, ref.row_start, plan.len_k):
            rc = fn(plan.valid.data_ptr(), L, HKV, N, sink, plan.tile_base.data_ptr(), ref.row_start.data_ptr(), idx.data_ptr(), n, st)
            assert rc == 0, lib.kvz_last_error()
            torch.cuda.synchronize()
        assert torch.equal(idx.cpu(), ref.idx.cpu()[:n])
        a.assert_clean()
