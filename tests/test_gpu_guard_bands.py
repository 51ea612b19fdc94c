"""Guard bands: every writing entry point of include/kvzip_hip.h, called through the C ABI on buffers carved from a guarded arena
(tests/guards.py).  The value tests take outputs and workspaces from torch.empty, where a write one row, one head stride or one
workspace sub-buffer too far lands in a neighbouring tensor unseen; here every output, workspace and metadata array is EXACTLY as
large as the ABI says, starts 256-byte aligned, and is surrounded by at least 64 KiB / one outermost stride of a byte pattern.

Each guarded call asserts: (1) KVZ_OK; (2) the result is bit-identical to the same call made the ordinary way (ops.* on torch.empty
buffers) and, where one exists, to the exact expectation (score_probes, attn_probes, fork_probes, index_select for byte movers);
(3) the guards, stride gaps and undeclared rows still hold the pattern and the read-only inputs are unchanged.  No tolerance anywhere.
"No initialisation needed" workspaces are run with their inside pre-filled with 0x00 and with 0xFF.  Every knob is restored in `finally`.

COVERAGE lists, per entry point, the buffers guarded here; tests/test_abi.py compares it with the header."""
import contextlib
import ctypes as C

import pytest
import torch

import attn_probes as ap
import fork_probes as fp
import score_probes as sp
import test_gpu_attn_exact as tae
import test_gpu_fork_attn as tfa
import test_gpu_score_exact as tse
from guards import Arena, frozen, interior

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])

# entry point -> (buffers carved from the arena, the size function that sizes its workspace or None)
COVERAGE = {
    "kvz_score_chunk": (("out [Hkv, m] in a wider head stride", "ws"), "kvz_score_workspace_bytes"),
    "kvz_score_chunk_async": (("out", "ws"), "kvz_score_workspace_bytes"),
    "kvz_score_chunk_log": (("log_out [Hkv, m] in a wider head stride", "ws"), "kvz_score_workspace_bytes"),
    "kvz_score_chunk_async_log": (("log_out", "ws of one set and of exactly three sets"), "kvz_score_workspace_bytes"),
    "kvz_update_score_async_log": (("k_cache / v_cache rows fill .. fill+t of a larger capacity", "log_out", "ws"), "kvz_score_workspace_bytes"),
    "kvz_score_tail_flush": (("log_out and ws of the pending calls",), "kvz_score_workspace_bytes"),
    "kvz_score_tail_flush_async": (("log_out and ws of the pending calls",), "kvz_score_workspace_bytes"),
    "kvz_score_from_stats_log": (("log_out",), None),
    "kvz_score_from_stats_async_log": (("log_out",), None),
    "kvz_score_log_fill": (("log, odd n",), None),
    "kvz_score_finalize_log": (("out, odd n",), None),
    "kvz_score_finalize_log_hist": (("out, odd n", "select_ws"), "kvz_select_workspace_bytes"),
    "kvz_select_threshold": (("valid_out of n bytes", "row_counts", "thres_dev", "kept_dev", "ws"), "kvz_select_workspace_bytes"),
    "kvz_select_threshold_prehist": (("valid_out of n bytes", "row_counts", "thres_dev", "kept_dev", "ws"), "kvz_select_workspace_bytes"),
    "kvz_select_topk_rows": (("valid_out", "row_counts"), None),
    "kvz_select_heads": (("valid_heads", "row_counts", "thres_dev", "kept_dev"), None),
    "kvz_rowmax16": (("out",), None),
    "kvz_compact_plan": (("len_k", "cu_len_k", "seg_start", "max_len_k", "tile_base"), "kvz_compact_plan_bytes"),
    "kvz_compact_plan_heads": (("len_k", "cu_len_k", "seg_start", "max_len_k", "tile_base"), "kvz_compact_plan_bytes"),
    "kvz_compact_layer": (("k_out / v_out of sum(len_k) + Hkv*slack rows, slack rows as gaps",), None),
    "kvz_compact_layers": (("k_out / v_out of every layer, slack rows as gaps",), None),
    "kvz_compact_layers_heads": (("k_out / v_out of every layer, slack rows as gaps",), None),
    "kvz_update_flatten_view": (("out",), None),
    "kvz_append_inplace": (("k_cache / v_cache: the t new rows of each head",), None),
    "kvz_dense_append": (("k_cache / v_cache: rows fill .. fill+t of each head",), None),
    "kvz_varlen_attn": (("out", "ws"), "kvz_varlen_attn_workspace_bytes"),
    "kvz_varlen_attn_append": (("out", "ws", "k_cache / v_cache: one row per head"), "kvz_varlen_attn_workspace_bytes"),
    "kvz_add_i32": (("the 4-byte counter",), None),
    "kvz_flash_fwd": (("out in both layouts and inside a wider strided tensor", "lse_out", "ws (and ws = NULL)"), "kvz_flash_workspace_bytes"),
    "kvz_flash_fwd_window": (("out", "win_stats in a wider head stride"), None),
    "kvz_fork_attn_append": (("out", "ws", "tail_k / tail_v: row tail_len[b] of active branches"), "kvz_fork_attn_workspace_bytes"),
    "kvz_attn_merge_lse": (("out, also aliasing o1",), None),
}


def _ops():
    from kvzip_amd import ops
    return ops


def _lib():
    return _ops()._lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, who):
    assert rc == 0, f"{who}: code {rc}: {_lib().kvz_last_error()}"


def _same(a, b):
    """bit equality of two tensors of the same dtype size and element count (any strides)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.numel() == b.numel() and torch.equal(a.view(-1).view(torch.uint8), b.view(-1).view(torch.uint8))


knobs = tae.knobs


def _wide(m):
    """a head stride wider than m whose rows stay 16-byte aligned"""
    return (m + 7) // 8 * 8 + 24


def test_arena_on_the_device_sees_a_stray_row():
    """The self-test's fault model once on device memory: a torch copy one row past a [Hkv, rows, D] buffer with a wider head stride."""
    a = Arena(DEV)
    t = a.carve("out", ((3, 40, 64), F16), strides=(64 * 64, 64, 1), names=("head", "row", "elem"))
    t.copy_(torch.randn(3, 40, 64).half())
    a.assert_clean()
    slab, start = a.raw(t)
    slab[start + (1 * 64 * 64 + 40 * 64) * 2:][:128] = 0
    (v,) = a.check()
    assert v.where == "gap" and v.at.startswith("head 1 of 3, row 40 of 40") and v.count >= 120, str(v)
    slab[start + 3 * 64 * 64 * 2:][:128] = 0
    assert [x.where for x in a.check()] == ["after", "gap"]


# ====================================================================================================================================
# scoring
# ====================================================================================================================================
class _ScoreBufs:
    """Guarded buffers of one probe: ws of `sets` x kvz_score_workspace_bytes, out and log_out with a head stride wider than m."""

    def __init__(self, d, sets=1):
        self.d, self.a = d, Arena(DEV)
        p = d.p
        self.need = d.ws_bytes()
        self.ws = self.a.carve("score_ws", sets * self.need, guard=self.need)
        self.hs = _wide(p.m)
        self.out = self.a.carve("out", ((d.Hkv, p.m), p.dtype), strides=(self.hs, 1), names=("head", "score"))
        self.log = self.a.carve("log_out", ((d.Hkv, p.m), torch.int32), strides=(self.hs, 1), names=("head", "score"))

    def reset(self, st):
        self.out.fill_(float("nan"))
        for h in range(self.d.Hkv):      # (the rows only: the gaps between them keep the pattern)
            _ok(_lib().kvz_score_log_fill(self.log[h].data_ptr(), self.d.p.m, st), "kvz_score_log_fill")

    def finalize(self, st):
        for h in range(self.d.Hkv):
            _ok(_lib().kvz_score_finalize_log(self.log[h].data_ptr(), self.d.p.m, self.out[h].data_ptr(), self.d.dt, st), "kvz_score_finalize_log")
        torch.cuda.synchronize()
        return self.out.cpu().contiguous()


def _chunk(d, b, st):
    p = d.p
    return _lib().kvz_score_chunk(d.q.data_ptr(), d.q.stride(1), d.k.data_ptr(), d.k.stride(1), p.klen, p.sink, p.start, p.end, d.q_len, d.Hkv,
                                  d.G, d.D, d.dt, b.out.data_ptr(), b.hs, b.ws.data_ptr(), b.ws.numel(), st)


def _chunk_log(d, b, st):
    p = d.p
    return _lib().kvz_score_chunk_log(d.q.data_ptr(), d.q.stride(1), d.k.data_ptr(), d.k.stride(1), p.klen, p.sink, p.start, p.end, d.q_len,
                                      d.Hkv, d.G, d.D, d.dt, b.log.data_ptr(), b.hs, b.ws.data_ptr(), b.ws.numel(), st)


def _expect(d, got, ordinary, what):
    tse._check(d.p, got, what)
    assert _same(got, ordinary), f"{what}: differs from the ordinary call"


def _sync_entry_points(d, b, knob_list, what):
    st = _st()
    for knob in knob_list:
        with tse._knob(knob), frozen(d.q, d.k_store):
            b.reset(st)
            _ok(_chunk_log(d, b, st), "kvz_score_chunk_log")
            got = b.finalize(st)
        b.a.assert_clean()              # (before the ordinary call: a finding is reported by the layer that names its place)
        _expect(d, got, tse._run_log(d, knob)[0], f"{what} chunk_log knob {knob}")
        with tse._knob(knob), frozen(d.q, d.k_store):
            b.reset(st)
            _ok(_chunk(d, b, st), "kvz_score_chunk")
            torch.cuda.synchronize()
        b.a.assert_clean()
        _expect(d, b.out.cpu().contiguous(), tse._run_chunk(d, knob), f"{what} score_chunk knob {knob}")


@DTYPES
@pytest.mark.parametrize("name", list(tse.GEOMS))
def test_scoring_synchronous_entry_points(name, dtype):
    """kvz_score_chunk and kvz_score_chunk_log + kvz_score_finalize_log under score_prune 0 / 1 / 3 / 4 / 6 on a workspace of exactly
    kvz_score_workspace_bytes, out / log_out in a head stride wider than m."""
    d = tse._Dev(tse._probe(name, dtype, "hot"))
    _sync_entry_points(d, _ScoreBufs(d), (0, 1, 3, 4, 6), f"{name}/{dtype}")


@pytest.mark.parametrize("name,dtype", [("m3_q7", F16), ("d64", BF16), ("headline_later", F16), ("headline_later", BF16)])
def test_scoring_workspace_needs_no_initialisation(name, dtype):
    """The same calls on a workspace whose inside holds 0x00 and then 0xFF bytes: the same bits."""
    d = tse._Dev(tse._probe(name, dtype, "cold"))
    b = _ScoreBufs(d)
    for fill in (0x00, 0xFF):
        interior(b.ws, fill)
        _sync_entry_points(d, b, (0, 1, 3, 4), f"{name}/{dtype} ws filled with {fill:#04x}")
        interior(b.ws, fill)
        _sync_entry_points(d, b, (4, 0), f"{name}/{dtype} ws filled with {fill:#04x}, second order")


def _async_log(d, b, a, slot, st_side):
    p = d.p
    return _lib().kvz_score_chunk_async_log(a.h, slot, a.cur, st_side, d.q.data_ptr(), d.q.stride(1), d.k.data_ptr(), d.k.stride(1), p.klen,
                                            p.sink, p.start, p.end, d.q_len, d.Hkv, d.G, d.D, d.dt, b.log.data_ptr(), b.hs, b.ws.data_ptr(),
                                            b.ws.numel())


@DTYPES
@pytest.mark.parametrize("name", tse.ASYNC_GEOMS)
def test_scoring_asynchronous_entry_points(name, dtype):
    """kvz_score_chunk_async_log (one set: knob 3; exactly three sets: knobs 3 and 6, flushed), kvz_score_chunk_async and
    kvz_update_score_async_log into a dense cache with capacity beyond fill + t."""
    lib = _lib()
    d = tse._Dev(tse._probe(name, dtype, "hot"))
    p = d.p
    for sets, knob_list in ((1, (3,)), (3, (3, 6))):
        b = _ScoreBufs(d, sets)
        a = tse._Async()
        try:
            for knob in knob_list:
                with tse._knob(knob), frozen(d.q, d.k_store):
                    b.reset(a.cur)
                    _ok(_async_log(d, b, a, 0, a.side.cuda_stream), "kvz_score_chunk_async_log")
                    assert lib.kvz_score_tail_flush_async(a.h, 0, b.ws.data_ptr(), a.side.cuda_stream) >= 0
                    _ok(lib.kvz_async_wait(a.h, -1, a.cur), "kvz_async_wait")
                    got = b.finalize(a.cur)
                _expect(d, got, tse._run_async(d, knob), f"{name}/{dtype} async_log knob {knob}, {sets} set(s)")
                b.a.assert_clean()
            with tse._knob(1), frozen(d.q, d.k_store):
                b.reset(a.cur)
                _ok(lib.kvz_score_chunk_async(a.h, 2, a.cur, a.side.cuda_stream, d.q.data_ptr(), d.q.stride(1), d.k.data_ptr(), d.k.stride(1),
                                              p.klen, p.sink, p.start, p.end, d.q_len, d.Hkv, d.G, d.D, d.dt, b.out.data_ptr(), b.hs,
                                              b.ws.data_ptr(), b.ws.numel()), "kvz_score_chunk_async")
                _ok(lib.kvz_async_wait(a.h, 2, a.cur), "kvz_async_wait")
                torch.cuda.synchronize()
            _expect(d, b.out.cpu().contiguous(), tse._run_chunk(d, 1), f"{name}/{dtype} chunk_async")
            b.a.assert_clean()
        finally:
            lib.kvz_score_tail_flush(b.ws.data_ptr())
            torch.cuda.synchronize()
            a.close()
    # the update call: the repeat chunk's rows land in rows fill .. fill + t of a cache with spare rows behind every head
    fill, t, cap = p.klen - d.q_len, d.q_len, p.klen + 5
    for knob in (3, 6):
        b = _ScoreBufs(d, 3)
        rows = torch.zeros(1, cap, 1, dtype=torch.bool)
        rows[0, :p.klen] = True
        kc = b.a.carve("k_cache", ((d.Hkv, cap, d.D), p.dtype), names=("head", "row", "elem"))
        vc = b.a.carve("v_cache", ((d.Hkv, cap, d.D), p.dtype), names=("head", "row", "elem"))
        b.a.declare(kc, rows)
        b.a.declare(vc, rows)
        kc[:, :fill] = d.k_store[0, :, :fill]
        kc[:, fill:p.klen] = 0
        vc[:, :p.klen] = 0
        ks = d.k_store[:, :, fill:p.klen].clone()
        vs = torch.ones_like(ks)
        a = tse._Async()
        try:
            with tse._knob(knob), frozen(d.q, ks, vs):
                b.reset(a.cur)
                _ok(lib.kvz_update_score_async_log(a.h, 1, a.cur, a.side.cuda_stream, kc.data_ptr(), vc.data_ptr(), kc.stride(0), fill,
                                                   ks.data_ptr(), vs.data_ptr(), ks.stride(1), ks.stride(2), vs.stride(1), vs.stride(2), t,
                                                   d.q.data_ptr(), d.q.stride(1), p.sink, p.start, p.end, d.q_len, d.Hkv, d.G, d.D, d.dt,
                                                   b.log.data_ptr(), b.hs, b.ws.data_ptr(), b.ws.numel()), "kvz_update_score_async_log")
                assert lib.kvz_score_tail_flush_async(a.h, 1, b.ws.data_ptr(), a.side.cuda_stream) >= 0
                _ok(lib.kvz_async_wait(a.h, -1, a.cur), "kvz_async_wait")
                got = b.finalize(a.cur)
        finally:
            lib.kvz_score_tail_flush(b.ws.data_ptr())
            torch.cuda.synchronize()
            a.close()
        _expect(d, got, tse._run_update(d, knob), f"{name}/{dtype} update_score_async_log knob {knob}")
        assert _same(kc[:, :p.klen], d.k_store[0, :, :p.klen]), "K rows: the old ones unchanged, the new ones the state's"
        assert _same(vc[:, :fill], torch.zeros_like(vc[:, :fill])) and _same(vc[:, fill:p.klen], vs[0])
        b.a.assert_clean()


@DTYPES
def test_scoring_pipelined_tail_on_exactly_three_sets(dtype):
    """Knob 6, five consecutive calls of mixed shapes on ONE workspace of exactly 3 x kvz_score_workspace_bytes (of the largest), a
    flush after the second call and at the end.  (The tail's host state is keyed by the workspace address: flushed before release.)"""
    lib = _lib()
    seq = [("headline_later", "cold"), ("hkv1", "hot"), ("headline_later", "hot"), ("hkv1", "cold"), ("headline_first", "cold")]
    devs = [tse._Dev(tse._probe(n, dtype, v)) for n, v in seq]
    need = max(d.ws_bytes() for d in devs)
    arena = Arena(DEV)
    ws = arena.carve("score_ws_x3", 3 * need, guard=need)
    logs = [arena.carve(f"log{c}", ((d.Hkv, d.p.m), torch.int32), strides=(_wide(d.p.m), 1), names=("head", "score")) for c, d in enumerate(devs)]
    outs = [arena.carve(f"out{c}", ((d.Hkv, d.p.m), dtype), strides=(_wide(d.p.m), 1), names=("head", "score")) for c, d in enumerate(devs)]
    side = torch.cuda.Stream(device=DEV)

    def fin(c):
        d = devs[c]
        for h in range(d.Hkv):
            _ok(lib.kvz_score_finalize_log(logs[c][h].data_ptr(), d.p.m, outs[c][h].data_ptr(), d.dt, side.cuda_stream), "finalize")

    with tse._knob(6), frozen(*[d.q for d in devs], *[d.k_store for d in devs]):
        a = tse._Async()
        try:
            for c, d in enumerate(devs):
                p = d.p
                outs[c].fill_(float("nan"))
                for h in range(d.Hkv):
                    _ok(lib.kvz_score_log_fill(logs[c][h].data_ptr(), p.m, a.cur), "kvz_score_log_fill")
                _ok(lib.kvz_score_chunk_async_log(a.h, c % 4, a.cur, side.cuda_stream, d.q.data_ptr(), d.q.stride(1), d.k.data_ptr(),
                                                  d.k.stride(1), p.klen, p.sink, p.start, p.end, d.q_len, d.Hkv, d.G, d.D, d.dt,
                                                  logs[c].data_ptr(), _wide(p.m), ws.data_ptr(), ws.numel()), "kvz_score_chunk_async_log")
                if c == 1:
                    assert lib.kvz_score_tail_flush(ws.data_ptr()) == 1, "calls 0 and 1 left phases pending"
                    side.synchronize()
                    fin(0), fin(1)
                    side.synchronize()
                    arena.assert_clean()
            assert lib.kvz_score_tail_flush(ws.data_ptr()) == 1
            side.synchronize()
            for c in range(2, len(devs)):
                fin(c)
            side.synchronize()
        finally:
            lib.kvz_score_tail_flush(ws.data_ptr())
            torch.cuda.synchronize()
            a.close()
    for c, d in enumerate(devs):
        tse._check(d.p, outs[c].cpu().contiguous(), f"tail call {c} ({seq[c][0]}/{seq[c][1]})")
    arena.assert_clean()


@DTYPES
@pytest.mark.parametrize("n", [1, 7, 4097, 100_003])
def test_log_fill_finalize_and_histogram_with_odd_n(n, dtype):
    """kvz_score_log_fill, kvz_score_finalize_log (entries never scored leave `out` untouched) and kvz_score_finalize_log_hist on
    buffers of exactly n words / n scores / kvz_select_workspace_bytes."""
    lib, ops = _lib(), _ops()
    st = _st()
    dt = ops._dtype_code(dtype)
    g = torch.Generator().manual_seed(n)
    vals = -(torch.rand(n, generator=g) * 9.0)
    bits = vals.view(torch.int32).clone()
    holes = torch.rand(n, generator=g) < 0.25
    a = Arena(DEV)
    log = a.carve("log", ((n,), torch.int32))
    out = a.carve("out", ((n,), dtype))
    out2 = a.carve("out_hist", ((n,), dtype))
    sel = a.carve("select_ws", int(lib.kvz_select_workspace_bytes()))
    _ok(lib.kvz_score_log_fill(log.data_ptr(), n, st), "kvz_score_log_fill")
    torch.cuda.synchronize()
    empty = log.cpu().clone()
    assert len(set(empty.tolist())) == 1
    a.assert_clean()
    log.copy_(torch.where(holes, empty, bits).to(DEV))
    prior = torch.full((n,), 0.5, dtype=dtype, device=DEV)
    out.copy_(prior)
    out2.copy_(prior)
    ref, ref2 = prior.clone(), prior.clone()
    log_plain = log.clone()
    sel_plain = ops.select_workspace(DEV)
    with frozen(log):
        _ok(lib.kvz_score_finalize_log(log.data_ptr(), n, out.data_ptr(), dt, st), "kvz_score_finalize_log")
        _ok(lib.kvz_score_finalize_log_hist(log.data_ptr(), n, out2.data_ptr(), dt, sel.data_ptr(), sel.numel(), st), "kvz_score_finalize_log_hist")
    _ok(lib.kvz_score_finalize_log(log_plain.data_ptr(), n, ref.data_ptr(), dt, st), "kvz_score_finalize_log")
    _ok(lib.kvz_score_finalize_log_hist(log_plain.data_ptr(), n, ref2.data_ptr(), dt, sel_plain.data_ptr(), sel_plain.numel(), st), "hist")
    torch.cuda.synchronize()
    assert _same(out, ref) and _same(out2, ref2) and _same(out, out2)
    assert _same(out.cpu()[holes], prior.cpu()[holes]), "entries never scored leave out untouched"
    assert not bool((out.cpu()[~holes] == 0.5).all()) or not bool((~holes).any())
    a.assert_clean()


# ====================================================================================================================================
# selection
# ====================================================================================================================================
SELECT_SHAPES = [(1, 13), (1, 4099), (224, 1000), (224, 4099), (384, 4096), (384, 13), (1000, 4096), (1000, 4099),
                 (1, 4096), (1, 4097), (1, 4103)]     # the last three: row_counts = NULL, n % 8 in {0, 1, 7}


@pytest.mark.parametrize("rows,row_len", SELECT_SHAPES)
def test_select_threshold_and_prehist(rows, row_len):
    lib, ops = _lib(), _ops()
    st = _st()
    dtype = F16 if (rows + row_len) % 2 else BF16
    dt = ops._dtype_code(dtype)
    n = rows * row_len
    with_rows = (rows, row_len) not in SELECT_SHAPES[-3:]
    g = torch.Generator().manual_seed(n)
    logs = -(torch.rand(n, generator=g) * 9.0)
    logs[::13] = 0.0
    log_bits = logs.view(torch.int32).clone()
    log_bits[logs == 0.0] = 1
    log_d = log_bits.to(DEV)
    a = Arena(DEV)
    score = a.carve("scores", ((n,), dtype))
    valid = a.carve("valid_out", n)
    counts = a.carve("row_counts", ((rows,), torch.int32)) if with_rows else None
    thres = a.carve("thres_dev", ((1,), torch.float32))
    kept = a.carve("kept_dev", ((1,), torch.int64))
    ws = a.carve("select_ws", int(lib.kvz_select_workspace_bytes()))
    _ok(lib.kvz_score_finalize_log_hist(log_d.data_ptr(), n, score.data_ptr(), dt, ws.data_ptr(), ws.numel(), st), "finalize_hist")
    a.assert_clean()
    plain = score.clone().view(rows, 1, 1, row_len)
    ratios = (0.0, 0.3, 0.97, 1.0)
    wants = {r: ops.select_threshold(plain, r, row_len=row_len if with_rows else None) for r in ratios}
    fails = []
    for sb in (1, 2, 3, 7, 0, 1024):
        for eb in (1, 5, 0, 4096):
            with knobs(sel_blocks=sb, emit_blocks=eb):
                for ratio in ratios:
                    wv, wt, wk, wr = wants[ratio]
                    for pre in (False, True):
                        if pre and ratio >= 1:
                            continue
                        fn = lib.kvz_select_threshold
                        if pre:
                            _ok(lib.kvz_score_finalize_log_hist(log_d.data_ptr(), n, score.data_ptr(), dt, ws.data_ptr(), ws.numel(), st), "hist")
                            fn = lib.kvz_select_threshold_prehist
                        valid.fill_(7)
                        with frozen(score):
                            _ok(fn(score.data_ptr(), n, float(ratio), dt, valid.data_ptr(), row_len if with_rows else n,
                                   counts.data_ptr() if with_rows else None, thres.data_ptr(), kept.data_ptr(), ws.data_ptr(), ws.numel(), st),
                                "kvz_select_threshold")
                        good = _same(valid, wv) and _same(thres, wt) and _same(kept, wk) and (not with_rows or _same(counts, wr))
                        v = a.check()
                        if not good or v:
                            fails.append((sb, eb, ratio, pre, good, [str(x) for x in v]))
    assert not fails, fails[:8]
    assert _same(score, plain)


@DTYPES
def test_select_topk_rows_heads_and_rowmax(dtype):
    lib, ops = _lib(), _ops()
    st = _st()
    dt = ops._dtype_code(dtype)
    g = torch.Generator().manual_seed(3)
    for rows, row_len in ((5, 1500), (3, 13), (2, 2049)):
        score = (torch.rand(rows, row_len, generator=g) * 0.01).to(dtype).to(DEV)
        for k in (0, row_len // 3, row_len):
            a = Arena(DEV)
            valid = a.carve("valid_out", rows * row_len)
            counts = a.carve("row_counts", ((rows,), torch.int32))
            with frozen(score):
                _ok(lib.kvz_select_topk_rows(score.data_ptr(), rows, row_len, k, dt, valid.data_ptr(), counts.data_ptr(), st), "kvz_select_topk_rows")
            wv, wc = ops.select_topk_rows(score, k)
            assert _same(valid, wv) and _same(counts, wc) and int(wc.sum()) == rows * k
            a.assert_clean()
    for rows in (1, 112, 384):
        hs = (torch.rand(rows, generator=g) * 0.01).to(dtype).to(DEV)
        for ratio in (0.3, 1.0, 1.5):
            a = Arena(DEV)
            valid = a.carve("valid_heads", rows)
            counts = a.carve("row_counts", ((rows,), torch.int32))
            thres = a.carve("thres_dev", ((1,), torch.float32))
            kept = a.carve("kept_dev", ((1,), torch.int64))
            with frozen(hs):
                _ok(lib.kvz_select_heads(hs.data_ptr(), rows, 1000, float(ratio), dt, valid.data_ptr(), counts.data_ptr(), thres.data_ptr(),
                                         kept.data_ptr(), st), "kvz_select_heads")
            wv, wt, wk, wc = ops.select_heads(hs, 1000, ratio)
            assert _same(valid, wv) and _same(thres, wt) and _same(kept, wk) and _same(counts, wc)
            a.assert_clean()
    for rows, row_len in ((7, 1001), (384, 13), (1, 1), (3, 70_001)):
        score = torch.randn(rows, row_len, generator=g).to(dtype).to(DEV)
        a = Arena(DEV)
        out = a.carve("rowmax", ((rows,), dtype))
        with frozen(score):
            _ok(lib.kvz_rowmax16(score.data_ptr(), rows, row_len, dt, out.data_ptr(), st), "kvz_rowmax16")
        assert _same(out, ops.rowmax(score)) and _same(out, score.float().amax(-1).to(dtype))
        a.assert_clean()


# ====================================================================================================================================
# compaction and append
# ====================================================================================================================================
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def _compact(mode, L, Hkv, sink, N, tail, slack, D, eb, seed):
    """Plan + gather on guarded metadata and outputs; `mode`: "layers" (batched), "layer" (one call per layer), "heads" (head level).
    Moved rows must equal index_select on the full mask, slack rows and everything around must hold the pattern."""
    lib, ops = _lib(), _ops()
    st = _st()
    klen = sink + N + tail
    nt = (klen + 1023) // 1024
    g = torch.Generator().manual_seed(seed)
    it = _INT[eb]
    K = [torch.randint(0, 100, (1, Hkv, klen, D), generator=g).to(it).to(DEV) for _ in range(L)]
    V = [torch.randint(0, 100, (1, Hkv, klen, D), generator=g).to(it).to(DEV) for _ in range(L)]
    if mode == "heads":
        vh = torch.rand(L, Hkv, generator=g) < 0.5
        vh[0, 0], vh[-1, -1] = False, True
        valid = vh.to(DEV)
        full = torch.cat([torch.ones(L, Hkv, sink, dtype=torch.bool), vh[..., None].expand(L, Hkv, N),
                          torch.ones(L, Hkv, tail, dtype=torch.bool)], -1)
        ordinary_valid = vh.view(L, 1, Hkv, 1).to(DEV).expand(L, 1, Hkv, N)
    else:
        vt = torch.rand(L, Hkv, N, generator=g) < 0.3
        vt[0, 0] = False                       # an all-evicted head
        vt[-1, -1] = True
        vt[0, 1, max(N - 5, 0):] = True        # kept up to the last word before sink + N
        valid = vt.to(DEV)
        full = torch.cat([torch.ones(L, Hkv, sink, dtype=torch.bool), vt, torch.ones(L, Hkv, tail, dtype=torch.bool)], -1)
        ordinary_valid = valid.view(L, 1, Hkv, N)
    lens = full.sum(-1)
    a = Arena(DEV)
    i32 = torch.int32
    len_k = a.carve("len_k", ((L, Hkv), i32), names=("layer", "head"))
    cu = a.carve("cu_len_k", ((L, Hkv + 1), i32), names=("layer", "head"))
    seg = a.carve("seg_start", ((L, Hkv), i32), names=("layer", "head"))
    mx = a.carve("max_len_k", ((L,), i32), names=("layer",))
    assert lib.kvz_compact_plan_bytes(L, Hkv, klen) == L * Hkv * nt * 4
    tb = a.carve("tile_base", ((L, Hkv, nt), i32), names=("layer", "head", "tile"))
    plan_fn = lib.kvz_compact_plan_heads if mode == "heads" else lib.kvz_compact_plan
    with frozen(valid):
        _ok(plan_fn(valid.data_ptr(), L, Hkv, N, sink, klen, slack, len_k.data_ptr(), cu.data_ptr(), seg.data_ptr(), mx.data_ptr(),
                    tb.data_ptr(), st), "kvz_compact_plan")
    plan = ops.compact_plan(ordinary_valid, sink, klen, slack=slack)
    assert _same(len_k, plan.len_k) and _same(cu, plan.cu_len_k) and _same(seg, plan.seg_start) and _same(mx, plan.max_len_k)
    assert _same(tb, plan.tile_base)
    assert _same(len_k, lens.int()), "len_k = popcount of the full mask"
    seg_h = [[int(lens[l, :h].sum()) + h * slack for h in range(Hkv)] for l in range(L)]
    assert seg.cpu().tolist() == seg_h
    totals = [int(lens[l].sum()) + Hkv * slack for l in range(L)]
    assert all(t > 0 for t in totals)
    outs = []
    for l in range(L):
        pair = []
        for kv in "kv":
            o = a.carve(f"{kv}_out{l}", ((totals[l], D), it), guard=1024 * D * eb, names=("row", "elem"))
            dec = torch.zeros(totals[l], 1, dtype=torch.bool)
            for h in range(Hkv):
                dec[seg_h[l][h]:seg_h[l][h] + int(lens[l, h])] = True
            a.declare(o, dec)
            pair.append(o)
        outs.append(pair)
    hs = K[0].stride(1)
    with frozen(valid, tb, seg, *K, *V):
        if mode == "layer":
            for l in range(L):
                _ok(lib.kvz_compact_layer(K[l].data_ptr(), V[l].data_ptr(), hs, valid[l].data_ptr(), tb[l].data_ptr(), seg[l].data_ptr(), Hkv, N,
                                          sink, klen, D, eb, outs[l][0].data_ptr(), outs[l][1].data_ptr(), st), "kvz_compact_layer")
        else:
            table = torch.tensor([[t.data_ptr() for t in K], [t.data_ptr() for t in V], [o[0].data_ptr() for o in outs],
                                  [o[1].data_ptr() for o in outs]], dtype=torch.int64).to(DEV)
            fn = lib.kvz_compact_layers_heads if mode == "heads" else lib.kvz_compact_layers
            with frozen(table):
                _ok(fn(table[0].data_ptr(), table[1].data_ptr(), hs, valid.data_ptr(), tb.data_ptr(), seg.data_ptr(), L, Hkv, N, sink, klen, D,
                       eb, table[2].data_ptr(), table[3].data_ptr(), st), "kvz_compact_layers")
        torch.cuda.synchronize()
    ko, vo = ops.compact_layers(K, V, plan, totals)
    for l in range(L):
        for h in range(Hkv):
            s, n = seg_h[l][h], int(lens[l, h])
            idx = full[l, h].nonzero().view(-1).to(DEV)
            for got, src, ordinary in ((outs[l][0], K[l], ko[l]), (outs[l][1], V[l], vo[l])):
                want = src[0, h].index_select(0, idx)
                assert _same(got[s:s + n], want), (mode, l, h, "moved rows != index_select on the full mask")
                assert _same(got[s:s + n], ordinary[s:s + n])
    a.assert_clean()


def _compact_geoms():
    for klen in (1023, 1024, 1025, 2047, 2048, 2049):
        for sink in (4, 5, 6, 7):
            for tail in (0, 9):
                yield sink, klen - sink - tail, tail


def test_compact_geometry_sweep_covers_both_mask_paths():
    """sink % 4 x N % 4 x tail, klen straddling one and two tiles: every (sink % 4, N % 4 in {0, 1, 3}) pair occurs."""
    seen = {(s % 4, n % 4) for s, n, _ in _compact_geoms()}
    assert {(s, n) for s in range(4) for n in (0, 1, 3)} <= seen


@pytest.mark.parametrize("slack", [0, 1, 37])
def test_compact_batched_gather_over_mask_geometries(slack):
    for i, (sink, N, tail) in enumerate(_compact_geoms()):
        _compact("layers", 2, 3, sink, N, tail, slack, 128, 2, seed=i)


@pytest.mark.parametrize("mode", ["layer", "heads"])
def test_compact_single_layer_and_head_level(mode):
    for i, (sink, N, tail) in enumerate(_compact_geoms()):
        if (sink + N + tail) in (1025, 2048) and sink in (4, 7):
            for slack in (0, 37):
                _compact(mode, 2, 3, sink, N, tail, slack, 128, 2, seed=i)


@pytest.mark.parametrize("D,eb", [(64, 1), (64, 2), (128, 2), (128, 4), (256, 4)], ids=["64B", "128B", "256B", "512B", "1024B"])
def test_compact_every_row_size(D, eb):
    """Row bytes 64 .. 1024: the five compact_gather_kernel<LPR> instantiations (the kernel moves bytes: integer views)."""
    for sink, tail, klen in ((8, 0, 2049), (5, 9, 1025)):
        for slack in (0, 1):
            _compact("layers", 2, 2, sink, klen - sink - tail, tail, slack, D, eb, seed=D + eb)


@pytest.mark.parametrize("t", [0, 1, 7])
def test_update_flatten_view(t):
    """A head of 0 rows and a head of 5000 rows x 256 B (80 000 16-byte chunks: one block's grid-stride loop wraps)."""
    lib = _lib()
    Hkv, D = 4, 128
    g = torch.Generator().manual_seed(t)
    lens = torch.tensor([5, 0, 5000, 40], dtype=torch.int32)
    cu = torch.cat([torch.zeros(1, dtype=torch.int32), lens.cumsum(0).int()])
    cache = torch.randn(int(cu[-1]), D, generator=g).half().to(DEV)
    state = torch.randn(Hkv * max(t, 1), D, generator=g).half().to(DEV)
    lens_d, cu_d = lens.to(DEV), cu.to(DEV)
    a = Arena(DEV)
    out = a.carve("out", ((int(cu[-1]) + Hkv * t, D), F16), names=("row", "elem"))
    with frozen(cache, state, lens_d, cu_d):
        _ok(lib.kvz_update_flatten_view(cache.data_ptr(), state.data_ptr(), lens_d.data_ptr(), cu_d.data_ptr(), Hkv, t, D, 2, out.data_ptr(),
                                        _st()), "kvz_update_flatten_view")
    want = torch.cat([torch.cat([cache[int(cu[h]):int(cu[h + 1])], state[h * t:(h + 1) * t]]) for h in range(Hkv)])
    assert _same(out, want)
    if t:
        assert _same(out, _ops().update_flatten_view(cache, state, lens_d, cu_d))
    a.assert_clean()


@pytest.mark.parametrize("t", [1, 7, 2026])
@pytest.mark.parametrize("which", ["inplace", "dense"])
def test_appends_touch_only_the_new_rows(which, t):
    """kvz_append_inplace (slack layout, len_offset > 0) and kvz_dense_append with strided state views: everything outside the t new
    rows of each head keeps the pattern."""
    lib, ops = _lib(), _ops()
    Hkv, D, off, spare = 3, 128, 2, 9
    g = torch.Generator(device=DEV).manual_seed(t)
    ks = torch.randn(1, t, Hkv, D, generator=g, device=DEV).half().transpose(1, 2)              # row stride Hkv * D
    vs = torch.randn(1, Hkv, t + 3, D, generator=g, device=DEV).half()[:, :, 2:2 + t]           # a row window of a longer tensor
    a = Arena(DEV)
    if which == "inplace":
        base = [7, 0, 50]
        seg_h = [0, 7 + off + t + spare, 7 + off + t + spare + off + t + spare]
        total = sum(base) + Hkv * (off + t + spare)
        kc = a.carve("k_cache", ((total, D), F16), names=("row", "elem"))
        vc = a.carve("v_cache", ((total, D), F16), names=("row", "elem"))
        dec = torch.zeros(total, 1, dtype=torch.bool)
        for h in range(Hkv):
            dec[seg_h[h] + base[h] + off:seg_h[h] + base[h] + off + t] = True
        seg = torch.tensor(seg_h, dtype=torch.int32, device=DEV)
        bl = torch.tensor(base, dtype=torch.int32, device=DEV)
        a.declare(kc, dec)
        a.declare(vc, dec)
        with frozen(ks, vs, seg, bl):
            _ok(lib.kvz_append_inplace(kc.data_ptr(), vc.data_ptr(), ks.data_ptr(), vs.data_ptr(), ks.stride(1), ks.stride(2), vs.stride(1),
                                       vs.stride(2), seg.data_ptr(), bl.data_ptr(), off, Hkv, t, D, 2, _st()), "kvz_append_inplace")
        k2, v2 = torch.zeros(total, D, dtype=F16, device=DEV), torch.zeros(total, D, dtype=F16, device=DEV)
        ops.append_inplace(k2, v2, ks, vs, seg, bl, len_offset=off)
        for h in range(Hkv):
            r = seg_h[h] + base[h] + off
            assert _same(kc[r:r + t], ks[0, h]) and _same(vc[r:r + t], vs[0, h])
            assert _same(kc[r:r + t], k2[r:r + t]) and _same(vc[r:r + t], v2[r:r + t])
    else:
        fill, cap = 13, 13 + t + spare
        kc = a.carve("k_cache", ((Hkv, cap, D), F16), names=("head", "row", "elem"))
        vc = a.carve("v_cache", ((Hkv, cap, D), F16), names=("head", "row", "elem"))
        dec = torch.zeros(1, cap, 1, dtype=torch.bool)
        dec[0, fill:fill + t] = True
        a.declare(kc, dec)
        a.declare(vc, dec)
        with frozen(ks, vs):
            _ok(lib.kvz_dense_append(kc.data_ptr(), vc.data_ptr(), kc.stride(0), fill, ks.data_ptr(), vs.data_ptr(), ks.stride(1), ks.stride(2),
                                     vs.stride(1), vs.stride(2), Hkv, t, D, 2, _st()), "kvz_dense_append")
        assert _same(kc[:, fill:fill + t], ks[0]) and _same(vc[:, fill:fill + t], vs[0])
    a.assert_clean()


# ====================================================================================================================================
# attention
# ====================================================================================================================================
def _decode(d, a, items, fill=None):
    """kvz_varlen_attn on a guarded out and a workspace of exactly the size function's value under the current knob."""
    lib, ops = _lib(), _ops()
    p = d.p
    HQ, G, D = p.q.shape
    Hkv = HQ // p.q_len
    need = int(lib.kvz_varlen_attn_workspace_bytes(Hkv, G, p.q_len, D, max(p.lens)))
    ws = a.carve(f"attn_ws_items{items}_{fill}", need, guard=need)
    out = a.carve(f"out_items{items}_{fill}", ((HQ, G, D), p.dtype), names=("row", "group", "elem"))
    if fill is not None:
        interior(ws, fill)
    kl = torch.tensor(p.lens, dtype=torch.int32, device=DEV)
    with frozen(d.q, d.k, d.v, d.ks, kl):
        _ok(lib.kvz_varlen_attn(d.q.data_ptr(), d.k.data_ptr(), d.v.data_ptr(), d.ks.data_ptr(), kl.data_ptr(), 0, None,
                                ops._meta_host(p.starts, p.lens, Hkv), Hkv, G, p.q_len, D, max(max(p.lens), 1), float(p.scale),
                                1 if p.causal else 0, ops._dtype_code(p.dtype), out.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "kvz_varlen_attn")
    return out


@DTYPES
@pytest.mark.parametrize("D", [64, 128])
def test_decode_attention(dtype, D):
    """RAGGED heads, attn_items in {1, Hkv, default, 1024}; the workspace is sized under that knob and dirty (0x00, 0xFF)."""
    Hkv = len(tae.RAGGED)
    for G, q_len in ((7, 1), (8, 8), (1, 5)):
        for make in (ap.uniform_probe, ap.weighted_probe):
            p = make(tae.RAGGED, q_len, G, D, dtype, seed=G)
            want = ap.expected(p, "div")
            d = tae._Dev(p)
            a = Arena(DEV)
            for items in (1, Hkv, 0, 1024):
                with knobs(attn_items=items):
                    ordinary = tae._attn(d, p.lens)
                    for fill in (0x00, 0xFF):
                        out = _decode(d, a, items, fill)
                        assert ap.bits_equal(out.cpu(), want)[0] and _same(out, ordinary), (G, q_len, p.kind, items, fill)
            a.assert_clean()


@DTYPES
def test_decode_append_writes_one_row_per_head(dtype):
    """kvz_varlen_attn_append with a host and a device offset (advanced by kvz_add_i32 on a guarded 4-byte counter): exactly the row
    k_start + k_len + k_len_offset + *offset_dev of each head changes; the slack rows behind the segments keep the pattern."""
    lib, ops = _lib(), _ops()
    base, host_off, dev_off = [256, 0, 100, 17], 1, 2
    seen = [n + host_off + dev_off for n in base]         # keys in the cache before the call
    after = [n + 1 for n in seen]
    Hkv, G, D = 4, 7, 128
    for p in (ap.uniform_probe(after, 1, G, D, dtype, items=(2,), seed=5), ap.weighted_probe(after, 1, G, D, dtype, spread=8, seed=6)):
        want = ap.expected(p, "div")
        d = tae._Dev(p)
        rows = p.k.shape[0]
        new_rows = torch.tensor([s + n for s, n in zip(p.starts, seen)], device=DEV)
        ks_state = torch.zeros(1, Hkv, 3, D, dtype=dtype, device=DEV)[:, :, 1:2]
        vs_state = torch.zeros(1, Hkv, 5, D, dtype=dtype, device=DEV)[:, :, 2:3]
        ks_state[0, :, 0] = d.k[new_rows]
        vs_state[0, :, 0] = d.v[new_rows]
        kl = torch.tensor(base, dtype=torch.int32, device=DEV)
        dec = torch.zeros(rows, 1, dtype=torch.bool)
        for s, n in zip(p.starts, after):
            dec[s:s + n] = True
        for items in (2, 0, 1024):
            with knobs(attn_items=items):
                a = Arena(DEV)
                kc = a.carve("k_cache", ((rows, D), dtype), names=("row", "elem"))
                vc = a.carve("v_cache", ((rows, D), dtype), names=("row", "elem"))
                a.declare(kc, dec)
                a.declare(vc, dec)
                idx = dec.view(-1).nonzero().view(-1).to(DEV)
                kc[idx], vc[idx] = d.k[idx], d.v[idx]
                kc[new_rows], vc[new_rows] = ap.SLACK_VALUE, ap.SLACK_VALUE
                counter = a.carve("offset_dev", ((1,), torch.int32))
                counter.zero_()
                _ok(lib.kvz_add_i32(counter.data_ptr(), dev_off, _st()), "kvz_add_i32")
                need = int(lib.kvz_varlen_attn_workspace_bytes(Hkv, G, 1, D, max(after)))
                ws = a.carve("attn_ws", need, guard=need)
                out = a.carve("out", ((Hkv, G, D), dtype), names=("head", "group", "elem"))
                with frozen(d.q, ks_state, vs_state, d.ks, kl, counter):
                    _ok(lib.kvz_varlen_attn_append(d.q.data_ptr(), kc.data_ptr(), vc.data_ptr(), ks_state.data_ptr(), vs_state.data_ptr(),
                                                   ks_state.stride(1), vs_state.stride(1), d.ks.data_ptr(), kl.data_ptr(), host_off,
                                                   counter.data_ptr(), ops._meta_host(p.starts, base, Hkv), Hkv, G, D, max(after), float(p.scale),
                                                   ops._dtype_code(dtype), out.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "kvz_varlen_attn_append")
                assert int(counter.item()) == dev_off
                assert ap.bits_equal(out.cpu(), want)[0], (p.kind, items)
                assert _same(kc[idx], d.k[idx]) and _same(vc[idx], d.v[idx]), "one row per head written, every other row as before"
                k2, v2 = d.k.clone(), d.v.clone()
                ordinary = ops.varlen_attn_append(d.q, k2, v2, ks_state, vs_state, d.ks, kl, host_off + dev_off, max(after), softmax_scale=p.scale,
                                                  workspace=ops.attn_workspace(Hkv, G, 1, D, DEV))
                assert _same(out, ordinary)
                a.assert_clean()


def _flash(p, a, tag, layout, ws_mode, want, want_lse=None):
    """kvz_flash_fwd on a probe's flat cache; out in layout "rows" ([Hkv*q_len, G, D], exact), "heads" ([H, q_len, D], exact) or "wide"
    ([Hkv*q_len, G, D] inside a wider strided tensor); ws of exactly kvz_flash_workspace_bytes, or NULL."""
    lib, ops = _lib(), _ops()
    HQ, G, D = p.q.shape
    q_len = p.q_len
    Hkv = HQ // q_len
    q, k, v = p.q.to(DEV), p.k.to(DEV), p.v.to(DEV)
    names = ("head", "pos", "group", "elem")
    if layout == "rows":
        out = a.carve(f"out_{tag}", ((Hkv, q_len, G, D), p.dtype), names=names)
    elif layout == "wide":
        pos = G * D + 32
        out = a.carve(f"out_{tag}", ((Hkv, q_len, G, D), p.dtype), strides=(q_len * pos + 64, pos, D, 1), names=names)
    else:
        out = a.carve(f"out_{tag}", ((Hkv, G, q_len, D), p.dtype), names=("head", "group", "pos", "elem")).permute(0, 2, 1, 3)
    lse = a.carve(f"lse_{tag}", ((Hkv, q_len * G), torch.float32), names=("head", "row"))
    need = int(lib.kvz_flash_workspace_bytes(Hkv, G, q_len, D)) if ws_mode != "null" else 0
    ws = a.carve(f"flash_ws_{tag}", need, guard=max(need, 1)) if need else None
    if ws is not None and ws_mode in (0x00, 0xFF):
        interior(ws, ws_mode)
    with frozen(q, k, v):
        _ok(lib.kvz_flash_fwd(q.data_ptr(), q_len * G * D, D, G * D, k.data_ptr(), v.data_ptr(), None, None, 0, ops._meta_host(p.starts, p.lens, Hkv),
                              Hkv, G, q_len, D, float(p.scale), 1 if p.causal else 0, ops._dtype_code(p.dtype), out.data_ptr(), out.stride(0),
                              out.stride(2), out.stride(1), lse.data_ptr(), ws.data_ptr() if ws is not None else None, need, _st()), "kvz_flash_fwd")
    torch.cuda.synchronize()
    ok = ap.bits_equal(out.cpu().reshape(HQ, G, D), want)[0]
    if want_lse is not None:
        ok = ok and _same(lse.view(Hkv, q_len, G), want_lse)
    return ok, need


@DTYPES
def test_flash_fwd_ragged_layouts_workspaces_and_knobs(dtype):
    """The MULTI shapes (heads shorter than q_len: rows that see no key) under the flash2_* sweep of test_multi_row_kernels_exact."""
    ops = _ops()
    fails = []
    for name, D, kn in tae._multi_configs():
        for lens, q_len, G in tae.MULTI:
            for causal in (True, False):
                p = ap.weighted_probe(lens, q_len, G, D, dtype, causal=causal, spread=6, seed=q_len, headroom=ap.F2_DEFER)
                want = ap.expected(p, "rcp")
                Hkv = len(lens)
                qd = p.q.to(DEV).view(Hkv, q_len, G, D).permute(0, 2, 1, 3).reshape(1, Hkv * G, q_len, D)
                a = Arena(DEV)
                with knobs(**kn):
                    o_ord, lse_ord = ops.flash_fwd_ragged(qd, p.k.to(DEV), p.v.to(DEV), p.starts, p.lens, causal, softmax_scale=p.scale)
                    assert ap.bits_equal(o_ord.cpu().reshape(-1, G, D), want)[0]
                    for layout, ws_mode in (("rows", 0x00), ("rows", 0xFF), ("heads", "exact"), ("wide", "exact"), ("wide", "null")):
                        ok, need = _flash(p, a, f"{layout}_{ws_mode}", layout, ws_mode, want, lse_ord if ws_mode != "null" else None)
                        v = a.check()
                        if not ok or v:
                            fails.append((name, q_len, causal, layout, ws_mode, ok, [str(x) for x in v]))
                    if not causal or min(lens) >= q_len:
                        continue
                    assert bool(torch.isinf(lse_ord).any()), "a row that sees no key has lse -inf"
    assert not fails, fails[:6]


@DTYPES
def test_flash_fwd_dense_cache_views(dtype):
    """The dense shapes of test_flash_fwd_dense_exact_output_and_lse: K, V are views of a cache with spare rows, out is [1, q, H, D]."""
    lib, ops = _lib(), _ops()
    for (Hkv, G, q_len, klen, D), kn in (((4, 7, 300, 300, 128), {}), ((4, 7, 300, 300, 128), dict(flash2_min_blocks=1)),
                                         ((8, 8, 65, 200, 64), {}), ((2, 7, 1, 77, 128), {})):
        p = ap.uniform_probe([klen] * Hkv, q_len, G, D, dtype, seed=klen)
        want = ap.expected(p, "rcp").view(Hkv, q_len, G, D).permute(1, 0, 2, 3).reshape(1, q_len, Hkv * G, D)
        cap = klen + 9
        q, kv, vv = tae._dense_from_probe(p, Hkv, klen, cap)
        H = Hkv * G
        a = Arena(DEV)
        with knobs(**kn):
            o_ord, lse_ord = ops.flash_fwd(q, kv, vv, causal=True, softmax_scale=p.scale, return_lse=True)
            for fill in (0x00, 0xFF):
                out = a.carve(f"out{fill}", ((q_len, H, D), dtype), names=("pos", "head", "elem"))
                lse = a.carve(f"lse{fill}", ((Hkv, q_len, G), torch.float32), names=("head", "pos", "group"))
                need = int(lib.kvz_flash_workspace_bytes(Hkv, G, q_len, D))
                ws = interior(a.carve(f"flash_ws{fill}", need, guard=need), fill) if need else None
                with frozen(q, kv, vv):
                    _ok(lib.kvz_flash_fwd(q.data_ptr(), G * q.stride(1), q.stride(1), q.stride(2), kv.data_ptr(), vv.data_ptr(), None, None, 0,
                                          ops._meta_host([h * cap for h in range(Hkv)], [klen] * Hkv, Hkv), Hkv, G, q_len, D, float(p.scale), 1,
                                          ops._dtype_code(dtype), out.data_ptr(), G * D, D, H * D, lse.data_ptr(),
                                          ws.data_ptr() if need else None, need, _st()), "kvz_flash_fwd")
                assert ap.bits_equal(out.cpu().view(1, q_len, H, D), want)[0] and _same(out, o_ord)
                assert _same(lse.permute(0, 2, 1).reshape(1, H, q_len), lse_ord)
        a.assert_clean()


@DTYPES
@pytest.mark.parametrize("name", ["headline_first", "hkv1"])
def test_flash_fwd_window_and_score_from_stats(name, dtype):
    """kvz_flash_fwd_window with win_stats_head_stride larger than G*q_len, then kvz_score_from_stats_log (and its asynchronous form)
    on those statistics, frozen."""
    lib, ops = _lib(), _ops()
    p = tse._probe(name, dtype, "hot")
    d = tse._Dev(p)
    R = d.G * d.q_len
    stride = (R + 127) // 128 * 128 + 128
    v_store = torch.zeros_like(d.k_store)
    v = v_store[:, :, :p.klen]
    H = d.Hkv * d.G
    st = _st()
    b = _ScoreBufs(d)
    stats = b.a.carve("win_stats", ((d.Hkv, R, 2), torch.float32), strides=(stride * 2, 2, 1), names=("head", "row", "m_l"))
    out = b.a.carve("fwd_out", ((d.q_len, H, d.D), dtype), names=("pos", "head", "elem"))
    plain_stats = torch.full((d.Hkv, stride, 2), float("nan"), dtype=torch.float32, device=DEV)
    step = d.k.stride(1) // d.D if d.Hkv > 1 else p.klen
    meta = ops._meta_host([h * step for h in range(d.Hkv)], [p.klen] * d.Hkv, d.Hkv)
    with knobs(flash2_min_blocks=1):
        o_ord = ops.flash_fwd_window(d.q, d.k, v, p.sink, p.start, p.end, plain_stats)
        assert o_ord is not None
        with frozen(d.q, d.k_store, v_store):
            _ok(lib.kvz_flash_fwd_window(d.q.data_ptr(), d.G * d.q.stride(1), d.q.stride(1), d.q.stride(2), d.k.data_ptr(), v.data_ptr(), meta,
                                         d.Hkv, d.G, d.q_len, d.D, 1.0 / d.D ** 0.5, d.dt, out.data_ptr(), d.G * d.D, d.D, H * d.D, p.sink, p.start,
                                         p.end, stats.data_ptr(), stride, st), "kvz_flash_fwd_window")
        assert _same(out, o_ord) and _same(stats, plain_stats[:, :R])
        assert torch.equal(stats[..., 1].cpu(), p.l.float()), "l'_r is the exact count"
        b.a.assert_clean()
        a = tse._Async()
        try:
            for form in ("sync", "async"):
                b.reset(st)
                with frozen(d.q, d.k_store, stats):
                    if form == "sync":
                        _ok(lib.kvz_score_from_stats_log(d.q.data_ptr(), d.q.stride(1), d.k.data_ptr(), d.k.stride(1), p.klen, p.sink, p.start, p.end,
                                                         d.q_len, d.Hkv, d.G, d.D, d.dt, stats.data_ptr(), stride, b.log.data_ptr(), b.hs, st),
                            "kvz_score_from_stats_log")
                    else:
                        _ok(lib.kvz_score_from_stats_async_log(a.h, 0, a.cur, a.side.cuda_stream, d.q.data_ptr(), d.q.stride(1), d.k.data_ptr(),
                                                               d.k.stride(1), p.klen, p.sink, p.start, p.end, d.q_len, d.Hkv, d.G, d.D, d.dt,
                                                               stats.data_ptr(), stride, b.log.data_ptr(), b.hs), "kvz_score_from_stats_async_log")
                        _ok(lib.kvz_async_wait(a.h, -1, a.cur), "kvz_async_wait")
                    got = b.finalize(st)
                tse._check(p, got, f"{name}/{dtype} from_stats {form}")
                b.a.assert_clean()
        finally:
            torch.cuda.synchronize()
            a.close()


@DTYPES
@pytest.mark.parametrize("G,B,D", tfa.GEOMS)
def test_fork_attn_append(G, B, D, dtype):
    """GEOMS of test_gpu_fork_attn: tail_len in {0, 1, 37, tail_cap - 1} and one inactive branch (-1: no tail write, output rows zero).
    Only row tail_len[b] of an active branch may change; the rows behind it, every row of an inactive branch and the surroundings
    keep the pattern; the shared cache is frozen; ws is exact and dirty (0x00, 0xFF)."""
    lib, ops = _lib(), _ops()
    cap, Hkv = 64, len(tfa.LENS)
    with knobs(attn_items=tfa.ITEMS):
        for make in (fp.uniform_case, fp.weighted_case):
            c = make(tfa.LENS, B, G, D, dtype, tfa._tail_lens(B, cap, inactive=B - 2), cap, seed=B)
            want = fp.expected_out(c)
            etk, etv = fp.expected_tails(c)
            ordinary = tfa._run(c)[0]
            q, k, v = c.q.to(DEV), c.k.to(DEV), c.v.to(DEV)
            kn = c.k_new.to(DEV)
            vn = c.v_new.to(DEV).transpose(1, 2).contiguous().transpose(1, 2)
            ks = torch.tensor(c.starts, dtype=torch.int32, device=DEV)
            kl = torch.tensor(c.lens, dtype=torch.int32, device=DEV)
            a = Arena(DEV)
            tk = a.carve("tail_k", ((B, Hkv, cap, D), dtype), names=("branch", "head", "row", "elem"))
            tv = a.carve("tail_v", ((B, Hkv, cap, D), dtype), names=("branch", "head", "row", "elem"))
            dec = torch.zeros(B, 1, cap, 1, dtype=torch.bool)
            for bb, t in enumerate(c.tail_len):
                if t >= 0:
                    dec[bb, 0, :t + 1] = True
                    tk[bb, :, :t], tv[bb, :, :t] = c.tail_k[bb, :, :t].to(DEV), c.tail_v[bb, :, :t].to(DEV)
            a.declare(tk, dec)
            a.declare(tv, dec)
            need = int(lib.kvz_fork_attn_workspace_bytes(B, Hkv, G, D, 0))
            ws = a.carve("fork_ws", need, guard=need)
            out = a.carve("out", ((B, Hkv, G, D), dtype), names=("branch", "head", "group", "elem"))
            tl = (C.c_int32 * B)(*c.tail_len)
            for fill in (0x00, 0xFF):
                interior(ws, fill)
                out.fill_(float("nan"))
                with frozen(q, k, v, kn, vn, ks, kl):
                    _ok(lib.kvz_fork_attn_append(q.data_ptr(), k.data_ptr(), v.data_ptr(), ks.data_ptr(), kl.data_ptr(), 0,
                                                 ops._meta_host(c.starts, c.lens, Hkv), tk.data_ptr(), tv.data_ptr(), cap, tl, kn.data_ptr(),
                                                 vn.data_ptr(), kn.stride(0), kn.stride(1), vn.stride(0), vn.stride(1), B, Hkv, G, D, float(c.scale),
                                                 ops._dtype_code(dtype), out.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "kvz_fork_attn_append")
                assert ap.bits_equal(out.cpu(), want)[0] and _same(out, ordinary), (c.kind, fill)
                for bb, t in enumerate(c.tail_len):
                    if t >= 0:
                        assert _same(tk[bb, :, :t + 1], etk[bb, :, :t + 1]) and _same(tv[bb, :, :t + 1], etv[bb, :, :t + 1]), (c.kind, bb)
                    else:
                        assert bool((out[bb] == 0).all())
                a.assert_clean()


@DTYPES
@pytest.mark.parametrize("D", [64, 128])
def test_attn_merge_lse(dtype, D):
    lib, ops = _lib(), _ops()
    g = torch.Generator().manual_seed(D)
    for rows in (1, 6, 77, 1001):
        o1 = torch.randn(rows, D, generator=g).to(dtype).to(DEV)
        o2 = torch.randn(rows, D, generator=g).to(dtype).to(DEV)
        l1 = torch.randn(rows, generator=g).to(DEV)
        l2 = torch.randn(rows, generator=g).to(DEV)
        l1[::5], l2[::3] = float("-inf"), float("-inf")
        want = ops.attn_merge_lse(o1, l1, o2, l2)
        a = Arena(DEV)
        out = a.carve("out", ((rows, D), dtype), names=("row", "elem"))
        alias = a.carve("o1_and_out", ((rows, D), dtype), names=("row", "elem"))
        alias.copy_(o1)
        with frozen(o1, l1, o2, l2):
            _ok(lib.kvz_attn_merge_lse(o1.data_ptr(), l1.data_ptr(), o2.data_ptr(), l2.data_ptr(), out.data_ptr(), rows, D, ops._dtype_code(dtype),
                                       _st()), "kvz_attn_merge_lse")
            _ok(lib.kvz_attn_merge_lse(alias.data_ptr(), l1.data_ptr(), o2.data_ptr(), l2.data_ptr(), alias.data_ptr(), rows, D,
                                       ops._dtype_code(dtype), _st()), "kvz_attn_merge_lse")
        assert _same(out, want) and _same(alias, want)
        both = (torch.isinf(l1) & torch.isinf(l2)).cpu()
        assert bool((out.cpu()[both] == 0).all())
        a.assert_clean()
