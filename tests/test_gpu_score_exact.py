"""Scoring kernels against inputs whose correct scores are known exactly (tests/score_probes.py): BIT equality, no tolerance.

The random-input scoring tests compare with the oracle under fixed parity bounds, and the pruned-path / tail tests compare knobs with
each other.  A fault in what every knob shares - the pass-A statistics, the merge, n_r, the log encoding, the finalize - or one key
counted wrongly in one row's l_r passes both.  Here every logit is 0 or dead, every l_r an exact count, every score half(1 / min l_r):
one key dropped or counted twice at a tile, unit, block or causal edge, a (row, key) pair lost by the group bounds or the candidate-key
pass, a tie decided the wrong way, moves a score that is compared bit for bit.

Entry points: kvz_score_chunk (ops.score_chunk), kvz_score_chunk_log + kvz_score_finalize_log, kvz_score_finalize_log_hist +
kvz_select_threshold_prehist, kvz_score_chunk_async_log, kvz_update_score_async_log, the pipelined tail (knob 6, a workspace of three
sets, kvz_score_tail_flush in the middle) and kvz_score_from_stats_log on the statistics of kvz_flash_fwd_window.  Knobs: score_prune
0 / 1 / 3 / 4 / 6 and the two-pass path of q_len < 32.  Every knob is restored in `finally`."""
import contextlib
import functools

import pytest
import torch

import kvzip_oracle as orc
import score_probes as sp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16

# name: (Hkv, G, D, sink, start, m, q_len, tail_gap, slack)
GEOMS = {
    "headline_first": (4, 7, 128, 32, 32, 2000, 2013, 100, 0),
    "headline_later": (4, 7, 128, 32, 2032, 2000, 2026, 50, 0),
    "far": (2, 7, 128, 32, 128_032, 2000, 2026, 0, 0),
    "d64": (2, 4, 64, 16, 116, 300, 310, 7, 5),
    "g1": (8, 1, 128, 0, 5, 33, 40, 0, 3),
    "g8_d64": (2, 8, 64, 30, 430, 513, 77, 0, 0),
    "hkv1": (1, 7, 128, 4, 1004, 777, 790, 0, 8),
    "m1_q1": (2, 7, 128, 0, 0, 1, 1, 0, 0),
    "m3_q7": (2, 7, 128, 4, 4, 3, 7, 0, 2),
    "m5_q31": (1, 8, 64, 30, 30, 5, 31, 0, 0),
    "m33_q32": (2, 7, 128, 32, 40, 33, 32, 0, 1),
    "m1_q33": (1, 7, 128, 30, 31, 1, 33, 0, 0),
    "m3_q129": (2, 7, 128, 0, 9, 3, 129, 0, 0),
    "m33_q257": (2, 7, 64, 4, 4, 33, 257, 0, 4),
    "m5_q257": (1, 1, 128, 32, 32, 5, 257, 0, 0),
}
LOG_KNOBS = (0, 1, 3, 4)


@functools.lru_cache(maxsize=8)
def _probe(name, dtype, variant):
    Hkv, G, D, sink, start, m, q_len, gap, slack = GEOMS[name]
    return sp.score_probe(Hkv, G, q_len, D, dtype, sink, start, m, variant, tail_gap=gap, slack=slack, seed=len(name))


def _ops():
    from kvzip_amd import ops
    return ops


def _lib():
    return _ops()._lib.load()


@contextlib.contextmanager
def _knob(v):
    lib = _lib()
    prev = lib.kvz_debug_set_tunable(b"score_prune", int(v))
    try:
        yield
    finally:
        lib.kvz_debug_set_tunable(b"score_prune", prev)


class _Dev:
    """The probe's tensors on the device; K keeps its head stride (slack rows behind every head)."""

    def __init__(self, p):
        self.p = p
        self.q = p.q.to(DEV)
        self.k_store = p.k_store.to(DEV)
        self.k = self.k_store[:, :, :p.klen]
        _, self.H, self.q_len, self.D = p.q.shape
        self.Hkv = p.k_store.shape[1]
        self.G = self.H // self.Hkv
        self.dt = _ops()._dtype_code(p.dtype)

    def ws_bytes(self):
        return _lib().kvz_score_workspace_bytes(self.Hkv, self.G, self.q_len, self.p.m, self.p.sink)

    def nan_out(self):
        """score buffer holding NaN: an entry a kernel leaves untouched never equals the expected bits"""
        return torch.full((self.Hkv, self.p.m), float("nan"), dtype=self.p.dtype, device=DEV)

    def new_log(self, st):
        log = torch.empty(self.Hkv, self.p.m, dtype=torch.int32, device=DEV)
        _ops().check(_lib().kvz_score_log_fill(log.data_ptr(), log.numel(), st), "kvz_score_log_fill")
        return log

    def finalize(self, log, st):
        out = self.nan_out()
        _ops().check(_lib().kvz_score_finalize_log(log.data_ptr(), log.numel(), out.data_ptr(), self.dt, st), "kvz_score_finalize_log")
        return out

    def chunk_log(self, log, ws, st):
        p = self.p
        return _lib().kvz_score_chunk_log(self.q.data_ptr(), self.q.stride(1), self.k.data_ptr(), self.k.stride(1), p.klen, p.sink, p.start,
                                          p.end, self.q_len, self.Hkv, self.G, self.D, self.dt, log.data_ptr(), p.m, ws.data_ptr(), ws.numel(),
                                          st)


def _check(p, got, what):
    ok, _ = sp.bits_equal(got, p.want)
    assert ok, f"{what}: " + sp.describe_mismatch(p, got)


# ---- the synchronous entry points --------------------------------------------------------------------------------------------------
def _run_chunk(d, knob):
    """ops.score_chunk (kvz_score_chunk: the colpart finalize; knobs >= 3 fall back to 1 without a log buffer)"""
    with _knob(knob):
        out = d.nan_out().view(1, d.Hkv, d.p.m)
        _ops().score_chunk(d.q, d.k, d.p.sink, d.p.start, d.p.end, out=out)
        torch.cuda.synchronize()
    return out[0].cpu()


def _run_log(d, knob):
    """kvz_score_chunk_log + kvz_score_finalize_log (the deferred path)"""
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(d.ws_bytes(), dtype=torch.uint8, device=DEV)
    with _knob(knob):
        log = d.new_log(st)
        _ops().check(d.chunk_log(log, ws, st), "kvz_score_chunk_log")
        out = d.finalize(log, st)
        torch.cuda.synchronize()
    return out.cpu(), log


@pytest.mark.parametrize("variant", ["hot", "cold"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_synchronous_entry_points_are_bit_exact(name, dtype, variant):
    p = _probe(name, dtype, variant)
    d = _Dev(p)
    knobs = LOG_KNOBS if d.q_len >= 32 else (0, 3)   # (q_len < 32: the two-pass kernels whatever the knob)
    for knob in knobs:
        got, _ = _run_log(d, knob)
        _check(p, got, f"{name}/{variant} chunk_log knob {knob}")
    for knob in (0, 1):
        _check(p, _run_chunk(d, knob), f"{name}/{variant} score_chunk knob {knob}")


# ---- the asynchronous entry points ---------------------------------------------------------------------------------------------------
class _Async:
    def __init__(self):
        lib = _lib()
        self.h = lib.kvz_async_create(4)
        assert self.h >= 0
        self.side = torch.cuda.Stream(device=DEV)
        self.cur = torch.cuda.current_stream().cuda_stream

    def close(self):
        _lib().kvz_async_destroy(self.h)


def _ws3(d):
    return torch.empty(3 * ((d.ws_bytes() + 255) // 256 * 256), dtype=torch.uint8, device=DEV)


def _run_async(d, knob):
    """kvz_score_chunk_async_log on a side stream (knob 6: the pipelined tail, flushed before the wait)"""
    lib, ops = _lib(), _ops()
    a = _Async()
    ws = _ws3(d)
    try:
        with _knob(knob):
            log = d.new_log(a.cur)
            ops.check(lib.kvz_score_chunk_async_log(a.h, 0, a.cur, a.side.cuda_stream, d.q.data_ptr(), d.q.stride(1), d.k.data_ptr(),
                                                    d.k.stride(1), d.p.klen, d.p.sink, d.p.start, d.p.end, d.q_len, d.Hkv, d.G, d.D, d.dt,
                                                    log.data_ptr(), d.p.m, ws.data_ptr(), ws.numel()), "kvz_score_chunk_async_log")
            assert lib.kvz_score_tail_flush_async(a.h, 0, ws.data_ptr(), a.side.cuda_stream) >= 0
            ops.check(lib.kvz_async_wait(a.h, -1, a.cur), "kvz_async_wait")
            out = d.finalize(log, a.cur)
            torch.cuda.synchronize()
    finally:
        lib.kvz_score_tail_flush(ws.data_ptr())
        torch.cuda.synchronize()
        a.close()
    return out.cpu()


def _run_update(d, knob):
    """kvz_update_score_async_log: the repeat chunk's K (and V) are appended to the dense cache on the caller's stream, then scored"""
    lib, ops = _lib(), _ops()
    p = d.p
    fill, t = p.klen - d.q_len, d.q_len
    kc = torch.zeros_like(d.k_store)                  # (the rows to be appended hold 0: live for every row until the append lands)
    kc[:, :, :fill] = d.k_store[:, :, :fill]
    vc = torch.zeros_like(kc)
    ks = d.k_store[:, :, fill:p.klen].clone()
    vs = torch.ones_like(ks)
    a = _Async()
    ws = _ws3(d)
    try:
        with _knob(knob):
            log = d.new_log(a.cur)
            ops.check(lib.kvz_update_score_async_log(a.h, 1, a.cur, a.side.cuda_stream, kc.data_ptr(), vc.data_ptr(), kc.stride(1), fill,
                                                     ks.data_ptr(), vs.data_ptr(), ks.stride(1), ks.stride(2), vs.stride(1), vs.stride(2), t,
                                                     d.q.data_ptr(), d.q.stride(1), p.sink, p.start, p.end, d.q_len, d.Hkv, d.G, d.D, d.dt,
                                                     log.data_ptr(), p.m, ws.data_ptr(), ws.numel()), "kvz_update_score_async_log")
            assert lib.kvz_score_tail_flush_async(a.h, 1, ws.data_ptr(), a.side.cuda_stream) >= 0
            ops.check(lib.kvz_async_wait(a.h, -1, a.cur), "kvz_async_wait")
            out = d.finalize(log, a.cur)
            torch.cuda.synchronize()
    finally:
        lib.kvz_score_tail_flush(ws.data_ptr())
        torch.cuda.synchronize()
        a.close()
    assert torch.equal(kc[:, :, fill:p.klen].view(torch.int16), ks.view(torch.int16))
    assert torch.equal(vc[:, :, fill:p.klen].view(torch.int16), vs.view(torch.int16))
    return out.cpu()


ASYNC_GEOMS = ["headline_first", "headline_later", "d64", "g1", "g8_d64", "m33_q32", "m3_q7", "m33_q257"]


@pytest.mark.parametrize("variant", ["hot", "cold"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ASYNC_GEOMS)
def test_asynchronous_entry_points_are_bit_exact(name, dtype, variant):
    p = _probe(name, dtype, variant)
    d = _Dev(p)
    for knob in (3, 6):
        _check(p, _run_async(d, knob), f"{name}/{variant} chunk_async_log knob {knob}")
    _check(p, _run_update(d, 6), f"{name}/{variant} update_score_async_log knob 6")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_pipelined_tail_with_a_flush_in_the_middle(dtype):
    """Five calls of one side stream on one workspace of three sets (knob 6): the bounds and candidate-key phases of call i run in the
    launches of calls i+1 and i+2.  kvz_score_tail_flush after the second call completes calls 0 and 1; the last flush the rest.  The
    calls mix probes of three shapes (one template instance: the pipeline continues across them)."""
    lib, ops = _lib(), _ops()
    seq = [("headline_later", "cold"), ("hkv1", "hot"), ("headline_later", "hot"), ("hkv1", "cold"), ("headline_first", "cold")]
    devs = [_Dev(_probe(n, dtype, v)) for n, v in seq]
    nbytes = max(3 * ((d.ws_bytes() + 255) // 256 * 256) for d in devs)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    logs, outs = [], []
    with _knob(6):
        a = _Async()
        try:
            for c, d in enumerate(devs):
                log = d.new_log(a.cur)
                logs.append(log)
                ops.check(lib.kvz_score_chunk_async_log(a.h, c % 4, a.cur, side.cuda_stream, d.q.data_ptr(), d.q.stride(1), d.k.data_ptr(),
                                                        d.k.stride(1), d.p.klen, d.p.sink, d.p.start, d.p.end, d.q_len, d.Hkv, d.G, d.D,
                                                        d.dt, log.data_ptr(), d.p.m, ws.data_ptr(), ws.numel()), "kvz_score_chunk_async_log")
                if c == 1:
                    assert lib.kvz_score_tail_flush(ws.data_ptr()) == 1, "calls 0 and 1 left phases pending"
                    side.synchronize()
                    for cc in (0, 1):
                        outs.append(devs[cc].finalize(logs[cc], side.cuda_stream))
                    side.synchronize()
            assert lib.kvz_score_tail_flush(ws.data_ptr()) == 1
            side.synchronize()
            for cc in range(2, len(devs)):
                outs.append(devs[cc].finalize(logs[cc], side.cuda_stream))
            side.synchronize()
        finally:
            lib.kvz_score_tail_flush(ws.data_ptr())
            torch.cuda.synchronize()
            a.close()
    for c, (d, out) in enumerate(zip(devs, outs)):
        _check(d.p, out.cpu(), f"tail call {c} ({seq[c][0]}/{seq[c][1]})")


# ---- finalize with the selection histogram, then the selection -----------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["hot", "cold"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["headline_first", "g8_d64", "m33_q257"])
def test_finalize_with_histogram_and_selection(name, dtype, variant):
    """kvz_score_finalize_log_hist + kvz_select_threshold_prehist on the log buffer of a probe: the scores are the expected bits, and the
    threshold and mask are the oracle's selection on the expected scores (the probes hold many equal scores: ties at the threshold)."""
    lib, ops = _lib(), _ops()
    p = _probe(name, dtype, variant)
    d = _Dev(p)
    _, log = _run_log(d, 3)
    st = torch.cuda.current_stream().cuda_stream
    sel = ops.select_workspace(DEV)
    want = p.want.view(1, 1, d.Hkv, p.m)
    for ratio in (0.05, 0.3, 0.5, 0.9):
        out = d.nan_out()
        ops.check(lib.kvz_score_finalize_log_hist(log.data_ptr(), log.numel(), out.data_ptr(), d.dt, sel.data_ptr(), sel.numel(), st),
                  "kvz_score_finalize_log_hist")
        valid, thres, kept, rows = ops.select_threshold(out.view(1, 1, d.Hkv, p.m), ratio, row_len=p.m, prehist=sel)
        torch.cuda.synchronize()
        _check(p, out.cpu(), f"{name}/{variant} finalize_log_hist")
        v_ref, t_ref = orc.threshold(want, ratio)
        assert float(thres.item()) == t_ref, (ratio, float(thres.item()), t_ref)
        assert torch.equal(valid.cpu(), v_ref), ratio
        assert int(kept.item()) == int(v_ref.sum()) and torch.equal(rows.cpu(), v_ref.view(-1, p.m).sum(-1).int())


# ---- pass B on the statistics of the scoring forward -------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["hot", "cold"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["headline_first", "hkv1"])
def test_score_from_forward_statistics(name, dtype, variant):
    """kvz_flash_fwd_window writes (m_r, l'_r) of the window from its own QK^T tiles: m_r = 0 and l'_r the exact count for every row;
    kvz_score_from_stats_log on them returns the expected bits."""
    lib, ops = _lib(), _ops()
    p = _probe(name, dtype, variant)
    d = _Dev(p)
    R = d.G * d.q_len
    stride = (R + 127) // 128 * 128
    stats = torch.full((d.Hkv, stride, 2), float("nan"), dtype=torch.float32, device=DEV)
    v_store = torch.zeros_like(d.k_store)
    v = v_store[:, :, :p.klen]
    st = torch.cuda.current_stream().cuda_stream
    prev = lib.kvz_debug_set_tunable(b"flash2_min_blocks", 1)
    try:
        o = ops.flash_fwd_window(d.q, d.k, v, p.sink, p.start, p.end, stats)
        assert o is not None, "the 32-row kernel takes this shape"
        log = d.new_log(st)
        ops.check(lib.kvz_score_from_stats_log(d.q.data_ptr(), d.q.stride(1), d.k.data_ptr(), d.k.stride(1), p.klen, p.sink, p.start, p.end,
                                               d.q_len, d.Hkv, d.G, d.D, d.dt, stats.data_ptr(), stats.stride(0) // 2, log.data_ptr(), p.m,
                                               st), "kvz_score_from_stats_log")
        out = d.finalize(log, st)
        torch.cuda.synchronize()
    finally:
        lib.kvz_debug_set_tunable(b"flash2_min_blocks", prev)
    s = stats[:, :R].cpu()
    assert bool((s[..., 0] == 0).all()), "m_r of a row with a live key is 0"
    assert torch.equal(s[..., 1], p.l.float()), "l'_r is the exact count"
    _check(p, out.cpu(), f"{name}/{variant} from_stats")
