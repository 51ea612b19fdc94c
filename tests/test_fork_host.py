"""CPU: the forked-decode entry points validate their arguments on the host before any launch, and the probe helpers of the exact
GPU tests (tests/fork_probes.py) produce what they promise."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_probes as ap
import fork_probes as fp


def _lib():
    from kvzip_amd import _lib
    return _lib.load()


def _call(lib, B=2, Hkv=4, G=7, D=128, tail_cap=8, tail_len=None, q=16, ws=16, ws_bytes=1 << 30, meta=True, k_start=16, dtype=0):
    tl = (C.c_int32 * max(B, 1))(*(tail_len if tail_len is not None else [0] * max(B, 1)))
    mh = (C.c_int32 * (2 * Hkv))(*([0] * Hkv + [10] * Hkv)) if meta else None
    return lib.kvz_fork_attn_append(q, 16, 16, k_start, k_start, 0, mh, 16, 16, tail_cap, tl, 16, 16, 8 * D, D, 8 * D, D, B, Hkv, G, D, 0.1,
                                    dtype, 16, ws, ws_bytes, None)


def test_fork_argument_validation_without_gpu():
    """Bad arguments are rejected on the host before any launch (error code + message)."""
    lib = _lib()
    assert _call(lib, D=96) == -4 and b"head_dim" in lib.kvz_last_error()
    assert _call(lib, B=5, G=13) == -4 and b"query rows" in lib.kvz_last_error()          # B*G = 65
    assert _call(lib, B=13, G=5) == -4 and b"query rows" in lib.kvz_last_error()          # B*G = 65
    assert _call(lib, B=17, G=1) == -4                                                     # more than 16 branches
    assert _call(lib, Hkv=65) == -4 and b"KV heads" in lib.kvz_last_error()
    assert _call(lib, q=None) == -1 and b"null pointer" in lib.kvz_last_error()
    assert _call(lib, ws=None) == -1 and b"null pointer" in lib.kvz_last_error()
    assert _call(lib, meta=False, k_start=None) == -1 and b"null pointer" in lib.kvz_last_error()
    assert _call(lib, B=0) == -1 and b"bad shape" in lib.kvz_last_error()
    assert _call(lib, dtype=3) == -1 and b"dtype" in lib.kvz_last_error()
    assert _call(lib, q=24) == -1 and b"aligned" in lib.kvz_last_error()
    # the new row must fit: tail_len in [-1, tail_cap)
    assert _call(lib, tail_len=[0, 8]) == -1 and b"tail_len[1]" in lib.kvz_last_error()
    assert _call(lib, tail_len=[-2, 0]) == -1 and b"tail_len[0]" in lib.kvz_last_error()
    assert _call(lib, ws_bytes=64) == -2 and b"workspace" in lib.kvz_last_error()
    from kvzip_amd import _lib as L
    with pytest.raises(L.KvzError):
        L.check(_call(lib, D=96), "kvz_fork_attn_append")


def test_merge_lse_argument_validation_without_gpu():
    lib = _lib()
    assert lib.kvz_attn_merge_lse(16, 16, 16, 16, 16, 10, 96, 0, None) == -4 and b"head_dim" in lib.kvz_last_error()
    assert lib.kvz_attn_merge_lse(None, 16, 16, 16, 16, 10, 128, 0, None) == -1 and b"null pointer" in lib.kvz_last_error()
    assert lib.kvz_attn_merge_lse(16, 16, 16, 16, 16, -1, 128, 0, None) == -1 and b"bad shape" in lib.kvz_last_error()
    assert lib.kvz_attn_merge_lse(16, 16, 16, 16, 16, 10, 128, 2, None) == -1 and b"dtype" in lib.kvz_last_error()
    assert lib.kvz_attn_merge_lse(16, 16, 24, 16, 16, 10, 128, 0, None) == -1 and b"aligned" in lib.kvz_last_error()
    assert lib.kvz_attn_merge_lse(16, 16, 16, 16, 16, 0, 128, 0, None) == 0      # nothing to do, nothing launched


def test_fork_workspace_bytes():
    lib = _lib()
    w = lib.kvz_fork_attn_workspace_bytes
    assert w(2, 4, 7, 128, 131104) > 0
    assert w(2, 4, 7, 128, 131104) == w(2, 4, 7, 128, 0) == w(2, 4, 7, 128, 5)     # no dependence on the key lengths
    assert w(0, 4, 7, 128, 100) == 0
    assert w(9, 4, 7, 128, 0) > w(2, 4, 7, 128, 0)                                  # four row tiles of partials, not one
    # at least the partial results of one item per CU-sized launch: [items][row tiles x 16][D + 2] floats
    assert w(2, 4, 7, 128, 0) >= 64 * 16 * (128 + 2) * 4


def test_fork_items_formula():
    # default knob on 256 CUs: the decode kernel's 252 items less the tail blocks, so that one launch stays within one block per CU
    assert fp.fork_items(0, 2, 4, 7) == 252 - 8
    assert fp.fork_items(0, 9, 4, 7) == 252 - 36
    assert fp.fork_items(0, 1, 1, 64) == 255 - 2          # one branch of 64 rows: two tail blocks
    assert fp.fork_items(16, 9, 4, 7) == 16               # a small knob is taken as it is
    assert fp.fork_items(0, 16, 64, 4) == 64              # never below a quarter of the CUs


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_probe_expectations(dtype):
    """The uniform probe's expectation is the key count it claims, the marks sit on distinct dims, and one key of the wrong branch
    or one tail row too many moves the expectation by whole 16-bit steps."""
    lens, B, G, D = [5, 70, 300], 3, 7, 128
    c = fp.uniform_case(lens, B, G, D, dtype, tail_len=[0, 37, -1], tail_cap=64)
    e = fp.expected_out(c).float()
    assert e.shape == (B, 3, G, D) and bool((e[2] == 0).all())                     # inactive branch: zeros
    for b, t in ((0, 0), (1, 37)):
        for h, n in enumerate(lens):
            l = np.float32(n + t + 1)
            want = lambda x: float(torch.tensor(np.float32(x) / l).to(dtype))  # noqa: E731
            assert float(e[b, h, 0, D - 2]) == want(1)                              # the new row, once
            assert float(e[b, h, 0, D - 3]) == want(t)                              # the old tail rows
            assert float(e[b, h, 0, D - 1]) == want((b + 1) * (t + 1))             # ... all of THIS branch
    # a fault model: branch 1 reads one row more of its tail (an unused row: SLACK_VALUE), or branch 0's new row on top of its own
    c2 = fp.uniform_case(lens, B, G, D, dtype, tail_len=[0, 37, -1], tail_cap=64)
    c2.tail_len[1] = 38
    e2 = fp.expected_out(c2)
    assert int(ap.steps(e2[1], fp.expected_out(c)[1]).max()) >= 4
    tk, tv = fp.expected_tails(c)
    assert torch.equal(tk[2], c.tail_k[2]) and torch.equal(tv[1, :, 37], c.v_new[1, :, 0]) and torch.equal(tv[1, :, 38:], c.tail_v[1, :, 38:])


def test_weighted_probe_sums_are_exact():
    c = fp.weighted_case([5, 700, 130], 2, 4, 64, torch.float16, tail_len=[1, 31], tail_cap=32)
    e = fp.expected_out(c)     # (finalize asserts that every sum is exact in fp32)
    assert e.shape == (2, 3, 4, 64) and bool(torch.isfinite(e.float()).all())
    k, v, starts, lens = fp.concat_for_oracle(c, 1)
    assert lens == [5 + 32, 700 + 32, 130 + 32] and k.shape[0] == sum(lens) and starts == [0, 37, 37 + 732]
