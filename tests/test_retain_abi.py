"""CPU: the entry points of the indexed attention of RetainCache (include/kvzip_hip_retain.h) are exported and bound, and validate
their arguments on the host before any launch (no compute calls: there is no GPU here)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = "kvzip_hip_retain.h"
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    lib = os.path.join(ROOT, "kvzip_amd", "libkvzip_hip.so")
    if not os.path.exists(lib):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "kvzip_amd", "csrc"), "-j8"])
    assert os.path.exists(lib)


def _declared_symbols(header=HEADER):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(kvz_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    from kvzip_amd import _lib
    syms = _declared_symbols()
    assert syms == ["kvz_retain_attn", "kvz_retain_attn_append", "kvz_retain_attn_workspace_bytes", "kvz_retain_index",
                    "kvz_retain_index_heads"]
    lib = C.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/{HEADER} but not exported"
    assert sorted(_lib.RETAIN_SIGNATURES) == syms
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.MULTI_SIGNATURES) | set(_lib.PREFILL_SIGNATURES)
              | set(_lib.MULTI_PREFILL_SIGNATURES) | set(_lib.BRANCH_SIGNATURES) | set(_lib.SPEC_SIGNATURES))
    assert not set(_lib.RETAIN_SIGNATURES) & others
    bound = _lib.load()
    for s, (res, args) in _lib.RETAIN_SIGNATURES.items():
        assert getattr(bound, s).argtypes == args and getattr(bound, s).restype == res


def test_other_headers_are_untouched_by_the_new_entry_points():
    inc = os.path.join(ROOT, "include")
    for h in sorted(os.listdir(inc)):
        if h != HEADER:
            assert "kvz_retain" not in open(os.path.join(inc, h)).read(), h
    from kvzip_amd import _lib
    assert _lib.load().kvz_abi_version() == _lib.ABI_VERSION == 6


def test_library_without_the_symbols_asks_for_a_rebuild(monkeypatch):
    """Same ABI version, older build: load() must say "rebuild" and name the header, not die with an AttributeError."""
    from kvzip_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.RETAIN_SIGNATURES, "kvz_retain_entry_point_of_a_newer_header", (C.c_int, []))
    with pytest.raises(_lib.KvzError, match=r"kvzip_hip_retain\.h.*rebuild"):
        _lib.load()
    assert _lib._lib is None


def test_workspace_bytes_equal_the_decode_kernels():
    from kvzip_amd import _lib
    lib = _lib.load()
    w, wv = lib.kvz_retain_attn_workspace_bytes, lib.kvz_varlen_attn_workspace_bytes
    assert w(0, 7, 1, 128) == 0 and w(4, 0, 1, 128) == 0 and w(4, 7, 0, 128) == 0 and w(4, 7, 1, 0) == 0 and w(-1, 7, 1, 128) == 0
    for Hkv in (1, 4, 8, 64):
        for G in (1, 4, 7):
            for q_len in (1, 3, 9):
                for D in (64, 128):
                    assert w(Hkv, G, q_len, D) == wv(Hkv, G, q_len, D, 0) > 0, (Hkv, G, q_len, D)
    # beyond the row count at which kvz_varlen_attn hands over to the multi-row kernel these calls take nothing
    assert w(4, 7, 9, 128) > 0 and w(4, 7, 10, 128) == 0 and w(4, 1, 64, 128) > 0 and w(4, 1, 65, 128) == 0


def _meta(Hkv, starts=None, counts=None):
    return (C.c_int32 * (2 * Hkv))(*(starts if starts is not None else [100 * i for i in range(Hkv)]),
                                   *(counts if counts is not None else [100] * Hkv))


def _attn(lib, Hkv=4, G=7, q_len=1, D=128, q=16, k=16, v=16, head_stride=None, capacity=2048, idx=16, idx_len=1000, meta="ok",
          starts=None, counts=None, ctx_end=1000, fill=1010, out=16, ws=16, ws_bytes=1 << 30, dtype=0):
    mh = _meta(Hkv, starts, counts) if meta == "ok" else None
    hs = capacity * D if head_stride is None else head_stride   # (made-up device addresses: nothing is dereferenced before a launch)
    return lib.kvz_retain_attn(q, k, v, hs, capacity, idx, idx_len, mh, ctx_end, fill, Hkv, G, q_len, D, 0.1, 1, dtype, out, ws, ws_bytes,
                               None)


def _append(lib, Hkv=4, G=7, D=128, q=16, k=16, v=16, head_stride=None, capacity=2048, kn=16, vn=16, kn_stride=128, vn_stride=128,
            idx=16, idx_len=1000, meta="ok", starts=None, counts=None, ctx_end=1000, fill=1010, out=16, ws=16, ws_bytes=1 << 30, dtype=0):
    mh = _meta(Hkv, starts, counts) if meta == "ok" else None
    hs = capacity * D if head_stride is None else head_stride
    return lib.kvz_retain_attn_append(q, k, v, hs, capacity, kn, vn, kn_stride, vn_stride, idx, idx_len, mh, ctx_end, fill, Hkv, G, D, 0.1,
                                      dtype, out, ws, ws_bytes, None)


def test_attention_argument_validation_without_gpu():
    """Bad arguments are rejected on the host before any launch (error code + a telling message); nothing here is dereferenced on a
    device."""
    from kvzip_amd import _lib
    lib = _lib.load()
    err = lib.kvz_last_error
    for call, who, ptrs in ((_attn, b"kvz_retain_attn:", ("q", "k", "v", "idx", "out", "ws")),
                            (_append, b"kvz_retain_attn_append:", ("q", "k", "v", "kn", "vn", "idx", "out", "ws"))):
        for name in ptrs:
            assert call(lib, **{name: None}) == EINVAL and b"null pointer" in err() and who in err(), name
        assert call(lib, meta="none") == EINVAL and b"null pointer" in err()
        for name in ptrs:
            bad = 18 if name == "idx" else 24        # (the index holds 4-byte entries; everything else moves in 16-byte vectors)
            assert call(lib, **{name: bad}) == EINVAL and b"aligned" in err(), name
        assert call(lib, head_stride=2048 * 128 + 4) == EINVAL and b"multiple of 8" in err()
        assert call(lib, head_stride=2047 * 128) == EINVAL and b"hold capacity" in err()
        assert call(lib, Hkv=0) == EINVAL and b"bad shape" in err()
        assert call(lib, G=0) == EINVAL and b"bad shape" in err()
        assert call(lib, dtype=3) == EINVAL and b"dtype" in err()
        assert call(lib, ctx_end=-1) == EINVAL and b"ctx_end = -1" in err()
        assert call(lib, idx_len=0) == EINVAL and b"idx_len = 0" in err()
        assert call(lib, counts=[100, 100, -1, 100]) == EINVAL and b"head 2" in err() and b"negative" in err()
        assert call(lib, starts=[0, -4, 200, 300]) == EINVAL and b"head 1" in err() and b"negative" in err()
        assert call(lib, starts=[0, 100, 200, 901]) == EINVAL and b"head 3" in err()                 # start + count > idx_len
        assert call(lib, counts=[100, 1001, 100, 100], idx_len=5000) == EINVAL and b"head 1" in err()    # count > ctx_end
        assert call(lib, D=96) == EUNSUPPORTED and b"head_dim 96" in err()
        assert call(lib, Hkv=65) == EUNSUPPORTED and b"Hkv <= 64" in err()
        assert call(lib, G=65) == EUNSUPPORTED and b"q_len*G <= 64" in err()
        assert call(lib, ws_bytes=64) == EWORKSPACE and b"workspace too small" in err()
        need = lib.kvz_retain_attn_workspace_bytes(4, 7, 1, 128)
        assert call(lib, ws_bytes=need - 1) == EWORKSPACE and b"workspace too small" in err()
    # q_len > 0, and q_len * G within the decode kernel's rows
    assert _attn(lib, q_len=0) == EINVAL and b"bad shape" in err()
    assert _attn(lib, q_len=10, fill=1010) == EUNSUPPORTED and b"q_len*G <= 64" in err()
    # fill: the rows of the query positions are in the store (plain form) / the context is (append form); the new row must fit
    assert _attn(lib, q_len=3, fill=1002) == EINVAL and b"fill = 1002" in err()
    assert _attn(lib, q_len=1, fill=1000) == EINVAL and b"fill = 1000" in err()
    assert _attn(lib, fill=2049) == EINVAL and b"exceeds capacity" in err()
    assert _append(lib, fill=999) == EINVAL and b"fill = 999" in err()
    assert _append(lib, fill=2048) == EINVAL and b"exceeds capacity = 2048" in err()
    for name in ("kn_stride", "vn_stride"):
        assert _append(lib, **{name: 132}) == EINVAL and b"multiples of 8" in err(), name
    with pytest.raises(_lib.KvzError, match="head_dim"):
        _lib.check(_attn(lib, D=96), "kvz_retain_attn")


def test_index_argument_validation_without_gpu():
    from kvzip_amd import _lib
    lib = _lib.load()
    err = lib.kvz_last_error
    for fn, who in ((lib.kvz_retain_index, b"kvz_retain_index:"), (lib.kvz_retain_index_heads, b"kvz_retain_index_heads:")):
        def call(valid=16, layers=2, Hkv=3, N=100, sink=5, tile_base=16, row_start=16, idx=16, idx_len=100):
            return fn(valid, layers, Hkv, N, sink, tile_base, row_start, idx, idx_len, None)
        for name in ("valid", "tile_base", "row_start", "idx"):
            assert call(**{name: None}) == EINVAL and b"null pointer" in err() and who in err(), name
        for name in ("tile_base", "row_start", "idx"):
            assert call(**{name: 18}) == EINVAL and b"aligned" in err(), name
        assert call(layers=0) == EINVAL and b"bad shape" in err()
        assert call(Hkv=0) == EINVAL and b"bad shape" in err()
        assert call(layers=300, Hkv=300) == EINVAL and b"bad shape" in err()
        assert call(N=-1) == EINVAL and b"bad context" in err()
        assert call(sink=-1) == EINVAL and b"bad context" in err()
        assert call(N=0, sink=0) == EINVAL and b"bad context" in err()
        assert call(idx_len=-1) == EINVAL and b"idx_len = -1" in err()


def test_retain_cache_flag_and_index_bookkeeping_on_the_host():
    """``indexed`` is a constructor flag (default on) that reaches the cache through cache_kwargs; without an index (never pruned, a
    replaced mask, adopt_dense) the cache says it does not take the indexed route."""
    import types
    import torch
    from kvzip_amd.kvcache import RetainCache
    cfg = types.SimpleNamespace(num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2)
    kv = RetainCache(cfg, (0, 16), device="cpu", dtype=torch.float16, verbose=False)
    assert kv.indexed is True and kv._index is None
    assert RetainCache(cfg, (0, 16), device="cpu", dtype=torch.float16, verbose=False, indexed=False).indexed is False
    q = torch.zeros(1, 8, 1, 64, dtype=torch.float16)
    assert not kv.index_takes(q)
    kv.pruned, kv.valid = True, torch.ones(2, 1, 2, 16, dtype=torch.bool)
    kv._index, kv._index_valid = object(), kv.valid
    assert not kv.index_takes(q)                      # (a CPU tensor: the kernels run on the device only)
    kv.valid = kv.valid.clone()                       # somebody replaced the mask: the index is not of this mask any more
    assert kv._index_valid is not kv.valid and not kv.index_takes(q)
    kv.adopt_dense([torch.zeros(1, 2, 32, 64)] * 2, [torch.zeros(1, 2, 32, 64)] * 2, 16)
    assert kv._index is None and kv._index_valid is None
