"""CPU: the entry points of the batched decode over several independent caches (include/kvzip_hip_multi.h) are exported and bound,
validate their arguments on the host before any launch, and kvcache.CacheBatch refuses what it cannot batch (no compute calls: there
is no GPU here)."""
import ctypes as C
import os
import re
import types

import pytest
import torch

import multi_probes as mp
from conftest import ROOT

HEADER = "kvzip_hip_multi.h"
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
    assert syms == ["kvz_multi_attn_append", "kvz_multi_attn_workspace_bytes"]
    lib = C.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/{HEADER} but not exported"
    assert sorted(_lib.MULTI_SIGNATURES) == syms
    assert not set(_lib.MULTI_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES))
    bound = _lib.load()
    for s, (res, args) in _lib.MULTI_SIGNATURES.items():
        assert getattr(bound, s).argtypes == args and getattr(bound, s).restype == res


def test_main_header_is_untouched_by_the_new_entry_points():
    for h in ("kvzip_hip.h", "kvzip_hip_tighten.h"):
        assert "kvz_multi" not in open(os.path.join(ROOT, "include", h)).read()
    from kvzip_amd import _lib
    assert _lib.load().kvz_abi_version() == _lib.ABI_VERSION == 6


def test_library_without_the_symbols_asks_for_a_rebuild(monkeypatch):
    """Same ABI version, older build: load() must say "rebuild" and name the header, not die with an AttributeError."""
    from kvzip_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.MULTI_SIGNATURES, "kvz_multi_entry_point_of_a_newer_header", (C.c_int, []))
    with pytest.raises(_lib.KvzError, match=r"kvzip_hip_multi\.h.*rebuild"):
        _lib.load()
    assert _lib._lib is None


def test_workspace_bytes():
    from kvzip_amd import _lib
    w = _lib.load().kvz_multi_attn_workspace_bytes
    assert w(0, 4, 7, 128) == 0 and w(-1, 4, 7, 128) == 0 and w(2, 0, 7, 128) == 0
    # at least the partial results of one item per CU-sized launch: [items][16 rows][D + 2] floats
    assert w(2, 4, 7, 128) >= 256 * 16 * (128 + 2) * 4
    assert w(2, 4, 20, 128) > w(2, 4, 7, 128)                  # two row tiles of partials, not one
    assert w(16, 8, 7, 128) >= (128 + 64) * 16 * (128 + 2) * 4  # 128 segments: a quarter of the CUs of items + one per segment


def _call(lib, B=2, Hkv=4, G=7, D=128, slack=8, offset=None, starts=None, lens=None, q=16, kp=16, vp=16, kn=16, out=16, ws=16,
          ws_bytes=1 << 30, dtype=0, kn_stride=None, null=()):
    n = max(B, 1)
    k_ptrs = (C.c_void_p * n)(*([kp] * n))
    v_ptrs = (C.c_void_p * n)(*([vp] * n))
    seg = (C.c_int32 * (n * Hkv))(*(starts if starts is not None else [1000 * i for i in range(n * Hkv)]))
    ln = (C.c_int32 * (n * Hkv))(*(lens if lens is not None else [10] * (n * Hkv)))
    sl = (C.c_int32 * n)(*([slack] * n))
    off = (C.c_int32 * n)(*(offset if offset is not None else [0] * n))
    args = dict(q=q, k_ptrs=k_ptrs, v_ptrs=v_ptrs, seg=seg, ln=ln, sl=sl, off=off, kn=kn, vn=kn)
    for name in null:
        args[name] = None
    st = kn_stride if kn_stride is not None else Hkv * D
    return lib.kvz_multi_attn_append(args["q"], args["k_ptrs"], args["v_ptrs"], args["seg"], args["ln"], args["sl"], args["off"],
                                     args["kn"], args["vn"], st, D, st, D, B, Hkv, G, D, 0.1, dtype, out, ws, ws_bytes, None)


def test_argument_validation_without_gpu():
    """Bad arguments are rejected on the host before any launch (error code + a telling message); nothing here is dereferenced on a
    device."""
    from kvzip_amd import _lib
    lib = _lib.load()
    err = lib.kvz_last_error
    for name in ("q", "k_ptrs", "v_ptrs", "seg", "ln", "sl", "off", "kn"):
        assert _call(lib, null=(name,)) == EINVAL and b"null pointer" in err(), name
    assert _call(lib, out=None) == EINVAL and b"null pointer" in err()
    assert _call(lib, ws=None) == EINVAL and b"null pointer" in err()
    assert _call(lib, kp=None) == EINVAL and b"null K or V pointer of cache 0" in err()
    assert _call(lib, B=0) == EINVAL and b"bad shape" in err()
    assert _call(lib, B=17, Hkv=1) == EUNSUPPORTED and b"17 caches" in err() and b"B <= 16" in err()
    assert _call(lib, B=9, Hkv=16) == EUNSUPPORTED and b"B*Hkv <= 128" in err()          # 144 segments
    assert _call(lib, B=1, Hkv=65) == EUNSUPPORTED and b"Hkv <= 64" in err()
    assert _call(lib, G=65) == EUNSUPPORTED and b"G <= 64" in err()
    assert _call(lib, D=96) == EUNSUPPORTED and b"head_dim 96" in err()
    assert _call(lib, dtype=3) == EINVAL and b"dtype" in err()
    assert _call(lib, q=24) == EINVAL and b"aligned" in err()
    assert _call(lib, vp=24) == EINVAL and b"cache 0" in err() and b"aligned" in err()
    assert _call(lib, kn_stride=4 * 128 + 4) == EINVAL and b"multiples of 8" in err()
    # the new row must fit behind every segment: offset in [-1, slack)
    assert _call(lib, offset=[0, 8]) == EINVAL and b"offset[1] = 8" in err() and b"slack = 8" in err()
    assert _call(lib, offset=[-2, 0]) == EINVAL and b"offset[0] = -2" in err()
    assert _call(lib, lens=[10, 10, -1, 10, 10, 10, 10, 10]) == EINVAL and b"cache 0, head 2" in err()
    assert _call(lib, starts=[0, 10, 20, 2 ** 31 - 12, 0, 10, 20, 30]) == EINVAL and b"cache 0, head 3" in err()
    assert _call(lib, ws_bytes=64) == EWORKSPACE and b"workspace too small" in err()
    need = lib.kvz_multi_attn_workspace_bytes(2, 4, 7, 128)
    assert _call(lib, ws_bytes=need - 1) == EWORKSPACE and b"workspace too small" in err()
    with pytest.raises(_lib.KvzError, match="head_dim"):
        _lib.check(_call(lib, D=96), "kvz_multi_attn_append")


# ---- CacheBatch: what it refuses (host logic only; caches built on the CPU, their state set by hand) --------------------------------------
def _cfg(L=2, H=8, Hkv=2):
    return types.SimpleNamespace(num_hidden_layers=L, num_attention_heads=H, num_key_value_heads=Hkv)


def _pruned(cfg=None, layout="slack", dtype=torch.float16, pruned=True):
    from kvzip_amd.kvcache import EvictCache
    kv = EvictCache(cfg or _cfg(), (0, 16), device="cpu", dtype=dtype, layout=layout, verbose=False)
    if pruned:
        kv.pruned = True
        kv.info = {"flatten": True, "layout": layout, "offset": [0] * kv.n_layers}
    return kv


def test_cache_batch_refuses_what_it_cannot_batch():
    from kvzip_amd.kvcache import CacheBatch, ForkedCache, RetainCache
    from kvzip_amd.ops import KvzError
    ok = CacheBatch([_pruned(), _pruned()])
    assert ok.layout == "multi" and ok.n_caches == 2 and ok.pruned and not ok.get_score and ok.active == [True, True]
    ok.retire(1)
    assert ok.active == [True, False]
    with pytest.raises(KvzError, match="at least one"):
        CacheBatch([])
    with pytest.raises(KvzError, match="not pruned"):
        CacheBatch([_pruned(), _pruned(pruned=False)])
    with pytest.raises(KvzError, match="packed layout"):
        CacheBatch([_pruned(layout="packed"), _pruned()])
    fork = ForkedCache.__new__(ForkedCache)            # (a fork of a pruned cache: refused by what it is)
    with pytest.raises(KvzError, match="ForkedCache"):
        CacheBatch([_pruned(), fork])
    with pytest.raises(KvzError, match="RetainCache"):
        CacheBatch([RetainCache(_cfg(), (0, 16), device="cpu", dtype=torch.float16, verbose=False)])
    with pytest.raises(KvzError, match="geometry"):
        CacheBatch([_pruned(), _pruned(_cfg(Hkv=4))])                   # other KV heads (and other G)
    with pytest.raises(KvzError, match="geometry"):
        CacheBatch([_pruned(), _pruned(_cfg(L=3))])
    with pytest.raises(KvzError, match="geometry"):
        CacheBatch([_pruned(), _pruned(dtype=torch.bfloat16)])
    one = _pruned()
    with pytest.raises(KvzError, match="twice"):
        CacheBatch([one, one])
    with pytest.raises(KvzError, match="at most 16 caches"):
        CacheBatch([_pruned() for _ in range(17)])
    with pytest.raises(KvzError, match="128 segments"):
        CacheBatch([_pruned(_cfg(H=32, Hkv=16)) for _ in range(9)])
    CacheBatch([_pruned(_cfg(H=32, Hkv=16)) for _ in range(8)])        # the limit itself


def test_generate_multi_wants_one_query_per_cache():
    from kvzip_amd.wrapper import ModelKVzip
    m = ModelKVzip.__new__(ModelKVzip)      # (the check needs neither a model nor a device)
    m.device = torch.device("cpu")
    with pytest.raises(ValueError, match="one query per cache"):
        ModelKVzip.generate_multi.__wrapped__.__wrapped__(m, [torch.zeros(1, 3, dtype=torch.long)], [])


def test_probe_expectations():
    """The uniform probe's expectation is the key count it claims, and one key too many, or the new row of another cache, moves it by
    whole 16-bit steps."""
    import attn_probes as ap
    import numpy as np
    lens, off, G, D = [[300, 37], [0, 129]], [0, 5], 7, 128
    for dtype in (torch.float16, torch.bfloat16):
        c = mp.uniform_case(lens, off, G, D, dtype, slack=8, items=(16,))
        e = mp.expected_out(c).float()
        assert c.segment_lengths() == [301, 38, 6, 135]
        for b in range(2):
            for h in range(2):
                l = np.float32(lens[b][h] + off[b] + 1)
                want = lambda x: float(torch.tensor(np.float32(x) / l).to(dtype))  # noqa: E731
                assert float(e[b, h, 0, D - 2]) == want(1)                                  # the new row, once
                assert float(e[b, h, 0, D - 3]) == want(off[b])                             # the rows appended before
                assert float(e[b, h, 0, D - 1]) == want((b + 1) * (off[b] + 1))             # ... all of THIS cache
        c2 = mp.uniform_case(lens, off, G, D, dtype, slack=8, items=(16,))
        c2.offset[1] = 6                                                                    # one slack row read as a key
        assert int(ap.steps(mp.expected_out(c2)[1], mp.expected_out(c)[1]).max()) >= 4
        ek, ev = mp.expected_arenas(c)
        r = c.row0[1] + c.starts[1][1] + 129 + 5
        assert torch.equal(ev[r], c.v_new[1, 1, 0]) and float(c.arena_v[r, 0]) == ap.SLACK_VALUE
        assert int((ek != c.arena_k).any(-1).sum()) <= 4 and int((ev != c.arena_v).any(-1).sum()) == 4
    mp.expected_out(mp.weighted_case(lens, [0, -1], 4, 64, torch.float16))     # (finalize asserts that every sum is exact in fp32)
    inactive = mp.expected_out(mp.uniform_case(lens, [0, -1], G, D, torch.float16))
    assert bool((inactive[1] == 0).all()) and bool((inactive[0] != 0).any())
