"""CPU: the entry points of the verify step of speculative decoding (include/kvzip_hip_spec.h) are exported and bound, and validate
their arguments on the host before any launch (no compute calls: there is no GPU here)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = "kvzip_hip_spec.h"
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
    assert syms == ["kvz_spec_attn_append", "kvz_spec_attn_workspace_bytes"]
    lib = C.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/{HEADER} but not exported"
    assert sorted(_lib.SPEC_SIGNATURES) == syms
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.MULTI_SIGNATURES) | set(_lib.PREFILL_SIGNATURES)
              | set(_lib.MULTI_PREFILL_SIGNATURES) | set(_lib.BRANCH_SIGNATURES))
    assert not set(_lib.SPEC_SIGNATURES) & others
    bound = _lib.load()
    for s, (res, args) in _lib.SPEC_SIGNATURES.items():
        assert getattr(bound, s).argtypes == args and getattr(bound, s).restype == res


def test_other_headers_are_untouched_by_the_new_entry_points():
    inc = os.path.join(ROOT, "include")
    for h in sorted(os.listdir(inc)):
        if h != HEADER:
            assert "kvz_spec" not in open(os.path.join(inc, h)).read(), h
    from kvzip_amd import _lib
    assert _lib.load().kvz_abi_version() == _lib.ABI_VERSION == 6


def test_library_without_the_symbols_asks_for_a_rebuild(monkeypatch):
    """Same ABI version, older build: load() must say "rebuild" and name the header, not die with an AttributeError."""
    from kvzip_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.SPEC_SIGNATURES, "kvz_spec_entry_point_of_a_newer_header", (C.c_int, []))
    with pytest.raises(_lib.KvzError, match=r"kvzip_hip_spec\.h.*rebuild"):
        _lib.load()
    assert _lib._lib is None


def test_workspace_bytes():
    from kvzip_amd import _lib
    w = _lib.load().kvz_spec_attn_workspace_bytes
    assert w(0, 4, 7, 128) == 0 and w(-1, 4, 7, 128) == 0 and w(2, 0, 7, 128) == 0 and w(2, 4, 0, 128) == 0 and w(2, 4, 7, 0) == 0
    # at least the partial results of one item per CU-sized launch and of the triangles: [items][16 rows][D + 2] floats
    assert w(2, 4, 7, 128) >= (256 + 4) * 16 * (128 + 2) * 4
    assert w(4, 4, 7, 128) > w(2, 4, 7, 128)                  # two row tiles of partials, not one
    assert w(4, 4, 7, 128) == w(3, 4, 7, 128)                 # (it depends on the number of row tiles, on no key length)


def _call(lib, t=4, Hkv=4, G=7, D=128, slack=8, offset=0, meta="both", starts=None, lens=None, q=16, kc=16, vc=16, kn=16, vn=16, out=16,
          ws=16, ws_bytes=1 << 30, dtype=0, strides=None):
    mh = None
    if meta in ("both", "host"):
        mh = (C.c_int32 * (2 * Hkv))(*(starts if starts is not None else [1000 * i for i in range(Hkv)]),
                                     *(lens if lens is not None else [10] * Hkv))
    dev = 32 if meta in ("both", "device") else None          # (made-up device addresses: nothing is dereferenced before a launch)
    st = strides if strides is not None else (t * D, D, D, Hkv * D)
    return lib.kvz_spec_attn_append(q, kc, vc, dev, dev, offset, mh, slack, kn, vn, st[0], st[1], st[2], st[3], t, Hkv, G, D, 0.1, dtype,
                                    out, ws, ws_bytes, None)


def test_argument_validation_without_gpu():
    """Bad arguments are rejected on the host before any launch (error code + a telling message); nothing here is dereferenced on a
    device."""
    from kvzip_amd import _lib
    lib = _lib.load()
    err = lib.kvz_last_error
    for name in ("q", "kc", "vc", "kn", "vn", "out", "ws"):
        assert _call(lib, **{name: None}) == EINVAL and b"null pointer" in err(), name
    assert _call(lib, meta="none") == EINVAL and b"no segment metadata" in err()
    for name in ("q", "kc", "vc", "kn", "vn", "out", "ws"):
        assert _call(lib, **{name: 24}) == EINVAL and b"aligned" in err(), name
    for i in range(4):
        st = [4 * 128, 128, 128, 4 * 128]
        st[i] += 4
        assert _call(lib, strides=st) == EINVAL and b"multiples of 8" in err(), i
    assert _call(lib, t=0) == EINVAL and b"t = 0" in err()
    assert _call(lib, t=-3) == EINVAL and b"t = -3" in err()
    assert _call(lib, offset=-1) == EINVAL and b"k_len_offset = -1" in err()
    assert _call(lib, t=4, offset=5, slack=8) == EINVAL and b"exceeds slack = 8" in err()
    assert _call(lib, t=4, offset=4, slack=8) != EINVAL or b"slack" not in err()       # (the limit itself passes this check)
    assert _call(lib, Hkv=0) == EINVAL and b"bad shape" in err()
    assert _call(lib, dtype=3) == EINVAL and b"dtype" in err()
    assert _call(lib, lens=[10, 10, -1, 10]) == EINVAL and b"head 2" in err()
    assert _call(lib, D=96) == EUNSUPPORTED and b"head_dim 96" in err()
    assert _call(lib, Hkv=65, slack=8) == EUNSUPPORTED and b"Hkv <= 64" in err()
    assert _call(lib, t=10, G=7, slack=16) == EUNSUPPORTED and b"t*G <= 64" in err()
    assert _call(lib, t=1, G=65) == EUNSUPPORTED and b"t*G <= 64" in err()
    assert _call(lib, ws_bytes=64) == EWORKSPACE and b"workspace too small" in err()
    need = lib.kvz_spec_attn_workspace_bytes(4, 4, 7, 128)
    assert _call(lib, ws_bytes=need - 1) == EWORKSPACE and b"workspace too small" in err()
    with pytest.raises(_lib.KvzError, match="head_dim"):
        _lib.check(_call(lib, D=96), "kvz_spec_attn_append")


def test_rewind_and_verifying_are_host_bookkeeping():
    """EvictCache.rewind decrements every layer's offset and the token count, refuses more than was appended and a packed-layout or
    dense cache; verifying() is a flag that is set only inside the block."""
    import types
    import torch
    from kvzip_amd.kvcache import EvictCache
    from kvzip_amd.ops import KvzError
    cfg = types.SimpleNamespace(num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2)

    def cache(layout="slack", pruned=True):
        kv = EvictCache(cfg, (0, 16), device="cpu", dtype=torch.float16, layout=layout, verbose=False)
        if pruned:
            kv.pruned = True
            kv.info = {"flatten": True, "layout": layout, "offset": [5, 5]}
            kv._seen_tokens = 21
        return kv
    kv = cache()
    kv.rewind(0)
    kv.rewind(3)
    assert kv.info["offset"] == [2, 2] and kv._seen_tokens == 18
    with pytest.raises(KvzError, match="rewind: 3 positions, but 2"):
        kv.rewind(3)
    with pytest.raises(KvzError, match="rewind"):
        kv.rewind(-1)
    assert kv.info["offset"] == [2, 2] and kv._seen_tokens == 18
    kv.rewind(2)
    assert kv.info["offset"] == [0, 0] and kv._seen_tokens == 16
    with pytest.raises(KvzError, match="slack-layout"):
        cache(layout="packed").rewind(1)
    with pytest.raises(KvzError, match="slack-layout"):
        cache(pruned=False).rewind(1)
    assert not getattr(kv, "_verifying", False)
    with kv.verifying():
        assert kv._verifying
    assert not kv._verifying


def test_generate_speculative_refuses_sampling_and_other_caches():
    import types
    import torch
    from kvzip_amd.kvcache import EvictCache
    from kvzip_amd.wrapper import ModelKVzip
    m = ModelKVzip.__new__(ModelKVzip)      # (the checks need neither a model nor a device)
    m.device = torch.device("cpu")
    m.config = types.SimpleNamespace(num_hidden_layers=2, num_attention_heads=28, num_key_value_heads=4)
    fn = ModelKVzip.generate_speculative.__wrapped__.__wrapped__
    m.gen_kwargs = {"do_sample": True}
    with pytest.raises(ValueError, match="greedy"):
        fn(m, torch.zeros(1, 3, dtype=torch.long), None)
    m.gen_kwargs = {"do_sample": False, "max_new_tokens": 4}
    dense = EvictCache(m.config, (0, 16), device="cpu", dtype=torch.float16, verbose=False)
    with pytest.raises(ValueError, match="use generate"):
        fn(m, torch.zeros(1, 3, dtype=torch.long), dense)
    # the draft length: 32 // G - 1 by default (t*G <= 32), a request capped at 64 // G - 1
    assert m._draft_len() == 3 and m._draft_len(100) == 8 and m._draft_len(2) == 2 and m._draft_len(0) == 0
    m.config = types.SimpleNamespace(num_attention_heads=32, num_key_value_heads=8)
    assert m._draft_len() == 7 and m._draft_len(100) == 15
