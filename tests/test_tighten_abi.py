"""CPU: the entry points for tightening a pruned cache (include/kvzip_hip_tighten.h) are exported and bound, validate their
arguments on the host, and ModelKVzip.eval_ratios_evict refuses rising ratios before it touches the cache (no compute calls:
there is no GPU here)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = "kvzip_hip_tighten.h"


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    lib = os.path.join(ROOT, "kvzip_amd", "libkvzip_hip.so")
    if not os.path.exists(lib):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "kvzip_amd", "csrc"), "-j8"])
    assert os.path.exists(lib)


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(kvz_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    from kvzip_amd import _lib
    syms = _declared_symbols()
    assert syms == ["kvz_mask_resurrects", "kvz_recompact_layers"]
    assert not [s for s in syms if s.startswith("kvz_debug_")]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/{HEADER} but not exported"
    assert sorted(_lib.EXT_SIGNATURES) == syms
    assert not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)
    bound = _lib.load()
    for s, (res, args) in _lib.EXT_SIGNATURES.items():
        assert getattr(bound, s).argtypes == args and getattr(bound, s).restype == res


def test_main_header_is_untouched_by_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "kvzip_hip.h")).read()
    assert "kvz_recompact" not in text and "kvz_mask_resurrects" not in text
    from kvzip_amd import _lib
    assert _lib.load().kvz_abi_version() == _lib.ABI_VERSION == 6


def test_library_without_the_symbols_asks_for_a_rebuild(monkeypatch):
    """Same ABI version, older build: load() must say "rebuild", not die with an AttributeError."""
    from kvzip_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.EXT_SIGNATURES, "kvz_entry_point_of_a_newer_header", (ctypes.c_int, []))
    with pytest.raises(_lib.KvzError, match="rebuild"):
        _lib.load()
    assert _lib._lib is None


def _recompact_args(**over):
    p = 4096  # never dereferenced: validation fails first
    a = dict(k_ptrs=p, v_ptrs=p, old_valid=p, old_tok1=1, old_tile_base=p, old_seg_start=p, old_len_k=p, new_valid=p, new_tok1=1,
             new_tile_base=p, new_seg_start=p, new_len_k=p, tail_rows=None, layers=2, Hkv=3, N=100, sink=4, klen=104, D=64, elem_bytes=2,
             k_out_ptrs=p, v_out_ptrs=p, stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("over,word", [
    (dict(k_ptrs=None), b"null pointer"),
    (dict(new_len_k=None), b"null pointer"),
    (dict(v_out_ptrs=None), b"null pointer"),
    (dict(D=12, elem_bytes=2), b"D*elem_bytes = 24"),
    (dict(D=1024, elem_bytes=2), b"D*elem_bytes = 2048"),
    (dict(layers=0), b"bad shape"),
    (dict(Hkv=0), b"bad shape"),
    (dict(N=0), b"bad shape"),
    (dict(klen=103), b"klen"),
])
def test_recompact_argument_validation_without_gpu(over, word):
    from kvzip_amd import _lib
    lib = _lib.load()
    rc = lib.kvz_recompact_layers(*_recompact_args(**over))
    assert rc == -1 and word in lib.kvz_last_error(), (rc, lib.kvz_last_error())
    with pytest.raises(_lib.KvzError):
        _lib.check(rc, "kvz_recompact_layers")


@pytest.mark.parametrize("args,word", [
    ((None, 1, 4096, 1, 6, 100, 4096, None), b"null pointer"),
    ((4096, 1, 4096, 1, 6, 100, None, None), b"null pointer"),
    ((4096, 1, 4096, 1, 0, 100, 4096, None), b"bad shape"),
    ((4096, 1, 4096, 1, 6, 0, 4096, None), b"bad shape"),
])
def test_mask_resurrects_argument_validation_without_gpu(args, word):
    from kvzip_amd import _lib
    lib = _lib.load()
    rc = lib.kvz_mask_resurrects(*args)
    assert rc == -1 and word in lib.kvz_last_error(), (rc, lib.kvz_last_error())


class _StubCache:
    def __init__(self):
        self.calls = []

    def prune(self, ratio, level="pair"):
        self.calls.append((ratio, level))
        raise RuntimeError("the cache was used")


def test_eval_ratios_evict_rejects_rising_ratios_before_using_the_cache():
    from kvzip_amd.wrapper import ModelKVzip
    m = ModelKVzip.__new__(ModelKVzip)      # (the check needs neither a model nor a device)
    kv = _StubCache()
    with pytest.raises(ValueError, match="non-increasing"):
        m.eval_ratios_evict(kv, [0.3, 0.5], lambda c: None)
    with pytest.raises(ValueError, match="non-increasing"):
        m.eval_ratios_evict(kv, iter([0.9, 0.3, 0.5]), lambda c: None)
    assert kv.calls == []
    with pytest.raises(RuntimeError, match="the cache was used"):   # falling (and equal) ratios do reach the cache
        m.eval_ratios_evict(kv, [0.5, 0.5, 0.3], lambda c: None, level="head")
    assert kv.calls == [(0.5, "head")]
