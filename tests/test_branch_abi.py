"""CPU: the entry point of include/kvzip_hip_branch.h (moving tail rows between the branch slots of a fork) is exported and bound, and
validates its arguments on the host before any launch (no compute calls: there is no GPU here)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = "kvzip_hip_branch.h"
EINVAL, EUNSUPPORTED = -1, -4


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
    assert syms == ["kvz_fork_branch_copy"]
    lib = C.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/{HEADER} but not exported"
    assert sorted(_lib.BRANCH_SIGNATURES) == syms
    assert not set(_lib.BRANCH_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.MULTI_SIGNATURES)
                                              | set(_lib.PREFILL_SIGNATURES) | set(_lib.MULTI_PREFILL_SIGNATURES))
    bound = _lib.load()
    for s, (res, args) in _lib.BRANCH_SIGNATURES.items():
        assert getattr(bound, s).argtypes == args and getattr(bound, s).restype == res


def test_other_headers_are_untouched_by_the_new_entry_point():
    for h in ("kvzip_hip.h", "kvzip_hip_tighten.h", "kvzip_hip_multi.h", "kvzip_hip_prefill.h", "kvzip_hip_multi_prefill.h",
              "kvzip_hip_debug.h"):
        assert "kvz_fork_branch" not in open(os.path.join(ROOT, "include", h)).read()
    from kvzip_amd import _lib
    assert _lib.load().kvz_abi_version() == _lib.ABI_VERSION == 6


def test_library_without_the_symbol_asks_for_a_rebuild(monkeypatch):
    """Same ABI version, older build: load() must say "rebuild" and name the header, not die with an AttributeError."""
    from kvzip_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.BRANCH_SIGNATURES, "kvz_fork_branch_entry_point_of_a_newer_header", (C.c_int, []))
    with pytest.raises(_lib.KvzError, match=r"kvzip_hip_branch\.h.*rebuild"):
        _lib.load()
    assert _lib._lib is None


def _call(lib, L=3, caps=(8, 40, 40), B=5, Hkv=3, D=128, elem=2, pairs=((0, 1),), rows=(1,), kp=4096, vp=8192, null=(), kp_at=None):
    k = (C.c_void_p * L)(*([kp] * L))
    v = (C.c_void_p * L)(*([vp] * L))
    if kp_at is not None:
        k[kp_at[0]] = kp_at[1]
    cap = (C.c_int32 * L)(*caps[:L])
    n = max(len(pairs), 1)
    a = dict(k=k, v=v, cap=cap, src=(C.c_int32 * n)(*[s for s, _ in pairs]), dst=(C.c_int32 * n)(*[d for _, d in pairs]),
             rows=(C.c_int32 * n)(*rows))
    for name in null:
        a[name] = None
    return lib.kvz_fork_branch_copy(a["k"], a["v"], a["cap"], L, B, Hkv, D, elem, a["src"], a["dst"], a["rows"], len(pairs), None)


def test_argument_validation_without_gpu():
    """Every refusal of the header comes before any launch (the addresses here are made up: nothing is dereferenced on a device),
    and so do the two no-ops."""
    from kvzip_amd import _lib
    lib = _lib.load()
    err = lib.kvz_last_error
    for name in ("k", "v", "cap", "src", "dst", "rows"):
        assert _call(lib, null=(name,)) == EINVAL and b"null pointer" in err(), name
    assert _call(lib, kp_at=(1, None)) == EINVAL and b"layer 1" in err()
    assert _call(lib, kp_at=(2, 4096 + 8)) == EINVAL and b"layer 2" in err() and b"aligned" in err()
    assert _call(lib, L=0) == EINVAL and b"bad shape" in err()
    assert _call(lib, B=0) == EINVAL and b"bad shape" in err()
    assert _call(lib, pairs=((5, 1),)) == EINVAL and b"outside [0, 5)" in err()
    assert _call(lib, pairs=((0, -1),)) == EINVAL and b"outside [0, 5)" in err()
    assert _call(lib, pairs=((2, 2),)) == EINVAL and b"onto itself" in err()
    assert _call(lib, pairs=((0, 1), (1, 2)), rows=(1, 1)) == EINVAL and b"both a source and a destination" in err()
    assert _call(lib, pairs=((1, 2), (0, 1)), rows=(1, 1)) == EINVAL and b"both a source and a destination" in err()
    assert _call(lib, pairs=((0, 2), (1, 2)), rows=(1, 1)) == EINVAL and b"destination twice" in err()
    assert _call(lib, rows=(-1,)) == EINVAL and b"rows[0] = -1" in err()
    assert _call(lib, rows=(9,)) == EINVAL and b"capacity 8" in err()                 # fits layers 1 and 2, not layer 0
    assert _call(lib, rows=(33,)) == EINVAL and b"capacity 8" in err()
    assert _call(lib, D=4) == EUNSUPPORTED and b"multiple of 16" in err()              # 8 bytes per row
    assert _call(lib, D=100, elem=1) == EUNSUPPORTED and b"multiple of 16" in err()
    assert _call(lib, B=17) == EUNSUPPORTED and b"B <= 16" in err()
    assert _call(lib, Hkv=65) == EUNSUPPORTED and b"Hkv <= 64" in err()
    with pytest.raises(_lib.KvzError, match="onto itself"):
        _lib.check(_call(lib, pairs=((2, 2),)), "kvz_fork_branch_copy")
    # nothing to move: success, nothing launched (there is no device here)
    assert _call(lib, pairs=(), rows=()) == 0
    assert _call(lib, pairs=(), rows=(), null=("src", "dst", "rows")) == 0
    assert _call(lib, pairs=((0, 1), (0, 2), (3, 4)), rows=(0, 0, 0)) == 0
