"""CPU: the entry points of the packed first step of a forked decode (include/kvzip_hip_prefill.h) are exported and bound, validate
their arguments on the host before any launch, and kvcache.ForkedCache refuses a packing it cannot run (no compute calls: there is
no GPU here)."""
import ctypes as C
import os
import re
import types

import pytest
import torch

import prefill_probes as pp
from conftest import ROOT

HEADER = "kvzip_hip_prefill.h"
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
    assert syms == ["kvz_fork_prefill_tail", "kvz_fork_prefill_workspace_bytes"]
    lib = C.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/{HEADER} but not exported"
    assert sorted(_lib.PREFILL_SIGNATURES) == syms
    assert not set(_lib.PREFILL_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.MULTI_SIGNATURES))
    bound = _lib.load()
    for s, (res, args) in _lib.PREFILL_SIGNATURES.items():
        assert getattr(bound, s).argtypes == args and getattr(bound, s).restype == res


def test_other_headers_are_untouched_by_the_new_entry_points():
    for h in ("kvzip_hip.h", "kvzip_hip_tighten.h", "kvzip_hip_multi.h", "kvzip_hip_debug.h"):
        assert "kvz_fork_prefill" not in open(os.path.join(ROOT, "include", h)).read()
    from kvzip_amd import _lib
    assert _lib.load().kvz_abi_version() == _lib.ABI_VERSION == 6


def test_library_without_the_symbols_asks_for_a_rebuild(monkeypatch):
    """Same ABI version, older build: load() must say "rebuild" and name the header, not die with an AttributeError."""
    from kvzip_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.PREFILL_SIGNATURES, "kvz_fork_prefill_entry_point_of_a_newer_header", (C.c_int, []))
    with pytest.raises(_lib.KvzError, match=r"kvzip_hip_prefill\.h.*rebuild"):
        _lib.load()
    assert _lib._lib is None


def test_workspace_bytes():
    """No workspace: a wave walks the whole tail of its rows (the GPU guard test covers a non-zero size, should one ever come)."""
    from kvzip_amd import _lib
    w = _lib.load().kvz_fork_prefill_workspace_bytes
    assert w(84, 3, 4, 7, 128) == 0 and w(0, 1, 1, 1, 64) == 0


def _call(lib, B=3, Hkv=4, G=7, D=128, cu=None, tl=None, cap=64, q=16, tk=16, tv=16, kn=16, vn=16, osh=16, lse=16, out=16, dtype=0,
          qs=None, kns=None, branch=None, null=()):
    n = max(B, 1)
    cu_q = (C.c_int32 * (n + 1))(*(cu if cu is not None else [5 * i for i in range(n + 1)]))
    tail_len = (C.c_int32 * n)(*(tl if tl is not None else [0] * n))
    br = (C.c_int32 * n)(*branch) if branch is not None else None
    a = dict(q=q, cu=cu_q, tk=tk, tv=tv, tl=tail_len, kn=kn, vn=vn, osh=osh, lse=lse, out=out)
    for name in null:
        a[name] = None
    qs = qs if qs is not None else (G * D, D, Hkv * G * D)
    kns = kns if kns is not None else (D, Hkv * D)
    return lib.kvz_fork_prefill_tail(a["q"], qs[0], qs[1], qs[2], a["cu"], a["tk"], a["tv"], cap, a["tl"], a["kn"], a["vn"], kns[0], kns[1],
                                     kns[0], kns[1], a["osh"], a["lse"], a["out"], br, B, Hkv, G, D, 0.1, dtype, None, 0, None)


def test_argument_validation_without_gpu():
    """Bad arguments are rejected on the host before any launch (error code + a telling message); nothing here is dereferenced on a
    device."""
    from kvzip_amd import _lib
    lib = _lib.load()
    err = lib.kvz_last_error
    for name in ("q", "cu", "tk", "tv", "tl", "kn", "vn", "osh", "lse", "out"):
        assert _call(lib, null=(name,)) == EINVAL and b"null pointer" in err(), name
    assert _call(lib, B=0) == EINVAL and b"bad shape" in err()
    assert _call(lib, D=96) == EUNSUPPORTED and b"head_dim 96" in err()
    assert _call(lib, B=17) == EUNSUPPORTED and b"17 branches" in err() and b"B <= 16" in err()
    assert _call(lib, Hkv=65) == EUNSUPPORTED and b"Hkv <= 64" in err()
    assert _call(lib, G=65) == EUNSUPPORTED and b"G <= 64" in err()
    assert _call(lib, dtype=3) == EINVAL and b"dtype" in err()
    for name in ("q", "tk", "tv", "kn", "vn", "osh", "out"):
        assert _call(lib, **{name: 24}) == EINVAL and b"aligned" in err(), name
    assert _call(lib, lse=18) == EINVAL and b"aligned" in err()
    assert _call(lib, qs=(7 * 128, 128, 28 * 128 + 4)) == EINVAL and b"strides of q" in err() and b"multiples of 8" in err()
    assert _call(lib, kns=(128, 4 * 128 + 4)) == EINVAL and b"new rows" in err() and b"multiples of 8" in err()
    assert _call(lib, cu=[1, 5, 10, 15]) == EINVAL and b"cu_q[0] = 1" in err()
    assert _call(lib, cu=[0, 5, 4, 15]) == EINVAL and b"cu_q decreases at branch 1" in err()
    assert _call(lib, tl=[0, -1, 0]) == EINVAL and b"tail_len[1] = -1" in err()
    assert _call(lib, tl=[0, 60, 0]) == EINVAL and b"branch 1" in err() and b"tail_cap = 64" in err()       # 60 + 5 rows
    assert _call(lib, branch=[0, 1, 1]) == EINVAL and b"permutation" in err()
    assert _call(lib, branch=[0, 1, 3]) == EINVAL and b"permutation" in err()
    assert _call(lib, branch=[2, 0, 1], tl=[60, 0, 0]) == EINVAL and b"branch 0" in err()                    # the run of tail 0 is the second
    with pytest.raises(_lib.KvzError, match="head_dim"):
        _lib.check(_call(lib, D=96), "kvz_fork_prefill_tail")
    # T = 0: a successful no-op - nothing is launched (there is no device here), whatever the tails hold
    assert _call(lib, cu=[0, 0, 0, 0], tl=[3, 64, 0]) == 0
    assert _call(lib, cu=[0, 0, 0, 0], cap=0) == 0


# ---- ForkedCache.select_packed: what it refuses (host logic only; the fork is put together by hand) ----------------------------------
def _fork(n_branches=3, n_layers=2):
    from kvzip_amd.kvcache import ForkedCache
    f = ForkedCache.__new__(ForkedCache)
    f.base = types.SimpleNamespace(_layout_epoch=0, info={"flatten": True, "offset": [0] * n_layers})
    f._epoch, f._offset = 0, [0] * n_layers
    f.n_branches, f.n_layers, f.n_heads_kv, f.n_group_kv = n_branches, n_layers, 2, 2
    f.active = [True] * n_branches
    f.tail_len = [[0] * n_branches for _ in range(n_layers)]
    f._branch, f._packed = 0, None
    return f


def test_select_packed_refuses_what_it_cannot_run():
    from kvzip_amd.ops import KvzError
    f = _fork()
    f.select_packed([2, 0, 1], [11, 3, 70])
    assert f._packed == ([2, 0, 1], [11, 3, 70])
    f.select_packed([1], [4])                      # a part of the branches, in any order, is fine
    with pytest.raises(KvzError, match="twice"):
        f.select_packed([0, 1, 0], [1, 2, 3])
    with pytest.raises(KvzError, match="2 branches and 3 lengths"):
        f.select_packed([0, 1], [1, 2, 3])
    with pytest.raises(KvzError, match="no branch 3"):
        f.select_packed([0, 3], [1, 2])
    with pytest.raises(KvzError, match="negative length"):
        f.select_packed([0, 1], [1, -2])
    with pytest.raises(KvzError, match="at least one"):
        f.select_packed([], [])
    f.retire(1)
    with pytest.raises(KvzError, match="branch 1 is retired"):
        f.select_packed([0, 1], [1, 2])
    f.select_packed([0, 2], [1, 2])
    assert f._packed == ([0, 2], [1, 2])           # (a refused packing leaves the selected one alone)


def test_first_step_wants_the_packed_length():
    from kvzip_amd.ops import KvzError
    f = _fork()
    f.select_packed([2, 0, 1], [11, 3, 70])
    q = torch.zeros(1, 4, 83, 64, dtype=torch.float16)
    k = torch.zeros(1, 2, 83, 64, dtype=torch.float16)
    with pytest.raises(KvzError, match=r"\[1, H, 84, D\].*83 positions"):
        f.first_step(q, k, k, 0)
    with pytest.raises(KvzError, match="batch 2"):
        f.first_step(torch.zeros(2, 4, 84, 64), k, k, 0)
    assert f._packed is not None and f.tail_len[0] == [0, 0, 0]     # nothing happened
    f.base._layout_epoch = 1                                        # a stale fork raises before anything else, as the other hooks do
    with pytest.raises(KvzError, match="re-laid out"):
        f.first_step(q, k, k, 0)


def test_generate_batch_has_the_switch():
    from kvzip_amd.wrapper import ModelKVzip
    m = ModelKVzip.__new__(ModelKVzip)
    m.fork_packed_first = True
    assert m._packs_first_steps([11, 3, 70]) and not m._packs_first_steps([11, 0])
    m.fork_packed_first = False
    assert not m._packs_first_steps([11, 3, 70])


# ---- the probe helpers' own expectations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_probe_expectations(dtype):
    """The uniform probe's expectation is the key count it claims, dim D - 1 is the branch number, and one key too many, or a row of
    another branch, moves an output by at least one whole 16-bit step."""
    import attn_probes as ap
    import numpy as np
    lengths, tail_len, G, D = [5, 0, 17], [31, 3, 0], 7, 128
    c = pp.uniform_case(lengths, tail_len, G, D, dtype, tail_cap=40)
    assert c.cu_q == [0, 5, 5, 22] and c.lengths == lengths
    e = pp.expected_out(c)
    ef = e.float()
    for b in (0, 2):
        for p in range(lengths[b]):
            i, n = c.cu_q[b] + p, np.float32(tail_len[b] + p + 1)
            want = lambda x: float(torch.tensor(np.float32(x) / n).to(dtype))  # noqa: E731
            assert float(ef[1, i, 3, D - 2]) == want(p + 1)                      # its branch's new rows up to itself
            assert float(ef[1, i, 3, D - 3]) == want(tail_len[b])                # the old tail rows
            assert float(ef[0, i, 0, D - 1]) == b + 1                            # ... all of THIS branch, exactly
    for fault in ("key+1", "foreign"):
        bad = pp.expected_out(c, fault)
        st = ap.steps(bad, e).amax(dim=(0, 2, 3))                                # worst step count per packed position
        for b in (0, 2):
            for p in range(lengths[b]):
                if fault == "key+1" and p == lengths[b] - 1:
                    assert int(st[c.cu_q[b] + p]) == 0                           # (the branch's last position has no next row)
                else:
                    assert int(st[c.cu_q[b] + p]) >= 1, (fault, b, p)
    # the tails afterwards: the new rows behind the old ones, everything else as before (the branch without positions included)
    ek, ev = pp.expected_tails(c)
    assert torch.equal(ev[0, :, 31:36], c.v_new[:, 0:5]) and torch.equal(ek[2, :, 0:17], c.k_new[:, 5:22])
    assert torch.equal(ek[1], c.tail_k[1]) and torch.equal(ev[1], c.tail_v[1]) and float(ev[0, 0, 36, 0]) == ap.SLACK_VALUE
    assert int((ev != c.tail_v).any(-1).sum()) == 2 * (5 + 17)
    # weighted probe and the merge: finalize asserts that every sum is exact in fp32, expected_out that the float64 quotient agrees
    w = pp.weighted_case(lengths, tail_len, 4, 64, dtype, tail_cap=40)
    pp.expected_out(w)
    m = pp.with_shared(c)
    em = pp.expected_out(m)
    assert bool(torch.isfinite(em.float()).all()) and int(ap.steps(em, e).max()) >= 1
    none = torch.isinf(m.lse_shared)
    assert bool(none.any()) and ap.bits_equal(em[none], e[none])[0]              # a shared side without keys changes nothing
    pp.expected_out(pp.with_shared(w))
    q, k, v = pp.as_model_tensors(w)
    assert q.shape == (1, 8, 22, 64) and k.shape == (1, 2, 22, 64) and k.stride(-1) == 1 and k.stride(2) == 2 * 64
    assert torch.equal(q[0, 1 * 4 + 3, 9], w.q[1, 9, 3]) and torch.equal(v[0, 1, 9], w.v_new[1, 9])
