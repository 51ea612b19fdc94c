"""CPU: the entry points of tree speculative decoding (include/kvzip_hip_tree.h) are exported and bound, and validate their arguments
on the host before any launch (no compute calls: there is no GPU here)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = "kvzip_hip_tree.h"
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
SYMBOLS = ["kvz_tree_attn_append", "kvz_tree_attn_workspace_bytes", "kvz_tree_keep_path"]


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
    assert syms == SYMBOLS
    lib = C.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/{HEADER} but not exported"
    assert sorted(_lib.TREE_SIGNATURES) == syms
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.MULTI_SIGNATURES) | set(_lib.PREFILL_SIGNATURES)
              | set(_lib.MULTI_PREFILL_SIGNATURES) | set(_lib.BRANCH_SIGNATURES) | set(_lib.SPEC_SIGNATURES) | set(_lib.RETAIN_SIGNATURES))
    assert not set(_lib.TREE_SIGNATURES) & others
    bound = _lib.load()
    for s, (res, args) in _lib.TREE_SIGNATURES.items():
        assert getattr(bound, s).argtypes == args and getattr(bound, s).restype == res


def test_other_headers_are_untouched_and_the_new_one_names_no_other_entry_point():
    inc = os.path.join(ROOT, "include")
    for h in sorted(os.listdir(inc)):
        if h != HEADER:
            assert "kvz_tree" not in open(os.path.join(inc, h)).read(), h
    text = open(os.path.join(inc, HEADER)).read()
    for other in ("kvz_spec", "kvz_retain", "kvz_multi", "kvz_fork_branch", "kvz_fork_prefill"):
        assert other not in text, other
    from kvzip_amd import _lib
    assert _lib.load().kvz_abi_version() == _lib.ABI_VERSION == 6


def test_library_without_the_symbols_asks_for_a_rebuild(monkeypatch):
    """Same ABI version, older build: load() must say "rebuild" and name the header, not die with an AttributeError."""
    from kvzip_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.TREE_SIGNATURES, "kvz_tree_entry_point_of_a_newer_header", (C.c_int, []))
    with pytest.raises(_lib.KvzError, match=r"kvzip_hip_tree\.h.*rebuild"):
        _lib.load()
    assert _lib._lib is None


def test_workspace_bytes_are_the_chain_calls():
    from kvzip_amd import _lib
    lib = _lib.load()
    w, chain = lib.kvz_tree_attn_workspace_bytes, lib.kvz_spec_attn_workspace_bytes
    assert w(0, 4, 7, 128) == 0 and w(-1, 4, 7, 128) == 0 and w(2, 0, 7, 128) == 0 and w(2, 4, 0, 128) == 0 and w(2, 4, 7, 0) == 0
    for t in (1, 2, 3, 4, 9, 16, 33, 64):
        for Hkv in (1, 4, 8, 64):
            for G in (1, 2, 4, 7):
                for D in (64, 128):
                    assert w(t, Hkv, G, D) == chain(t, Hkv, G, D) > 0, (t, Hkv, G, D)


def _chain(t):
    return [(1 << (p + 1)) - 1 for p in range(t)]


def _call(lib, t=4, Hkv=4, G=7, D=128, slack=8, offset=0, meta="both", starts=None, lens=None, q=16, kc=16, vc=16, kn=16, vn=16, out=16,
          ws=16, ws_bytes=1 << 30, dtype=0, strides=None, anc="chain"):
    mh = None
    if meta in ("both", "host"):
        mh = (C.c_int32 * (2 * Hkv))(*(starts if starts is not None else [1000 * i for i in range(Hkv)]),
                                     *(lens if lens is not None else [10] * Hkv))
    dev = 32 if meta in ("both", "device") else None          # (made-up device addresses: nothing is dereferenced before a launch)
    st = strides if strides is not None else (t * D, D, D, Hkv * D)
    if anc == "chain":
        anc = _chain(max(t, 0))
    masks = (C.c_uint64 * max(len(anc), 1))(*anc) if anc is not None else None
    return lib.kvz_tree_attn_append(q, kc, vc, dev, dev, offset, mh, slack, kn, vn, st[0], st[1], st[2], st[3], t, Hkv, G, D, 0.1, dtype,
                                    out, ws, ws_bytes, masks, None)


def test_verify_call_validates_like_the_chain_call():
    """Bad arguments are rejected on the host before any launch (error code + a telling message that names THIS entry point)."""
    from kvzip_amd import _lib
    lib = _lib.load()
    err = lib.kvz_last_error
    for name in ("q", "kc", "vc", "kn", "vn", "out", "ws", "anc"):
        assert _call(lib, **{name: None}) == EINVAL and b"kvz_tree_attn_append: null pointer" in err(), name
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
    assert _call(lib, Hkv=0) == EINVAL and b"bad shape" in err()
    assert _call(lib, dtype=3) == EINVAL and b"dtype" in err()
    assert _call(lib, lens=[10, 10, -1, 10]) == EINVAL and b"head 2" in err()
    assert _call(lib, D=96) == EUNSUPPORTED and b"head_dim 96" in err()
    assert _call(lib, Hkv=65, slack=8) == EUNSUPPORTED and b"Hkv <= 64" in err()
    assert _call(lib, t=10, G=7, slack=16) == EUNSUPPORTED and b"t*G <= 64" in err()
    assert _call(lib, t=1, G=65) == EUNSUPPORTED and b"t*G <= 64" in err()
    assert _call(lib, t=65, G=1, slack=80) == EUNSUPPORTED and b"t*G <= 64" in err()
    assert _call(lib, ws_bytes=64) == EWORKSPACE and b"workspace too small" in err()
    need = lib.kvz_tree_attn_workspace_bytes(4, 4, 7, 128)
    assert _call(lib, ws_bytes=need - 1) == EWORKSPACE and b"workspace too small" in err()
    assert b"kvz_tree_attn_append" in err()
    with pytest.raises(_lib.KvzError, match="head_dim"):
        _lib.check(_call(lib, D=96), "kvz_tree_attn_append")


def test_verify_call_validates_the_masks():
    """A mask without its own bit, with a bit above its node, or with a bit at or above t: KVZ_EINVAL naming the node.  The checks come
    before the workspace check, and a valid tree gets as far as that one (ws_bytes = 0 here: nothing is ever launched)."""
    from kvzip_amd import _lib
    lib = _lib.load()
    err = lib.kvz_last_error
    ok = dict(ws_bytes=0)
    assert _call(lib, **ok) == EWORKSPACE
    assert _call(lib, anc=[1, 0b11, 0b101, 0b1011], **ok) == EWORKSPACE                       # a tree
    assert _call(lib, anc=[1, 0b10, 0b100, 0b1000], **ok) == EWORKSPACE                       # (no node sees the root: still well-formed)
    assert _call(lib, anc=[1, 0b11, 0b011, 0b1111], **ok) == EINVAL and b"node 2 lacks bit 2" in err()
    assert _call(lib, anc=[0, 0b11, 0b111, 0b1111], **ok) == EINVAL and b"node 0 lacks bit 0" in err()
    assert _call(lib, anc=[1, 0b111, 0b111, 0b1111], **ok) == EINVAL and b"node 1 has a bit above 1" in err()
    assert _call(lib, anc=[0b11, 0b11, 0b111, 0b1111], **ok) == EINVAL and b"node 0 has a bit above 0" in err()
    assert _call(lib, anc=[1, 0b11, 0b111, 0b11111], **ok) == EINVAL and b"node 3 has a bit at or above t = 4" in err()
    assert _call(lib, anc=[1, 0b11, 0b111, 0b1111 | (1 << 63)], **ok) == EINVAL and b"node 3 has a bit at or above t = 4" in err()
    assert _call(lib, anc=[1 | (1 << 40), 0b11, 0b111, 0b1111], **ok) == EINVAL and b"node 0 has a bit at or above t = 4" in err()
    # t = 64: bit 63 is a node's own bit, there is no bit at or above t, and the shifts stay defined
    kw = dict(t=64, G=1, Hkv=2, D=64, slack=64, ws_bytes=0)
    assert _call(lib, **kw) == EWORKSPACE
    star = [1] + [(1 << p) | 1 for p in range(1, 64)]
    assert _call(lib, anc=star, **kw) == EWORKSPACE
    bad = list(star); bad[63] = 1
    assert _call(lib, anc=bad, **kw) == EINVAL and b"node 63 lacks bit 63" in err()
    bad = list(star); bad[62] |= 1 << 63
    assert _call(lib, anc=bad, **kw) == EINVAL and b"node 62 has a bit above 62" in err()
    # t = 63: bit 63 is beyond the tree
    kw63 = dict(t=63, G=1, Hkv=2, D=64, slack=64, ws_bytes=0)
    bad = _chain(63); bad[5] |= 1 << 63
    assert _call(lib, anc=bad, **kw63) == EINVAL and b"node 5 has a bit at or above t = 63" in err()


def _keep(lib, L=2, Hkv=2, D=128, t=4, path=(0, 2), k=None, v=None, row0=None, dtype=0, n=None, null=()):
    kp = (C.c_void_p * L)(*(k if k is not None else [4096 * (i + 1) for i in range(L)]))
    vp = (C.c_void_p * L)(*(v if v is not None else [1 << 20 | 4096 * (i + 1) for i in range(L)]))
    r0 = (C.c_int32 * max(L * Hkv, 1))(*(row0 if row0 is not None else [100 * i for i in range(L * Hkv)]))
    ph = (C.c_int32 * max(len(path), 1))(*path)
    args = {"k": kp, "v": vp, "row0": r0, "path": ph}
    for x in null:
        args[x] = None
    return lib.kvz_tree_keep_path(L, args["k"], args["v"], args["row0"], args["path"], len(path) if n is None else n, t, Hkv, D, dtype, None)


def test_keep_path_validates_without_gpu():
    from kvzip_amd import _lib
    lib = _lib.load()
    err = lib.kvz_last_error
    for x in ("k", "v", "row0", "path"):
        assert _keep(lib, null=(x,)) == EINVAL and b"kvz_tree_keep_path: null pointer" in err(), x
    assert _keep(lib, k=[4096, 0]) == EINVAL and b"null K or V cache of layer 1" in err()
    assert _keep(lib, v=[0, 4096]) == EINVAL and b"null K or V cache of layer 0" in err()
    assert _keep(lib, k=[4096, 4104]) == EINVAL and b"layer 1 must be 16-byte aligned" in err()
    assert _keep(lib, v=[4100, 4096]) == EINVAL and b"layer 0 must be 16-byte aligned" in err()
    assert _keep(lib, path=(0, 2, 2)) == EINVAL and b"path[2] = 2 does not ascend" in err()
    assert _keep(lib, path=(2, 1)) == EINVAL and b"path[1] = 1 does not ascend" in err()
    assert _keep(lib, path=(1, 3, 2)) == EINVAL and b"path[2] = 2 does not ascend" in err()
    assert _keep(lib, path=(-1, 2)) == EINVAL and b"path[0] = -1 is below 0" in err()
    assert _keep(lib, path=(0, 4)) == EINVAL and b"path[1] = 4 names no node of the t = 4" in err()
    assert _keep(lib, path=(0, 1, 2, 3, 4)) == EINVAL and b"path[4] = 4 names no node" in err()
    assert _keep(lib, n=-1) == EINVAL and b"n = -1" in err()
    assert _keep(lib, t=65, path=(0, 64)) == EINVAL and b"t = 65" in err()
    assert _keep(lib, t=-1) == EINVAL and b"t = -1" in err()
    assert _keep(lib, row0=[0, 100, -5, 300]) == EINVAL and b"negative row0 of layer 1, head 0" in err()
    assert _keep(lib, L=0) == EINVAL and b"bad shape" in err()
    assert _keep(lib, Hkv=0) == EINVAL and b"bad shape" in err()
    assert _keep(lib, D=0) == EINVAL and b"bad shape" in err()
    assert _keep(lib, dtype=2) == EINVAL and b"dtype" in err()
    assert _keep(lib, D=68) == EUNSUPPORTED and b"136 bytes per row" in err()
    assert _keep(lib, D=1024) == EUNSUPPORTED and b"2048 bytes per row" in err()
    assert _keep(lib, Hkv=65) == EUNSUPPORTED and b"Hkv <= 64" in err()
    # nothing to move: OK without a launch (these addresses are made up: a launch would fault, and there is no GPU here)
    assert _keep(lib, path=(0, 1, 2)) == 0
    assert _keep(lib, path=(0,)) == 0
    assert _keep(lib, path=()) == 0
    assert _keep(lib, path=(), null=("path",)) == 0
    assert _keep(lib, t=64, path=tuple(range(64))) == 0
