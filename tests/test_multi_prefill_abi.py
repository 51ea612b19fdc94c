"""CPU: the entry points of the packed first step over several independent caches (include/kvzip_hip_multi_prefill.h) are exported
and bound, validate their arguments on the host before any launch, and kvcache.CacheBatch refuses a packing it cannot run (no compute
calls: there is no GPU here)."""
import ctypes as C
import os
import re
import types

import pytest
import torch

import multi_prefill_probes as mpp
from conftest import ROOT

HEADER = "kvzip_hip_multi_prefill.h"
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
    assert syms == ["kvz_multi_prefill", "kvz_multi_prefill_workspace_bytes"]
    lib = C.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/{HEADER} but not exported"
    assert sorted(_lib.MULTI_PREFILL_SIGNATURES) == syms
    assert not set(_lib.MULTI_PREFILL_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.MULTI_SIGNATURES)
                                                     | set(_lib.PREFILL_SIGNATURES))
    bound = _lib.load()
    for s, (res, args) in _lib.MULTI_PREFILL_SIGNATURES.items():
        assert getattr(bound, s).argtypes == args and getattr(bound, s).restype == res


def test_other_headers_are_untouched_by_the_new_entry_points():
    for h in ("kvzip_hip.h", "kvzip_hip_tighten.h", "kvzip_hip_multi.h", "kvzip_hip_prefill.h", "kvzip_hip_debug.h"):
        assert "kvz_multi_prefill" not in open(os.path.join(ROOT, "include", h)).read()
    from kvzip_amd import _lib
    assert _lib.load().kvz_abi_version() == _lib.ABI_VERSION == 6


def test_library_without_the_symbols_asks_for_a_rebuild(monkeypatch):
    """Same ABI version, older build: load() must say "rebuild" and name the header, not die with an AttributeError."""
    from kvzip_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.MULTI_PREFILL_SIGNATURES, "kvz_multi_prefill_entry_point_of_a_newer_header", (C.c_int, []))
    with pytest.raises(_lib.KvzError, match=r"kvzip_hip_multi_prefill\.h.*rebuild"):
        _lib.load()
    assert _lib._lib is None


def test_workspace_bytes():
    """The header's formula: items = target + 2 * Hkv * (T*G / 64 + B) slots of 64 rows of (D + 2) floats; no key length in it."""
    from kvzip_amd import _lib
    w = _lib.load().kvz_multi_prefill_workspace_bytes
    assert w(0, 2, 4, 7, 128) == 0 and w(-1, 2, 4, 7, 128) == 0 and w(5, 0, 4, 7, 128) == 0 and w(5, 2, 0, 7, 128) == 0
    a256 = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for T, B, Hkv, G, D in [(22, 3, 2, 7, 128), (1280, 8, 4, 7, 128), (96, 16, 8, 4, 64), (1, 1, 1, 1, 64)]:
        S = B * Hkv
        target = 256 - S if S < 192 else 64
        items = target + 2 * Hkv * (T * G // 64 + B)
        assert w(T, B, Hkv, G, D) == a256(items * 64 * 2 * 4) + a256(items * 64 * D * 4), (T, B, Hkv, G, D)


def _call(lib, B=3, Hkv=4, G=7, D=128, cu=None, slack=64, offset=None, starts=None, lens=None, q=16, kp=16, vp=16, kn=16, vn=16, out=16,
          ws=16, ws_bytes=1 << 32, dtype=0, qs=None, kns=None, null=()):
    n = max(B, 1)
    cu_q = (C.c_int32 * (n + 1))(*(cu if cu is not None else [5 * i for i in range(n + 1)]))
    k_ptrs = (C.c_void_p * n)(*([kp] * n))
    v_ptrs = (C.c_void_p * n)(*([vp] * n))
    seg = (C.c_int32 * (n * Hkv))(*(starts if starts is not None else [1000 * i for i in range(n * Hkv)]))
    ln = (C.c_int32 * (n * Hkv))(*(lens if lens is not None else [10] * (n * Hkv)))
    sl = (C.c_int32 * n)(*([slack] * n))
    off = (C.c_int32 * n)(*(offset if offset is not None else [0] * n))
    a = dict(q=q, cu=cu_q, k_ptrs=k_ptrs, v_ptrs=v_ptrs, seg=seg, ln=ln, sl=sl, off=off, kn=kn, vn=vn, out=out)
    for name in null:
        a[name] = None
    qs = qs if qs is not None else (G * D, D, Hkv * G * D)
    kns = kns if kns is not None else (D, Hkv * D)
    return lib.kvz_multi_prefill(a["q"], qs[0], qs[1], qs[2], a["cu"], a["k_ptrs"], a["v_ptrs"], a["seg"], a["ln"], a["sl"], a["off"],
                                 a["kn"], a["vn"], kns[0], kns[1], kns[0], kns[1], B, Hkv, G, D, 0.1, dtype, a["out"], ws, ws_bytes, None)


def test_argument_validation_without_gpu():
    """Bad arguments are rejected on the host before any launch (error code + a telling message); nothing here is dereferenced on a
    device."""
    from kvzip_amd import _lib
    lib = _lib.load()
    err = lib.kvz_last_error
    for name in ("q", "cu", "k_ptrs", "v_ptrs", "seg", "ln", "sl", "off", "kn", "vn", "out"):
        assert _call(lib, null=(name,)) == EINVAL and b"null pointer" in err(), name
    assert _call(lib, ws=None) == EINVAL and b"null pointer" in err()
    assert _call(lib, kp=None) == EINVAL and b"null K or V pointer of cache 0" in err()
    assert _call(lib, B=0) == EINVAL and b"bad shape" in err()
    assert _call(lib, D=96) == EUNSUPPORTED and b"head_dim 96" in err()
    assert _call(lib, B=17, Hkv=1) == EUNSUPPORTED and b"17 caches" in err() and b"B <= 16" in err()
    assert _call(lib, B=9, Hkv=16) == EUNSUPPORTED and b"B*Hkv <= 128" in err()          # 144 segments
    assert _call(lib, B=1, Hkv=65) == EUNSUPPORTED and b"Hkv <= 64" in err()
    assert _call(lib, G=65) == EUNSUPPORTED and b"G <= 64" in err()
    assert _call(lib, dtype=3) == EINVAL and b"dtype" in err()
    for name in ("q", "kn", "vn", "out", "ws"):
        assert _call(lib, **{name: 24}) == EINVAL and b"aligned" in err(), name
    assert _call(lib, vp=24) == EINVAL and b"cache 0" in err() and b"aligned" in err()
    assert _call(lib, qs=(7 * 128, 128, 28 * 128 + 4)) == EINVAL and b"strides of q" in err() and b"multiples of 8" in err()
    assert _call(lib, kns=(128, 4 * 128 + 4)) == EINVAL and b"new rows" in err() and b"multiples of 8" in err()
    assert _call(lib, cu=[1, 5, 10, 15]) == EINVAL and b"cu_q[0] = 1" in err()
    assert _call(lib, cu=[0, 5, 4, 15]) == EINVAL and b"cu_q decreases at cache 1" in err()
    # the new rows must fit behind every segment: offset + n_b <= slack, offset >= 0 - for the caches that take part
    assert _call(lib, offset=[0, 60, 0]) == EINVAL and b"cache 1" in err() and b"slack = 64" in err()        # 60 + 5 rows
    assert _call(lib, offset=[0, 59, 0], ws_bytes=64) == EWORKSPACE                                            # 59 + 5 fit exactly
    assert _call(lib, offset=[0, -1, 0]) == EINVAL and b"offset[1] = -1" in err()
    assert _call(lib, lens=[10, 10, -1, 10] + [10] * 8) == EINVAL and b"cache 0, head 2" in err()
    assert _call(lib, starts=[0, 10, 20, 2 ** 31 - 12] + [0] * 8) == EINVAL and b"cache 0, head 3" in err()
    assert _call(lib, ws_bytes=64) == EWORKSPACE and b"workspace too small" in err()
    need = lib.kvz_multi_prefill_workspace_bytes(15, 3, 4, 7, 128)
    assert _call(lib, ws_bytes=need - 1) == EWORKSPACE and b"workspace too small" in err()
    with pytest.raises(_lib.KvzError, match="head_dim"):
        _lib.check(_call(lib, D=96), "kvz_multi_prefill")
    # a cache without positions takes no part: whatever its offset, its pointers and its segments hold
    assert _call(lib, cu=[0, 5, 5, 10], offset=[0, -7, 0], ws_bytes=64) == EWORKSPACE
    assert _call(lib, cu=[0, 5, 5, 10], offset=[0, 999, 0], lens=[10] * 4 + [-1] * 4 + [10] * 4, ws_bytes=64) == EWORKSPACE
    # T = 0: a successful no-op - nothing is launched (there is no device here), whatever the caches hold; no workspace needed
    assert _call(lib, cu=[0, 0, 0, 0], offset=[3, 64, -1]) == 0
    assert _call(lib, cu=[0, 0, 0, 0], ws=None, ws_bytes=0, kp=None) == 0


# ---- CacheBatch.select_packed / first_step: what they refuse (host logic only; the batch is put together by hand) --------------------
def _batch(n=3, n_layers=2):
    from kvzip_amd.kvcache import CacheBatch
    b = CacheBatch.__new__(CacheBatch)
    b.caches = [types.SimpleNamespace(pruned=True, layout="slack", slack=8, _seen_tokens=100, _layout_epoch=0,
                                      info={"flatten": True, "offset": [0] * n_layers}) for _ in range(n)]
    b.n_caches, b.n_layers, b.n_heads_kv, b.n_group_kv = n, n_layers, 2, 2
    b.active = [True] * n
    b.pruned, b.get_score, b.layout = True, False, "multi"
    b._packed = b._pws = None
    b._tables = {}
    return b


def test_select_packed_refuses_what_it_cannot_run():
    from kvzip_amd.ops import KvzError
    f = _batch()
    f.select_packed([2, 0, 1], [11, 3, 70])
    assert f._packed == ([2, 0, 1], [11, 3, 70])
    f.select_packed([1], [4])                      # a part of the members, in any order, is fine
    with pytest.raises(KvzError, match="twice"):
        f.select_packed([0, 1, 0], [1, 2, 3])
    with pytest.raises(KvzError, match="2 members and 3 lengths"):
        f.select_packed([0, 1], [1, 2, 3])
    with pytest.raises(KvzError, match="no member 3"):
        f.select_packed([0, 3], [1, 2])
    with pytest.raises(KvzError, match="negative length"):
        f.select_packed([0, 1], [1, -2])
    with pytest.raises(KvzError, match="at least one"):
        f.select_packed([], [])
    f.retire(1)
    with pytest.raises(KvzError, match="member 1 is retired"):
        f.select_packed([0, 1], [1, 2])
    f.select_packed([0, 2], [1, 2])
    assert f._packed == ([0, 2], [1, 2])           # (a refused packing leaves the selected one alone)


def test_first_step_wants_a_packing_and_its_length():
    from kvzip_amd.ops import KvzError
    f = _batch()
    q = torch.zeros(1, 4, 83, 64, dtype=torch.float16)
    k = torch.zeros(1, 2, 83, 64, dtype=torch.float16)
    with pytest.raises(KvzError, match="needs a packing"):
        f.first_step(q, k, k, 0)
    f.select_packed([2, 0, 1], [11, 3, 70])
    with pytest.raises(KvzError, match=r"\[1, H, 84, D\].*83 positions"):
        f.first_step(q, k, k, 0)
    with pytest.raises(KvzError, match="batch 2"):
        f.first_step(torch.zeros(2, 4, 84, 64), k, k, 0)
    assert f._packed is not None                                     # nothing happened: no offset moved, no slack grew
    assert all(c.info["offset"] == [0, 0] and c._seen_tokens == 100 and c.slack == 8 and c._layout_epoch == 0 for c in f.caches)
    f.caches[0].pruned = False                                       # a member that left the slack layout is refused before anything moves
    with pytest.raises(KvzError, match="no longer a pruned slack-layout cache"):
        f.first_step(torch.zeros(1, 4, 84, 64), torch.zeros(1, 2, 84, 64), torch.zeros(1, 2, 84, 64), 0)
    assert all(c.info["offset"] == [0, 0] and c.slack == 8 for c in f.caches)


def test_attention_branch_without_a_packing_is_todays_error():
    """attn.py: a batch-1 forward over a CacheBatch with no packing selected raises what it raised before."""
    from kvzip_amd import attn
    from kvzip_amd.ops import KvzError
    f = _batch()
    mod = types.SimpleNamespace(head_dim=64, q_proj=torch.nn.Linear(8, 4 * 64, bias=False), k_proj=torch.nn.Linear(8, 2 * 64, bias=False),
                                v_proj=torch.nn.Linear(8, 2 * 64, bias=False), scaling=0.125, layer_idx=0,
                                config=types.SimpleNamespace(num_key_value_heads=2))
    cos = torch.ones(1, 5, 64)
    with pytest.raises(KvzError, match="first steps run at batch 1 on each cache's own path"):
        attn.llama_qwen_attn_forward(mod, torch.zeros(1, 5, 8), (cos, torch.zeros(1, 5, 64)), None, f)


def test_generate_multi_has_the_switch():
    from kvzip_amd.wrapper import ModelKVzip
    m = ModelKVzip.__new__(ModelKVzip)
    m.multi_packed_first = True
    assert m._packs_first_steps_multi([11, 3, 70]) and not m._packs_first_steps_multi([11, 0]) and not m._packs_first_steps_multi([11])
    m.multi_packed_first = False
    assert not m._packs_first_steps_multi([11, 3, 70])


# ---- CacheBatch._table: the tables of the decode order and of a packing order (host logic only) -----------------------------------------
def test_cache_batch_keeps_the_tables_of_both_orders(monkeypatch):
    """A generation alternates once between a packing order and the decode order: neither evicts the other's tables, and a member's
    layout change rebuilds both (no library call: the table is a stand-in that records what it was built from)."""
    from kvzip_amd import kvcache
    built = []
    monkeypatch.setattr(kvcache.ops, "MultiTable", lambda k, v, starts, lens, slack: built.append(k) or (k, starts, lens, slack))
    b = kvcache.CacheBatch.__new__(kvcache.CacheBatch)
    b.caches = [types.SimpleNamespace(_layout_epoch=0, slack=8 + i, key_cache=[f"k{i}.{l}" for l in range(2)],
                                      value_cache=[f"v{i}.{l}" for l in range(2)],
                                      info={"meta_host": [[10 * i, 10 * i + 1, 5, 6, 0, 0]] * 2}) for i in range(3)]
    b.n_caches, b.n_layers, b.n_heads_kv, b._tables = 3, 2, 2, {}
    packed = b._table(1, (2, 0, 1))
    assert packed == (["k2.1", "k0.1", "k1.1"], [[20, 21], [0, 1], [10, 11]], [[5, 6]] * 3, [10, 8, 9]) and len(built) == 2
    decode = b._table(1)
    assert decode[0] == ["k0.1", "k1.1", "k2.1"] and decode[3] == [8, 9, 10] and len(built) == 4
    assert b._table(0, (2, 0, 1))[0] == ["k2.0", "k0.0", "k1.0"] and b._table(1, (2, 0, 1)) is packed and b._table(1) is decode
    assert len(built) == 4                                               # both orders are kept: nothing was built again
    b.caches[1]._layout_epoch = 1                                        # slack growth / tighten of one member
    b.caches[1].key_cache = ["K1.0", "K1.1"]
    assert b._table(1)[0] == ["k0.1", "K1.1", "k2.1"] and b._table(1, (2, 0, 1))[0] == ["k2.1", "k0.1", "K1.1"] and len(built) == 8
    assert len(b._tables) == 2                                           # (the tables of the old layout are gone)


# ---- the probe helpers' own expectations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_probe_expectations(dtype):
    """The uniform probe's expectation is the key count it claims, dim D - 1 counts rows of THIS cache only, and one key too many, or a
    row of another cache, moves an output by at least one whole 16-bit step."""
    import attn_probes as ap
    import numpy as np
    lens, off, lengths, G, D = [[300, 37], [0, 129], [64, 255]], [0, 5, 1], [5, 0, 17], 7, 128
    c = mpp.uniform_case(lens, off, lengths, G, D, dtype, slack=40)
    assert c.cu_q == [0, 5, 5, 22] and c.lengths == lengths and c.old(1, 1) == 134
    e = mpp.expected_out(c)
    ef = e.float()
    for b in (0, 2):
        for p in range(lengths[b]):
            for h in range(2):
                i, n = c.cu_q[b] + p, np.float32(lens[b][h] + off[b] + p + 1)
                want = lambda x: float(torch.tensor(np.float32(x) / n).to(dtype))  # noqa: E731
                assert float(ef[h, i, 3, D - 2]) == want(p + 1)                      # its run's new rows up to itself
                assert float(ef[h, i, 3, D - 3]) == want(off[b])                     # the rows appended before
                assert float(ef[h, i, 0, D - 1]) == want((b + 1) * (off[b] + p + 1))  # ... all of THIS cache
    for fault in ("key+1", "foreign"):
        bad = mpp.expected_out(c, fault)
        st = ap.steps(bad, e).amax(dim=(0, 2, 3))                                # worst step count per packed position
        for b in (0, 2):
            for p in range(lengths[b]):
                if fault == "key+1" and p == lengths[b] - 1:
                    assert int(st[c.cu_q[b] + p]) == 0                           # (the run's last position has no next row)
                else:
                    assert int(st[c.cu_q[b] + p]) >= 1, (fault, b, p)
    # the arenas afterwards: the new rows behind the old ones, everything else as before (the cache without positions included)
    ek, ev = mpp.expected_arenas(c)
    r = c.row0[2] + c.starts[2][1] + 255 + 1
    assert torch.equal(ev[r:r + 17], c.v_new[1, 5:22]) and torch.equal(ek[r:r + 17], c.k_new[1, 5:22])
    assert float(c.arena_v[r, 0]) == ap.SLACK_VALUE and float(ev[r + 17, 0]) == ap.SLACK_VALUE
    lo, hi = c.row0[1], c.row0[1] + c.rows[1]
    assert torch.equal(ek[lo:hi], c.arena_k[lo:hi]) and torch.equal(ev[lo:hi], c.arena_v[lo:hi])
    assert int((ev != c.arena_v).any(-1).sum()) == 2 * (5 + 17)
    # weighted probe: finalize asserts that every sum is exact in fp32
    w = mpp.weighted_case(lens, off, [17, 3, 1], 4, 64, dtype, slack=40)
    mpp.expected_out(w)
    q, k, v = mpp.as_model_tensors(w)
    assert q.shape == (1, 8, 21, 64) and k.shape == (1, 2, 21, 64) and k.stride(-1) == 1 and k.stride(2) == 2 * 64
    assert torch.equal(q[0, 1 * 4 + 3, 9], w.q[1, 9, 3]) and torch.equal(v[0, 1, 9], w.v_new[1, 9])
    qq, kk, vv, starts, ln = mpp.concat_for_oracle(w, 0)
    assert qq.shape == (2 * 17, 4, 64) and ln == [300 + 17, 37 + 17] and starts == [0, 317] and kk.shape[0] == 317 + 54
