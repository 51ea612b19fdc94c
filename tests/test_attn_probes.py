"""CPU self-check of the exact attention probes (tests/attn_probes.py) that tests/test_gpu_attn_exact.py compares kernels with bit for bit:
1. the CPU oracle (fp32 softmax, one rounding) reproduces every predicted output up to its own single rounding;
2. the probes are sensitive: one marked key dropped or counted twice, or the causal limit moved by one, moves a predicted output by
   at least two 16-bit steps - faults that stay under the 1e-3 absolute bound of the random-input attention tests."""
import math

import pytest
import torch

import attn_probes as ap
import kvzip_oracle as orc

RAGGED = [0, 1, 15, 16, 17, 127, 128, 129, 1024]
LONG = [100_000, 129, 0, 4100]
ITEMS_LONG = (1, 2, 3, 4, 256 - 4, 1024)   # the sweep of the GPU test (Hkv = 4, default = 256 CUs - Hkv)


def _oracle_check(p, want):
    got = orc.varlen_attn(p.q, p.k, p.v, p.starts, p.lens, p.q_len, causal=p.causal, scale=p.scale)
    s = ap.steps(got, want)
    assert int(s.max()) <= 1, (p.kind, int(s.max()))
    return int((s != 0).sum())


def _cases():
    for dtype in (torch.float16, torch.bfloat16):
        for D in (64, 128):
            for q_len in (1, 5):
                yield f"ragged/{str(dtype)[6:]}/D{D}/q{q_len}", ap.uniform_probe(RAGGED, q_len, 7, D, dtype, causal=True, seed=D + q_len), "div"
            yield f"long/{str(dtype)[6:]}/D{D}", ap.uniform_probe(LONG, 1, 7, D, dtype, items=ITEMS_LONG, seed=D), "div"
        yield f"flash/{str(dtype)[6:]}/q20", ap.uniform_probe([0, 5, 130, 2100], 20, 7, 128, dtype, seed=3), "rcp"


def test_weighted_probes_match_the_oracle():
    for dtype in (torch.float16, torch.bfloat16):
        for lens, q_len, spread, head in (([0, 1, 17, 129, 1024], 5, 8, 0), ([100_000, 33], 1, 6, 0),
                                          ([0, 5, 130, 2100], 20, 6, ap.F2_DEFER)):
            p = ap.weighted_probe(lens, q_len, 7, 128, dtype, spread=spread, seed=q_len, headroom=head)
            for norm in ("div", "rcp"):
                want = ap.expected(p, norm)
                n = _oracle_check(p, want)
                print(f"\nWEIGHTED {str(dtype)[6:]} lens {lens} q_len {q_len} {norm}: oracle differs by one step in {n} of {want.numel()}")
    with pytest.raises(AssertionError):   # the exactness budget is enforced
        ap.weighted_probe([100_000], 1, 7, 128, torch.float16, spread=8)


def test_scale_folds_to_one():
    import numpy as np
    assert np.float32(ap.SCALE_ONE) * ap.LOG2E_F32 == np.float32(1.0)
    assert torch.tensor(ap.SCALE_ONE, dtype=torch.float32).item() == ap.SCALE_ONE


def test_uniform_probes_match_the_oracle_and_detect_one_key_faults():
    rows = []
    for name, p, norm in _cases():
        want = ap.expected(p, norm)
        n_off = _oracle_check(p, want)
        kf = ap.key_fault_steps(p, norm)
        cf = ap.causal_fault_steps(p, norm)
        for kind, (mn, lo, hi, cnt) in kf.items():
            rows.append((name, f"key {kind}", mn, lo, hi, cnt))
        for shift, (mn, lo, hi, cnt) in cf.items():
            rows.append((name, f"causal {shift:+d}", mn, lo, hi, cnt))
        assert n_off <= want.numel()
    print("\nPROBE SENSITIVITY (injected faults, expected output recomputed exactly; the random-input attention tests allow 1e-3)")
    print(f"{'probe':<24}{'fault':<12}{'min steps':>10}{'min |delta|':>13}{'max |delta|':>13}{'cases':>9}  under 1e-3?")
    for name, kind, mn, lo, hi, cnt in rows:
        print(f"{name:<24}{kind:<12}{mn:>10}{lo:>13.3e}{hi:>13.3e}{cnt:>9}  {'yes' if lo <= 1e-3 else ''}")
    worst = min(r[2] for r in rows)
    assert worst >= 2, [r for r in rows if r[2] < 2]
    # what makes the probes necessary: the one-key faults of the long head stay under the random-input bound
    under = {(r[0].split("/")[0], r[1]) for r in rows if r[3] <= 1e-3}
    assert {("long", "key drop"), ("long", "key dup"), ("long", "causal -1")} <= under, under
    kinds = {r[1] for r in rows}
    assert {"key drop", "key dup", "causal -1", "causal +1"} <= kinds


def test_decode_cut_restatement():
    # chunk of the decode kernel: a multiple of 128, never below 128, at most `items` splits in total beyond one per head
    for lens in ([0], [1, 2, 3], LONG, RAGGED):
        for items in (1, 2, 3, 7, 252, 1024):
            c = ap.decode_chunk(lens, items)
            assert c % 128 == 0 and c >= 128
            assert sum(max(1, math.ceil(n / c)) for n in lens) <= items + len(lens)
