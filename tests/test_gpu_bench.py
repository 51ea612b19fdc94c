"""GPU: bench.py end to end at a small size.  A plain run does only what its headline needs (set-up, warm-up, timed steps,
--dump-outputs, the result line); --full adds decode, the ragged decode layer, the box's copy rates and the CPU baseline with its
parity sample, and exits 0 only when that sample holds the bounds."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--model", "qwen2.5-0.5b", "--ctx", "8192", "--decode-tokens", "4"]
N_CTX = 8192


def _bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    lines = p.stdout.strip().splitlines()
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    d = json.loads(lines[0])
    assert d["metric"] == "kv_tokens_scored_and_pruned_per_s" and d["unit"] == "tokens/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f16" and d["steps"] == 2 and d["warmup"] == 1
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(N_CTX / (d["ms_per_step"] / 1e3), rel=1e-9)
    assert d["roofline_stages"]["score_rowstat"]["launches"] > 0 and d["roofline_stages"]["compact_gather"]["launches"] > 0
    return d


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path))
    assert d["config"]["full"] is False
    assert d["decode"] is None and d["cpu_baseline"] is None and "parity_sample" not in d and "parity_ok" not in d
    assert not any(k.startswith("decode_varlen_attn") for k in d["roofline_stages"])
    assert d["config"]["hbm_copy_GBps_this_box"] is None
    assert sorted(os.listdir(tmp_path)) == sorted(f"{n}.npy" for n in ("threshold", "real_ratio", "len_k", "score", "valid", "key", "value"))


@pytest.mark.gpu
def test_bench_full_run_measures_and_checks_the_rest():
    d = _bench("--full")
    assert d["config"]["full"] is True
    dec = d["decode"]
    assert dec["tokens"] == 4 and dec["ms_per_token"] > 0 and dec["ms_per_token_hip_graph"] > 0
    st = d["roofline_stages"]
    assert st["decode_varlen_attn"]["launches"] > 0 and st["decode_varlen_attn_ragged"]["launches"] > 0
    assert d["config"]["hbm_copy_GBps_this_box"] > 0 and st["compact_gather"]["frac_of_box_copy_kernel"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["parity_ok"] is True and d["parity_sample"]["violations"] == []
