"""-m gpu: what a plain `bench.py` run does against `bench.py --full` (small view count, one timed step)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ("secondary", "parity", "e2e", "e2e_error", "cpu_baseline", "preflight", "comm", "second_form")


def bench_line(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--views", "2", "--steps", "1", "--warmup", "1"] + list(args),
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_prints_the_headline_alone_and_full_adds_the_rest():
    plain = bench_line()
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["steps"] == 1 and plain["warmup"] == 1
    assert plain["roofline"]["launches_timed"] > 0
    assert not [k for k in EXTRAS if k in plain], plain.keys()
    full = bench_line("--full", "--no-cpu-baseline")
    assert full["parity"]["S2"]["finite"] and max(full["parity"]["S2"]["max_rel"]) <= 3e-2
    assert full["e2e"]["views"] == 2 and full["e2e"]["frames_per_s"] > 0
    assert "cpu_baseline" not in full
