"""CPU test of bench.py's command line: --legs, which only selects the legs of a --full run, is refused without --full
before anything touches a device."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_legs_need_full():
    r = subprocess.run([sys.executable, BENCH, "--legs", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--full" in r.stderr, r.stderr[-2000:]
