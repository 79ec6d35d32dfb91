"""What tests/test_arena_footprint.py checks and tests/golden/make_arena_footprints.py records: the host build, one run of tests/arena_footprint_worker.py per setting
of RBT_ARENA_SHARE (a child process: the switch is read once per process), and the file the figures are kept in."""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "arena_footprint_worker.py")
GOLDEN = os.path.join(HERE, "golden", "arena_footprints.json")
CASES = ["gof128_r3", "gof256_r3", "window_occ_40x44", "window_geo_152x104", "fanout", "rows_wave", "rows_1", "md5", "depth16_merged"]


def build_hostemu():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "hostemu")])


def run(share):
    r = subprocess.run([sys.executable, WORKER], env=dict(os.environ, RBT_ARENA_SHARE=share), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (share, r.stdout[-500:], r.stderr[-3000:])
    mem = {k: int(v) for k, v in re.findall(r"^MEM (\S+) (\d+)$", r.stdout, re.M)}
    assert re.search(r"^OK %d$" % len(mem), r.stdout, re.M), r.stdout[-500:]
    return mem
