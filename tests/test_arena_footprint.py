"""The device memory a job holds, to the byte. Every buffer of a call lives in one arena per decode / encode batch (rbt_decode.cpp decode_lay_out, rbt_transcode.cpp
encode_lay_out) plus a few allocations of the job's own (pooled planes, occupancy maps, hash sets, merged launch lists); Context.job_memory is their sum. For a fixed list of
calls (tests/arena_footprint_worker.py, host emulation, a child process per setting of RBT_ARENA_SHARE: the switch is read once per process) it must equal what
tests/golden/arena_footprints.json recorded (tests/golden/make_arena_footprints.py): an arena a byte larger or smaller means a buffer moved, grew or went missing."""
import json
import os
import re
import subprocess
import sys
import pytest

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


@pytest.mark.parametrize("share", ["0", "1"])
def test_job_memory_equals_the_recorded_footprint(share):
    build_hostemu()
    want = json.load(open(GOLDEN))["share_" + share]
    assert sorted(want) == sorted(CASES)
    got = run(share)
    print(got)
    assert got == want, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}
