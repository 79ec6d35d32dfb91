"""The device memory a job holds, to the byte. Every buffer of a call lives in one arena per decode / encode batch (rbt_decode.cpp decode_lay_out, rbt_transcode.cpp
encode_lay_out) plus a few allocations of the job's own (pooled planes, occupancy maps, hash sets, merged launch lists); Context.job_memory is their sum. For a fixed list of
calls (tests/arena_footprint_worker.py, host emulation, a child process per setting of RBT_ARENA_SHARE: the switch is read once per process) it must equal what
tests/golden/arena_footprints.json recorded (tests/golden/make_arena_footprints.py): an arena a byte larger or smaller means a buffer moved, grew or went missing."""
import json
import pytest
from arena_footprint_cases import CASES, GOLDEN, build_hostemu, run


@pytest.mark.parametrize("share", ["0", "1"])
def test_job_memory_equals_the_recorded_footprint(share):
    build_hostemu()
    want = json.load(open(GOLDEN))["share_" + share]
    assert sorted(want) == sorted(CASES)
    got = run(share)
    print(got)
    assert got == want, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}
