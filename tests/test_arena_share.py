"""Arena sharing on against off. The encoder keeps its coefficient levels and its reconstruction in buffers of the decoded input picture that are dead by then
(rbt_transcode.cpp setup_encode; RBT_ARENA_SHARE=0 gives it memory of its own). That is right only while the encoder's first write to a picture is ordered behind the
decoder's last read of it, so the same transcodes run with the switch off and on (tests/arena_share_worker.py, a child process each: the switch is read once per process)
and must give the same bytes - which the worker also holds against the oracle for the small cases."""
import os
import re
import subprocess
import sys
import pytest

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "arena_share_worker.py")


def run(kind, share, timeout):
    r = subprocess.run([sys.executable, WORKER, kind], env=dict(os.environ, RBT_ARENA_SHARE=share), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (share, r.stdout[-500:], r.stderr[-3000:])
    digests = dict(re.findall(r"^DIGEST (\S+) (\S+)$", r.stdout, re.M))
    mem = int(re.search(r"^MEM (\d+)$", r.stdout, re.M).group(1))
    assert re.search(r"^OK %d$" % len(digests), r.stdout, re.M), r.stdout[-500:]
    return digests, mem


def check(kind, names, timeout):
    off, mem_off = run(kind, "0", timeout)
    on, mem_on = run(kind, "1", timeout)
    assert sorted(off) == sorted(on) == sorted(names)
    assert off == on, "outputs depend on RBT_ARENA_SHARE: %s" % [k for k in off if off[k] != on[k]]
    assert mem_off > mem_on, "the switch changed nothing: the job holds %d bytes with sharing off, %d with it on" % (mem_off, mem_on)


def test_arena_sharing_on_equals_off_hostemu():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    check("hostemu", ["gof", "fanout", "window", "md5", "depth16"], 600)


@pytest.mark.gpu
def test_arena_sharing_on_equals_off_gpu():
    """the same list on the GPU, where the order of the two pictures' accesses is the order of kernels on HIP streams and events between them; plus the first GOF of the
    committed 1280 x 1280 fixture (its digest is compared between the two runs; tests/test_gpu_fullsize.py holds sixteen-frame parts of that fixture against the oracle)"""
    check("gpu", ["gof", "fanout", "window", "md5", "depth16", "fixture"], 600)
