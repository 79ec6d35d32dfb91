"""How many hardware queues the library asks the HIP runtime for (csrc/rbt_kernels.h hw_queues_wanted, used by dev_init): RBT_HW_QUEUES when it is an integer from 1 to 32,
else 16 - one per HIP stream. The helper is compiled as host code into a program of its own (tests/hw_queues_check.cpp)."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("", 16), ("1", 1), ("4", 4), ("16", 16), ("32", 32), ("33", 16), ("0", 16), ("-3", 16), ("abc", 16), ("8x", 16)]


def test_queue_request_from_the_environment():
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "hw_queues_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "hw_queues_check.cpp")], check=True)
        r = subprocess.run([exe] + [text for text, _ in CASES], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        got = [int(v) for v in r.stdout.split()]
        assert got[0] == 16, "RBT_HW_QUEUES unset"
        assert got[1:] == [want for _, want in CASES], list(zip([text for text, _ in CASES], got[1:]))
        assert max(got) <= 32
