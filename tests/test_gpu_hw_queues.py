"""The library's request for hardware queues holds against a value the environment already has: a process started with GPU_MAX_HW_QUEUES=4 has 16 there once its first
context exists (RBT_HW_QUEUES chooses another count from 1 to 32; anything else means 16), and transcodes as before. The request is read once per process, so every case
runs in a worker (tests/hw_queues_worker.py). This checks the request only; what the runtime makes of it shows in a kernel trace (profiles/r06_queues.txt)."""
import os
import subprocess
import sys
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("asked,want", [(None, "16"), ("8", "8"), ("64", "16")])
def test_queue_request_overwrites_the_environment(asked, want):
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    env.pop("RBT_HW_QUEUES", None)
    if asked is not None: env["RBT_HW_QUEUES"] = asked
    r = subprocess.run([sys.executable, os.path.join(HERE, "hw_queues_worker.py"), want], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "ok " + want, r.stdout[-2000:] + r.stderr[-2000:]
