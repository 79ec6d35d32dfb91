"""rbt_d1, rbt_d2 and rbt_color_metric as upload + score + release of two temporary clouds (host/rbt_pcc.cpp) - the kernel BODIES run as serial host code
(tests/hostemu, no GPU here): refusals with their code and text, edge clouds against brute force and the oracle, rbt_d2 == the score's D2 bit for bit, the memory
after a call (tests/metric_fold_cases.py). The GPU build of the same is tests/test_gpu_metric_fold.py."""
import os
import subprocess
import tempfile
import pytest
import rbt_lib
import metric_fold_cases as MF
import pcc_cases


@pytest.fixture(scope="module")
def ctx():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(__file__), "hostemu")])
    c = rbt_lib.module().Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


@pytest.mark.parametrize("which", MF.CALLS)
def test_refusals_keep_code_and_text(ctx, which):
    MF.check_refusals(rbt_lib.module(), ctx, which)


@pytest.mark.parametrize("name", sorted(MF.edge_cases()))
def test_edge_clouds(ctx, name):
    MF.check_edge(ctx, name)


def test_the_same_array_twice(ctx):
    MF.check_same_array(ctx)


@pytest.mark.parametrize("k", range(len(pcc_cases.d2_cases())))
def test_d2_is_the_score_bit_for_bit(ctx, k):
    MF.check_d2_determinism(ctx, k)


@pytest.mark.parametrize("which", MF.CALLS)
def test_memory_after_a_call(ctx, which):
    MF.check_memory_after_success(ctx, which)


def test_host_routine_under_the_sanitizers():
    """pcc_d1, pcc_d2 and pcc_color_metric over the serial stand-ins as a stand-alone host program (tests/metric_fold_check.cpp) built with the address and
    undefined-behaviour sanitizers, through one success and each refusal: a program of its own, nothing of it is loaded into this process"""
    here = os.path.dirname(os.path.abspath(__file__)); host = os.path.join(here, "..", "rabbit-transcoding_amd", "host")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "metric_fold_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DRBT_HOSTEMU", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-Wall", "-Wno-unused-function",
                        "-Wno-unknown-pragmas", "-o", exe, os.path.join(here, "metric_fold_check.cpp"), os.path.join(here, "hostemu", "rbt_kernels_hostemu.cpp"),
                        os.path.join(host, "rbt_pcc.cpp"), os.path.join(host, "rbt_hls.cpp")], check=True, capture_output=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
