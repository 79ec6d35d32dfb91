"""How one intra transform block is coded on the host build of the kernel bodies: the cases of tests/intra_tb_cases.py, each against the oracle, the
counters that say the cases reached the code in question, and the same bodies as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/intra_tb_check.cpp). The GPU run of the same cases: tests/test_gpu_intra_tb.py."""
import ctypes
import os
import struct
import subprocess
import tempfile
import numpy as np
import pytest
import rbt_lib
import intra_tb_cases as T

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def hostemu():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "hostemu")])


@pytest.fixture(scope="module")
def R():
    return rbt_lib.module()


@pytest.fixture(scope="module")
def ctx(hostemu, R):
    c = R.Context(lib_path=rbt_lib.HOSTEMU_LIB)
    yield c
    c.close()


def counters():
    """rbt_hostemu_intra_tb of the host build (csrc/rbt_encode.h), in the order of T.COUNTERS"""
    return list((ctypes.c_uint32 * len(T.COUNTERS)).in_dll(ctypes.CDLL(rbt_lib.HOSTEMU_LIB), "rbt_hostemu_intra_tb"))


@pytest.fixture(scope="module")
def reached(hostemu):
    """what the cases of this module add to the counters: every test that codes something goes through `count`"""
    total = [0] * len(T.COUNTERS)

    def count(fn):
        a = counters(); fn(); b = counters()
        d = [y - x for x, y in zip(a, b)]
        for k, v in enumerate(d): total[k] += v
        return d
    count.total = total
    return count


@pytest.mark.parametrize("log2_ctb", [4, 5, 6])
@pytest.mark.parametrize("rows", [-1, 0, 1])
def test_ten_bit_geometry_and_attribute(ctx, reached, log2_ctb, rows):
    d = reached(lambda: T.check_ten_bit(ctx, log2_ctb, rows))
    assert d[0] > 0 and d[1] > 0          # one block or four: both ways, in every structure


@pytest.mark.parametrize("log2_ctb", [4, 5, 6])
def test_eight_bit_lossless(ctx, reached, log2_ctb):
    reached(lambda: T.check_lossless(ctx, log2_ctb))


@pytest.mark.parametrize("bd,log2_ctb,rows", [(10, 5, -1), (10, 4, 1), (10, 6, 0), (8, 5, -1)])
def test_transform_skip(ctx, reached, bd, log2_ctb, rows):
    d = reached(lambda: T.check_transform_skip(ctx, bd, log2_ctb, rows))
    assert d[3] > 0                       # 4x4 blocks took transform skip


@pytest.mark.parametrize("w,h", T.SIZES)
@pytest.mark.parametrize("log2_ctb", [5, 6])
def test_occupancy_aware_coding(ctx, R, reached, w, h, log2_ctb):
    reached(lambda: T.check_occupancy_aware(ctx, R, w, h, log2_ctb))


@pytest.mark.parametrize("w,h", T.SIZES)
@pytest.mark.parametrize("log2_ctb,rows", [(5, -1), (4, 1), (6, 0)])
def test_transcode_with_the_inputs_modes_as_hints(ctx, R, reached, w, h, log2_ctb, rows):
    reached(lambda: T.check_transcode_hints(ctx, R, w, h, log2_ctb, rows))


@pytest.mark.parametrize("k", T.QP_MAP_DECODES)
def test_qp_map_decodes_to_the_encoders_reconstruction(ctx, R, reached, k):
    reached(lambda: T.check_qp_map_decodes(ctx, R, k))


@pytest.mark.parametrize("k", T.QP_MAP_UNIFORM)
def test_uniform_qp_map_is_the_constant_qp_stream(ctx, R, reached, k):
    reached(lambda: T.check_qp_map_uniform(ctx, R, k))


def test_the_cases_reached_every_path(reached):
    """runs last in this module: over the case set every counter moved - CUs coded as one block after four were tried, CUs kept as four, mode trials the runner-up won, 4x4
    blocks with transform skip, trials that left the tile poisoned (and every stream above still equalled the oracle's: nothing read the poison)"""
    print(dict(zip(T.COUNTERS, reached.total)))
    assert len(T.QP_MAP_DECODES) == 3 and len(T.QP_MAP_UNIFORM) == 1
    assert all(v > 0 for v in reached.total), dict(zip(T.COUNTERS, reached.total))


def _case_file(path, kind, w, h, bd, qp, log2_ctb, rows, lossless):
    """one case for tests/intra_tb_check.cpp: ten int32 (w, h, bit depth, frames, qp, gop, lossless, log2_ctb, rows, bytes of the oracle's stream), the source frames
    as uint16, the oracle's stream"""
    fr = T.source(kind, w, h, bd); want = T.oracle_encode(kind, w, h, bd, qp, log2_ctb, rows, lossless)[0]
    with open(path, "wb") as f:
        f.write(struct.pack("<10i", w, h, bd, fr.shape[0], qp, 1 if lossless else 2, lossless, log2_ctb, rows, len(want)))
        f.write(np.ascontiguousarray(fr, dtype="<u2").tobytes()); f.write(want)


def test_transform_block_bodies_under_the_sanitizers():
    """Two of the small cases coded by the host build of the kernel bodies as a stand-alone program (tests/intra_tb_check.cpp with the host emulation's sources) built with
    the address and undefined-behaviour sanitizers: the LDS structs are plain objects there, and an index past the end of the two arrays that went is an error, not a
    neighbour's sample. A program of its own, run as a child process: nothing of it is loaded into this one."""
    root = os.path.dirname(HERE); lib = os.path.join(root, "rabbit-transcoding_amd", "host")
    srcs = [os.path.join(HERE, "intra_tb_check.cpp"), os.path.join(HERE, "hostemu", "rbt_kernels_hostemu.cpp")] + [os.path.join(lib, n) for n in
            ("rbt_hls.cpp", "rbt_decode.cpp", "rbt_transcode.cpp", "rbt_pcc.cpp", "rbt_api.cpp", "rbt_v3c.cpp")]
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "intra_tb_check")
        # C++20: the codec's arithmetic shifts negative residuals left as H.265 writes it (the transform-skip scaling, from before this test), which the language defines
        # since C++20 and the sanitizer reports under C++17; everything else of -fsanitize=undefined is on
        flags = ["-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-DRBT_HOSTEMU", "-Wall", "-Wno-unused-function",
                 "-Wno-unknown-pragmas", "-Wno-unused-variable"]
        objs = [os.path.join(td, "%d.o" % k) for k in range(len(srcs))]
        jobs = [subprocess.Popen(["g++"] + flags + ["-c", s, "-o", o]) for s, o in zip(srcs, objs)]      # the eight sources side by side: the build is most of this test's time
        assert [j.wait() for j in jobs] == [0] * len(jobs)
        subprocess.run(["g++"] + flags + ["-o", exe] + objs, check=True)
        a, b = os.path.join(td, "steps.case"), os.path.join(td, "attr.case")
        _case_file(a, "steps", 96, 80, 10, 24, 5, -1, 0)       # transform skip, partial CTBs
        _case_file(b, "attr", 96, 80, 10, 32, 6, 0, 0)         # 64x64 CTBs partial on both edges: 32x32 blocks, the coded mode trial, Cb / Cr pairs as quarters
        r = subprocess.run([exe, a, b], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
