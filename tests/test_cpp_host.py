"""The C ABI driven from C++ (the reference's language): examples/rbt_pipeline.cpp walks GOFs with rbt_submit_gof ahead of
rbt_wait_gof, the way INTEGRATION.md patches the application's GOF loop. CPU: it must fail loudly without a GPU. GPU: its outputs
must equal the oracle's."""
import os
import struct
import subprocess
import numpy as np
import pytest
import oracle_lib as O
from parity_cases import r5_gof

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rabbit-transcoding_amd", "rbt_pipeline")


def _exe():
    if not os.path.exists(EXE):
        pytest.skip("rbt_pipeline not built (make -C rabbit-transcoding_amd)")
    return EXE


def _write(path, gofs):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(gofs)))
        for g in gofs:
            for s in g:
                f.write(struct.pack("<I", len(s))); f.write(s)


def _read(path):
    b = open(path, "rb").read(); n, = struct.unpack_from("<I", b, 0); o = 4; gofs = []
    for _ in range(n):
        g = []
        for _ in range(3):
            sz, = struct.unpack_from("<I", b, o); o += 4; g.append(b[o:o + sz]); o += sz
        gofs.append(g)
    return gofs


def _gofs(n):
    out = []
    for k in range(n):
        w, h = [(64, 64), (128, 64), (96, 96)][k % 3]
        out.append(r5_gof(w, h, 1 + k % 2, 700 + k)[0])
    return out


def test_cpp_host_fails_loudly_without_a_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    _write(tmp_path / "in.gofs", _gofs(1))
    r = subprocess.run([_exe(), str(tmp_path / "in.gofs"), str(tmp_path / "out.gofs")], capture_output=True, text=True)
    assert r.returncode == 1 and "no usable HIP device" in r.stderr and not (tmp_path / "out.gofs").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 3, 16])
def test_cpp_host_pipeline_equals_oracle(tmp_path, depth):
    gofs = _gofs(7)
    _write(tmp_path / "in.gofs", gofs)
    subprocess.check_call([_exe(), str(tmp_path / "in.gofs"), str(tmp_path / "out.gofs"), str(depth)])
    got = _read(tmp_path / "out.gofs")
    assert len(got) == len(gofs)
    for g, o in zip(gofs, got):
        assert o[0] == O.transcode_substream(g[0], 0, 8, rows_per_slice=-1) and o[1] == O.transcode_substream(g[1], 1, 24, rows_per_slice=-1) and o[2] == O.transcode_substream(g[2], 19, 32, rows_per_slice=-1)


@pytest.mark.gpu
def test_cpp_host_v3c_file_equals_oracle(tmp_path):
    """the file-level form (rbt_pipeline --v3c): V3C sample stream in, V3C sample stream out == the oracle's restatement of PccAppTranscoder's loop"""
    import v3c_synth as V
    units = []
    for g, s in enumerate(_gofs(5)):
        units += V.gof_units(s, 40 + g, aux=(g == 2))
    data = V.sample_stream(units, 3)
    (tmp_path / "in.bin").write_bytes(data)
    r = subprocess.run([_exe(), "--v3c", str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "4", "28", "37"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.bin").read_bytes() == O.v3c_transcode(data, 28, 37, 4)
    assert r.stdout.startswith("5 GOFs, 27 units;") and f"total {len(data)} ->" in r.stdout


def test_cpp_host_v3c_fails_loudly_without_a_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    (tmp_path / "in.bin").write_bytes(bytes([0x40]))
    r = subprocess.run([_exe(), "--v3c", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 1 and "no usable HIP device" in r.stderr and not (tmp_path / "out.bin").exists()


MULTI = os.path.join(ROOT, "rabbit-transcoding_amd", "rbt_multi_gpu")


@pytest.mark.gpu
@pytest.mark.parametrize("occupancy_rd", [0, 1])
def test_cpp_multi_gpu_host_one_rank_equals_oracle(tmp_path, occupancy_rd):
    """examples/rbt_multi_gpu.cpp --ranks 1: a parent that never touches the GPU starts the rank as a fresh process; the rank transcodes the GOFs its context owns
    (rbt_transcode_v3c), the parts are gathered on rank 0 through RCCL (ncclAllGather of sizes, grouped ncclSend / ncclRecv - here a communicator of one) and merged
    with rbt_v3c_index + rbt_v3c_write. Output == the oracle's walk of the same file, with and without occupancy-aware coding. More ranks need more GPUs than a box has."""
    if not os.path.exists(MULTI):
        pytest.skip("rbt_multi_gpu not built (make -C rabbit-transcoding_amd)")
    import v3c_synth as V
    units = []
    for g, s in enumerate(_gofs(5)):
        units += V.gof_units(s, 60 + g)
    data = V.sample_stream(units, 3)
    (tmp_path / "in.bin").write_bytes(data)
    r = subprocess.run([MULTI, "--ranks", "1", str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "4", "24", "32", "4", str(occupancy_rd)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.bin").read_bytes() == O.v3c_transcode(data, 24, 32, 4, occupancy_rd=occupancy_rd)
    assert "1 ranks, 5 GOFs:" in r.stdout          # (RCCL prints its version banner first)


def test_cpp_multi_gpu_host_fails_loudly_without_a_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    if not os.path.exists(MULTI):
        pytest.skip("rbt_multi_gpu not built")
    (tmp_path / "in.bin").write_bytes(bytes([0x40]))
    r = subprocess.run([MULTI, "--ranks", "2", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "no usable HIP device" in r.stderr and not (tmp_path / "out.bin").exists()


def _multi():
    if not os.path.exists(MULTI):
        pytest.skip("rbt_multi_gpu not built")
    return MULTI


@pytest.mark.parametrize("mode,ranks,want_rc,needle", [("ok", 3, 0, ""), ("fail:1", 2, 1, "rank 1 failed"), ("fail:0", 4, 1, "rank 0 failed"), ("hang:2", 3, 1, "deadline of 2 s passed")])
def test_cpp_multi_gpu_host_never_hangs_on_a_failed_or_silent_rank(tmp_path, mode, ranks, want_rc, needle):
    """round-3 review: a rank that failed before ncclCommInitRank left its peers blocked there and the parent in waitpid for ever. Now every rank publishes a status
    before anything of RCCL and enters the communicator only when all said ok; the parent reaps with waitpid(-1), raises an abort flag on the first failure or at its
    deadline and kills what is left. Exercised without a device through --selftest (status round, abort flag and supervision only): everything ends within seconds."""
    import time
    t0 = time.time()
    r = subprocess.run([_multi(), "--ranks", str(ranks), "--timeout", "2", "--selftest", mode, "x", "y"], capture_output=True, text=True, timeout=60)
    assert r.returncode == want_rc, (r.returncode, r.stderr)
    assert needle in r.stderr and time.time() - t0 < 15
    assert not [d for d in os.listdir("/tmp") if d.startswith("rbt_multi_gpu_") and os.path.exists(os.path.join("/tmp", d, "status.0"))]      # the scratch directory is cleaned up


@pytest.mark.gpu
def test_cpp_multi_gpu_host_reports_a_damaged_input(tmp_path):
    """--ranks 1 on a file whose geometry unit is damaged: non-zero exit with the library's message, no output file"""
    import v3c_synth as V
    units = []
    for g, s in enumerate(_gofs(2)):
        units += V.gof_units(s, 90 + g)
    bad = bytearray(units[3]); bad[40:len(bad) // 2] = bytes(len(bad) // 2 - 40); units[3] = bytes(bad)          # the first GOF's geometry video: slice data zeroed
    (tmp_path / "in.bin").write_bytes(V.sample_stream(units, 3))
    r = subprocess.run([_multi(), "--ranks", "1", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "rbt_transcode_v3c:" in r.stderr and not (tmp_path / "out.bin").exists()
