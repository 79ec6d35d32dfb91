"""Streams for the two instantiations of the slice parser (csrc/rbt_parse.h: the intra-only one for I slices, the general one for P slices), shared by
tests/test_gpu_parser_intra_path.py (the HIP build) and tests/test_hostemu_parser_intra_path.py (the same source as host code). gop=1 streams hold I slices only;
gop=2 streams alternate I and P pictures, and the P slices predict from the I picture before them, temporal candidates included - so the motion maps an I slice
leaves behind (mv 0, ref -1, no reference POC) are read by the general parser and by the deblocking. Every case decodes with ctx.decode and compares with the
oracle encoder's reconstruction (the decoder's per-4x4 maps are not reachable through the C ABI; what reads them - the P pictures, the loop filter - is)."""
import functools
import numpy as np
import oracle_lib as O
import synth

# three CTB columns at 64x64 (left, above, above-right neighbours and the last column all occur); 200x136 ends in a partial CTB on both edges
SIZES = [(192, 128), (200, 136)]
LOG2_CTBS = [6, 5, 4]
ROWS = [1, 0, -1, -2]     # one CTB row per slice, one slice per picture, wavefront rows as dependent slice segments, wavefront rows behind entry points
GRID = [(w, h, l, r) for (w, h) in SIZES for l in LOG2_CTBS for r in ROWS]
STRESS_SEEDS = [3, 7, 12, 22]   # random syntax (tests/parity_cases.py check_stress_decode): 30 % of the CUs of a P slice are intra CUs, with dQP, TS, SAO, NxN ...


@functools.lru_cache(maxsize=None)
def content(w, h):
    """three pictures of atlas-like content with detail (the second close to the first, so that the P picture finds motion)"""
    m = synth.make_maps(256, 192, 77)["attr"]
    y = m[:, :256 * 192].reshape(2, 192, 256)[:, :h, :w]; c = m[:, 256 * 192:].reshape(2, 2, 96, 128)[:, :, :h // 2, :w // 2]
    r = np.random.default_rng(w * 1000 + h)
    fr = np.stack([np.concatenate([y[i % 2].reshape(-1), c[i % 2].reshape(-1)]) for i in range(3)]).astype(np.int64)
    fr[1] = fr[0] + r.integers(-3, 4, fr[0].shape); fr[2] = fr[2] + r.integers(-24, 25, fr[2].shape)
    out = np.clip(fr, 0, 1023).astype(np.uint16); out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def grid_stream(w, h, log2_ctb, rows, gop):
    return O.encode(content(w, h), w, h, 10, 27, gop=gop, log2_ctb=log2_ctb, rows_per_slice=rows)


def check_grid(ctx, w, h, log2_ctb, rows, gop):
    bs, rec = grid_stream(w, h, log2_ctb, rows, gop)
    dec, dw, dh, bd, chk, fail = ctx.decode(bs)
    assert (dw, dh, bd, chk, fail) == (w, h, 10, 3, 0)
    assert np.array_equal(dec, rec)


def check_stress(ctx, seed):
    w = [64, 96, 128, 80][seed % 4]; h = [64, 80, 48, 128][(seed // 4) % 4]
    bd = 10 if seed % 3 else 8
    bs, rec = O.encode(np.zeros((5, w * h * 3 // 2), np.uint16), w, h, bd, qp=30, gop=2, stress_seed=seed, log2_ctb=0)
    dec, dw, dh, dbd, chk, fail = ctx.decode(bs)
    assert (dw, dh, dbd, chk, fail) == (w, h, bd, 5, 0) and np.array_equal(dec, rec)


def check_lossless(ctx):
    fr = np.random.default_rng(64).integers(0, 256, size=(2, 64 * 64 * 3 // 2), dtype=np.uint16)
    for log2_ctb, rows in ((6, 0), (5, -1), (4, 1)):
        bs, rec = O.encode(fr, 64, 64, 8, 8, gop=1, lossless=1, i_qp_offset=0, log2_ctb=log2_ctb, rows_per_slice=rows)
        dec, dw, dh, bd, chk, fail = ctx.decode(bs)
        assert (dw, dh, bd, chk, fail) == (64, 64, 8, 2, 0) and np.array_equal(dec, rec) and np.array_equal(dec, fr)


# RBT_PARSE_BANDS is read once per process: the banded (suspend / resume) parse of both instantiations runs in a child; `lib` is the library path or None
BANDS_CODE = """
import sys; sys.path.insert(0, 'tests')
import numpy as np, rbt_lib, oracle_lib as O, parser_intra_path_cases as K
R = rbt_lib.module(); c = R.Context(lib_path=%r) if %r else R.Context(device=0)
for gop in (1, 2):
    bs, rec = K.grid_stream(200, 136, 5, 0, gop)
    assert c.transcode_substream(bs, R.RBT_VIDEO_ATTRIBUTE, 32) == O.transcode_substream(bs, 19, 32)
print('OK')
"""


def run_banded(lib):
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", BANDS_CODE % (lib, lib)], cwd=root, env=dict(os.environ, RBT_PARSE_BANDS="2"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-500:], r.stderr[-2000:])
