"""Decoded picture hashes (H.265 D.3.19) restated from the text of Annex D, a NAL rewriter for hash SEIs, and the checks that
tests/test_picture_hash.py (host emulation) and tests/test_gpu_picture_hash.py (MI355X) run against a Context."""
import ctypes as C
import hashlib
import numpy as np
import oracle_lib as O
import rbt_lib
import synth

MD5, CRC, CHECKSUM = 1, 2, 3           # RBT_HASH_*: the SEI's hash_type is kind - 1
HASH_BYTES = {MD5: 16, CRC: 2, CHECKSUM: 4}
RBT_ERR_PARAM, RBT_ERR_MD5 = -4, -6


# ---------------------------------------------------------------------------------------------------- Annex D restated
def plane_bytes(plane, bit_depth):
    """pictureData of one component: one byte per sample at bit depth 8, else two (low byte first)"""
    plane = np.asarray(plane, dtype=np.uint16)
    return (plane & 0xFF).astype(np.uint8).tobytes() if bit_depth <= 8 else plane.astype("<u2").tobytes()


def crc_annex_d(data: bytes) -> int:
    """picture_crc: the bit loop of D.3.19, two zero bytes appended"""
    crc = 0xFFFF
    data = bytes(data) + b"\x00\x00"
    for bit_idx in range(len(data) * 8):
        data_byte = data[bit_idx >> 3]
        crc_msb = (crc >> 15) & 1
        bit_val = (data_byte >> (7 - (bit_idx & 7))) & 1
        crc = (((crc << 1) + bit_val) & 0xFFFF) ^ (crc_msb * 0x1021)
    return crc


def _crc_table():
    """T[v] = the register v * x^8 after eight more zero bits of the loop above (v * x^16 mod P)"""
    t = []
    for v in range(256):
        crc = v << 8
        for _ in range(8):
            msb = (crc >> 15) & 1
            crc = ((crc << 1) & 0xFFFF) ^ (msb * 0x1021)
        t.append(crc)
    return t


_T = _crc_table()


def crc_bytewise(data: bytes) -> int:
    """the same register, a byte at a time (tests check it against crc_annex_d)"""
    crc = 0xFFFF
    for b in bytes(data) + b"\x00\x00":
        crc = ((crc << 8) & 0xFFFF) ^ _T[crc >> 8] ^ b
    return crc


def checksum_annex_d(plane, bit_depth) -> int:
    """picture_checksum of D.3.19 (vectorised): sum of (byte ^ xorMask) mod 2^32"""
    plane = np.asarray(plane, dtype=np.int64)
    h, w = plane.shape
    x = np.arange(w, dtype=np.int64)[None, :]
    y = np.arange(h, dtype=np.int64)[:, None]
    mask = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8)
    s = int(((plane & 0xFF) ^ mask).sum())
    if bit_depth > 8:
        s += int(((plane >> 8) ^ mask).sum())
    return s & 0xFFFFFFFF


def planes(frame, w, h):
    frame = np.asarray(frame)
    ys, cs = w * h, (w // 2) * (h // 2)
    return [frame[:ys].reshape(h, w), frame[ys:ys + cs].reshape(h // 2, w // 2), frame[ys + cs:ys + 2 * cs].reshape(h // 2, w // 2)]


def component_hash(plane, bit_depth, kind) -> bytes:
    """one component's hash in SEI byte order (u(16) / u(32): most significant byte first)"""
    if kind == MD5:
        return hashlib.md5(plane_bytes(plane, bit_depth)).digest()
    if kind == CRC:
        return crc_bytewise(plane_bytes(plane, bit_depth)).to_bytes(2, "big")
    return checksum_annex_d(plane, bit_depth).to_bytes(4, "big")


def picture_hash(frame, w, h, bit_depth, kind):
    """-> [3][16] bytes like rbt_picture_hash (zero-padded)"""
    out = np.zeros((3, 16), np.uint8)
    for c, p in enumerate(planes(frame, w, h)):
        d = component_hash(p, bit_depth, kind)
        out[c, :len(d)] = np.frombuffer(d, np.uint8)
    return out


# ---------------------------------------------------------------------------------------------------- NAL units
def nal_units(stream: bytes):
    """Annex-B -> list of (start code, NAL unit as sent)"""
    out, i, n = [], 0, len(stream)
    starts = []
    while i + 3 <= n:
        if stream[i] == 0 and stream[i + 1] == 0 and stream[i + 2] == 1:
            sc = 4 if i > 0 and stream[i - 1] == 0 else 3
            starts.append((i + 3, sc))
            i += 3
        else:
            i += 1
    for k, (s, sc) in enumerate(starts):
        e = starts[k + 1][0] - starts[k + 1][1] if k + 1 < len(starts) else n
        out.append((sc, stream[s:e]))
    return out


def join(units) -> bytes:
    return b"".join((b"\x00\x00\x00\x01" if sc == 4 else b"\x00\x00\x01") + u for sc, u in units)


def unescape(nal: bytes) -> bytes:
    out, zeros = bytearray(), 0
    for b in nal:
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def escape(rbsp: bytes) -> bytes:
    """emulation prevention (7.4.2): 0x03 after two zero bytes in front of a byte <= 3"""
    out, zeros = bytearray(), 0
    for b in rbsp:
        if zeros >= 2 and b <= 3:
            out.append(3)
            zeros = 0
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def nal_type(u: bytes) -> int:
    return (u[0] >> 1) & 63


def hash_sei(kind, h) -> bytes:
    """suffix SEI NAL unit (as sent) with one decoded_picture_hash message (D.2.20)"""
    nb = HASH_BYTES[kind]
    payload = bytes([kind - 1]) + b"".join(bytes(h[c][:nb]) for c in range(3))
    return escape(bytes([40 << 1, 1, 132, len(payload)]) + payload + b"\x80")


def read_hash_seis(stream: bytes):
    """(kind, [3][16]) of every decoded picture hash SEI, in stream order"""
    res = []
    for _, u in nal_units(stream):
        if nal_type(u) != 40:
            continue
        r = unescape(u)
        assert r[2] == 132, "not a decoded picture hash SEI"
        size, kind = r[3], r[4] + 1
        nb = HASH_BYTES[kind]
        assert size == 1 + 3 * nb and r[4 + size] == 0x80
        h = np.zeros((3, 16), np.uint8)
        for c in range(3):
            h[c, :nb] = np.frombuffer(r[5 + c * nb:5 + (c + 1) * nb], np.uint8)
        res.append((kind, h))
    return res


def rewrite_hashes(stream: bytes, hashes, kind, flip=None) -> bytes:
    """every hash SEI of `stream` replaced (in order) by one of `kind` holding hashes[i]; flip = picture index whose first hash byte is inverted"""
    units, k = [], 0
    for sc, u in nal_units(stream):
        if nal_type(u) == 40:
            h = np.array(hashes[k], np.uint8).copy()
            if flip == k:
                h[0, 0] ^= 0xFF
            u = hash_sei(kind, h)
            k += 1
        units.append((sc, u))
    assert k == len(hashes), "one hash SEI per picture expected"
    return join(units)


def vcl(stream: bytes):
    return [u for _, u in nal_units(stream) if nal_type(u) < 32]


# ---------------------------------------------------------------------------------------------------- checks
def check_picture_hash(ctx, bit_depth, w, h, n, seed):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 1 << bit_depth, size=(n, w * h * 3 // 2), dtype=np.uint16)
    for kind in (MD5, CRC, CHECKSUM):
        got = ctx.picture_hash(frames, w, h, bit_depth, kind)
        for i in range(n):
            assert np.array_equal(got[i], picture_hash(frames[i], w, h, bit_depth, kind)), (kind, i)


def small_stream(seed=7, w=64, h=64, n_pc=2):
    geo, _, _ = synth.make_gof(w, h, n_pc, seed)
    src, _ = O.encode(geo, w, h, 10, 28, gop=2, log2_ctb=5, rows_per_slice=0, md5_sei=1)
    frames, dw, dh, bd, chk, fail = O.decode(src)
    assert (dw, dh, chk, fail) == (w, h, len(frames), 0)
    return src, frames, w, h, bd


def rewritten(src, frames, w, h, bd, kind, flip=None):
    return rewrite_hashes(src, [picture_hash(f, w, h, bd, kind) for f in frames], kind, flip)


def raw_decode(ctx, stream):
    """rbt_decode with verify_md5 = 1 through the C ABI: (return code, md5_checked, md5_failed, frames or None)"""
    R = rbt_lib.module()
    v = R.Video()
    rc = ctx.L.rbt_decode(ctx.h, stream, len(stream), 1, C.byref(v))
    frames = None
    if v.data:
        frames = np.ctypeslib.as_array(v.data, shape=(v.n_frames, v.width * v.height * 3 // 2)).copy()
        ctx.L.rbt_free(v.data)
    return rc, v.md5_checked, v.md5_failed, frames


def check_verify_kinds(ctx):
    R = rbt_lib.module()
    src, frames, w, h, bd = small_stream()
    n = len(frames)
    for kind in (MD5, CRC, CHECKSUM):
        good = rewritten(src, frames, w, h, bd, kind)
        assert [k for k, _ in read_hash_seis(good)] == [kind] * n
        rc, chk, fail, dec = raw_decode(ctx, good)
        assert (rc, chk, fail) == (0, n, 0) and np.array_equal(dec, frames), kind
        bad = rewritten(src, frames, w, h, bd, kind, flip=1)
        rc, chk, fail, dec = raw_decode(ctx, bad)
        assert (rc, chk, fail) == (RBT_ERR_MD5, n, 1), kind
        assert np.array_equal(dec, frames), "the pictures still come back"
        want = ctx.transcode_substream(good, R.RBT_VIDEO_GEOMETRY, 32, verify_md5=0)
        assert ctx.transcode_substream(good, R.RBT_VIDEO_GEOMETRY, 32, verify_md5=1) == want
        try:
            ctx.transcode_substream(bad, R.RBT_VIDEO_GEOMETRY, 32, verify_md5=1)
            raise AssertionError("a wrong %d hash passed" % kind)
        except R.RbtError as e:
            assert e.code == RBT_ERR_MD5 and "input 0" in str(e), str(e)


def check_output_kinds(ctx):
    R = rbt_lib.module()
    src, _, _, _, _ = small_stream(seed=11)
    md5_out = ctx.transcode_substream(src, R.RBT_VIDEO_GEOMETRY, 30, md5_sei=1)
    for kind in (MD5, CRC, CHECKSUM):
        out = ctx.transcode_substream(src, R.RBT_VIDEO_GEOMETRY, 30, md5_sei=kind)
        assert vcl(out) == vcl(md5_out), "the coded pictures do not depend on the hash kind"
        dec, w, h, bd, _, _ = O.decode(out)
        seis = read_hash_seis(out)
        assert len(seis) == len(dec)
        for (k, hh), f in zip(seis, dec):
            assert k == kind and np.array_equal(hh, picture_hash(f, w, h, bd, kind))
        rc, chk, fail, _ = raw_decode(ctx, out)
        assert (rc, chk, fail) == (0, len(dec), 0)
    # rbt_encode: the same kinds
    geo, _, _ = synth.make_gof(48, 32, 1, 5)
    for kind in (CRC, CHECKSUM):
        out = ctx.encode(geo, 48, 32, 10, 30, md5_sei=kind)
        dec, w, h, bd, _, _ = O.decode(out)
        assert [k for k, _ in read_hash_seis(out)] == [kind] * len(dec)
        for (_, hh), f in zip(read_hash_seis(out), dec):
            assert np.array_equal(hh, picture_hash(f, w, h, bd, kind))


def check_refused(ctx):
    R = rbt_lib.module()
    src, _, _, _, _ = small_stream(seed=3)
    geo, _, _ = synth.make_gof(32, 32, 1, 5)
    for call in (lambda: ctx.transcode_substream(src, R.RBT_VIDEO_GEOMETRY, 30, md5_sei=4),
                 lambda: ctx.transcode_substream(src, R.RBT_VIDEO_GEOMETRY, 30, md5_sei=-1),
                 lambda: ctx.encode(geo, 32, 32, 10, 30, md5_sei=4),
                 lambda: ctx.picture_hash(geo, 32, 32, 10, 4)):
        try:
            call()
            raise AssertionError("md5_sei / kind out of range accepted")
        except R.RbtError as e:
            assert e.code == RBT_ERR_PARAM
