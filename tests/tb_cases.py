"""Transform-block cases for rbt_selftest_tb (one block through the decoder's rc_tile_tb / rc_tile_tb_cpair) and the comparison with tests/tb_spec.py (H.265's text in
exact integers). ONE list, fixed seeds, shared by the serial host build of the bodies (tests/test_tb_spec.py) and the device (tests/test_gpu_tb_spec.py).

Residual: every (size, bit depth, DST / DCT / skip / bypass, luma and the Cb/Cr pair) at QP 0, 5, 6, 51, 51 + 6 (bd - 8) with uniformly random int16 levels, levels from
{-32768, 0, 32767}, 5 %-sparse levels, small levels, a single DC coefficient and basis-aligned blocks outer(sign(T[:, y]), sign(T[:, x])) * a - the ones that reach the largest
residual a size can have ((largest column sum of |T| * 32768) >> (20 - bd): 59584 at 32x32 10 bit, the only one beyond int16); the pair with only Cb, only Cr and both coded
at different qP. Intra blocks among them carry random neighbours and a rotating mode, so the add-and-clip of the prediction pass sees residuals far beyond +-2^bd.
Intra: all 35 modes x every size x both bit depths on random neighbours; neighbours all 0, all 2^bd - 1 (16x16 chroma DC: the packed 16+16-bit sum within 0.1 % of the sign
bit), a ramp; the two conditions of strong smoothing at 32x32 from both sides; twelve availability patterns (several with more than one run: the find-last-set path of
rc_nb_source); the block at the CTB's top-left, top edge, left edge, interior and bottom row of CTBs of 16, 32 and 64.

Availability is positional: a unit below the CTB, or right of the CTB in one of the CTB's own rows, is never available (legal_units); the patterns are masked with that."""
import functools
import numpy as np
import tb_spec as S

LUMA, CB, CR, PAIR = 0, 1, 2, 3
NB, UNITS = 129, 33
H_KIND, H_LOG2, H_BD, H_CTB, H_X0, H_Y0, H_STRONG, H_INTRA, H_MODE, H_CBF0, H_CBF1, H_TS, H_BYP, H_QP0, H_QP1 = range(15)


def unit_geometry(kind, log2):
    """(samples per unit, units per 2N samples, units in all)"""
    us = 4 if kind == LUMA else 2
    nu = (2 << log2) // us
    return us, nu, 2 * nu + 1


def unit_of_sample(kind, log2):
    """for each of the 4N+1 reference samples the index of its unit"""
    us, nu, _ = unit_geometry(kind, log2)
    two_n = 2 << log2
    return np.array([i // us if i < two_n else (nu if i == two_n else nu + 1 + (i - two_n - 1) // us) for i in range(2 * two_n + 1)])


def legal_units(kind, log2, log2_ctb, x0, y0):
    """the units that CAN be available at this position: not below the CTB's bottom, not right of the CTB in a row of the CTB itself"""
    us, nu, total = unit_geometry(kind, log2)
    nn = (1 << log2_ctb) >> (kind != LUMA)
    two_n = 2 << log2
    ok = np.zeros(total, dtype=bool)
    for p in range(total):
        if p < nu:
            ok[p] = y0 + two_n - 1 - p * us < nn
        elif p == nu:
            ok[p] = True
        else:
            ok[p] = y0 == 0 or x0 + (p - nu - 1) * us < nn
    return ok


def positions(kind, log2):
    """(log2_ctb, x0, y0): top-left, top edge, left edge, interior, bottom row of CTBs of 16, 32, 64 (samples of the block's component)"""
    n, out = 1 << log2, []
    for log2_ctb in (4, 5, 6):
        nn = (1 << log2_ctb) >> (kind != LUMA)
        if n > nn:
            continue
        cand = [(0, 0), (nn - n, 0), (0, n), (n, n), (n, nn - n), (0, nn - n)]
        for x0, y0 in cand:
            if x0 + n <= nn and y0 + n <= nn and (log2_ctb, x0, y0) not in out:
                out.append((log2_ctb, x0, y0))
    return out


AVAIL_PATTERNS = ("all", "none", "corner", "left", "above", "no_below_left", "no_above_right", "late_first", "even", "odd", "pairs", "random")


def avail_pattern(name, nu, total, rng):
    p = np.arange(total)
    if name == "all": return np.ones(total, bool)
    if name == "none": return np.zeros(total, bool)
    if name == "corner": return p == nu
    if name == "left": return p < nu
    if name == "above": return p > nu
    if name == "no_below_left": return p >= nu // 2
    if name == "no_above_right": return p <= nu + nu // 2
    if name == "late_first": return (p >= 1) & (p != nu + 1)                 # first available unit is not unit 0, and a hole after the corner: two runs
    if name == "even": return p % 2 == 0
    if name == "odd": return p % 2 == 1
    if name == "pairs": return (p // 2) % 2 == 1
    return rng.random(total) < 0.5


class Cases:
    def __init__(self):
        self.hdr, self.nb, self.uav, self.lev, self.ids, self.groups = [], [], [], [], [], []

    def add(self, group, kind, log2, bd, pos, strong, intra, mode, cbf, ts, byp, qp, nb, uav, lev):
        log2_ctb, x0, y0 = pos
        n, (_, _, total) = 1 << log2, unit_geometry(kind, log2)
        h = np.zeros(16, np.int32)
        h[:15] = (kind, log2, bd, log2_ctb, x0, y0, strong, intra, mode, cbf[0], cbf[1], ts, byp, qp[0], qp[1])
        a = np.zeros((2, NB), np.uint16); u = np.zeros(UNITS, np.uint8); l = np.zeros((2, 1024), np.int16)
        u[:total] = np.asarray(uav, bool) & legal_units(kind, log2, log2_ctb, x0, y0)
        for b in range(2 if kind == PAIR else 1):
            a[b, :4 * n + 1] = nb[b]
            l[b, :n * n] = np.asarray(lev[b]).reshape(-1)
        self.ids.append("%s/%d" % (group, len(self.ids))); self.groups.append(group)
        self.hdr.append(h); self.nb.append(a); self.uav.append(u); self.lev.append(l)

    def freeze(self):
        self.hdr = np.stack(self.hdr); self.nb = np.stack(self.nb); self.uav = np.stack(self.uav); self.lev = np.stack(self.lev)
        return self


def _levels(kind_of, n, use_dst, rng):
    if kind_of == "uniform": return rng.integers(-32768, 32768, (n, n))
    if kind_of == "extreme": return rng.choice(np.array([-32768, 0, 32767]), (n, n))
    if kind_of == "sparse": return np.where(rng.random((n, n)) < 0.05, rng.integers(-32768, 32768, (n, n)), 0)
    if kind_of == "small": return rng.integers(-300, 301, (n, n))
    if kind_of == "dc":
        l = np.zeros((n, n), np.int64); l[0, 0] = rng.integers(-32768, 32768); return l
    t = S.DST if use_dst else S.DCT[n]                                                # basis-aligned: every product of both stages has the sign of the target sample's
    y, x = rng.integers(0, n, 2)
    a = int(rng.integers(1, 32768)) * (1 if rng.random() < 0.5 else -1)
    return np.clip(np.outer(np.sign(t[:, y]), np.sign(t[:, x])) * a, -32768, 32767)


LEVEL_KINDS = ("uniform", "extreme", "sparse", "small", "dc", "basis")
NAMES = {LUMA: "luma", CB: "cb", CR: "cr", PAIR: "pair"}


def _neighbours(rng, n, bd, planes):
    return [rng.integers(0, 1 << bd, 4 * n + 1) for _ in range(planes)]


@functools.lru_cache(maxsize=None)
def build():
    C = Cases()
    rng = np.random.default_rng(20260265)
    modes_cycle = (1, 0, 26, 10, 2, 34, 18, 7, 15, 21, 29)
    k = 0
    # ---------------------------------------------------------------------------------------------- residual (intra ones: prediction + residual)
    for bd in (8, 10):
        qps = sorted({0, 5, 6, 51, 51 + 6 * (bd - 8)})
        for kind, sizes in ((LUMA, (2, 3, 4, 5)), (PAIR, (2, 3, 4))):
            planes = 2 if kind == PAIR else 1
            for log2 in sizes:
                n = 1 << log2; P = positions(kind, log2); _, nu, total = unit_geometry(kind, log2)
                for is_intra in (0, 1):
                    use_dst = kind == LUMA and log2 == 2 and is_intra
                    group = "res-%s-n%d-bd%d-%s-%s" % (NAMES[kind], n, bd, "dst" if use_dst else "dct", "intra" if is_intra else "inter")
                    reps = 3 if (log2 == 5 and bd == 10) else 1                        # the one size and depth whose residual can pass 32767
                    for lk in LEVEL_KINDS:
                        for qi, qp in enumerate(qps * (reps if lk in ("basis", "uniform", "extreme") else 1)):
                            k += 1
                            cbf = (1, 0) if kind == LUMA else ((1, 0), (0, 1), (1, 1))[k % 3]
                            qp2 = qps[(qi + 1 + k) % len(qps)] if qps[(qi + 1 + k) % len(qps)] != qp else qps[(qi + 2 + k) % len(qps)]
                            lev = [_levels(lk, n, use_dst, rng) if (cbf[b] or is_intra) else np.zeros((n, n), np.int64) for b in range(planes)]
                            C.add(group, kind, log2, bd, P[k % len(P)], 0, is_intra, modes_cycle[k % len(modes_cycle)] if is_intra else 0, cbf, 0, 0, (qp, qp2),
                                  _neighbours(rng, n, bd, planes), np.ones(total, bool), lev)
                    # cu_transquant_bypass: the levels are the residual
                    for lk in LEVEL_KINDS:
                        k += 1
                        cbf = (1, 0) if kind == LUMA else ((1, 0), (0, 1), (1, 1))[k % 3]
                        lev = [_levels(lk, n, use_dst, rng) if (cbf[b] or is_intra) else np.zeros((n, n), np.int64) for b in range(planes)]
                        C.add("bypass-%s-n%d-bd%d-%s" % (NAMES[kind], n, bd, "intra" if is_intra else "inter"), kind, log2, bd, P[k % len(P)], 0, is_intra,
                              modes_cycle[k % len(modes_cycle)] if is_intra else 0, cbf, 0, 1, (qps[k % len(qps)], qps[(k + 1) % len(qps)]), _neighbours(rng, n, bd, planes), np.ones(total, bool), lev)
        # transform skip: 4x4, one plane at a time (the decoder takes Cb / Cr with a skipped block through rc_tile_tb)
        for kind in (LUMA, CB, CR):
            P = positions(kind, 2); _, nu, total = unit_geometry(kind, 2)
            for is_intra in (0, 1):
                for lk in LEVEL_KINDS:
                    for qp in qps:
                        k += 1
                        C.add("skip-%s-n4-bd%d-%s" % (NAMES[kind], bd, "intra" if is_intra else "inter"), kind, 2, bd, P[k % len(P)], 0, is_intra, modes_cycle[k % len(modes_cycle)] if is_intra else 0,
                              (1, 0), 1, 0, (qp, qp), _neighbours(rng, 4, bd, 1), np.ones(total, bool), [_levels(lk, 4, False, rng)])
    # ---------------------------------------------------------------------------------------------- intra prediction alone (cbf = 0)
    for bd in (8, 10):
        maxv = (1 << bd) - 1
        for kind, sizes in ((LUMA, (2, 3, 4, 5)), (PAIR, (2, 3, 4))):
            planes = 2 if kind == PAIR else 1
            for log2 in sizes:
                n = 1 << log2; P = positions(kind, log2); _, nu, total = unit_geometry(kind, log2)
                garbage = lambda: [rng.integers(-32768, 32768, (n, n)) for _ in range(planes)]      # cbf = 0: whatever lies where the samples will be is not looked at
                tag = "%s-n%d-bd%d" % (NAMES[kind], n, bd)
                for mode in range(35):                                                  # every mode, random neighbours, rotating pattern and position
                    k += 1
                    C.add("modes-" + tag, kind, log2, bd, P[k % len(P)], k & 1, 1, mode, (0, 0), 0, 0, (0, 0), _neighbours(rng, n, bd, planes),
                          avail_pattern(AVAIL_PATTERNS[k % len(AVAIL_PATTERNS)] if k % 3 else "all", nu, total, rng), garbage())
                for mode in (0, 1, 2, 10, 18, 26, 34):                                  # flat and ramp content, everything available that can be
                    for content in ("zero", "max", "ramp"):
                        k += 1
                        ramp = np.arange(4 * n + 1) * maxv // (4 * n)
                        nb = [np.zeros(4 * n + 1, np.int64) if content == "zero" else np.full(4 * n + 1, maxv) if content == "max" else (ramp if b == 0 else ramp[::-1]) for b in range(planes)]
                        pos = [p for p in P if legal_units(kind, log2, *p).all()] if content == "max" else P
                        C.add("content-" + tag, kind, log2, bd, (pos or P)[k % len(pos or P)], 1, 1, mode, (0, 0), 0, 0, (0, 0), nb, np.ones(total, bool), garbage())
                for pat in AVAIL_PATTERNS:                                             # availability patterns where as much as possible of them is legal: top edge of the largest CTB
                    for mode in (0, 1, 14, 30):
                        k += 1
                        tops = [p for p in P if p[0] == 6 and p[2] == 0]
                        C.add("avail-" + tag, kind, log2, bd, tops[k % len(tops)] if k % 4 else P[k % len(P)], 1, 1, mode, (0, 0), 0, 0, (0, 0), _neighbours(rng, n, bd, planes),
                              avail_pattern(pat, nu, total, rng), garbage())
        # strong intra smoothing (8.4.4.2.3, 32x32 luma): both sides of `< 1 << (bd - 5)` on each of the two conditions, flag on and off; everything available
        thr = 1 << (bd - 5); c0 = 1 << (bd - 1)
        i = np.arange(129)
        for strong in (0, 1):
            for what, d in (("linear", 0), ("top_end", thr), ("top_end", thr - 1), ("top_end", -thr), ("left_end", thr), ("left_end", thr - 1), ("left_end", -(thr - 1)), ("corner", thr), ("corner", thr - 1)):
                for mode in (0, 2, 9, 18, 34):
                    k += 1
                    nb = np.where(i < 64, c0 - (64 - i), np.where(i == 64, c0, c0 + (i - 64)))      # left column falls by one per sample away from the corner, the row above rises
                    if what == "top_end": nb[128] += d
                    if what == "left_end": nb[0] += d
                    if what == "corner": nb[64] += d
                    C.add("strong-bd%d" % bd, LUMA, 5, bd, (6, (k % 2) * 32, 0), strong, 1, mode, (0, 0), 0, 0, (0, 0), [nb], np.ones(33, bool), [np.zeros((32, 32), np.int64)])
    C.freeze()
    # samples of units that are not available are not the block's business: give them values of their own so that a read of one shows
    noise = np.random.default_rng(77)
    for ci in range(len(C.ids)):
        kind, log2, bd = C.hdr[ci, H_KIND], C.hdr[ci, H_LOG2], C.hdr[ci, H_BD]
        gone = ~C.uav[ci].astype(bool)[unit_of_sample(kind, log2)]
        for b in range(2):
            C.nb[ci, b, :len(gone)][gone] = noise.integers(0, 1 << bd, int(gone.sum()))
    return C


def groups():
    return sorted(set(build().groups))


# ---------------------------------------------------------------------------------------------------------------------- the text's answer
@functools.lru_cache(maxsize=None)
def expected():
    """per case and plane: (pred [n, n] or None, res [n, n] exact or None), computed once"""
    C = build(); out = []
    for ci in range(len(C.ids)):
        h = C.hdr[ci]; kind, log2, bd = int(h[H_KIND]), int(h[H_LOG2]), int(h[H_BD]); n = 1 << log2
        av = C.uav[ci].astype(bool)[unit_of_sample(kind, log2)]
        per = []
        for b in range(2 if kind == PAIR else 1):
            c_idx = 0 if kind == LUMA else (b + 1 if kind == PAIR else kind)
            cbf = int(h[H_CBF0 + b]); qp = int(h[H_QP0 + b])
            per.append(S.block(c_idx, log2, bd, int(h[H_STRONG]), int(h[H_INTRA]), int(h[H_MODE]), cbf, int(h[H_TS]), int(h[H_BYP]), qp,
                               C.nb[ci, b, :4 * n + 1].astype(np.int64), av, C.lev[ci, b, :n * n].astype(np.int64)))
        out.append(per)
    return out


def compare(out, group, label):
    """out: uint16 [n_cases, 2, 1024] as a hook returned it. Intra blocks: the samples are the text's. Inter blocks: the routine leaves the residual as an int16 bit pattern for
    motion compensation to add, so those are compared after picture construction, Clip1(p + stored) against Clip1(p + exact) for p = 0, 2^(bd-1), 2^bd - 1.
    Returns the failures of the group as text lines (case id, plane, first differing sample: exact residual, what the routine left, the text's sample)."""
    C = build(); E = expected(); bad = []
    for ci in range(len(C.ids)):
        if C.groups[ci] != group:
            continue
        h = C.hdr[ci]; n = 1 << int(h[H_LOG2]); bd = int(h[H_BD])
        for b, (pred, res) in enumerate(E[ci]):
            got = out[ci, b, :n * n].reshape(n, n)
            if pred is not None:
                want = S.reconstruct(pred, 0 if res is None else res, bd)
                diff = got.astype(np.int64) != want
                stored = got.astype(np.int64)
            elif res is not None:
                stored = got.view(np.int16).astype(np.int64)
                diff = np.zeros((n, n), bool)
                for p in (0, 1 << (bd - 1), (1 << bd) - 1):
                    diff |= S.reconstruct(p, stored, bd) != S.reconstruct(p, res, bd)
                want = S.reconstruct(1 << (bd - 1), res, bd)
            else:
                continue
            if diff.any():
                y, x = np.argwhere(diff)[0]
                bad.append("%s %s plane %d: %d samples differ; at (x %d, y %d) exact residual %s, left in the tile %d, the text's sample %d (max |exact residual| %s)" % (
                    label, C.ids[ci], b, int(diff.sum()), x, y, "-" if res is None else int(res[y, x]), int(stored[y, x]), int(want[y, x]), "-" if res is None else int(np.abs(res).max())))
    return bad


def run_hook(ctx):
    C = build()
    return ctx.selftest_tb(C.hdr, C.nb, C.uav, C.lev)
