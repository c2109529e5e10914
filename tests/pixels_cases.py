"""Test helper shared by tests/test_pixels.py, tests/test_pixels_gpu.py and tests/test_pixels_mul_gpu.py
(DESIGN.md 4.9): the coefficient frames of the pixel tests, each computed once, the frames that tell the
device's two multipliers apart, and the sanitizer program tests/c/pixels_san.c, built and run once per
session."""
import functools
import os

import numpy as np

import jpgx
import oracle
import san_build
from conftest import PKG
from jfif_inputs import nblocks  # noqa: F401  (the pixel tests use it as P.nblocks)

QUALITIES = (1, 50, 90, 97)
# (W, H) per sample mode: 8x8 (16x16 for 4:2:x) is one lane group; 136x16 is 17 blocks per row, a run
# of 8 + 8 + 1 (272x16: 17 chroma blocks per row); 48x32 in 4:2:0 has chroma planes of 2 block rows,
# whose vertical neighbours are the clamped edge on both sides; 96x64
SIZES = {0: ((8, 8), (16, 16), (136, 16), (48, 32), (96, 64)),
         1: ((16, 16), (272, 16), (48, 32), (96, 64)),
         2: ((16, 16), (272, 16), (48, 32), (96, 64))}
EXTREME = (32767, -32767, -32768)
ENTRY = (1, 255, 65535)


@functools.lru_cache(maxsize=None)
def oracle_coef(kind, W, H, q, sr):
    """int16 [nb + 2 nbc][64]: the oracle's forward transform of a splitmix or a tie frame"""
    rgb = oracle.gen_splitmix(W * 131 + H, W, H) if kind == "splitmix" else oracle.gen_tie(W, H)
    full = oracle.blocks(rgb, q)
    if sr == 0:
        out = full.reshape(-1, 64)
    else:
        out = np.concatenate([full[0], oracle.chroma_sub(rgb, q, sr).reshape(-1, 64)])
    out = np.ascontiguousarray(out, np.int16)
    out.setflags(write=False)
    return out


def hostile_frames(W, H, sr):
    """(coef int16 [n][nblk][64], qt uint16 [n][2][64]): every coefficient +-32767 under a table of
    65535; one extreme coefficient per position (in every block) under table entries 1, 255, 65535;
    an all-zero table"""
    nb, nbc = nblocks(W, H, sr)
    nblk = nb + 2 * nbc
    coefs, qts = [], []
    alt = np.where(np.arange(nblk * 64) % 2 == 1, 32767, -32767).astype(np.int16).reshape(nblk, 64)
    for c in (np.full((nblk, 64), 32767, np.int16), np.full((nblk, 64), -32767, np.int16), alt):
        coefs.append(c)
        qts.append(np.full((2, 64), 65535, np.uint16))
    for k in range(64):
        for v in EXTREME:
            for e in ENTRY:
                c = np.zeros((nblk, 64), np.int16)
                c[:, k] = v
                coefs.append(c)
                qts.append(np.full((2, 64), e, np.uint16))
    rnd = np.random.default_rng(W + H + sr).integers(-32768, 32768, (nblk, 64)).astype(np.int16)
    coefs.append(rnd)
    qts.append(np.zeros((2, 64), np.uint16))
    # both sides of the kernels' table threshold (entries up to 63 choose the 24-bit multiplier for
    # pass 1 whatever the coefficients): the largest magnitudes it has to carry, and one entry above
    for c in (np.full((nblk, 64), -32768, np.int16), rnd):
        for e in (63, 64):
            coefs.append(c)
            qts.append(np.full((2, 64), e, np.uint16))
        one = np.full((2, 64), 63, np.uint16)
        one[1, 63] = 64
        coefs.append(c)
        qts.append(one)
    return np.stack(coefs), np.stack(qts)


def pillow_images():
    """the smooth, noise and 0/255-saturated 96x64 images of the Pillow parity tests"""
    yy, xx = np.mgrid[0:64, 0:96]
    smooth = np.stack([(2 * xx + yy) % 256, 255 - (3 * yy) % 256, (xx + 2 * yy) // 2 % 256], 2).astype(np.uint8)
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    sat = (rng.integers(0, 2, (64, 96, 3), dtype=np.uint8) * 255).astype(np.uint8)
    return dict(smooth=smooth, noise=noise, saturated=sat)


def fits_16_bits(coef, qt, nb):
    """libjpeg-turbo's SIMD multiplies coefficient and divisor in 16 bits: max |coef * qt| < 32768"""
    c = np.asarray(coef, np.int64).reshape(-1, 64)
    q = np.asarray(qt, np.int64).reshape(2, 64)
    return max(np.abs(c[:nb] * q[0]).max(), np.abs(c[nb:] * q[1]).max()) < 32768


def run_san():
    """tests/c/pixels_san.c with csrc/jpgx_pixels_host.cpp under the sanitizers, built and run once per
    session; returns (returncode, stdout, stderr)."""
    return san_build.run("pixels_san", [os.path.join(PKG, "csrc", "jpgx_pixels_host.cpp")], timeout=600)


def qt_of(q):
    return jpgx.jfif_qt(q)


# ---- the multiplier choice ---------------------------------------------------------------
# The kernels run pass 1 on the 24-bit multiplier where no table entry is above 63, and otherwise run by
# run where a vote over the wave finds every dequantised value inside 16 bits.  The host twin computes the
# contract whichever multiplier a kernel would have chosen, so a wrong choice shows only on inputs for
# which the 24-bit multiplier's products differ.  Every frame below carries that as a guard: the model of
# that multiplier (tests/idct_ref.py, m24=True) gives other pixels than the contract in the block that
# holds the large values.  A case is a dict: kind "plain" | "any" | "gray", W, H (the visible frame), sr,
# coefs int16 [n][nblk][64], qts uint16 [n][2][64] ([n][64] for gray), regions [n] of (y0, y1, x0, x1), the
# pixels the guard looks at, names [n].
THRESHOLD_TABLES = (65, 96, 128, 255, 256, 1024)
CANNOT_TELL = (63, 64)                  # tables at which the two multipliers agree on every pattern below
VOTE_TABLE = 1024                       # |d| <= 31 * 1024 < 2^15 for the background: the vote says small
BACKGROUND = 31
THRESHOLD_SIZE = (48, 32)


def _sampling(sr):
    return ((1, 1), (2, 1), (2, 2))[sr]


def _coded(W, H, sr, kind):
    if kind == "plain":
        return W, H
    hs, vs = (1, 1) if kind == "gray" else _sampling(sr)
    return -(-W // (8 * hs)) * 8 * hs, -(-H // (8 * vs)) * 8 * vs


def planes_of(W, H, sr, kind):
    """[(first block, blocks per row, block rows, hs, vs)] of the channels Y (, Cb, Cr) of the coded frame"""
    cw, ch = _coded(W, H, sr, kind)
    bw, bh = cw // 8, ch // 8
    if kind == "gray":
        return [(0, bw, bh, 1, 1)]
    hs, vs = _sampling(sr)
    cbw, cbh = bw // hs, bh // vs
    return [(0, bw, bh, 1, 1), (bw * bh, cbw, cbh, hs, vs), (bw * bh + cbw * cbh, cbw, cbh, hs, vs)]


def model_pixels(kind, coef, W, H, sr, qt, m24, channels=1):
    """the contract's pixels (m24 False) or the 24-bit multiplier's (True), by the numpy restatements"""
    import idct_ref
    import idct_ref_any
    if kind == "plain":
        return idct_ref.pixels(coef, W, H, sr, qt, m24)
    if kind == "any":
        return idct_ref_any.pixels(coef, W, H, sr, qt, m24)
    px = idct_ref.samples(coef, qt, -(-W // 8), -(-H // 8), m24)[:H, :W].astype(np.uint8)
    return px if channels == 1 else np.repeat(px[:, :, None], 3, 2)


def tells(case, k):
    """the guard of frame k: the model's pixels differ from the contract's inside the frame's region"""
    y0, y1, x0, x1 = case["regions"][k]
    a, b = (model_pixels(case["kind"], case["coefs"][k], case["W"], case["H"], case["sr"], case["qts"][k], m)
            for m in (False, True))
    return bool((a[y0:y1, x0:x1] != b[y0:y1, x0:x1]).any())


def _case(kind, W, H, sr, frames):
    coefs, qts, regions, names = zip(*frames)
    return dict(kind=kind, W=W, H=H, sr=sr, coefs=np.stack(coefs), qts=np.stack(qts), regions=list(regions),
                names=list(names))


def _patterns(nblk, seed):
    from idct_ref import ZZ
    odd = np.array([(ZZ[k] >> 3) & 1 for k in range(64)], bool)
    rows = np.zeros((nblk, 64), np.int16)
    rows[:, odd] = -32768
    return {"all -32768": np.full((nblk, 64), -32768, np.int16), "all 32767": np.full((nblk, 64), 32767, np.int16),
            "random": np.random.default_rng(seed).integers(-32768, 32768, (nblk, 64)).astype(np.int16),
            "-32768 in rows 1, 3, 5, 7": rows}


@functools.lru_cache(maxsize=None)
def threshold_case(sr, kind="plain"):
    """48 x 32, every block the same pattern (or random: at 96 a column tells only where four entries of one
    sign add up beyond 2^23, about one block in eight; the frame has 36 or more): uniform tables above the
    kernels' threshold of 63, and tables split at it.  A (table, pattern) pair is kept where the guard holds; it must for all -32768 and all
    32767 at every table and for the random blocks from 96 up.  Returns (case, kept names)"""
    W, H = THRESHOLD_SIZE
    gray = kind == "gray"
    nblk = sum(bw * bh for _, bw, bh, _, _ in planes_of(W, H, sr, kind))
    pats = _patterns(nblk, 77 + sr)
    tables = [("uniform %d" % t, (t, t)) for t in THRESHOLD_TABLES]
    if not gray:
        tables += [("luma 63, chroma 65", (63, 65)), ("luma 65, chroma 63", (65, 63)), ("luma 1, chroma 65", (1, 65))]
    frames = []
    for tname, (ty, tc) in tables:
        for pname, coef in pats.items():
            qt = np.full(64, ty, np.uint16) if gray else np.stack([np.full(64, ty, np.uint16), np.full(64, tc, np.uint16)])
            frames.append((coef, qt, (0, H, 0, W), "%s, %s" % (tname, pname)))
    case = _case(kind, W, H, sr, frames)
    keep = [k for k in range(len(frames)) if tells(case, k)]
    names = [case["names"][k] for k in keep]
    for t in THRESHOLD_TABLES:
        for pname in ("all -32768", "all 32767") + (("random",) if t >= 96 else ()):
            assert "uniform %d, %s" % (t, pname) in names, (sr, kind, t, pname)
    case = _case(kind, W, H, sr, [frames[k] for k in keep])
    return case, names


def cannot_tell_case(sr, kind="plain"):
    """the same patterns under uniform 63 and 64: in range for the 24-bit multiplier, which these cannot see"""
    W, H = THRESHOLD_SIZE
    nblk = sum(bw * bh for _, bw, bh, _, _ in planes_of(W, H, sr, kind))
    frames = []
    for t in CANNOT_TELL:
        for pname, coef in _patterns(nblk, 77 + sr).items():
            qt = np.full(64 if kind == "gray" else (2, 64), t, np.uint16)
            frames.append((coef, qt, (0, H, 0, W), "uniform %d, %s" % (t, pname)))
    return _case(kind, W, H, sr, frames)


def _region(plane, blk, W, H):
    """the pixels of block blk (an index inside its plane), clipped to the visible frame"""
    _, bw, _, hs, vs = plane
    by, bx = divmod(blk, bw)
    return (min(8 * vs * by, H), min(8 * vs * (by + 1), H), min(8 * hs * bx, W), min(8 * hs * (bx + 1), W))


def _vote_frame(kind, W, H, sr, planes, ch, blk, octet, value, seed):
    """a background in [-31, 31] under the uniform table 1024 with `value` at one position of zig-zag octet
    `octet` of block blk of channel ch: the first position of the octet at which the guard holds"""
    nblk = sum(bw * bh for _, bw, bh, _, _ in planes)
    rng = np.random.default_rng(seed)
    back = rng.integers(-BACKGROUND, BACKGROUND + 1, (nblk, 64)).astype(np.int16)
    qt = np.full(64 if kind == "gray" else (2, 64), VOTE_TABLE, np.uint16)
    region = _region(planes[ch], blk, W, H)
    for i in range(8):
        coef = back.copy()
        coef[planes[ch][0] + blk, 8 * octet + i] = value
        one = dict(kind=kind, W=W, H=H, sr=sr, coefs=coef[None], qts=qt[None], regions=[region])
        if tells(one, 0):
            return coef, qt, region, "%s block %d octet %d position %d value %d" % ("Y Cb Cr".split()[ch], blk, octet, i, value)
    raise AssertionError("no position of octet %d tells the multipliers apart: %r" % (octet, (kind, W, H, sr, ch, blk)))


@functools.lru_cache(maxsize=None)
def vote_lane_case(sr, ch, kind="plain"):
    """64 frames: one large coefficient per load lane (block b, zig-zag octet j) of run 0 in turn, in
    channel ch only.  128 x 16 in 4:2:x has 16 Y and 8 chroma blocks per row; 64 x 8 otherwise"""
    W, H = (64, 8) if sr == 0 or kind == "gray" else (128, 16)
    planes = planes_of(W, H, sr, kind)
    frames = [_vote_frame(kind, W, H, sr, planes, ch, lane >> 3, lane & 7, 32767 if lane % 3 else -32768,
                          1000 * sr + 100 * ch + lane) for lane in range(64)]
    return _case(kind, W, H, sr, frames)


@functools.lru_cache(maxsize=None)
def vote_run_case(W, H, sr, kind="plain"):
    """the large coefficient in exactly one run of a block row, each run of each channel in turn: 33 blocks
    per row are runs 0 .. 3 in one wave and run 4, one live block, in a second; 66 are three waves, the
    last with a run of two blocks"""
    planes = planes_of(W, H, sr, kind)
    frames = []
    for ch, (_, bw, bh, _, _) in enumerate(planes):
        nruns = -(-bw // 8)
        for run in range(nruns):
            n = min(8, bw - 8 * run)
            b = n - 1 if n < 8 else (3 * run + 1) % 8
            by = run % bh
            frames.append(_vote_frame(kind, W, H, sr, planes, ch, by * bw + 8 * run + b, (5 * run + 2) % 8,
                                      -32768 if run % 2 else 32767, 5000 + 100 * ch + run))
    return _case(kind, W, H, sr, frames)


def multiplier_cases():
    """[(id, case, channels)]: every kernel's threshold frames, every channel of every kernel lane by lane,
    every run of the 33- and 66-block rows through the plain, the any-size and the one-component calls
    (channels: the one-component call's 1 or 3, else None)"""
    out = [("threshold %d" % sr, threshold_case(sr)[0], None) for sr in (0, 1, 2)]
    out += [("threshold gray %d" % c, threshold_case(0, "gray")[0], c) for c in (1, 3)]
    out += [("lanes %d %s" % (sr, "Y Cb Cr".split()[ch]), vote_lane_case(sr, ch), None) for sr in (0, 1, 2) for ch in (0, 1, 2)]
    out += [("lanes gray %d" % c, vote_lane_case(0, 0, "gray"), c) for c in (1, 3)]
    out += [("runs %dx%d %d" % (W, H, sr), vote_run_case(W, H, sr), None) for W, H, sr in ((264, 8, 0), (528, 16, 1), (528, 16, 2))]
    out += [("runs any %dx%d %d" % (W, H, sr), vote_run_case(W, H, sr, "any"), None)
            for W, H, sr in ((259, 5, 0), (523, 13, 1), (523, 13, 2))]
    out += [("runs gray %d" % c, vote_run_case(264, 8, 0, "gray"), c) for c in (1, 3)]
    return out


def host_pixels(case, k, channels=None):
    """the host twin's pixels of frame k"""
    import jpgx.compat as C
    coef, qt, W, H, sr = case["coefs"][k], case["qts"][k], case["W"], case["H"], case["sr"]
    if case["kind"] == "gray":
        return C.pixels_host_gray(coef, W, H, qt, channels, nthreads=1)
    return C.pixels_host(coef, W, H, sr, qt, 1, any_size=case["kind"] == "any")
