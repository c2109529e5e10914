"""Test helper: the coefficient frames that tests/test_jfif_gpu.py, tests/test_jfif_opt.py,
tests/test_jfif_pinned.py, tests/test_jfif_read.py and tests/test_jfif_decode_gpu.py share, so that
they hold the writers and the decoders to the very same inputs; and, below, the frames of
tests/test_jfif_gpu_passes.py, which tests/jfif_bits.py makes into guarded cases."""
import numpy as np

CASES = {
    # name: (W, H, q, sr, rr, seed)
    "one_block": (8, 8, 50, 0, 1, 1),
    "64x48_rr1": (64, 48, 50, 0, 1, 2),
    "128x64_rr3": (128, 64, 75, 0, 3, 3),             # intervals of 3, 3 and 2 rows
    "128x64_auto": (128, 64, 75, 0, -1, 3),
    "single_interval": (64, 48, 50, 0, 100, 4),       # rr >= MCU rows: one interval, DRI still written
    "q10_16bit_dqt": (64, 48, 10, 0, 2, 5),           # SOF1
    "q97": (64, 48, 97, 0, 2, 6),
    "422_64x64": (64, 64, 75, 1, 1, 41),
    "422_96x64": (96, 64, 75, 1, 3, 61),
    "420_64x64": (64, 64, 75, 2, 1, 42),
    "420_96x64": (96, 64, 75, 2, -1, 62),
    "420_one_mcu": (16, 16, 50, 2, 1, 7),
    "rst_wraps": (64, 96, 50, 0, 1, 8),               # 12 intervals: RST0..RST7, RST0..RST2
}


def nblocks(W, H, sr):
    nb = (W // 8) * (H // 8)
    return nb, (nb, nb // 2, nb // 4)[sr]


def scan_rows(W, H, sr):
    """[(row of the [nb + 2 nbc][64] coefficient array, component)] of the frame's blocks in scan
    order: MCU by MCU, hs x vs luma blocks, Cb, Cr (T.81 A.2.3)"""
    hs, vs = (1, 2, 2)[sr], (1, 1, 2)[sr]
    bpr = W // 8
    nb, nbc = nblocks(W, H, sr)
    cpr = bpr // hs
    out = []
    for my in range(H // 8 // vs):
        for mx in range(cpr):
            for dy in range(vs):
                for dx in range(hs):
                    out.append(((my * vs + dy) * bpr + mx * hs + dx, 0))
            out.append((nb + my * cpr + mx, 1))
            out.append((nb + nbc + my * cpr + mx, 2))
    return out


def lap(W, H, sr, seed, scale=6.0):
    """laplacian AC, uniform DC in [-300, 300): [nb + 2 nbc][64] (for sr 0 that is [3][nb][64])"""
    rng = np.random.default_rng(seed)
    nb, nbc = nblocks(W, H, sr)
    coef = rng.laplace(0, scale, size=(nb + 2 * nbc, 64)).astype(np.int16)
    coef[:, 0] = rng.integers(-300, 300, size=nb + 2 * nbc)
    return np.ascontiguousarray(coef)


def scan_of(data):
    """the entropy-coded bytes between the SOS segment and EOI"""
    at = data.index(b"\xff\xda")
    return data[at + 14:-2]


def hand_made(sr, W=64, H=32):
    """(W, H, coef): every rule of the block walk in a 64 x 32 frame"""
    nb, nbc = nblocks(W, H, sr)
    coef = np.zeros((nb + 2 * nbc, 64), np.int16)
    coef[1, 63] = 5                                  # three ZRLs, no EOB
    coef[2, 63] = -1
    coef[nb + 1, 63] = -700                          # the same in a chroma block
    coef[3, 20] = -3                                 # one ZRL, a run of 3, EOB
    coef[nb + nbc + 2, 20] = 1023
    coef[5, 1:64] = 1                                # 63 codes, no EOB
    coef[6, 16] = 1                                  # run of exactly 15: no ZRL
    coef[7, 17] = 1                                  # run of exactly 16: ZRL + run 0
    coef[8, 33] = 2000                               # AC clamp to 1023
    coef[9, 33] = -2000
    # DC steps of +-2047 and beyond between neighbours of a component (the clamp)
    dcs = np.array([0, 2047, 0, -2047, 2047, -2048, 2047, 4000, -4000, 1, 0, 32767, -32768, 0], np.int16)
    coef[10:10 + dcs.size, 0] = dcs
    coef[nb:nb + 4, 0] = [1500, -1500, 1500, -600]
    return W, H, coef


def stuffing_heavy(sr, W=64, H=96, seed=0):
    """(W, H, q, coef): a 64 x 96 frame of extreme values, whose scan is full of 0xFF bytes"""
    q = 50
    nb, nbc = nblocks(W, H, sr)
    vals = np.array([0, 0, 0, 1, -1, 1023, -1023, 32767, -32768, 2047, -2047], np.int16)
    coef = np.ascontiguousarray(np.random.default_rng(seed).choice(vals, (nb + 2 * nbc, 64)))
    return W, H, q, coef


def stuffing_guard(ref):
    """(stuffed pairs, intervals ending FF 00 FF Dn) of a stuffing-heavy file; a different numpy
    must not empty the case"""
    scan = scan_of(ref)
    pairs = scan.count(b"\xff\x00")
    endings = sum(scan.count(b"\xff\x00\xff" + bytes([0xd0 + m])) for m in range(8))
    print(f"stuffed pairs {pairs}, intervals ending FF 00 FF Dn {endings}")
    return pairs, endings


# ---- inputs of tests/test_jfif_gpu_passes.py: the device coder's multi-pass paths -----------------
# The coder's kernels work in passes of 256 lanes: 256 blocks of an interval, 4,096 unstuffed bytes
# of an interval (256 lanes x 16 bytes), 256 intervals of a frame.  Quality 50 throughout.
PASS = 256
SEAM_FRAMES = {0: (64, 176), 1: (64, 272), 2: (64, 352)}   # 528, 544, 528 blocks: the smallest with two seams
SEAMS = (256, 512)                                         # the first blocks of the second and third pass
ONE = 1000                                                 # restart_rows of a single-interval frame (>= MCU rows)
STUFF_SEEDS = {0: 0, 1: 0, 2: 1}                            # per sampling; held by the guard of tests/jfif_bits.py


def zeros(W, H, sr):
    nb, nbc = nblocks(W, H, sr)
    return np.zeros((nb + 2 * nbc, 64), np.int16)


def seam_hand_made(sr):
    """(W, H, coef): hand_made's rules in the four blocks around each seam of SEAM_FRAMES[sr] (scan
    blocks 254..257 and 510..513): three ZRLs and no EOB, 63 codes, a run of exactly 16 and the AC
    clamp, one per block, in another order and with the other sign at the second seam; hand_made's
    further blocks two blocks further out; and from eight blocks before a seam to eight after it
    hand_made's DC sequence per component, placed so that a component's first block among the four
    holds -32768 after 32767"""
    W, H = SEAM_FRAMES[sr]
    coef = zeros(W, H, sr)
    rows = scan_rows(W, H, sr)
    dcs = [0, 2047, 0, -2047, 2047, -2048, 32767, -32768, 32767, 4000, -4000, 1, 0, 2047, -2047, 0]

    def ac(row, kind, sign):
        if kind == 0:
            coef[row, 63] = 5 * sign                 # three ZRLs, no EOB
        elif kind == 1:
            coef[row, 1:64] = sign                   # 63 codes, no EOB
        elif kind == 2:
            coef[row, 17] = sign                     # run of exactly 16: ZRL + run 0
        elif kind == 3:
            coef[row, 33] = 2000 * sign              # AC clamp to 1023
        elif kind == 4:
            coef[row, 63] = -700 * sign              # three ZRLs, no EOB, 10 additional bits
        elif kind == 5:
            coef[row, 20] = -3 * sign                # one ZRL, a run of 3, EOB
        elif kind == 6:
            coef[row, 16] = sign                     # run of exactly 15: no ZRL
        else:
            coef[row, 20] = 1023 * sign

    for n, seam in enumerate(SEAMS):
        sign = -1 if n else 1
        for comp in range(3):
            mine = [s for s in range(seam - 8, seam + 8) if rows[s][1] == comp]
            first = next(i for i, s in enumerate(mine) if s >= seam - 2)
            for i, s in enumerate(mine):
                coef[rows[s][0], 0] = dcs[i - first + 7]
        for k, s in enumerate(range(seam - 2, seam + 2)):
            ac(rows[s][0], (k + n) % 4, sign)
        for k, s in enumerate((seam - 4, seam - 3, seam + 2, seam + 3)):
            ac(rows[s][0], 4 + (k + n) % 4, sign)
    return W, H, coef


def seam_maximal(n):
    """(W, H, coef): the 4:4:4 all-zero frame with block 255 (a luma block) maximal -- a DC step of
    2047 and 63 coefficients of +-1023 -- and n coefficients of 1 in the luma block before it
    (block 252), which move where block 255 starts"""
    W, H = SEAM_FRAMES[0]
    coef = zeros(W, H, 0)
    rows = scan_rows(W, H, 0)
    assert rows[255][1] == 0 and rows[252][1] == 0
    coef[rows[255][0], 0] = 2047
    coef[rows[255][0], 1:64] = [1023 if k & 1 else -1023 for k in range(63)]
    coef[rows[252][0], 1:1 + n] = 1
    return W, H, coef


def seam_shifted(n):
    """(W, H, coef): the 4:4:4 all-zero frame with n coefficients of 1 in the last luma block but one
    before the first seam (block 252): they move the bit at which block 256 starts"""
    W, H = SEAM_FRAMES[0]
    coef = zeros(W, H, 0)
    coef[scan_rows(W, H, 0)[252][0], 1:1 + n] = 1
    return W, H, coef


def tall(W, H, sr, kind):
    """coef of a frame of one MCU column, coded with one MCU row per interval: more than 256 intervals"""
    assert W == (8, 16, 16)[sr]
    return {"lap": lambda: lap(W, H, sr, 300 + H + sr), "stuffing": lambda: stuffing_heavy(sr, W, H)[3],
            "zeros": lambda: zeros(W, H, sr)}[kind]()


TALL = [(8, 2048, 0), (8, 2056, 0), (8, 2064, 0), (8, 4112, 0), (16, 2064, 1), (16, 4128, 2)]
BOTH = (704, 2064)                                         # 264 blocks per interval and 258 intervals


def trimmed(target, optimize=False):
    """(W, H, coef): 64 x 48 Laplacian content in one interval whose unstuffed stream is exactly
    `target` bytes in the host writer's file: the blocks are zeroed from the scan's end until the
    stream is shorter, then coefficients of one value are added to the first zeroed block until it is
    exactly that long (the block before it goes too when no count fits)"""
    import jpgx.compat as C
    W, H = 64, 48
    full = lap(W, H, 0, 4)
    rows = scan_rows(W, H, 0)

    def length(coef):
        data = C.write_jfif_ex(coef, W, H, 50, 0, restart_rows=ONE, nthreads=1, optimize=optimize)
        return len(scan_of(data).replace(b"\xff\x00", b"\xff"))

    for cut in range(len(rows), 0, -1):
        coef = full.copy()
        for row, _ in rows[cut:]:
            coef[row] = 0
        if length(coef) > target:
            continue
        for v in (0, 1, 3, 15, 255):
            for n in range(1, 64):
                coef[rows[cut][0], 1:1 + n] = v
                if length(coef) == target:
                    return W, H, coef
                if not v:
                    break
            coef[rows[cut][0], 1:] = 0
    raise AssertionError(f"no trimmed frame of {target} bytes")
