"""Test helper: the coefficient frames that tests/test_jfif_gpu.py, tests/test_jfif_opt.py,
tests/test_jfif_pinned.py, tests/test_jfif_read.py and tests/test_jfif_decode_gpu.py share, so that
they hold the writers and the decoders to the very same inputs."""
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


def stuffing_heavy(sr, W=64, H=96):
    """(W, H, q, coef): a 64 x 96 frame of extreme values, whose scan is full of 0xFF bytes"""
    q = 50
    nb, nbc = nblocks(W, H, sr)
    vals = np.array([0, 0, 0, 1, -1, 1023, -1023, 32767, -32768, 2047, -2047], np.int16)
    coef = np.ascontiguousarray(np.random.default_rng(0).choice(vals, (nb + 2 * nbc, 64)))
    return W, H, q, coef


def stuffing_guard(ref):
    """(stuffed pairs, intervals ending FF 00 FF Dn) of a stuffing-heavy file; a different numpy
    must not empty the case"""
    scan = scan_of(ref)
    pairs = scan.count(b"\xff\x00")
    endings = sum(scan.count(b"\xff\x00\xff" + bytes([0xd0 + m])) for m in range(8))
    print(f"stuffed pairs {pairs}, intervals ending FF 00 FF Dn {endings}")
    return pairs, endings
