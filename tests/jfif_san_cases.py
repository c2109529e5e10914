"""Test helper: tests/c/jfif_read_san.c's inputs, regenerated (tests/test_jfif_read.py,
tests/test_jfif_decode_gpu.py), and the program itself, built and run once per session.

The program draws its coefficients and its single-byte corruptions from splitmix64 streams of fixed
seeds and prints each file's length and FNV-1a hash and its first SHOWN corruptions with the host
decoder's result.  files() / flips() restate the generators, so that a test can hold the very bytes
the shared decoding routines have seen under AddressSanitizer before it hands them to a GPU."""
import os

import numpy as np

import jpgx.compat as C
import san_build
from conftest import PKG
from jfif_decode import decode

COEF_SEED = 0x6A66696672656164
FLIP_SEED = 0x73616E666C697073
FLIPS, SHOWN = 2000, 48
M64 = (1 << 64) - 1
# the program's file order: index -> (W, H, sample_ratio, optimize)
FILES = [(64 if big else 16, 64 if big else 16, sr, opt) for big in (1, 0) for sr in (0, 1, 2) for opt in (0, 1)]
HAVE_CC = san_build.HAVE_CC
# The GPU test's corrupt inputs all derive from the program's file 6 (16x16, 4:4:4, Annex K.3 tables):
# its length and FNV-1a hash as the program prints them, and the corruption undefined_code_flip() finds
# in its sweep.  tests/test_jfif_read.py holds the program to these values under the sanitizers;
# tests/test_jfif_decode_gpu.py holds the bytes it uploads to them, and runs no sanitizer itself.
GPU_FILE = (6, 1086, 0xE802EB6FA02B181A)
GPU_FLIP = (630, 42)


def splitmix(seed, k):
    """the k-th output (k = 1, 2, ...; an int or a numpy array) of the stream that starts at seed"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & M64) + np.asarray(k, np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def fnv1a(data: bytes) -> int:
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & M64
    return h


def coefficients(idx: int, n: int) -> np.ndarray:
    """coef_at(idx, 0 .. n-1) of the program: int16 [n / 64][64], inside the writers' clamps"""
    i = np.arange(n, dtype=np.uint64)
    r = splitmix(COEF_SEED + idx, i + np.uint64(1))
    t = (r % np.uint64(64)).astype(np.int64)
    ac = np.where(t < 40, 0, np.where(t < 62, t - 51, ((r >> np.uint64(8)) % np.uint64(2001)).astype(np.int64) - 1000))
    dc = (r % np.uint64(601)).astype(np.int64) - 300
    return np.where(i % np.uint64(64) == 0, dc, ac).astype(np.int16).reshape(-1, 64)


def file_of(idx: int):
    """(bytes, W, H, sample_ratio, coefficients) of the program's file `idx`"""
    W, H, sr, opt = FILES[idx]
    nb = (W // 8) * (H // 8)
    nbc = (nb, nb // 2, nb // 4)[sr]
    coef = coefficients(idx, (nb + 2 * nbc) * 64)
    data = C.write_jfif_ex(coef, W, H, 75, sr, restart_rows=1, nthreads=1, optimize=bool(opt))
    return data, W, H, sr, coef


def flips(idx: int, data: bytes, count: int = SHOWN):
    """the program's first `count` corruptions of file idx: [(position, new byte value)]"""
    out = []
    for k in range(count):
        pos = int(splitmix(FLIP_SEED + idx, 2 * k + 1)) % len(data)
        val = data[pos] ^ (1 + int(splitmix(FLIP_SEED + idx, 2 * k + 2)) % 255)
        out.append((pos, val))
    return out


def flipped(data: bytes, pos: int, val: int) -> bytes:
    b = bytearray(data)
    b[pos] = val
    return bytes(b)


def drop_first_rst(data: bytes) -> bytes:
    at = C.jfif_info(data)["scan_offset"]
    while not (data[at] == 0xFF and data[at + 1] & 0xF8 == 0xD0):
        at += 1
    return data[:at] + data[at + 2:]


def undefined_code_flip(idx=6):
    """the first of the sanitizer sweep's corruptions of its 16x16 4:4:4 file that lands in the scan
    and makes the independent decoder meet a code that is in no table"""
    data, W, H, sr, _ = file_of(idx)
    scan = C.jfif_info(data)["scan_offset"]
    for pos, val in flips(idx, data, FLIPS):
        if pos < scan or pos >= len(data) - 2:
            continue
        try:
            decode(flipped(data, pos, val))
        except ValueError as e:
            assert "bad Huffman code" in str(e)
            return data, pos, val
        except (AssertionError, IndexError, KeyError):
            pass
    raise AssertionError("the sweep holds no such corruption")


def run_program():
    """tests/c/jfif_read_san.c with the host layer and the host decoder under the sanitizers, built and
    run once per session; returns (returncode, stdout, stderr)."""
    return san_build.run("jfif_read_san", san_build.HOST_LAYER + [os.path.join(PKG, "csrc", "jpgx_jfif_read.cpp")])


def assert_clean():
    rc, out, err = run_program()
    assert rc == 0 and "jfif_read_san: clean" in out, (out[-2000:], err[-4000:])
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-4000:]
    return out
