"""The entropy stage's JFIF writer with restart intervals coded on host threads
(csrc/jpgx_jfif_write.cpp jpgx_write_jfif_ex; SURVEY.md 8f(1), parity unpinned: the reference's
huffman_encode never terminates, src/huffman.c:23-235).  Checked against two independent
decoders written from T.81 -- tests/jfif_decode.py (Python, small frames) and tests/c/jfif_dec.c
(C, restart intervals decoded on threads, for big frames) -- and against PIL (libjpeg)."""
import ctypes
import hashlib
import io
import os
import subprocess

import numpy as np
import pytest

import jpgx
import jpgx.compat as C
import oracle as O
from conftest import REPO
from jfif_decode import decode

# The round-3 writer (commit 35a1b94, one interval, bit-at-a-time) on these inputs: the rewrite
# must emit the very same bytes when no restart interval is asked for.
ROUND3_SHA = {
    (64, 48, 50, 0, 11): "87f792ca6fb8f071a2d79b9393601c1bc51bccd27ed0b5c5eb413e3c41e3e6b3",
    (128, 64, 90, 0, 12): "b568db83168cb36e1eebe95a30d2a8198808bacfdd045e8b41b8ba0356c2d4ec",
    (64, 64, 10, 0, 13): "a665dd7abffe4e0b6275bd7461771dd4c7d2df322364ef2cae23cf2ecd1ba41a",
    (96, 32, 97, 0, 14): "cca7e3297f84544078286d80e76b445620239e94d4be8f451bd4c8f7486a1283",
    (64, 48, 75, 1, 15): "2155d48595c74214abd23de90d93c76c4f9af8700722be175af53ae80122d620",
    (64, 64, 50, 2, 16): "59f937fba1c53478dacde38e29365ba05d2fb09f590c29e2841384cc07b9620d",
}


def _coef(W, H, q, sr, seed):
    if sr == 0:
        return np.ascontiguousarray(O.blocks(O.gen_splitmix(seed, W, H), q).astype(np.int16))
    rng = np.random.default_rng(seed)
    nb = (W // 8) * (H // 8)
    nbc = nb // 2 if sr == 1 else nb // 4
    coef = rng.laplace(0, 6, size=(nb + 2 * nbc, 64)).astype(np.int16)
    coef[:, 0] = rng.integers(-300, 300, size=nb + 2 * nbc)
    return np.ascontiguousarray(coef)


def _flat(c):
    return np.concatenate([np.asarray(x).reshape(-1, 64) for x in c]) if isinstance(c, list) \
        else np.asarray(c).reshape(-1, 64)


@pytest.mark.parametrize("key", sorted(ROUND3_SHA))
def test_no_restart_bytes_equal_round3_writer(key):
    W, H, q, sr, seed = key
    coef = _coef(*key)
    data = C.write_jfif_ex(coef, W, H, q, sr, restart_rows=0, nthreads=1)
    assert hashlib.sha256(data).hexdigest() == ROUND3_SHA[key]
    old_api = C.write_jfif_sub(coef, W, H, q, sr) if sr else C.write_jfif(coef, W, H, q)
    assert old_api == data


@pytest.mark.parametrize("sr", [0, 1, 2])
@pytest.mark.parametrize("rows", [1, 2, 3, -1])
def test_restart_roundtrip(sr, rows):
    W, H, q = 64, 64, 75
    coef = _coef(W, H, q, sr, 40 + sr)
    data = C.write_jfif_ex(coef, W, H, q, sr, restart_rows=rows, nthreads=3)
    d = decode(data)
    mcu_rows = H // (16 if sr == 2 else 8)
    cpr = W // (16 if sr else 8)
    rr = rows if rows > 0 else d["restart_interval"] // cpr
    assert d["restart_interval"] == rr * cpr
    assert d["restarts"] == (mcu_rows + rr - 1) // rr - 1
    assert np.array_equal(_flat(d["coef"]), coef.reshape(-1, 64).astype(np.int32))


@pytest.mark.parametrize("rows", [1, 5])
def test_output_independent_of_thread_count(rows):
    W, H, q = 128, 96, 90
    coef = _coef(W, H, q, 0, 77)
    ref = C.write_jfif_ex(coef, W, H, q, 0, restart_rows=rows, nthreads=1)
    for t in (2, 3, 5, 8, 64):
        assert C.write_jfif_ex(coef, W, H, q, 0, restart_rows=rows, nthreads=t) == ref


def test_restart_bad_args():
    coef = _coef(64, 64, 50, 0, 1)
    lib = jpgx.lib
    buf = np.zeros(1 << 16, np.uint8)
    n = ctypes.c_size_t()
    # interval too long for DRI's 16 bits: 65535 / (64 / 8) = 8191 rows at most
    rc = lib.jpgx_write_jfif_ex(coef.ctypes.data, 64, 64, 50, 0, 8192, 1, buf.ctypes.data, buf.size,
                                ctypes.byref(n))
    assert rc == jpgx.EARG
    rc = lib.jpgx_write_jfif_ex(coef.ctypes.data, 64, 64, 50, 0, -2, 1, buf.ctypes.data, buf.size,
                                ctypes.byref(n))
    assert rc == jpgx.EARG
    # cap too small: EARG and the size needed
    rc = lib.jpgx_write_jfif_ex(coef.ctypes.data, 64, 64, 50, 0, 1, 2, buf.ctypes.data, 100,
                                ctypes.byref(n))
    assert rc == jpgx.EARG and n.value > 100
    assert len(C.write_jfif_ex(coef, 64, 64, 50, 0, 1, 2)) == n.value


def test_restart_decodes_with_pil():
    Image = pytest.importorskip("PIL.Image")
    W, H, q = 64, 48, 90
    coef = _coef(W, H, q, 0, 5)
    a = np.asarray(Image.open(io.BytesIO(C.write_jfif_ex(coef, W, H, q, 0, 0, 1))).convert("RGB"))
    b = np.asarray(Image.open(io.BytesIO(C.write_jfif_ex(coef, W, H, q, 0, 1, 4))).convert("RGB"))
    assert np.array_equal(a, b)


@pytest.fixture(scope="module")
def jfd():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "jfd"], check=True)
    lib = ctypes.CDLL(os.path.join(REPO, "tests", "c", "_build", "libjfd.so"))
    lib.jfd_decode.restype = ctypes.c_int
    lib.jfd_decode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                               ctypes.c_int, ctypes.c_void_p]
    return lib


def jfd_decode(lib, data, nelems, nthreads=8):
    buf = np.frombuffer(data, np.uint8)
    out = np.zeros(nelems, np.int16)
    info = np.zeros(6, np.int32)
    rc = lib.jfd_decode(buf.ctypes.data, buf.size, out.ctypes.data, out.size, nthreads, info.ctypes.data)
    assert rc == 0, f"jfif_dec.c check at line {-rc}"
    return out.reshape(-1, 64), info


@pytest.mark.parametrize("sr,rows", [(0, 0), (0, 1), (0, 3), (1, 2), (2, 1), (2, 0)])
def test_c_decoder_matches_python_decoder(jfd, sr, rows):
    W, H, q = 96, 64, 50
    coef = _coef(W, H, q, sr, 60 + sr)
    data = C.write_jfif_ex(coef, W, H, q, sr, restart_rows=rows, nthreads=2)
    got, info = jfd_decode(jfd, data, coef.size)
    assert np.array_equal(got, _flat(decode(data)["coef"]))
    assert np.array_equal(got, coef.reshape(-1, 64))
    assert list(info[:2]) == [W, H]


def test_big_frame_threads_roundtrip(jfd):
    """A 2048 x 1024 frame of oracle-shaped coefficients (random-laplacian AC, so every code
    length and run occurs): 8 coding threads, intervals of 4 MCU rows, the C decoder on 8
    threads returns every coefficient."""
    W, H = 2048, 1024
    rng = np.random.default_rng(9)
    nb = (W // 8) * (H // 8)
    coef = rng.laplace(0, 4, size=(3 * nb, 64)).astype(np.int16)
    coef[:, 0] = rng.integers(-1000, 1000, size=3 * nb)
    coef[:, 40:] *= (rng.random((3 * nb, 1)) < 0.2)          # runs of zeros, EOBs and ZRLs
    data = C.write_jfif_ex(coef, W, H, 50, 0, restart_rows=4, nthreads=8)
    got, info = jfd_decode(jfd, data, coef.size)
    assert info[4] == 4 * (W // 8) and info[5] == H // 8 // 4 - 1
    assert np.array_equal(got, coef)
