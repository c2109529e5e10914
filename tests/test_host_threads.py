"""The host twins' thread fan-out (csrc/jx_par.h): the count a call takes and the split of its items.
The writer's count is observable -- it enters the automatic restart interval, a stated count above 64
included -- and nothing else about the threads is: every twin's output is its one-thread output."""
import struct

import numpy as np
import pytest

import jpgx.compat as C


def _dri(data):
    """the file's restart interval, in MCUs"""
    p = data.index(b"\xff\xdd")
    assert data[p + 2:p + 4] == b"\x00\x04"
    return struct.unpack(">H", data[p + 4:p + 6])[0]


@pytest.mark.parametrize("T, dri", [(1, 130), (64, 3), (65, 2), (200, 1)])
def test_writer_takes_a_stated_thread_count_as_it_is(T, dri):
    """8 x 4160 4:4:4 has 520 MCU rows of one MCU: the automatic interval is ceil(520 / 4T) rows, and T
    is not clamped to 64"""
    W, H = 8, 4160
    coef = np.zeros((3, H // 8, 64), np.int16)
    assert _dri(C.write_jfif_ex(coef, W, H, 50, 0, restart_rows=-1, nthreads=T)) == dri == -(-520 // (4 * T))


# 0: one per CPU; 3: more threads than the frame's 2 MCU rows; 64: the clamp
THREADS = (0, 1, 3, 64)


def _frame16(seed):
    rng = np.random.default_rng(seed)
    coef = rng.laplace(0, 6, size=(3, 4, 64)).astype(np.int16)
    coef[:, :, 0] = rng.integers(-300, 300, size=(3, 4))
    return coef


def test_write_jfif_ex_is_the_same_on_any_thread_count():
    coef = _frame16(1)
    for opt in (False, True):
        one = C.write_jfif_ex(coef, 16, 16, 75, 0, restart_rows=1, nthreads=1, optimize=opt)
        for t in THREADS:
            assert C.write_jfif_ex(coef, 16, 16, 75, 0, restart_rows=1, nthreads=t, optimize=opt) == one, (opt, t)


def test_read_jfif_is_the_same_on_any_thread_count():
    coef = _frame16(2)
    data = C.write_jfif_ex(coef, 16, 16, 75, 0, restart_rows=1, nthreads=1)
    one = C.read_jfif(data, 1)
    assert np.array_equal(one["coef"], coef)
    for t in THREADS:
        got = C.read_jfif(data, t)
        assert np.array_equal(got["coef"], one["coef"]) and np.array_equal(got["qt"], one["qt"]), t
    # a damaged interval is refused whichever thread meets it
    bad = bytearray(data)
    bad[-3] = 0xFF                      # a bare FF before EOI, in the second interval
    for t in THREADS:
        with pytest.raises(C.JpgxError) as e:
            C.read_jfif(bytes(bad), t)
        assert e.value.rc == -10, t     # EJFIF_SCAN


def test_pixels_host_is_the_same_on_any_thread_count():
    coef = _frame16(3)
    qt = np.full((2, 64), 3, np.uint16)
    for sr in (0, 2):
        c = coef.reshape(-1, 64)[:12 if sr == 0 else 6]
        one = C.pixels_host(c, 16, 16, sr, qt, nthreads=1)
        for t in THREADS:
            assert np.array_equal(C.pixels_host(c, 16, 16, sr, qt, nthreads=t), one), (sr, t)


def test_pixels_host_gray_is_the_same_on_any_thread_count():
    coef = _frame16(4)[0]
    qt = np.full(64, 3, np.uint16)
    for channels in (1, 3):
        one = C.pixels_host_gray(coef, 16, 16, qt, channels, nthreads=1)
        for t in THREADS:
            assert np.array_equal(C.pixels_host_gray(coef, 16, 16, qt, channels, nthreads=t), one), (channels, t)
