"""The seams of the device JFIF decoder, on the CPU ("The device decoder's seams"): the
guards of tests/jfif_dec_seams.py, which hold every case of tests/test_jfif_decode_gpu_seams.py to its
purpose, the scan builder held to the host writer and to three decoders, and the host twin of k_jd_sub
(jpgx_read_jfif_sub, jpgx_read_jfif_sub_gray: csrc/jx_jfif_sub.h's routines) == the host reader on every
case in the shapes (16, 2), (16, 4), (32, 3) and the kernel's own.

The oracle is the host reader, jpgx.compat.read_jfif / read_jfif_gray, for status, coefficients and
tables; the independent decoders tests/jfif_decode.py and tests/jfif_decode_gray.py and the builder's
own int64 bookkeeping stand beside it.  Every comparison is ==."""
import numpy as np
import pytest

import any_cases as A
import jfif_dec_seams as D
import jfif_sub_cases as K
import jpgx
import jpgx.compat as C
from jfif_decode import decode
from jfif_decode_gray import decode as decode_gray

SCAN = jpgx.EJFIF_SCAN


def _twin(c, shape):
    try:
        r = (C.read_jfif_sub_gray if c.gray else C.read_jfif_sub)(c.data, *shape)
    except jpgx.JpgxError as e:
        return e.rc, None, None
    return 0, r["coef"].reshape(-1, 64), r["qt"]


def _twin_is_the_reader(c):
    rc, want, wqt = D.host(c)
    assert rc == c.rc
    for shape in K.SHAPES:
        got_rc, got, qt = _twin(c, shape)
        assert got_rc == rc, shape
        if rc == 0:
            assert got.dtype == np.int16 and np.array_equal(got, want), shape
            assert np.array_equal(qt, wqt)
    return want


def _independent(c):
    """int [blocks][64] of the decoders written from T.81 alone"""
    if c.gray:
        return decode_gray(c.data)["coef"]
    coef = decode(c.data)["coef"]
    return coef.reshape(-1, 64) if c.sr == 0 else np.concatenate(coef)


# ---- the builder -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,q,rr,optimize", [(0, 50, 1, False), (1, 50, 1, False), (2, 50, 1, False),
                                              (0, 90, 0, True), (2, 50, 2, True)])
def test_builder_writes_the_host_writer_s_bytes(sr, q, rr, optimize):
    """the oracle's coefficients of 64 x 48, the builder's codes taken from the writer's own DHT segments
    (Annex K.3's and a per-image set): the same bytes, and what the builder says it wrote is what the
    host reader and the independent decoder read"""
    coef, data = A.project_file(sr, q, rr, optimize)
    mine, scan = D.from_coef(data, coef, 64, 48, sr, C.jfif_info(data)["restart_interval"])
    assert mine == data
    want = D.expected(scan, 64, 48, sr)
    assert np.array_equal(want, coef)
    c = D.Case(mine, 64, 48, sr)
    assert np.array_equal(D.host(c)[1], want) and np.array_equal(_independent(c), want)


def test_builder_pads_stuffs_and_restarts():
    """a unit of ones that ends a byte early: FF 00, a pad of one-bits, RST0 .. RST7 and RST0 again"""
    head = D.colour_header(0, 8 * 10, 8, dri=1)
    s = D.Scan(head)
    for k in range(10):
        if k:
            s.restart()
        s.mcu([(2047 if k & 1 else -2047, [(0, 1023), (0, 255)])], cb=(k, ()), cr=(-k, [(15, 0), (15, 0), (15, 0), (14, -1)]))
    data = s.file(head)
    assert data.count(b"\xff\x00") >= 5 and [data[b - 1] for b, _ in K.intervals(data)[1:]] == [0xd0 + k % 8 for k in range(9)]
    c = D.Case(data, 80, 8, 0, D.expected(s, 80, 8, 0))
    assert int(c.want[1, 0]) == 2047 and int(c.want[2 * 10 + 3, 63]) == -1
    assert np.array_equal(_twin_is_the_reader(c), c.want) and np.array_equal(_independent(c), c.want)


# ---- 1 .. 3: tiles, the halo, interval lengths ---------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(D.SEAM_CASES))
def test_seam_case(name):
    c = D.guarded(D.SEAM_CASES[name]())
    assert np.array_equal(_twin_is_the_reader(c), c.want)
    if not name.startswith("length_2"):               # the others have at most 3,100 blocks: 0.2 s each
        assert np.array_equal(_independent(c), c.want)


# ---- 4: refusals ---------------------------------------------------------------------------------------------
def test_refusals_are_listed():
    assert sorted(D.refusals()) == sorted(D.REFUSALS)


@pytest.mark.parametrize("name", D.REFUSALS)
def test_refusal(name):
    bad, good = D.refusals()[name]
    D.guarded(bad)
    assert (bad.W, bad.H, bad.sr) == (good.W, good.H, good.sr) and bad.data != good.data
    _twin_is_the_reader(bad)


# ---- 6: alignments ---------------------------------------------------------------------------------------------
def test_alignment_stride():
    for c in (D.ff_case("ff_then_seam"), D.short_case()):
        stride = D.odd_stride(len(c.data))
        assert stride >= len(c.data) and stride % 16 == 1
        D.guard_residues(0x7f0000001000, stride, c)
        with pytest.raises(AssertionError):
            D.guard_residues(0, stride + 1, c)
    short = D.guarded(D.short_case())
    _twin_is_the_reader(short)


# ---- 7: most rounds --------------------------------------------------------------------------------------------
def test_most_rounds():
    c = D.guarded(D.rounds_case())
    want = _twin_is_the_reader(c)
    assert np.array_equal(_independent(c), want)
    assert np.array_equal(want, D.maximal(c.W, c.H))
    # one block fewer does not fill a tile: the frame is the smallest
    W, H = 88, 8
    assert C.read_jfif_sub(K.write(D.maximal(W, H), W, H, 50, 0, 0))["stats"]["rounds_max"] < D.TILE - 1


# ---- 8: DC predictors ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,n", D.DC_SHAPES)
def test_dc_chunks(sr, n):
    kinds = set()
    for variant in D.dc_variants(sr):
        c = D.guarded(D.dc_case(sr, n, variant))
        kinds.add((variant[0], c.rc))
        _twin_is_the_reader(c)
        if c.rc == 0:
            assert np.array_equal(_independent(c), c.want)
            assert c.want[:, 0].min() >= -32768 and c.want[:, 0].max() <= 32767
            if variant[0] == "hold":
                assert int(c.want[:, 0].max() if variant[2] > 0 else c.want[:, 0].min()) == (32767 if variant[2] > 0 else -32768)
    assert kinds == {("random", 0), ("hold", 0), ("over", SCAN)}


# ---- 9, 10: k_jd_frame's passes, the gray grid -------------------------------------------------------------------
def test_frame_passes():
    c = D.guarded(D.passes_case())
    _twin_is_the_reader(c)
    _twin_is_the_reader(c.small)


def test_gray_grid_stride():
    c = D.guarded(D.grid_case())
    assert np.array_equal(_twin_is_the_reader(c), c.want) and np.array_equal(_independent(c), c.want)
