"""The decode at 1/2, 1/4 and 1/8 of the size on the host: jpgx_pixels_host_scaled and
jpgx_pixels_host_gray_scaled against the contract's numpy restatement (tests/idct_ref_scaled.py) and
against Pillow's draft decode (libjpeg-turbo's scale_denom), the rules that are easy to lose, each in a
test of its own, the refusals and the exports.  Every comparison is ==."""
import ctypes

import numpy as np
import pytest

import any_cases as A
import idct_ref_scaled as RS
import jpgx
import jpgx.compat as C
import scaled_cases as S

pillow = pytest.mark.skipif(not S.have_pillow(), reason="needs Pillow")
SAMP_IDS = [str(s) for s in S.SAMPLINGS]


def _channels(gray):
    return (1, 3) if gray else (1,)


@pillow
@pytest.mark.parametrize("samp", S.SAMPLINGS, ids=SAMP_IDS)
@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_twin_equals_the_restatement(size, samp):
    W, H = size
    gray = samp == "gray"
    for data in S.files(W, H, samp):
        r = S.read(data, gray)
        for d in S.SCALES:
            for ch in _channels(gray):
                got, want = S.host_pixels(r, gray, d, ch), S.ref_pixels(r, gray, d, ch)
                assert got.shape == want.shape == (S.out_size(W, H, d)[::-1] + ((3,) if ch == 3 or not gray else ()))
                assert np.array_equal(got, want), (W, H, samp, d, ch)
        # d = 1 is the any-size routine's call
        if gray:
            assert np.array_equal(S.host_raw_d1(r, True), C.pixels_host_gray(r["coef"], W, H, r["qt"], nthreads=1))
        else:
            assert np.array_equal(S.host_raw_d1(r, False),
                                  C.pixels_host(r["coef"], W, H, samp, r["qt"], nthreads=1, any_size=True))


@pillow
@pytest.mark.parametrize("samp", S.SAMPLINGS, ids=SAMP_IDS)
@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_twin_equals_pillows_draft_decode(size, samp):
    W, H = size
    gray = samp == "gray"
    for data in S.files(W, H, samp):
        r = S.read(data, gray)
        assert S.fits_16_bits(r, gray)
        for d in S.SCALES:
            if not S.pinned(W, H, d):
                continue                # compared with the restatement above
            want = S.draft_pixels(data, d, "L" if gray else "RGB")
            assert np.array_equal(S.host_pixels(r, gray, d), want), (W, H, samp, d)


@pillow
@pytest.mark.parametrize("sr", (0, 1, 2))
def test_host_twin_equals_pillow_on_this_projects_files(sr):
    for W, H, _, data in A.project_files(sr):
        r = S.read(data, False)
        assert (r["width"], r["height"]) == (W, H) and S.fits_16_bits(r, False)
        for d in S.SCALES:
            got = S.host_pixels(r, False, d)
            assert np.array_equal(got, S.ref_pixels(r, False, d)), (W, H, sr, d)
            assert np.array_equal(got, S.draft_pixels(data, d, "RGB")), (W, H, sr, d)


@pytest.mark.parametrize("samp", S.SAMPLINGS, ids=SAMP_IDS)
def test_hostile_frames(samp):
    W, H = S.HOSTILE_SIZE
    gray = samp == "gray"
    coefs, qts = S.hostile_frames(samp)
    for k in range(len(coefs)):
        for d in S.SCALES:
            if gray:
                got = C.pixels_host_gray(coefs[k], W, H, qts[k], nthreads=1, scale=d)
                want = RS.pixels_gray(coefs[k], W, H, qts[k], d)
            else:
                got = C.pixels_host(coefs[k], W, H, samp, qts[k], nthreads=1, scale=d)
                want = RS.pixels(coefs[k], W, H, samp, qts[k], d)
            assert np.array_equal(got, want), (samp, k, d)


def test_the_thread_count_does_not_matter():
    coefs, qts = S.hostile_frames(2, 100, 75)
    for d in S.SCALES:
        one = C.pixels_host(coefs[0], 100, 75, 2, qts[0], nthreads=1, scale=d)
        assert np.array_equal(C.pixels_host(coefs[0], 100, 75, 2, qts[0], nthreads=5, scale=d), one)


# ---- rules that are easy to lose ---------------------------------------------------------------
def _chroma_steps(W, H, d):
    """a 4:2:2 frame whose chroma differs from block to block and inside a block, under a table of 1"""
    g = RS.geometry(W, H, 1, d)
    nb, nbc = g["bw"] * g["bh"], g["cbw"] * g["cbh"]
    coef = np.zeros((nb + 2 * nbc, 64), np.int16)
    rng = np.random.default_rng(W + d)
    coef[nb:, 0] = rng.integers(-900, 900, 2 * nbc)
    coef[nb:, 1:6] = rng.integers(-200, 200, (2 * nbc, 5))
    return g, coef, np.ones((2, 64), np.uint16)


def _chroma_planes(g, coef, qt):
    nb, nbc = g["bw"] * g["bh"], g["cbw"] * g["cbh"]
    return [RS.samples(coef[nb + k * nbc:nb + (k + 1) * nbc], qt[1], g["cbw"], g["cbh"], g["n"]) for k in (0, 1)]


def test_422_at_one_eighth_replicates_whatever_wc_is():
    W, H = 64, 48
    g, coef, qt = _chroma_steps(W, H, 8)
    assert g["n"] == 1 and g["wc"] == 4 > 2
    cb, cr = _chroma_planes(g, coef, qt)
    y = np.full((g["oh"], g["ow"]), 128, RS.I32)        # Y's coefficients are zero
    want = RS.rgb(y, np.repeat(cb, 2, axis=1)[:g["oh"], :g["ow"]], np.repeat(cr, 2, axis=1)[:g["oh"], :g["ow"]])
    assert np.array_equal(C.pixels_host(coef, W, H, 1, qt, nthreads=1, scale=8), want)
    # and the triangle filter would have given other pixels
    tri = RS.rgb(y, RS.h2v1(cb, 4, True)[:g["oh"], :g["ow"]], RS.h2v1(cr, 4, True)[:g["oh"], :g["ow"]])
    assert not np.array_equal(tri, want)


def test_422_at_one_half_clamps_at_wc_and_replicates_two_samples():
    # 100: even, no multiple of 16; wc = 25 of the plane's 28 samples per row
    W, H = 100, 8
    g, coef, qt = _chroma_steps(W, H, 2)
    assert (g["n"], g["wc"], g["cbw"] * g["n"]) == (4, 25, 28)
    cb, cr = _chroma_planes(g, coef, qt)
    assert (cb[:, 24] != cb[:, 25]).any()               # the sample beyond wc - 1 differs: a clamp at the plane shows
    y = np.full((g["oh"], g["ow"]), 128, RS.I32)
    want = RS.rgb(y, RS.h2v1(cb, 25, True)[:g["oh"], :g["ow"]], RS.h2v1(cr, 25, True)[:g["oh"], :g["ow"]])
    got = C.pixels_host(coef, W, H, 1, qt, nthreads=1, scale=2)
    assert np.array_equal(got, want)
    unclamped = RS.rgb(y, RS.h2v1(cb, 28, True)[:g["oh"], :g["ow"]], RS.h2v1(cr, 28, True)[:g["oh"], :g["ow"]])
    assert not np.array_equal(unclamped[:, -1], want[:, -1])
    # W = 7: wc = 2, each sample twice
    W = 7
    g, coef, qt = _chroma_steps(W, H, 2)
    assert g["wc"] == 2 and g["ow"] == 4
    cb, cr = _chroma_planes(g, coef, qt)
    assert (cb[:, 0] != cb[:, 1]).any()
    y = np.full((g["oh"], 4), 128, RS.I32)
    want = RS.rgb(y, np.repeat(cb[:, :2], 2, axis=1)[:g["oh"]], np.repeat(cr[:, :2], 2, axis=1)[:g["oh"]])
    assert np.array_equal(C.pixels_host(coef, W, H, 1, qt, nthreads=1, scale=2), want)


def _without(coef_nat_mask):
    """two one-block frames that differ exactly in the natural positions of the mask"""
    rng = np.random.default_rng(5)
    nat = rng.integers(-300, 300, 64)
    other = np.where(coef_nat_mask, rng.integers(-300, 300, 64), nat)
    assert (other != nat)[coef_nat_mask].any()
    zz = np.asarray(RS.ZZ)
    a, b = np.zeros((1, 64), np.int16), np.zeros((1, 64), np.int16)
    a[0], b[0] = nat[zz], other[zz]
    return a, b


def test_input_4_has_no_influence_on_the_4_point_result():
    rows, cols = np.mgrid[0:8, 0:8]
    a, b = _without(((rows == 4) | (cols == 4)).reshape(64))
    qt = np.full(64, 3, np.uint16)
    assert np.array_equal(C.pixels_host_gray(a, 8, 8, qt, scale=2), C.pixels_host_gray(b, 8, 8, qt, scale=2))
    assert not np.array_equal(C.pixels_host_gray(a, 8, 8, qt), C.pixels_host_gray(b, 8, 8, qt))


def test_inputs_2_4_6_have_no_influence_on_the_2_point_result():
    rows, cols = np.mgrid[0:8, 0:8]
    even = lambda v: (v == 2) | (v == 4) | (v == 6)
    a, b = _without((even(rows) | even(cols)).reshape(64))
    qt = np.full(64, 3, np.uint16)
    assert np.array_equal(C.pixels_host_gray(a, 8, 8, qt, scale=4), C.pixels_host_gray(b, 8, 8, qt, scale=4))
    assert not np.array_equal(C.pixels_host_gray(a, 8, 8, qt, scale=2), C.pixels_host_gray(b, 8, 8, qt, scale=2))


def test_the_one_point_sample_is_the_descaled_dc():
    coef = np.zeros((1, 64), np.int16)
    coef[0, 1:] = 77                    # no other coefficient matters
    for dc, q, want in ((0, 1, 128), (4, 1, 129), (3, 1, 128), (-4, 1, 128), (-5, 1, 127), (100, 16, 255),
                        (-100, 16, 0), (32767, 65535, None), (-32768, 65535, None)):
        coef[0, 0] = dc
        got = C.pixels_host_gray(coef, 8, 8, np.full(64, q, np.uint16), scale=8)
        assert got.shape == (1, 1)
        d = np.array([dc * q], np.int64).astype(RS.I32)            # wraps
        with np.errstate(over="ignore"):
            ref = int(RS.range_limit((d + RS.I32(4)) >> RS.I32(3))[0])
        assert want is None or want == ref
        assert got[0, 0] == ref, (dc, q)


# ---- refusals and exports -------------------------------------------------------------------------
def test_scaled_size():
    assert jpgx.scaled_size(263, 21, 1) == (263, 21)
    assert jpgx.scaled_size(263, 21, 2) == (132, 11)
    assert jpgx.scaled_size(263, 21, 4) == (66, 6)
    assert jpgx.scaled_size(263, 21, 8) == (33, 3)
    assert jpgx.scaled_size(1, 1, 8) == (1, 1) and jpgx.scaled_size(65535, 65535, 8) == (8192, 8192)
    for bad in (0, 3, 16, -2, 2.0, True, None):
        with pytest.raises(ValueError):
            jpgx.scaled_size(8, 8, bad)
    for W, H in ((0, 8), (8, 0), (65536, 8), (8, -1)):
        with pytest.raises(ValueError):
            jpgx.scaled_size(W, H, 2)
    ow, oh = ctypes.c_int(), ctypes.c_int()
    assert jpgx.lib.jpgx_scaled_size(8, 8, 3, ctypes.byref(ow), ctypes.byref(oh)) == jpgx.EARG
    assert jpgx.lib.jpgx_scaled_size(8, 8, 2, None, ctypes.byref(oh)) == jpgx.EARG


def test_size_queries_return_0_for_bad_arguments():
    q = jpgx.lib.jpgx_pixels_gpu_scaled_workspace_size
    assert q(64, 48, 0, 2, 1) == 0 and q(64, 48, 1, 8, 1) == 0           # no workspace: fused
    assert q(64, 48, 1, 2, 3) == 3 * 2 * (4 * 6) * 16                     # 4 x 6 chroma blocks of 4 x 4
    assert q(64, 48, 1, 4, 1) == 2 * 24 * 4
    assert q(64, 48, 2, 2, 1) == 2 * 12 * 64 and q(64, 48, 2, 4, 1) == 2 * 12 * 16 and q(64, 48, 2, 8, 1) == 2 * 12 * 4
    assert q(64, 48, 2, 1, 1) == jpgx.lib.jpgx_pixels_gpu_any_workspace_size(64, 48, 2, 1) != 0
    for args in ((64, 48, 2, 3, 1), (64, 48, 2, 0, 1), (64, 48, 2, 16, 1), (64, 48, 3, 2, 1), (0, 48, 2, 2, 1),
                 (64, 65536, 2, 2, 1), (64, 48, 2, 2, 0), (64, 48, 2, 2, 65536)):
        assert q(*args) == 0, args


def test_host_twins_refuse():
    coef = np.zeros((6 + 12, 64), np.int16)
    qt = np.ones((2, 64), np.uint16)
    for bad in (0, 3, 16, -1):
        with pytest.raises(ValueError):
            C.pixels_host(coef, 24, 16, 0, qt, scale=bad)
        with pytest.raises(ValueError):
            C.pixels_host_gray(coef, 24, 16, qt[0], scale=bad)
        out = np.zeros(4096, np.uint8)
        assert jpgx.lib.jpgx_pixels_host_scaled(coef.ctypes.data, 24, 16, 0, bad, qt.ctypes.data, out.ctypes.data,
                                                256, 1) == jpgx.EARG
        assert jpgx.lib.jpgx_pixels_host_gray_scaled(coef.ctypes.data, 24, 16, bad, qt.ctypes.data, out.ctypes.data,
                                                     256, 1, 1) == jpgx.EARG
    with pytest.raises(jpgx.JpgxError) as e:            # a pitch below the scaled row
        C.pixels_host(coef, 24, 16, 0, qt, scale=2, pitch=35)
    assert e.value.rc == jpgx.EARG
    assert C.pixels_host(coef, 24, 16, 0, qt, scale=2, pitch=36).shape == (8, 12, 3)
    with pytest.raises(jpgx.JpgxError) as e:
        C.pixels_host_gray(coef, 24, 16, qt[0], channels=3, scale=4, pitch=17)
    assert e.value.rc == jpgx.EARG
    with pytest.raises(jpgx.JpgxError) as e:
        C.pixels_host(coef, 24, 16, 3, qt, scale=2)
    assert e.value.rc == jpgx.ESAMPLE


def test_device_entry_points_refuse_before_any_device_call():
    torch = pytest.importorskip("torch")
    coef = torch.zeros((1, 18, 64), dtype=torch.int16)
    qt = torch.ones((2, 64), dtype=torch.int16).view(torch.uint16)
    with pytest.raises(ValueError):                     # host tensors
        jpgx.pixels_gpu(coef, 24, 16, 0, d_qt=qt, scale=2)
    with pytest.raises(ValueError):
        jpgx.pixels_gpu_gray(coef, 24, 16, qt[0], scale=2)
    for bad in (0, 3, 16, "2"):
        with pytest.raises(ValueError):
            jpgx.pixels_gpu(coef, 24, 16, 0, d_qt=qt, scale=bad)
        with pytest.raises(ValueError):
            jpgx.pixels_gpu_gray(coef, 24, 16, qt[0], scale=bad)
        with pytest.raises(ValueError):
            jpgx.decode_jpeg(b"", "cuda", scale=bad)
    # the raw calls: nothing is dereferenced before the argument checks
    L = jpgx.lib
    p, n = 0x1000, None
    assert L.jpgx_pixels_gpu_scaled(p, 18 * 64, 1, 24, 16, 0, 3, p, 0, n, p, 40, 320, n, 0, n) == jpgx.EARG
    assert L.jpgx_pixels_gpu_scaled(p, 18 * 64, 1, 24, 16, 3, 2, p, 0, n, p, 40, 320, n, 0, n) == jpgx.ESAMPLE
    assert L.jpgx_pixels_gpu_scaled(p, 18 * 64, 1, 24, 70000, 0, 2, p, 0, n, p, 40, 320, n, 0, n) == jpgx.EGEOMETRY
    assert L.jpgx_pixels_gpu_scaled(p, 18 * 64, 1, 24, 16, 0, 2, p, 0, n, p, 32, 320, n, 0, n) == jpgx.EARG   # 3 * 12 = 36
    assert L.jpgx_pixels_gpu_scaled(p, 18 * 64, 1, 24, 16, 0, 2, p, 0, n, p, 44, 352, n, 0, n) == jpgx.EARG   # no multiple of 8
    assert L.jpgx_pixels_gpu_scaled(p, 18 * 64, 1, 24, 16, 0, 2, p, 0, n, p, 40, 312, n, 0, n) == jpgx.EARG   # 8 rows
    assert L.jpgx_pixels_gpu_scaled(p, 16 * 64, 1, 24, 16, 1, 2, p, 0, n, p, 40, 320, n, 0, n) == jpgx.EWORKSPACE
    assert L.jpgx_pixels_gpu_scaled(p, 16 * 64, 1, 24, 16, 1, 2, p, 0, n, p, 40, 320, n, 1 << 20, n) == jpgx.EARG
    assert L.jpgx_pixels_gpu_gray_scaled(p, 6 * 64, 1, 24, 16, 5, p, 0, n, p, 8, 64, 1, n) == jpgx.EARG
    assert L.jpgx_pixels_gpu_gray_scaled(p, 6 * 64, 1, 24, 16, 4, p, 0, n, p, 8, 64, 2, n) == jpgx.EARG      # channels
    assert L.jpgx_pixels_gpu_gray_scaled(p, 6 * 64, 1, 24, 16, 4, p, 0, n, p, 4, 64, 1, n) == jpgx.EARG      # ow = 6
    assert L.jpgx_pixels_gpu_gray_scaled(p, 6 * 64, 1, 24, 16, 4, p, 0, n, p, 8, 24, 1, n) == jpgx.EARG      # 4 rows
    assert L.jpgx_pixels_gpu_gray_scaled(p, 6 * 64, 1, 0, 16, 4, p, 0, n, p, 8, 64, 1, n) == jpgx.EGEOMETRY


def test_exports():
    new = ["jpgx_scaled_size", "jpgx_pixels_gpu_scaled_workspace_size", "jpgx_pixels_gpu_scaled",
           "jpgx_pixels_gpu_gray_scaled"]
    compat = ["jpgx_pixels_host_scaled", "jpgx_pixels_host_gray_scaled"]
    assert set(new) <= set(jpgx.EXPORTS) and set(compat) <= set(jpgx.COMPAT_EXPORTS)
    for path in (jpgx.LIB_PATH, jpgx.ALT_LIB_PATH):
        L = ctypes.CDLL(path)
        for name in new + compat:
            assert hasattr(L, name), (path, name)


@pytest.mark.skipif(not A.san_build.HAVE_CC, reason="needs gcc and g++")
def test_host_twins_under_asan_ubsan():
    """tests/c/pixels_scaled_san.c: a stand-alone program with the host pixel source, both built with
    the sanitizers; nothing is loaded into Python"""
    import os
    from conftest import PKG
    rc, out, err = A.san_build.run("pixels_scaled_san", [os.path.join(PKG, "csrc", "jpgx_pixels_host.cpp")], timeout=600)
    assert rc == 0 and out.rstrip().endswith("pixels_scaled_san: clean"), (out[-2000:], err[-4000:])
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-4000:]
    assert "frames " + str(4 * 303 * 4 * (3 + 2)) in out
