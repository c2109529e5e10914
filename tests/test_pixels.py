"""The pixel half of the decoder on the host: jpgx_pixels_host against the numpy
restatement of the contract (tests/idct_ref.py) and against Pillow's libjpeg decode, jpgx_jfif_qt,
jpgx_pixels_gpu's argument checks (no device is touched) and the sanitizer program
tests/c/pixels_san.c.  The arithmetic is integer: every comparison is ==."""
import io
import shutil

import numpy as np
import pytest

import idct_ref
import jpgx
import jpgx.compat as C
import pixels_cases as P

L = jpgx.lib


# ---- the host routine against the contract ---------------------------------------------------------
@pytest.mark.parametrize("sr", [0, 1, 2])
@pytest.mark.parametrize("kind", ["splitmix", "tie"])
def test_host_equals_the_contract(kind, sr):
    for W, H in P.SIZES[sr]:
        for q in P.QUALITIES:
            coef, qt = P.oracle_coef(kind, W, H, q, sr), P.qt_of(q)
            want = idct_ref.pixels(coef, W, H, sr, qt)
            assert want.shape == (H, W, 3)
            for nt in (1, 2, 5, 64):
                assert np.array_equal(C.pixels_host(coef, W, H, sr, qt, nt), want), (W, H, q, nt)


def test_the_frames_are_not_trivial():
    """the grid's pixels use the whole range in every plane (what the reference's forward path makes
    of an image is its own matter: the parity with libjpeg below is on the same coefficients)"""
    for sr in (0, 1, 2):
        got = C.pixels_host(P.oracle_coef("splitmix", 96, 64, 97, sr), 96, 64, sr, P.qt_of(97), 1)
        for k in range(3):
            assert got[..., k].std() > 40 and len(np.unique(got[..., k])) > 200


@pytest.mark.parametrize("sr", [0, 1, 2])
def test_padded_pitch_and_sentinels(sr):
    W, H = 48, 32
    coef, qt = P.oracle_coef("splitmix", W, H, 50, sr), P.qt_of(50)
    want = idct_ref.pixels(coef, W, H, sr, qt)
    for pitch in (3 * W + 1, 3 * W + 40):
        buf = np.full((H, pitch), 0x7A, np.uint8)
        assert L.jpgx_pixels_host(coef.ctypes.data, W, H, sr, qt.ctypes.data, buf.ctypes.data, pitch, 2) == 0
        assert np.array_equal(buf[:, :3 * W].reshape(H, W, 3), want)
        assert (buf[:, 3 * W:] == 0x7A).all()


@pytest.mark.parametrize("sr", [0, 1, 2])
def test_hostile_values(sr):
    """the wrap arithmetic and the wrapping range table: extreme coefficients and tables"""
    for W, H in ((16, 16), (48, 32)):
        coefs, qts = P.hostile_frames(W, H, sr)
        step = 1 if (W, H) == (16, 16) else 7           # the larger shape takes every 7th frame
        seen = set()
        for k in sorted(set(range(0, len(coefs), step)) | set(range(len(coefs) - 6, len(coefs)))):
            want = idct_ref.pixels(coefs[k], W, H, sr, qts[k])
            got = C.pixels_host(coefs[k], W, H, sr, qts[k], 2)
            assert np.array_equal(got, want), (W, H, k)
            seen.update(np.unique(got).tolist())
        assert len(seen) > 64                            # the outputs are not all clamped to 0 / 255


def test_host_argument_checks():
    coef, qt, out = np.zeros((3, 1, 64), np.int16), P.qt_of(50), np.zeros((8, 24), np.uint8)
    call = lambda c, w, h, sr, q, o, pitch, nt: L.jpgx_pixels_host(c, w, h, sr, q, o, pitch, nt)
    c, q, o = coef.ctypes.data, qt.ctypes.data, out.ctypes.data
    assert call(c, 8, 8, 0, q, o, 24, 1) == 0
    assert call(None, 8, 8, 0, q, o, 24, 1) == jpgx.EARG
    assert call(c, 8, 8, 0, None, o, 24, 1) == jpgx.EARG
    assert call(c, 8, 8, 0, q, None, 24, 1) == jpgx.EARG
    assert call(c, 8, 8, 0, q, o, 23, 1) == jpgx.EARG
    assert call(c, 8, 8, 0, q, o, 24, -1) == jpgx.EARG
    assert call(c, 8, 8, 3, q, o, 24, 1) == jpgx.ESAMPLE
    assert call(c, 8, 8, 1, q, o, 24, 1) == jpgx.EGEOMETRY
    assert call(c, 16, 8, 2, q, o, 48, 1) == jpgx.EGEOMETRY
    assert call(c, 12, 8, 0, q, o, 36, 1) == jpgx.EGEOMETRY


# ---- Pillow (libjpeg) parity -------------------------------------------------------------------------
def _decode_host(data):
    r = C.read_jfif(data, 1)
    W, H, sr = r["width"], r["height"], r["sample_ratio"]
    nb = (W // 8) * (H // 8)
    # libjpeg-turbo's SIMD multiplies coefficient and divisor in 16 bits: a condition, not a tolerance
    assert P.fits_16_bits(r["coef"], r["qt"], nb)
    return C.pixels_host(r["coef"], W, H, sr, r["qt"], 2)


def _pillow(data):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("name", ["smooth", "noise", "saturated"])
def test_pillow_parity_on_pillow_s_files(name, sub):
    Image = pytest.importorskip("PIL.Image")
    img = P.pillow_images()[name]
    for q in (10, 50, 90, 100):
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", quality=q, subsampling=sub)
        data = b.getvalue()
        assert C.jfif_info(data)["sample_ratio"] == sub
        assert np.array_equal(_decode_host(data), _pillow(data)), (name, q, sub)


@pytest.mark.parametrize("sr", [0, 1, 2])
def test_pillow_parity_on_this_project_s_files(sr):
    """jpgx_write_jfif_sub's files and their variants (Annex K.3 and per-image Huffman tables, with
    and without restart intervals) from the oracle's coefficients.  q 1 writes 16-bit DQT entries in
    an SOF1 frame; all four qualities meet the 16-bit condition (asserted in _decode_host)."""
    pytest.importorskip("PIL.Image")
    W, H = 96, 64
    for kind in ("splitmix", "tie"):
        for q in P.QUALITIES:
            coef = P.oracle_coef(kind, W, H, q, sr)
            files = [C.write_jfif_sub(coef, W, H, q, sr) if sr else C.write_jfif(coef.reshape(3, -1, 64), W, H, q)]
            files += [C.write_jfif_ex(coef, W, H, q, sr, restart_rows=rr, nthreads=1, optimize=opt)
                      for rr, opt in ((0, True), (1, False), (2, True))]
            want = C.pixels_host(coef, W, H, sr, P.qt_of(q), 1)
            for k, data in enumerate(files):
                got = _decode_host(data)
                assert np.array_equal(got, _pillow(data)), (kind, q, k)
                assert np.array_equal(got, want)         # inside the writers' clamps the coefficients come back


# ---- jpgx_jfif_qt ------------------------------------------------------------------------------------
def test_jfif_qt_is_the_writers_dqt():
    coef = np.zeros((3, 1, 64), np.int16)
    for q in (1, 23, 24, 50, 75, 97):
        back = C.read_jfif(C.write_jfif(coef, 8, 8, q), 1)["qt"]
        got = jpgx.jfif_qt(q)
        assert got.dtype == np.uint16 and got.shape == (2, 64) and np.array_equal(got, back), q
    assert jpgx.jfif_qt(23).max() > 255 >= jpgx.jfif_qt(24).max()
    qt = np.zeros((2, 64), np.uint16)
    for q in (0, 98):
        assert L.jpgx_jfif_qt(q, qt.ctypes.data) == jpgx.EQUALITY
        with pytest.raises(jpgx.JpgxError):
            jpgx.jfif_qt(q)


# ---- jpgx_pixels_gpu: every refusal happens before a device call, so none needs a device ---------------
def _gpu_call(coef=0x10000, cstride=3 * 4 * 64, nf=1, W=16, H=16, sr=0, qt=0x20000, qstride=0, status=None,
              rgb=0x30000, pitch=48, ostride=48 * 16, ws=None, wsb=0):
    return L.jpgx_pixels_gpu(coef, cstride, nf, W, H, sr, qt, qstride, status, rgb, pitch, ostride, ws, wsb, None)


def test_gpu_entry_point_argument_checks():
    E = jpgx.EARG
    assert _gpu_call(coef=None) == E and _gpu_call(qt=None) == E and _gpu_call(rgb=None) == E
    assert _gpu_call(coef=0x10008) == E                  # 16-byte alignment
    assert _gpu_call(qt=0x20001) == E                    # 2-byte
    assert _gpu_call(status=0x40002) == E                # 4-byte
    assert _gpu_call(rgb=0x30004) == E                   # 8-byte
    assert _gpu_call(nf=0) == E and _gpu_call(nf=65536, cstride=768) == E
    assert _gpu_call(cstride=3 * 4 * 64 - 64) == E and _gpu_call(cstride=3 * 4 * 64 + 32) == E
    assert _gpu_call(qstride=1) == E and _gpu_call(qstride=127) == E
    assert _gpu_call(pitch=47) == E and _gpu_call(pitch=40) == E and _gpu_call(pitch=52, ostride=52 * 16) == E
    assert _gpu_call(ostride=48 * 16 - 8) == E and _gpu_call(pitch=56, ostride=56 * 16 + 4) == E
    assert _gpu_call(sr=3) == jpgx.ESAMPLE and _gpu_call(sr=-1) == jpgx.ESAMPLE
    assert _gpu_call(W=12, pitch=40) == jpgx.EGEOMETRY and _gpu_call(H=12) == jpgx.EGEOMETRY
    assert _gpu_call(W=24, sr=1, pitch=72, ostride=72 * 16) == jpgx.EGEOMETRY
    assert _gpu_call(H=24, sr=2, ostride=48 * 24) == jpgx.EGEOMETRY
    # 4:2:x needs the chroma planes
    for sr, per, need in ((1, 4 + 4, 2 * 2 * 64), (2, 4 + 2, 2 * 64)):
        assert L.jpgx_pixels_gpu_workspace_size(16, 16, sr, 1) == need
        assert L.jpgx_pixels_gpu_workspace_size(16, 16, sr, 5) == 5 * need
        assert _gpu_call(sr=sr, cstride=per * 64, ws=0x50000, wsb=need - 1) == jpgx.EWORKSPACE
        assert _gpu_call(sr=sr, cstride=per * 64, ws=None, wsb=need) == E
        assert _gpu_call(sr=sr, cstride=per * 64, ws=0x50008, wsb=need) == E
        assert _gpu_call(sr=sr, cstride=per * 64 - 64, ws=0x50000, wsb=need) == E


def test_gpu_workspace_query():
    q = L.jpgx_pixels_gpu_workspace_size
    assert q(16, 16, 0, 1) == 0 and q(3840, 2160, 0, 8) == 0
    assert q(3840, 2160, 1, 8) == 8 * 2 * 1920 * 2160 and q(3840, 2160, 2, 8) == 8 * 2 * 1920 * 1080
    for bad in ((16, 16, 3, 1), (16, 16, -1, 1), (12, 16, 0, 1), (24, 16, 1, 1), (16, 24, 2, 1), (16, 16, 1, 0),
                (16, 16, 1, 65536), (0, 16, 0, 1)):
        assert q(*bad) == 0, bad


def test_exports():
    for name in ("jpgx_pixels_gpu_workspace_size", "jpgx_pixels_gpu", "jpgx_jfif_qt", "jpgx_pixels_host"):
        assert name in jpgx.EXPORTS + jpgx.COMPAT_EXPORTS
        assert hasattr(L, name) and hasattr(jpgx.alt_library(), name)


# ---- the host routine under the sanitizers -------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="needs gcc and g++")
def test_host_routine_under_asan_ubsan():
    rc, out, err = P.run_san()
    assert rc == 0 and out.rstrip().endswith("pixels_san: clean"), (out[-2000:], err[-4000:])
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-4000:]
    assert "frames " + str(6 * (3 + 576 + 1 + 2000)) in out
