"""The pixel half of the decoder on the host: jpgx_pixels_host against the numpy
restatement of the contract (tests/idct_ref.py) and against Pillow's libjpeg decode, jpgx_jfif_qt,
jpgx_pixels_gpu's argument checks (no device is touched) and the sanitizer program
tests/c/pixels_san.c; the model of the device's 24-bit multiplier (idct_ref.mul24) and the guards of the
frames that pin the kernels' choice of multiplier (tests/pixels_cases.py; the device side is
tests/test_pixels_mul_gpu.py).  The arithmetic is integer: every comparison is ==."""
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


# ---- the multiplier choice: a model of the 24-bit multiplier, and frames on which it shows ------------------
def test_mul24_is_the_24_bit_multiplier():
    m = lambda a, c: int(idct_ref.mul24(np.array([a], np.int64).astype(np.int32), np.int32(c))[0])   # noqa: E731
    assert m(3, -7) == -21 and m(-1, -1) == 1 and m(0x7FFFFF, 2) == 0xFFFFFE
    assert m(0x800000, 1) == -0x800000                      # bit 23 is the sign
    assert m(0x1000000, 5) == 0 and m(0x1000003, 5) == 15   # bits 24 .. 31 are not read
    assert m(-0x800001, 1) == 0x7FFFFF
    assert m(0x7FFFFF, 0x7FFFFF) == (0x7FFFFF * 0x7FFFFF) % (1 << 32) - (1 << 32)      # the product's low 32 bits
    rng = np.random.default_rng(24)
    a = rng.integers(-(1 << 23), 1 << 23, 4096).astype(np.int32)
    c = rng.integers(-(1 << 23), 1 << 23, 4096).astype(np.int32)
    with np.errstate(over="ignore"):
        assert np.array_equal(idct_ref.mul24(a, c), a * c)          # in range: the 32-bit multiplier's


def test_the_model_is_the_contract_where_the_kernels_may_use_it():
    """random full-range blocks under uniform 63 and 64: every number that is multiplied is inside 24 bits"""
    blocks = np.random.default_rng(63).integers(-32768, 32768, (500, 64)).astype(np.int16)
    for t in (1, 63, 64):
        qt = np.full(64, t, np.uint16)
        assert np.array_equal(idct_ref.samples(blocks, qt, 20, 25, m24=True), idct_ref.samples(blocks, qt, 20, 25)), t
    # and it is not vacuous: under 255 most samples differ
    qt = np.full(64, 255, np.uint16)
    assert (idct_ref.samples(blocks, qt, 20, 25, m24=True) != idct_ref.samples(blocks, qt, 20, 25)).mean() > 0.5


def test_63_and_64_cannot_tell_the_multipliers_apart():
    for sr in (0, 1, 2):
        case = P.cannot_tell_case(sr)
        assert len(case["names"]) == 8
        for k, name in enumerate(case["names"]):
            assert not P.tells(case, k), (sr, name)
            assert np.array_equal(P.host_pixels(case, k), P.model_pixels("plain", case["coefs"][k], 48, 32, sr, case["qts"][k], False))


MUL = P.multiplier_cases()


@pytest.mark.parametrize("name", [m[0] for m in MUL])
def test_multiplier_cases_tell_and_the_host_is_the_contract(name):
    """every frame's guard, and the host twin == the restatement on it"""
    case, channels = next(m[1:] for m in MUL if m[0] == name)
    assert len(case["names"]) == len(case["coefs"]) == len(case["qts"]) == len(case["regions"]) >= 5
    for k, what in enumerate(case["names"]):
        y0, y1, x0, x1 = case["regions"][k]
        assert y0 < y1 <= case["H"] and x0 < x1 <= case["W"], what
        assert P.tells(case, k), (name, what)
        want = P.model_pixels(case["kind"], case["coefs"][k], case["W"], case["H"], case["sr"], case["qts"][k], False,
                              channels or 1)
        assert np.array_equal(P.host_pixels(case, k, channels), want), (name, what)


def test_multiplier_cases_cover_what_they_are_for():
    from idct_ref import ZZ
    for sr in (0, 1, 2):
        names = P.threshold_case(sr)[1]
        assert any(n.startswith("luma 63, chroma 65") for n in names) and any(n.startswith("luma 65, chroma 63") for n in names)
        assert sum(n.endswith("random") for n in names) >= 5            # from 96 up
    for sr in (0, 1, 2):
        for ch in (0, 1, 2):
            case = P.vote_lane_case(sr, ch)
            first = P.planes_of(case["W"], case["H"], sr, "plain")[ch][0]
            lanes = set()
            for k in range(64):
                c = case["coefs"][k].astype(np.int32)
                big = np.argwhere(np.abs(c) > P.BACKGROUND)
                assert len(big) == 1                                    # one large value, in one channel
                blk, pos = int(big[0][0]) - first, int(big[0][1])
                assert 0 <= blk < 8 and (ZZ[pos] >> 3) % 4 != 0         # natural rows 0 and 4 are never multiplied
                lanes.add((blk, pos >> 3))
            assert len(lanes) == 64                                     # no load lane is left out
    for W, H, sr, kind, per_row in ((264, 8, 0, "plain", (33, 33, 33)), (528, 16, 1, "plain", (66, 33, 33)),
                                    (523, 13, 2, "any", (66, 33, 33)), (264, 8, 0, "gray", (33,))):
        case = P.vote_run_case(W, H, sr, kind)
        planes = P.planes_of(W, H, sr, kind)
        assert tuple(p[1] for p in planes) == per_row
        runs = set()
        for k in range(len(case["names"])):
            big = np.argwhere(np.abs(case["coefs"][k].astype(np.int32)) > P.BACKGROUND)
            assert len(big) == 1
            ch = max(i for i, p in enumerate(planes) if p[0] <= big[0][0])
            runs.add((ch, (int(big[0][0]) - planes[ch][0]) % planes[ch][1] // 8))
        assert runs == {(ch, r) for ch, p in enumerate(planes) for r in range(-(-p[1] // 8))}
        assert any("block 32 " in n for n in case["names"])             # the tail's single live block


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
