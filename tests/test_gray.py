"""One-component (grayscale) baseline files on the host (csrc/jpgx_jfif_read.cpp: jpgx_jfif_info_of_gray,
jpgx_read_jfif_gray, jpgx_read_jfif_sub_gray; csrc/jpgx_pixels_host.cpp: jpgx_pixels_host_gray;
DESIGN.md 3, 4.8, 4.9): the committed files of tests/golden/gray_fixtures/ against an independent decoder
(tests/jfif_decode_gray.py), the twin of k_jd_sub_gray against the reader, the pixels against the
contract's numpy restatement and, where it is installed, against Pillow.  Every comparison is ==."""
import numpy as np
import pytest

import any_cases as A
import gray_cases as G
import jfif_decode_gray as D
import jfif_sub_cases as S
import jpgx
import jpgx.compat as C

pillow = pytest.mark.skipif(not G.have_pillow(), reason="needs Pillow")
FIXTURES = G.all_fixtures()
FILL = 0x7A


def _rc(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except jpgx.JpgxError as e:
        return e.rc
    return 0


def _segment(data, markers):
    """index of the 0xFF of the first segment with one of `markers`"""
    i = 2
    while data[i + 1] not in markers:
        i += 2 + (data[i + 2] << 8 | data[i + 3])
    return i


def _patch(data, at, val):
    b = bytearray(data)
    b[at] = val
    return bytes(b)


# ---- 1. coefficients and info ------------------------------------------------------------------------------
def test_fixture_set():
    assert len(FIXTURES) == 4 * len(G.SIZES) + 1 + len(G.PATCHED)
    assert sum(len(d) for _, _, _, d in FIXTURES) < 128 * 1024
    assert {W % 8 for W, _ in G.SIZES} == set(range(8)) and len({3 * W % 8 for W, _ in G.SIZES}) == 8


def test_coefficients_are_the_independent_decoder_s():
    for name, W, H, data in FIXTURES:
        want = D.decode(data)
        r = G.host(data)
        info = C.jfif_info_gray(data)
        assert (want["width"], want["height"]) == (W, H) == (r["width"], r["height"]), name
        assert np.array_equal(r["coef"], want["coef"]) and r["coef"].dtype == np.int16, name
        assert np.array_equal(r["qt"], want["qt"]), name
        assert (info["width"], info["height"], info["sample_ratio"]) == (W, H, 0), name
        assert info["nb_y"] == -(-W // 8) * -(-H // 8) == len(r["coef"]) and info["nb_c"] == 0, name
        assert info["restart_interval"] == want["restart_interval"] == r["restart_interval"], name   # in blocks
        assert r["coef"][:, 0].any() or W * H == 1, name


def test_restart_layouts_of_the_fixtures():
    """what the issue builds the fixtures for: intervals that straddle block rows, RSTn wrapping, 99 intervals"""
    f = G.files_of(21, 13)
    assert [D.decode(x)["restart_interval"] for x in f] == [3, 0, 2, 1]          # 3 blocks per row
    f = G.files_of(263, 21)
    assert [D.decode(x)["restarts"] for x in f] == [2, 0, 49, 98]
    scan = C.jfif_info_gray(G.big_file())["scan_offset"]
    s, t = jpgx.jfif_decode_sub_shape()
    assert (len(G.big_file()) - 2 - scan) // (s * t) == 5


def test_sampling_factors_are_ignored():
    base = G.host(G.files_of(21, 13)[2])
    for s, data in zip(G.PATCHED, G.patched_files()):
        assert D.decode(data)["sampling"] == (s >> 4, s & 15)
        r = G.host(data)
        assert np.array_equal(r["coef"], base["coef"]) and np.array_equal(r["qt"], base["qt"])
        assert C.jfif_info_gray(data) == C.jfif_info_gray(G.files_of(21, 13)[2])


# ---- 2. the sub-interval host twin -----------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.SHAPES)
def test_twin_equals_reader(shape):
    for name, W, H, data in FIXTURES:
        r, s = G.host(data), C.read_jfif_sub_gray(data, *shape)
        assert np.array_equal(s["coef"], r["coef"]) and np.array_equal(s["qt"], r["qt"]), (name, shape)
        assert s["restart_interval"] == r["restart_interval"]
    for data in G.damaged_sample(64):
        a = G.host_status(data, 21, 13)
        b = G.host_status(data, 21, 13, lambda d: C.read_jfif_sub_gray(d, *shape))
        assert a[0] == b[0]
        if a[0] == 0:
            assert np.array_equal(a[1]["coef"], b[1]["coef"]) and np.array_equal(a[1]["qt"], b[1]["qt"])


# ---- 3. pixels -----------------------------------------------------------------------------------------------
def test_pixels_are_the_contract_s():
    for name, W, H, data in FIXTURES:
        r = G.host(data)
        px = C.pixels_host_gray(r["coef"], W, H, r["qt"], 1, nthreads=1 + len(data) % 3)
        assert px.shape == (H, W) and np.array_equal(px, G.range_limit_ref(r["coef"], r["qt"], W, H)), name
        rgb = C.pixels_host_gray(r["coef"], W, H, r["qt"], 3)
        assert rgb.shape == (H, W, 3) and np.array_equal(rgb, np.repeat(px[:, :, None], 3, 2)), name


@pillow
def test_pixels_are_pillow_s():
    for name, W, H, data in FIXTURES:
        r = G.host(data)
        # Pillow wrote these files from 8-bit images: none is outside libjpeg-turbo's 16-bit products
        assert G.fits_16_bits(r), name
        assert np.array_equal(C.pixels_host_gray(r["coef"], W, H, r["qt"], 1), G.pillow_pixels(data)), name
        assert np.array_equal(C.pixels_host_gray(r["coef"], W, H, r["qt"], 3), G.pillow_pixels(data, "RGB")), name


@pillow
def test_patched_sampling_pixels():
    base = G.files_of(21, 13)[2]
    want = C.pixels_host_gray(G.host(base)["coef"], 21, 13, G.host(base)["qt"])
    for data in G.patched_files():
        r = G.host(data)
        got = C.pixels_host_gray(r["coef"], 21, 13, r["qt"])
        assert np.array_equal(got, want) and np.array_equal(got, G.pillow_pixels(data))


def test_patched_sampling_pixels_without_pillow():
    base = G.host(G.files_of(21, 13)[2])
    for data in G.patched_files():
        r = G.host(data)
        assert np.array_equal(C.pixels_host_gray(r["coef"], 21, 13, r["qt"]),
                              C.pixels_host_gray(base["coef"], 21, 13, base["qt"]))


# ---- 4. hostile values ------------------------------------------------------------------------------------
def test_hostile_values_wrap_like_the_restatement():
    W, H = 21, 13
    coefs, qts = G.hostile_frames(W, H)
    for k in range(len(coefs)):
        px = C.pixels_host_gray(coefs[k], W, H, qts[k], 1, nthreads=1)
        assert np.array_equal(px, G.range_limit_ref(coefs[k], qts[k], W, H)), k
        assert np.array_equal(C.pixels_host_gray(coefs[k], W, H, qts[k], 3, nthreads=2), np.repeat(px[:, :, None], 3, 2)), k


@pytest.mark.parametrize("channels", [1, 3])
def test_padded_pitch_keeps_its_sentinel(channels):
    import ctypes
    for W, H in ((21, 13), (65, 17), (1, 1)):
        r = G.host(G.files_of(W, H)[1])
        pitch, spare = channels * W + 11, 2
        buf = np.full((H + spare, pitch), FILL, np.uint8)
        rc = jpgx.lib.jpgx_pixels_host_gray(r["coef"].ctypes.data, W, H, r["qt"].ctypes.data, buf.ctypes.data,
                                            ctypes.c_size_t(pitch), channels, 2)
        assert rc == 0
        want = C.pixels_host_gray(r["coef"], W, H, r["qt"], channels).reshape(H, channels * W)
        assert np.array_equal(buf[:H, :channels * W], want)
        assert (buf[:H, channels * W:] == FILL).all() and (buf[H:] == FILL).all()


# ---- 5. refusals ---------------------------------------------------------------------------------------------
def _colour_files():
    files = [data for sr in (0, 1, 2) for _, _, _, data in A.project_files(sr)]
    if A.have_pillow():
        files += [f for sr in (0, 1, 2) for W, H in A.SIZES for f in A.pillow_files(W, H, sr)]
    return files


def test_colour_files_are_refused_by_the_gray_readers():
    files = _colour_files()
    assert len(files) >= 15
    for data in files:
        assert _rc(C.jfif_info_gray, data) == jpgx.EJFIF_HEADER
        assert _rc(C.read_jfif_gray, data) == jpgx.EJFIF_HEADER
        assert _rc(C.read_jfif_sub_gray, data) == jpgx.EJFIF_HEADER


def test_gray_files_are_refused_by_the_colour_readers():
    for name, W, H, data in FIXTURES:
        for any_size in (False, True):
            assert _rc(C.jfif_info, data, any_size=any_size) == jpgx.EJFIF_HEADER, name
            assert _rc(C.read_jfif, data, any_size=any_size) == jpgx.EJFIF_HEADER, name
            assert _rc(C.read_jfif_sub, data, any_size=any_size) == jpgx.EJFIF_HEADER, name


def test_pixel_argument_checks():
    r = G.host(G.files_of(8, 8)[1])
    px = lambda *a, **kw: _rc(C.pixels_host_gray, r["coef"], *a, **kw)   # noqa: E731
    assert px(8, 8, r["qt"], 1) == 0 and px(8, 8, r["qt"], 3) == 0
    for ch in (0, 2, 4):
        assert px(8, 8, r["qt"], ch) == jpgx.EARG
    assert px(8, 8, r["qt"], 1, pitch=7) == jpgx.EARG and px(8, 8, r["qt"], 3, pitch=23) == jpgx.EARG
    for W, H in ((0, 8), (8, 0), (65536, 8), (8, 65536)):
        assert px(W, H, r["qt"], 1) == jpgx.EGEOMETRY
    assert _rc(C.read_jfif_sub_gray, G.files_of(8, 8)[1], 15, 2) == jpgx.EARG


def test_header_refusals():
    data = G.files_of(21, 13)[2]
    sof, sos = _segment(data, (0xC0, 0xC1)), _segment(data, (0xDA,))
    assert data[sof + 9] == 1 and data[sos + 4] == 1 and data[sos + 6] == 0x00
    bad = {"Nf = 2": _patch(data, sof + 9, 2), "Ns = 2": _patch(data, sos + 4, 2),
           "an absent DC table": _patch(data, sos + 6, 0x10), "an absent AC table": _patch(data, sos + 6, 0x01),
           "an absent DQT": _patch(data, sof + 12, 1), "Tq = 4": _patch(data, sof + 12, 4),
           "another component id": _patch(data, sos + 5, data[sos + 5] ^ 1),
           "Ss = 1": _patch(data, sos + 7, 1), "Se = 62": _patch(data, sos + 8, 62), "Al = 1": _patch(data, sos + 9, 1),
           "12-bit samples": _patch(data, sof + 4, 12)}
    for s in (0x01, 0x10, 0x51, 0x15, 0x00, 0xff):
        bad["sampling %02x" % s] = _patch(data, sof + 11, s)
    for why, d in bad.items():
        assert _rc(C.jfif_info_gray, d) == jpgx.EJFIF_HEADER, why
        assert _rc(C.read_jfif_gray, d) == jpgx.EJFIF_HEADER, why
        assert _rc(C.read_jfif_sub_gray, d) == jpgx.EJFIF_HEADER, why
    for s in (0x11, 0x14, 0x44, 0x31):                   # every factor 1 .. 4 is taken, and ignored
        assert np.array_equal(C.read_jfif_gray(_patch(data, sof + 11, s))["coef"], G.host(data)["coef"])
    assert _rc(C.read_jfif_gray, _patch(data, sof + 10, 200)) == jpgx.EJFIF_HEADER   # any component id, if SOS names it
    assert _rc(C.read_jfif_gray, _patch(_patch(data, sof + 10, 200), sos + 5, 200)) == 0


def test_exports():
    for name in ("jpgx_jfif_decode_gpu_gray_workspace_size", "jpgx_jfif_decode_gpu_gray", "jpgx_pixels_gpu_gray"):
        assert name in jpgx.EXPORTS and hasattr(jpgx.lib, name) and hasattr(jpgx.alt_library(), name)
    for name in ("jpgx_jfif_info_of_gray", "jpgx_read_jfif_gray", "jpgx_read_jfif_sub_gray", "jpgx_pixels_host_gray"):
        assert name in jpgx.COMPAT_EXPORTS and hasattr(jpgx.lib, name) and hasattr(jpgx.alt_library(), name)
    assert jpgx.lib.jpgx_jfif_decode_gpu_gray_workspace_size(21, 13, 1, 4096, 0) > 0
    assert jpgx.lib.jpgx_jfif_decode_gpu_gray_workspace_size(21, 13, 1, 4096, 2) == 0
    assert jpgx.lib.jpgx_jfif_decode_gpu_gray_workspace_size(0, 13, 1, 4096, 0) == 0
    assert jpgx.lib.jpgx_jfif_decode_gpu_gray_workspace_size(21, 65536, 1, 4096, 0) == 0


# ---- 11. the device entry points refuse bad arguments before any device call --------------------------------
# (these run without a device: a call that got as far as a launch would fail differently, and the fake
# addresses are never touched)
L = jpgx.lib
SUB = jpgx.JFIF_DECODE_SUBINTERVAL


def _dec_call(files=0x10000, fstride=1 << 16, lens=0x20000, nf=1, W=21, H=13, flags=0, coef=0x30000, cstride=6 * 64,
              qt=0x40000, status=0x50000, ws=0x60000, wsb=None):
    if wsb is None:
        wsb = L.jpgx_jfif_decode_gpu_gray_workspace_size(W, H, max(nf, 1), fstride, 0) or 1 << 20
    return L.jpgx_jfif_decode_gpu_gray(files, fstride, lens, nf, W, H, flags, coef, cstride, qt, status, ws, wsb, None)


@pytest.mark.parametrize("flags", [0, SUB])
def test_decoder_refuses_bad_arguments_without_a_device(flags):
    def call(**kw):
        return _dec_call(flags=flags, **kw)
    E = jpgx.EARG
    for name in ("files", "lens", "coef", "status", "ws"):
        assert call(**{name: None}) == E, name
    assert call(lens=0x20004) == E and call(coef=0x30008) == E and call(status=0x50002) == E
    assert call(qt=0x40001) == E and call(ws=0x60008) == E
    assert call(nf=0) == E and call(nf=65536) == E
    assert call(fstride=0) == E and call(fstride=1 << 32) == E
    for side in (0, 65536, -8):
        assert call(W=side) == E and call(H=side) == E
    # 21 x 13 codes 3 x 2 blocks
    assert call(cstride=6 * 64 + 32) == E and call(cstride=6 * 64 - 64) == E
    # the order is the _any call's: EARG before EWORKSPACE; EGEOMETRY does not occur
    assert call(cstride=32, wsb=1) == E and call(wsb=1) == jpgx.EWORKSPACE
    for unknown in (2, 3, 4, 1 << 31):
        assert _dec_call(flags=unknown) == E and _dec_call(flags=unknown, W=0) == E
        assert L.jpgx_jfif_decode_gpu_gray_workspace_size(21, 13, 1, 1 << 16, unknown) == 0
    for W, H, nb in ((21, 13, 6), (1, 1, 1), (263, 200, 33 * 25), (65535, 1, 8192)):
        for f in (0, SUB):
            want = L.jpgx_jfif_decode_gpu_gray_workspace_size(W, H, 2, 4097, f)
            assert want > 0 and want % 16 == 0
            assert _dec_call(W=W, H=H, nf=2, fstride=4097, cstride=nb * 64, flags=f, wsb=want - 1) == jpgx.EWORKSPACE
    # the workspace is sized by the blocks: 4 bytes more per block and frame, rounded up to 16 per part
    a, b = (L.jpgx_jfif_decode_gpu_gray_workspace_size(8 * n, 8, 1, 4096, 0) for n in (4, 8))
    assert b - a == 16
    for bad in (dict(nf=0), dict(nf=65536), dict(W=0), dict(H=65536), dict(cap=0), dict(cap=1 << 32)):
        a = dict(W=21, H=13, nf=1, cap=1 << 16)
        a.update(bad)
        assert L.jpgx_jfif_decode_gpu_gray_workspace_size(a["W"], a["H"], a["nf"], a["cap"], flags) == 0, bad


def _px_call(coef=0x10000, cstride=6 * 64, nf=1, W=21, H=13, qt=0x20000, qstride=0, status=None, out=0x30000, pitch=24,
             ostride=24 * 13, channels=1):
    return L.jpgx_pixels_gpu_gray(coef, cstride, nf, W, H, qt, qstride, status, out, pitch, ostride, channels, None)


def test_pixels_refuse_bad_arguments_without_a_device():
    call, E = _px_call, jpgx.EARG
    assert call(coef=None) == E and call(qt=None) == E and call(out=None) == E
    assert call(coef=0x10008) == E and call(qt=0x20001) == E and call(status=0x40002) == E and call(out=0x30004) == E
    assert call(nf=0) == E and call(nf=65536) == E
    for ch in (0, 2, 4, -1):
        assert call(channels=ch) == E
    assert call(cstride=6 * 64 - 64) == E and call(cstride=6 * 64 + 32) == E
    assert call(qstride=1) == E and call(qstride=63) == E
    assert call(pitch=16) == E and call(pitch=20, ostride=20 * 13) == E            # W = 21
    assert call(channels=3, pitch=56, ostride=56 * 13) == E                        # 3 W = 63
    assert call(channels=3, pitch=60, ostride=60 * 13) == E
    assert call(ostride=24 * 13 - 8) == E and call(pitch=32, ostride=32 * 13 + 4) == E
    # a side outside 1 .. 65535 has the _any call's code; before it, the _any call's EARGs
    for side in (0, 65536):
        assert call(W=side) == jpgx.EGEOMETRY and call(H=side) == jpgx.EGEOMETRY
        assert call(W=side, nf=0) == E and call(W=side, channels=2) == E


# ---- 6. sanitizers -------------------------------------------------------------------------------------------
@pytest.mark.skipif(not G.san_build.HAVE_CC, reason="needs gcc and g++")
def test_damaged_files_under_the_sanitizers():
    rc, out, err = G.run_san()
    assert rc == 0 and "gray_san: clean" in out, (out[-2000:], err[-4000:])
    small = [d for _, _, _, d in FIXTURES if len(d) <= G.SAN_MAX]
    want = sum(1 + 4 * len(d) for d in small)
    print(out)
    assert "files %d cases %d " % (len(small), want) in out
