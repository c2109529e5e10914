"""Baseline JFIF files of any width and height, on the host: the _any readers
against an independent decoder (tests/jfif_decode.py), the twin of k_jd_sub against the reader,
jpgx_pixels_host_any against the numpy restatement of the contract (tests/idct_ref_any.py) and against
Pillow's libjpeg decode, the _any calls against the plain ones at sizes both take, the argument checks
of the two device entry points (no device is touched) and the sanitizer program tests/c/any_san.c.
Every comparison is ==."""
import numpy as np
import pytest

import any_cases as A
import idct_ref_any as R
import jpgx
import jpgx.compat as C
import pixels_cases as P
from jfif_decode import decode

L = jpgx.lib
SUB = jpgx.JFIF_DECODE_SUBINTERVAL
pillow = pytest.mark.skipif(not A.have_pillow(), reason="needs Pillow")


def _rc(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except jpgx.JpgxError as e:
        return e.rc
    return 0


def _check_file(data, W, H, sr, against_pillow):
    """one file through the readers and the pixel routine; returns (read_jfif's dict, the pixels)"""
    r = C.read_jfif(data, 1, any_size=True)
    assert (r["width"], r["height"], r["sample_ratio"]) == (W, H, sr)
    nb, nbc = R.nblocks(W, H, sr)
    info = C.jfif_info(data, any_size=True)
    assert (info["nb_y"], info["nb_c"]) == (nb, nbc)
    ind = decode(data)
    assert (ind["width"], ind["height"], ind["sampling"]) == (W, H, R.sampling(sr))
    coef = r["coef"].reshape(-1, 64)
    assert coef.shape == (nb + 2 * nbc, 64)
    assert np.array_equal(coef, np.concatenate([np.asarray(c).reshape(-1, 64) for c in ind["coef"]]))
    assert np.array_equal(r["qt"][0], ind["dqt"][ind["qsel"][0]]) and np.array_equal(r["qt"][1], ind["dqt"][ind["qsel"][1]])
    for shape in ((0, 0), (16, 2)):
        s = C.read_jfif_sub(data, *shape, any_size=True)
        assert np.array_equal(s["coef"], r["coef"]) and np.array_equal(s["qt"], r["qt"]), shape
        assert (s["width"], s["height"], s["restart_interval"]) == (W, H, r["restart_interval"])
    assert np.array_equal(C.read_jfif(data, 3, any_size=True)["coef"], r["coef"])
    want = R.pixels(r["coef"], W, H, sr, r["qt"])
    assert want.shape == (H, W, 3)
    got = C.pixels_host(r["coef"], W, H, sr, r["qt"], 2, any_size=True)
    assert np.array_equal(got, want)
    assert np.array_equal(C.pixels_host(r["coef"], W, H, sr, r["qt"], 5, any_size=True), want)
    if against_pillow:
        assert A.fits_16_bits(r)                     # a condition of the comparison, not a tolerance
        assert np.array_equal(got, A.pillow_pixels(data))
    return r, got


# ---- the readers and the pixels: Pillow's files ---------------------------------------------------------
@pillow
@pytest.mark.parametrize("sr", [0, 1, 2])
@pytest.mark.parametrize("W,H", A.SIZES)
def test_pillow_s_files(W, H, sr):
    for kind in A.KINDS:
        for q in A.QUALITIES:
            for writer in range(len(A.WRITERS)):
                data = A.pillow_file(kind, W, H, sr, q, writer)
                r, _ = _check_file(data, W, H, sr, True)
                assert (r["restart_interval"] > 0) == (writer == 0)


# ---- this project's files with the SOF patched down ------------------------------------------------------
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_this_project_s_files_patched_down(sr):
    for W, H, coef, data in A.project_files(sr):
        assert _rc(C.read_jfif, data, 1) == jpgx.EJFIF_HEADER        # the plain reader refuses the size
        r, got = _check_file(data, W, H, sr, A.have_pillow())
        assert np.array_equal(r["coef"].reshape(-1, 64), coef)       # inside the writers' clamps
    # the pixels are not the crop of the coded frame's: the clamps are at the component's real extent
    if sr:
        W, H, coef, data = A.project_files(sr)[0]                    # 50 wide: the last column reads p[wc]
        qt = C.read_jfif(data, 1, any_size=True)["qt"]
        whole = C.pixels_host(coef, *A.BASE, sr, qt, 1)
        got = C.pixels_host(coef, W, H, sr, qt, 1, any_size=True)
        assert np.array_equal(got[:H - 2, :W - 1], whole[:H - 2, :W - 1])
        assert not np.array_equal(got, whole[:H, :W])


def test_the_replication_rule_is_exercised():
    """with wc <= 2 no filter runs: a frame whose two chroma samples differ shows it"""
    for sr in (1, 2):
        nb, nbc = R.nblocks(4, 4, sr)
        coef = np.zeros((nb + 2 * nbc, 64), np.int16)
        coef[nb, 1] = 300                            # a horizontal ramp in Cb
        coef[nb + nbc, 8] = -300                     # a vertical one in Cr
        qt = np.ones((2, 64), np.uint16)
        got = C.pixels_host(coef, 4, 4, sr, qt, 1, any_size=True)
        assert np.array_equal(got, R.pixels(coef, 4, 4, sr, qt))
        assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 2], got[:, 3])
        assert not np.array_equal(got[:, 1], got[:, 2])
        if sr == 2:
            assert np.array_equal(got[0], got[1]) and np.array_equal(got[2], got[3]) and not np.array_equal(got[1], got[2])


# ---- sizes both families take ----------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_mcu_multiples_equal_the_plain_calls(sr):
    for W, H in P.SIZES[sr]:
        coef, qt = P.oracle_coef("splitmix", W, H, 50, sr), P.qt_of(50)
        assert jpgx.coded_size(W, H, sr) == (W, H)
        assert np.array_equal(C.pixels_host(coef, W, H, sr, qt, 2, any_size=True), C.pixels_host(coef, W, H, sr, qt, 2))
        for rr, opt in ((1, False), (0, True)):
            data = C.write_jfif_ex(coef, W, H, 50, sr, restart_rows=rr, nthreads=1, optimize=opt)
            assert C.jfif_info(data, any_size=True) == C.jfif_info(data)
            a, b = C.read_jfif(data, 1, any_size=True), C.read_jfif(data, 1)
            assert all(np.array_equal(a[k], b[k]) for k in a)
            a, b = C.read_jfif_sub(data, any_size=True), C.read_jfif_sub(data)
            assert a["stats"] == b["stats"] and all(np.array_equal(a[k], b[k]) for k in a if k != "stats")
        for nf, cap in ((1, 1 << 16), (3, 40000)):
            for flags in (0, SUB):
                assert (L.jpgx_jfif_decode_gpu_any_workspace_size(W, H, sr, nf, cap, flags)
                        == L.jpgx_jfif_decode_gpu_workspace_size_ex(W, H, sr, nf, cap, flags) > 0)
            assert L.jpgx_pixels_gpu_any_workspace_size(W, H, sr, nf) == L.jpgx_pixels_gpu_workspace_size(W, H, sr, nf)


def test_workspaces_are_the_coded_frame_s():
    for (W, H, sr) in ((57, 41, 0), (50, 42, 1), (49, 33, 2), (1, 1, 2), (3839, 2159, 2)):
        cw, ch = jpgx.coded_size(W, H, sr)
        assert (cw, ch) == R.coded(W, H, sr)
        assert L.jpgx_pixels_gpu_any_workspace_size(W, H, sr, 3) == L.jpgx_pixels_gpu_workspace_size(cw, ch, sr, 3)
        for flags in (0, SUB):
            assert (L.jpgx_jfif_decode_gpu_any_workspace_size(W, H, sr, 3, 40000, flags)
                    == L.jpgx_jfif_decode_gpu_workspace_size_ex(cw, ch, sr, 3, 40000, flags) > 0)
    assert jpgx.coded_size(65535, 65535, 2) == (65536, 65536)
    for bad in ((0, 8, 0), (8, 65536, 0), (8, 8, 3), (8, 8, -1)):
        with pytest.raises(jpgx.JpgxError):
            jpgx.coded_size(*bad)


def test_the_plain_entry_points_still_refuse():
    coef = np.zeros((3 * 64, 64), np.int16)
    data = A.patch_size(C.write_jfif_ex(coef, 64, 64, 50, 0, restart_rows=1, nthreads=1), 60, 64)
    assert _rc(C.jfif_info, data) == jpgx.EJFIF_HEADER and _rc(C.read_jfif, data, 1) == jpgx.EJFIF_HEADER
    assert _rc(C.read_jfif_sub, data) == jpgx.EJFIF_HEADER
    assert C.jfif_info(data, any_size=True)["width"] == 60
    assert _rc(C.pixels_host, coef, 60, 64, 0, P.qt_of(50)) == jpgx.EGEOMETRY
    assert L.jpgx_jfif_decode_gpu_workspace_size_ex(60, 64, 0, 1, 1 << 16, 0) == 0
    assert L.jpgx_pixels_gpu_workspace_size(60, 64, 1, 1) == 0
    assert _dec_call(L.jpgx_jfif_decode_gpu_ex, W=60, wsb=1 << 20) == jpgx.EGEOMETRY
    assert _px_call(L.jpgx_pixels_gpu, W=60, H=64, cstride=3 * 64 * 64, pitch=184, ostride=184 * 64) == jpgx.EGEOMETRY


# ---- the device entry points refuse bad arguments before any device call ----------------------------------
def _dec_call(fn, files=0x10000, fstride=1 << 16, lens=0x20000, nf=1, W=60, H=64, sr=0, flags=0, coef=0x30000,
              cstride=3 * 64 * 64, qt=0x40000, status=0x50000, ws=0x60000, wsb=None):
    if wsb is None:
        wsb = L.jpgx_jfif_decode_gpu_any_workspace_size(W, H, sr, max(nf, 1), fstride, 0) or 1 << 20
    return fn(files, fstride, lens, nf, W, H, sr, flags, coef, cstride, qt, status, ws, wsb, None)


@pytest.mark.parametrize("flags", [0, SUB])
def test_decoder_refuses_bad_arguments_without_a_device(flags):
    def call(**kw):
        return _dec_call(L.jpgx_jfif_decode_gpu_any, flags=flags, **kw)
    E = jpgx.EARG
    for name in ("files", "lens", "coef", "status", "ws"):
        assert call(**{name: None}) == E, name
    assert call(lens=0x20004) == E and call(coef=0x30008) == E and call(status=0x50002) == E
    assert call(qt=0x40001) == E and call(ws=0x60008) == E
    assert call(nf=0) == E and call(nf=65536) == E
    assert call(fstride=0) == E and call(fstride=1 << 32) == E
    assert call(sr=3) == E and call(sr=-1) == E
    for side in (0, 65536, -8):
        assert call(W=side) == E and call(H=side) == E
    # the coded frame of 60 x 64 is 64 x 64 (4:4:4), of 50 x 33 in 4:2:0 it is 64 x 48: 48 + 2 * 12 blocks
    assert call(cstride=3 * 64 * 64 + 32) == E and call(cstride=3 * 64 * 64 - 64) == E
    assert call(W=50, H=33, sr=2, cstride=72 * 64 - 64) == E
    assert call(W=57, cstride=3 * 64 * 64 - 64) == E
    # the order is _ex's: EARG before EWORKSPACE; EGEOMETRY does not occur
    assert call(cstride=32, wsb=1) == E and call(wsb=1) == jpgx.EWORKSPACE
    for W, H, sr, nblk in ((60, 64, 0, 3 * 64), (50, 33, 2, 72), (49, 41, 1, 96), (1, 1, 2, 6), (65535, 1, 0, 3 * 8192)):
        for f in (0, SUB):
            want = L.jpgx_jfif_decode_gpu_any_workspace_size(W, H, sr, 2, 4097, f)
            assert want > 0 and want % 16 == 0
            assert _dec_call(L.jpgx_jfif_decode_gpu_any, W=W, H=H, sr=sr, nf=2, fstride=4097, cstride=nblk * 64,
                             flags=f, wsb=want - 1) == jpgx.EWORKSPACE


def test_decoder_flags_and_size_query():
    size = L.jpgx_jfif_decode_gpu_any_workspace_size
    for unknown in (2, 3, 4, 1 << 31):
        assert _dec_call(L.jpgx_jfif_decode_gpu_any, flags=unknown) == jpgx.EARG
        assert _dec_call(L.jpgx_jfif_decode_gpu_any, flags=unknown, W=0) == jpgx.EARG
        assert size(60, 64, 0, 1, 1 << 16, unknown) == 0
    for bad in (dict(nf=0), dict(nf=65536), dict(sr=3), dict(W=0), dict(H=65536), dict(cap=0), dict(cap=1 << 32)):
        a = dict(W=60, H=64, sr=0, nf=1, cap=1 << 16)
        a.update(bad)
        for flags in (0, SUB):
            assert size(a["W"], a["H"], a["sr"], a["nf"], a["cap"], flags) == 0, bad


def _px_call(fn, coef=0x10000, cstride=3 * 6 * 64, nf=1, W=17, H=15, sr=0, qt=0x20000, qstride=0, status=None,
             rgb=0x30000, pitch=56, ostride=56 * 15, ws=None, wsb=0):
    return fn(coef, cstride, nf, W, H, sr, qt, qstride, status, rgb, pitch, ostride, ws, wsb, None)


def test_pixels_refuse_bad_arguments_without_a_device():
    def call(**kw):
        return _px_call(L.jpgx_pixels_gpu_any, **kw)
    E = jpgx.EARG
    assert call(coef=None) == E and call(qt=None) == E and call(rgb=None) == E
    assert call(coef=0x10008) == E and call(qt=0x20001) == E and call(status=0x40002) == E and call(rgb=0x30004) == E
    assert call(nf=0) == E and call(nf=65536) == E
    # 17 x 15 codes 3 x 2 blocks (4:4:4); 4:2:x code 32 x 16: 8 + 2 * 4 and 8 + 2 * 2 blocks
    assert call(cstride=3 * 6 * 64 - 64) == E and call(cstride=3 * 6 * 64 + 32) == E
    assert call(qstride=1) == E and call(qstride=127) == E
    assert call(pitch=50) == E and call(pitch=48) == E and call(pitch=52, ostride=52 * 15) == E     # 3 W = 51
    assert call(ostride=56 * 15 - 8) == E and call(pitch=64, ostride=64 * 15 + 4) == E
    assert call(sr=3) == jpgx.ESAMPLE and call(sr=-1) == jpgx.ESAMPLE
    # a side outside 1 .. 65535 has the sibling's code; before it, the sibling's EARGs
    for side in (0, 65536):
        assert call(W=side) == jpgx.EGEOMETRY and call(H=side) == jpgx.EGEOMETRY
        assert call(W=side, nf=0) == E and call(W=side, sr=3) == jpgx.ESAMPLE
        assert L.jpgx_pixels_gpu_any_workspace_size(side, 15, 1, 1) == 0
    for sr, per, need in ((1, 8 + 8, 2 * 4 * 64), (2, 8 + 4, 2 * 2 * 64)):
        assert L.jpgx_pixels_gpu_any_workspace_size(17, 15, sr, 1) == need
        assert L.jpgx_pixels_gpu_any_workspace_size(17, 15, sr, 5) == 5 * need
        assert call(sr=sr, cstride=per * 64, ws=0x50000, wsb=need - 1) == jpgx.EWORKSPACE
        assert call(sr=sr, cstride=per * 64, ws=None, wsb=need) == E
        assert call(sr=sr, cstride=per * 64, ws=0x50008, wsb=need) == E
        assert call(sr=sr, cstride=per * 64 - 64, ws=0x50000, wsb=need) == E
    assert L.jpgx_pixels_gpu_any_workspace_size(17, 15, 0, 1) == 0
    for bad in ((17, 15, 3, 1), (17, 15, 1, 0), (17, 15, 1, 65536)):
        assert L.jpgx_pixels_gpu_any_workspace_size(*bad) == 0


def test_exports_and_bindings():
    for name in ("jpgx_coded_size", "jpgx_jfif_decode_gpu_any_workspace_size", "jpgx_jfif_decode_gpu_any",
                 "jpgx_pixels_gpu_any_workspace_size", "jpgx_pixels_gpu_any"):
        assert name in jpgx.EXPORTS and hasattr(L, name) and hasattr(jpgx.alt_library(), name)
    for name in ("jpgx_jfif_info_of_any", "jpgx_read_jfif_any", "jpgx_read_jfif_sub_any", "jpgx_pixels_host_any"):
        assert name in jpgx.COMPAT_EXPORTS and hasattr(L, name) and hasattr(jpgx.alt_library(), name)
    torch = pytest.importorskip("torch")
    files, lens = torch.zeros((1, 4096), dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError):
        jpgx.jfif_decode_gpu(files, lens, 60, 64, any_size=True)     # host tensors
    with pytest.raises(ValueError):
        jpgx.decode_jpeg(A.project_files(0)[0][3], "cpu", any_size=True)
    with pytest.raises(ValueError):
        jpgx.pixels_gpu(torch.zeros((1, 64), dtype=torch.int16), 0, 8, any_size=True)


# ---- the host routines under the sanitizers ----------------------------------------------------------------
@pytest.mark.skipif(not A.san_build.HAVE_CC, reason="needs gcc and g++")
def test_host_routines_under_asan_ubsan():
    rc, out, err = A.run_san()
    assert rc == 0 and out.rstrip().endswith("any_san: clean"), (out[-2000:], err[-4000:])
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-4000:]
    counts = [ln.split() for ln in out.splitlines() if ln.startswith("cases ")][0]
    cases, ok, header, scan = (int(counts[k]) for k in (1, 3, 5, 7))
    # 2 * (64 + 128 + 256) sizes, decoded twice and once refused; two files' truncations and corruptions
    assert ok >= 2 * 2 * 448 and header >= 2 * 448 and scan >= 1000 and cases >= 8000
