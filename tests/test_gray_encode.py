"""The encode side of the one-component family on the host: the helper's oracle pinned
to the pinned oracle, k_gray's restatement on the host (csrc/jx_gray.h: arithmetic, guard band, exact pass,
load rule) against it, the host writer jpgx_write_jfif_gray against the host reader, an independent
decoder and Pillow, the refusals, the exports and the sanitizer program tests/c/gray_enc_san.c.
Every comparison is ==."""
import ctypes

import numpy as np
import pytest

import gray_cases
import gray_enc_cases as G
import jfif_decode_gray as D
import jpgx
import jpgx.compat as C
import oracle
import san_build
from conftest import PKG

L = jpgx.lib


# ---- 1. the oracle ------------------------------------------------------------------------------------------
def test_helper_pipeline_is_the_pinned_oracle_s():
    """tiling, transposition and zig-zag of the helper, pinned once: the reference's double Y samples in its
    own operation order through the helper's per-block pipeline are oracle.blocks' Y on every block that
    is not the last of its block row (those carry the reference's x0 = -8 quirk)"""
    W, H = 40, 24
    rgb = oracle.gen_splitmix(77, W, H)
    R, Gc, B = (rgb[:, :, k].astype(np.float64) for k in range(3))
    y = 0.299 * R + 0.587 * Gc + 0.114 * B - 128
    for q in G.QUALITIES:
        mine, ref = G.coefficients(y, q), oracle.blocks(rgb, q)[0]
        keep = np.arange(len(ref)) % (W // 8) != W // 8 - 1
        assert keep.sum() == (W // 8 - 1) * (H // 8) and np.array_equal(mine[keep], ref[keep]), q


def test_flat_blocks_tie_in_dc_and_round_toward_zero():
    """q 50, flat g: the real DC is 8 (g - 128) / 16, a tie for all 128 odd g; the reference's doubles fall
    off it toward zero"""
    flat = G.blocks_of(G.flat())
    assert np.array_equal(G.exact_ties(flat, 50)[:, 3], np.arange(256) % 2 == 1)
    dc = G.gray_oracle(G.flat(), 50)[:, 0].astype(int)
    assert dc[1] == -63 and dc[253] == 62
    odd = np.arange(1, 256, 2)
    assert np.array_equal(dc[odd], np.trunc((odd - 128) / 2.0).astype(int))


def test_tie_selection():
    t = G.exact_ties(G.ties4(), G.TIE_QUALITY)[:, :3]
    assert len(G.ties4()) == G.TIE_COUNT and t.any(axis=1).all() and (t.sum(axis=0) >= 32).all(), t.sum(axis=0)


def test_luminance_never_reaches_the_coder_s_clamps():
    """q 97, every divisor 1: the basis functions' sign patterns give the largest |AC|, 1020 < 1023; DC spans
    8 (0 - 128) .. 8 (255 - 128), so the largest |DC difference| is 2040 < 2047"""
    o = G.gray_oracle(G.extremes(), 97).astype(int)
    assert np.abs(o[:, 1:]).max() == 1020 and (o[:, 0].min(), o[:, 0].max()) == (-1024, 1016)
    assert np.abs(o[:, 0][:, None] - o[:, 0][None, :]).max() == 2040


# ---- 2. k_gray on the host ----------------------------------------------------------------------------------
def _inputs():
    for W, H in G.SIZES:
        yield "noise %dx%d" % (W, H), G.noise(W, H), G.QUALITIES
        yield "ramp %dx%d" % (W, H), G.ramp(W, H), G.QUALITIES
    yield "flat", G.flat(), G.QUALITIES
    yield "extremes", G.extremes(), (97,)
    yield "ties", G.ties4_image(), (90,)


def test_host_restatement_is_the_oracle():
    for name, img, qs in _inputs():
        for q in qs:
            want = G.gray_oracle(img, q)
            assert np.array_equal(G.host_blocks(img, q), want), (name, q)
            assert np.array_equal(G.host_blocks(img, q, force=True), want), (name, q, "force")


def test_guard_band():
    for q in (1, 23, 50, 90, 97):
        w, lim = jpgx.guard_band_gray(q)
        assert w.shape == lim.shape == (64,) and (lim > 0).all() and (lim < 0.5).all() and (w != 0).all(), q
        wc, _ = jpgx.guard_band(q)
        assert np.array_equal(w, wc[0]), q                    # the luminance scales of the colour path
    buf = (ctypes.c_float * 64)()
    assert L.jpgx_guard_band_gray(0, buf, buf) == jpgx.EQUALITY and L.jpgx_guard_band_gray(98, buf, buf) == jpgx.EQUALITY
    assert L.jpgx_guard_band_gray(50, None, buf) == jpgx.EARG


def test_band_self_test():
    """the kernel's fp32 sequence on the host: no unflagged coefficient differs from the exact value, and
    every exact tie is flagged"""
    fn = L.jx_selftest_gray
    fn.argtypes = [ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]
    fn.restype = ctypes.c_longlong
    sets = (("flat", G.blocks_of(G.flat())), ("ties", G.ties4()), ("noise", G.blocks_of(G.noise(2056, 8))))
    for q in G.QUALITIES:
        flagged = ctypes.c_longlong()
        assert fn(4000, 0x6772 + q, q, ctypes.byref(flagged)) == 0, q
        assert 0 < flagged.value < 4000 * 64 // 8, (q, flagged.value)
        for name, blocks in sets:
            bad, nfl, flags = G.selftest_blocks(blocks, q)
            assert bad == 0 and nfl == flags.sum(), (name, q, bad)
            ties = G.exact_ties(blocks, q)
            for k, (u, v) in enumerate(G.TIE_COEFS + ((0, 0),)):
                assert flags[ties[:, k], v, u].all(), (name, q, u, v)
    assert G.exact_ties(G.ties4(), 90)[:, :3].sum() >= 96 and G.exact_ties(G.blocks_of(G.flat()), 50)[:, 3].sum() == 128
    assert fn(1, 1, 0, None) == -1


def test_load_rule_stays_inside_the_image():
    """jx_gray_load_block lane by lane with every load checked: only bytes [0, W) of rows 0 .. H - 1 are
    touched, wide loads are aligned, and the assembled blocks are the edge frame"""
    fn = L.jx_gray_load_trace
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_size_t,
                   ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_longlong
    rng = np.random.default_rng(5)
    kinds = set()
    for W in (1, 7, 8, 9, 21, 65):
        for H in (1, 7, 8, 9, 21, 65):
            for pitch in (W, W + 1, W + 13, (W + 7) // 8 * 8, (W + 3) // 4 * 4 + 4):
                for off in range(4):
                    n = off + pitch * (H - 1) + W
                    raw = np.zeros(n + 64 + 8, np.uint8)                  # the frame ends with its last pixel,
                    base = -raw.ctypes.data % 8                            # from an 8-byte aligned address + off
                    buf = raw[base:base + n]
                    buf[:] = rng.integers(0, 256, n, dtype=np.uint8)
                    touched = np.zeros(n, np.uint8)
                    blocks = np.zeros((G.nblocks(W, H), 64), np.uint8)
                    assert fn(buf.ctypes.data, n, off, W, H, pitch, touched.ctypes.data, blocks.ctypes.data) == 0, \
                        (W, H, pitch, off)
                    img = np.lib.stride_tricks.as_strided(buf[off:], (H, W), (pitch, 1))
                    allowed = np.zeros(n, bool)
                    for r in range(H):
                        allowed[off + r * pitch:off + r * pitch + W] = True
                    assert not touched[~allowed].any(), (W, H, pitch, off)
                    assert touched[allowed].all(), (W, H, pitch, off)         # and every pixel is read
                    assert np.array_equal(blocks.reshape(-1, 8, 8), G.blocks_of(G.edge_frame(img))), (W, H, pitch, off)
                    kinds |= set(np.unique(touched).tolist())
    assert {1, 2, 4} <= kinds                                           # bytes, 4-byte and 8-byte loads all ran


# ---- 3. the host writer -------------------------------------------------------------------------------------
def _segments(data):
    """[(marker, payload)] up to and including SOS"""
    assert data[:2] == b"\xff\xd8"
    out, i = [], 2
    while True:
        assert data[i] == 0xFF
        m, ln = data[i + 1], data[i + 2] << 8 | data[i + 3]
        out.append((m, data[i + 4:i + 2 + ln]))
        i += 2 + ln
        if m == 0xDA:
            return out


def _cases():
    k = 0
    for W, H in G.SIZES:
        for rr in (0, 1, 2, -1):
            for opt in (False, True):
                q = G.QUALITIES[k % 3] if k % 7 else 20             # q 20: a 16-bit table, SOF1
                img = G.noise(W, H) if k % 2 else G.ramp(W, H)
                k += 1
                yield W, H, rr, opt, q, G.gray_oracle(img, q if q != 20 else 50)


def test_writer_round_trip_and_structure():
    for W, H, rr, opt, q, coef in _cases():
        bw, bh = -(-W // 8), -(-H // 8)
        data = C.write_jfif_gray(coef, W, H, q, rr, nthreads=1, optimize=opt)
        what = (W, H, rr, opt, q)
        r = C.read_jfif_gray(data)
        assert np.array_equal(r["coef"], coef) and np.array_equal(r["qt"], jpgx.jfif_qt(q)[0]), what
        assert (r["width"], r["height"]) == (W, H), what
        rows = rr if rr >= 0 else -(-bh // 4)                        # auto at one thread: 4 intervals
        assert r["restart_interval"] == rows * bw, what
        if rr >= 0:
            assert C.write_jfif_gray(coef, W, H, q, rr, nthreads=3, optimize=opt) == data, what
        d = D.decode(data)
        assert (d["width"], d["height"], d["sampling"]) == (W, H, (1, 1)), what
        assert np.array_equal(d["coef"], coef) and list(d["qt"]) == list(jpgx.jfif_qt(q)[0]), what
        assert d["restart_interval"] == rows * bw and d["restarts"] == (-(-bh // rows) - 1 if rows else 0), what
        seg = _segments(data)
        kinds = [m for m, _ in seg]
        assert kinds == [0xE0, 0xDB, 0xC1 if q == 20 else 0xC0, 0xC4, 0xC4] + ([0xDD] if rows else []) + [0xDA], what
        by = dict((m, p) for m, p in seg if m != 0xC4)
        assert by[0xDB][0] == (0x10 if q == 20 else 0x00) and len(by[0xDB]) == (129 if q == 20 else 65), what
        sof = by[0xC1 if q == 20 else 0xC0]
        assert sof[5] == 1 and tuple(sof[6:9]) == (1, 0x11, 0) and len(sof) == 9, what
        assert [p[0] for m, p in seg if m == 0xC4] == [0x00, 0x10], what
        assert bytes(by[0xDA]) == bytes([1, 1, 0x00, 0, 63, 0]), what
        assert data[-2:] == b"\xff\xd9" and len(data) <= C.lib.jpgx_jfif_bound(8 * bw, 8 * bh), what
        if opt:
            assert len(data) <= len(C.write_jfif_gray(coef, W, H, q, rr, nthreads=1)), what
        else:                                                        # the colour writer's APP0 and K.3 tables
            colour = C.write_jfif_ex(np.zeros((3, 1, 64), np.int16), 8, 8, 50, restart_rows=0, nthreads=1)
            cseg = _segments(colour)
            assert cseg[0] == seg[0] and [p for m, p in cseg if m == 0xC4][:2] == [p for m, p in seg if m == 0xC4], what


def test_a_restart_interval_must_fit_dri():
    W, H = 2056, 8 * 40
    coef = np.zeros((G.nblocks(W, H), 64), np.int16)
    assert len(C.write_jfif_gray(coef, W, H, 50, 65535 // 257)) > 0
    with pytest.raises(jpgx.JpgxError) as e:
        C.write_jfif_gray(coef, W, H, 50, 65535 // 257 + 1)
    assert e.value.rc == jpgx.EARG


@pytest.mark.skipif(not gray_cases.have_pillow(), reason="needs Pillow")
def test_pillow_opens_every_file():
    skipped = total = 0
    for W, H, rr, opt, q, coef in _cases():
        data = C.write_jfif_gray(coef, W, H, q, rr, optimize=opt)
        px = gray_cases.pillow_pixels(data)                          # asserts mode L
        assert px.shape == (H, W)
        total += 1
        r = {"coef": coef, "qt": jpgx.jfif_qt(q)[0]}
        if not gray_cases.fits_16_bits(r):
            skipped += 1
            continue
        assert np.array_equal(px, C.pixels_host_gray(coef, W, H, r["qt"], 1)), (W, H, rr, opt, q)
    assert skipped * 8 <= total, (skipped, total)


def _rc(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except jpgx.JpgxError as e:
        return e.rc
    return 0


def test_writer_refusals():
    coef = np.zeros((4, 64), np.int16)
    w = lambda *a, **kw: _rc(C.write_jfif_gray, coef, *a, **kw)    # noqa: E731
    assert w(12, 9, 50) == 0
    assert w(0, 9, 50) == jpgx.EARG and w(12, 65536, 50) == jpgx.EARG and w(-1, 9, 50) == jpgx.EARG
    assert w(12, 9, 0) == jpgx.EQUALITY and w(12, 9, 98) == jpgx.EQUALITY
    assert w(12, 9, 50, -2) == jpgx.EARG and w(12, 9, 50, 0, nthreads=-1) == jpgx.EARG
    n = ctypes.c_size_t()
    buf = np.zeros(4096, np.uint8)
    call = lambda c, flags, out, cap: L.jpgx_write_jfif_gray(c, 12, 9, 50, 0, 1, flags, out, cap, ctypes.byref(n))  # noqa: E731
    assert call(coef.ctypes.data, 0, buf.ctypes.data, 4096) == 0 and n.value > 0
    need = n.value
    assert call(coef.ctypes.data, 2, buf.ctypes.data, 4096) == jpgx.EARG
    assert call(None, 0, buf.ctypes.data, 4096) == jpgx.EARG and call(coef.ctypes.data, 0, None, 4096) == jpgx.EARG
    assert call(coef.ctypes.data, 0, buf.ctypes.data, need - 1) == jpgx.EARG and n.value == need
    with pytest.raises(ValueError):
        C.write_jfif_gray(coef[:3], 12, 9, 50)


def test_exports_and_bindings():
    for name in ("jpgx_blocks_gpu_gray", "jpgx_jfif_gpu_gray_workspace_size", "jpgx_jfif_gpu_gray",
                 "jpgx_guard_band_gray"):
        assert name in jpgx.EXPORTS and hasattr(L, name) and hasattr(jpgx.alt_library(), name)
    assert "jpgx_write_jfif_gray" in jpgx.COMPAT_EXPORTS and hasattr(L, "jpgx_write_jfif_gray")
    size = L.jpgx_jfif_gpu_gray_workspace_size
    assert size(21, 13, -1, 2, 4096, 0) > 0 and size(21, 13, 1, 2, 4096, 1) > size(21, 13, 1, 2, 4096, 0)
    assert size(21, 13, 0, 2, 4096, 0) == 0 and size(21, 13, 1, 2, 4096, 2) == 0 and size(0, 13, 1, 2, 4096, 0) == 0
    assert size(2056, 8, 65535 // 257 + 1, 1, 4096, 0) == 0 and size(21, 13, 1, 0, 4096, 0) == 0
    # the forward path's refusals come before any device call: quality, geometry, then the arguments
    fwd = lambda *a: L.jpgx_blocks_gpu_gray(*a)                    # noqa: E731
    p, o = 0x1000, 0x2000                                          # never dereferenced: every call is refused
    assert fwd(p, 8, 64, 1, 8, 8, 0, 0, o, 64, None) == jpgx.EQUALITY
    assert fwd(p, 8, 64, 1, 8, 8, 98, 0, o, 64, None) == jpgx.EQUALITY
    assert fwd(None, 8, 64, 1, 0, 8, 98, 0, o, 64, None) == jpgx.EQUALITY
    assert fwd(p, 8, 64, 1, 0, 8, 50, 0, o, 64, None) == jpgx.EGEOMETRY
    assert fwd(None, 8, 64, 1, 8, 65536, 50, 0, o, 64, None) == jpgx.EGEOMETRY
    assert fwd(None, 8, 64, 1, 8, 8, 50, 0, o, 64, None) == jpgx.EARG
    assert fwd(p, 8, 64, 1, 8, 8, 50, 0, None, 64, None) == jpgx.EARG
    assert fwd(p, 8, 64, 1, 8, 8, 50, 2, o, 64, None) == jpgx.EARG
    assert fwd(p, 7, 64, 1, 8, 8, 50, 0, o, 64, None) == jpgx.EARG
    assert fwd(p, 8, 64, 0, 8, 8, 50, 0, o, 64, None) == jpgx.EARG
    assert fwd(p, 8, 64, 65536, 8, 8, 50, 0, o, 64, None) == jpgx.EARG
    assert fwd(p, 8, 64, 1, 8, 8, 50, 0, o + 8, 64, None) == jpgx.EARG
    assert fwd(p, 8, 64, 1, 8, 8, 50, 0, o, 63, None) == jpgx.EARG
    assert fwd(p, 8, 64, 1, 9, 8, 50, 0, o, 64, None) == jpgx.EARG          # two blocks need 128


def test_python_refuses_host_tensors():
    torch = pytest.importorskip("torch")
    host = torch.zeros((15, 17), dtype=torch.uint8)
    with pytest.raises(ValueError):
        jpgx.encode_blocks_gray(host, 50)
    with pytest.raises(ValueError):
        jpgx.encode_jpeg(host, 50, gray=True)
    with pytest.raises(ValueError):
        jpgx.jfif_gpu_gray(torch.zeros((1, 6, 64), dtype=torch.int16), 17, 15, 50)


# ---- the host routines under the sanitizers ----------------------------------------------------------------
@pytest.mark.skipif(not san_build.HAVE_CC, reason="needs gcc and g++")
def test_host_routines_under_asan_ubsan():
    import os
    libs = san_build.HOST_LAYER + [os.path.join(PKG, "csrc", "jpgx_jfif_read.cpp")]
    rc, out, err = san_build.run("gray_enc_san", libs, timeout=900)
    assert rc == 0 and out.rstrip().endswith("gray_enc_san: clean"), (out[-2000:], err[-4000:])
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-4000:]
    counts = [ln.split() for ln in out.splitlines() if ln.startswith("sizes ")][0]
    sizes, files = int(counts[1]), int(counts[3])
    assert sizes >= 40 * 40 + len(G.SIZES) and files == 2 * sizes       # every size, both flag values
