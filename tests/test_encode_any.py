"""Images of any width and height on the way to a file, on the host: jpgx_write_jfif_any
against the existing writer's file for the coded size with the SOF patched, the readers and Pillow on its
files, jpgx_pad_edge against numpy's edge padding, the refusals of every new entry point (no device is
touched), the exports, the Python argument checks and the sanitizer program tests/c/encode_any_san.c.
Every comparison is ==."""
import ctypes
import io

import numpy as np
import pytest

import any_cases as A
import encode_any_cases as E
import jpgx
import jpgx.compat as C
import pixels_cases as P

L = jpgx.lib
pillow = pytest.mark.skipif(not E.have_pillow(), reason="needs Pillow")
CPU_SIZES = ((1, 1), (17, 15), (33, 16), (30, 22), (263, 21), (667, 9))


def _rc(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except jpgx.JpgxError as e:
        return e.rc
    return 0


# ---- the file ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [0, 1, 2])
@pytest.mark.parametrize("W,H", CPU_SIZES)
def test_file_is_the_coded_size_s_with_the_sof_patched(W, H, sr):
    cw, ch = E.coded(W, H, sr)
    assert jpgx.coded_size(W, H, sr) == (cw, ch)
    for q in E.QUALITIES:
        coef = P.oracle_coef("splitmix", cw, ch, q, sr)
        for rr in (0, 1, 2):
            for opt in (False, True):
                got = C.write_jfif_ex(coef, W, H, q, sr, restart_rows=rr, nthreads=1, optimize=opt, any_size=True)
                whole = C.write_jfif_ex(coef, cw, ch, q, sr, restart_rows=rr, nthreads=1, optimize=opt)
                assert got == A.patch_size(whole, W, H), (q, rr, opt)
                assert len(got) <= L.jpgx_jfif_bound(cw, ch)
                r = C.read_jfif(got, 1, any_size=True)
                assert (r["width"], r["height"], r["sample_ratio"]) == (W, H, sr)
                assert np.array_equal(r["coef"].reshape(-1, 64), coef)          # inside the writers' clamps
                # the restart interval counts MCUs of the coded frame
                assert r["restart_interval"] == rr * (cw // (16 if sr else 8))
        # the thread count does not show
        assert C.write_jfif_ex(coef, W, H, 90, sr, restart_rows=1, nthreads=3, any_size=True) == \
            C.write_jfif_ex(coef, W, H, 90, sr, restart_rows=1, nthreads=1, any_size=True)


@pytest.mark.parametrize("sr", [0, 1, 2])
def test_mcu_multiples_equal_the_plain_writer(sr):
    for W, H in E.BOTH[1 if sr else 0:] + ((64, 48),):
        coef = P.oracle_coef("splitmix", W, H, 50, sr)
        for rr, opt in ((0, False), (1, True), (-1, False)):
            assert C.write_jfif_ex(coef, W, H, 50, sr, restart_rows=rr, nthreads=2, optimize=opt, any_size=True) == \
                C.write_jfif_ex(coef, W, H, 50, sr, restart_rows=rr, nthreads=2, optimize=opt)
    # and the plain writer still refuses what it refused
    coef = np.zeros((3 * 6, 64), np.int16)
    assert _rc(C.write_jfif_ex, coef, 17, 15, 50, 0) == jpgx.EARG
    assert _rc(C.write_jfif_ex, coef, 24, 8, 50, 1) == jpgx.EGEOMETRY


@pillow
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_pillow_opens_the_file_as_w_x_h(sr):
    from PIL import Image
    for W, H in CPU_SIZES:
        for kind, q, opt in (("smooth", 90, False), ("splitmix", 50, True)):
            coef = E.oracle_coef(kind, W, H, q, sr)
            data = C.write_jfif_ex(coef, W, H, q, sr, restart_rows=1, nthreads=1, optimize=opt, any_size=True)
            im = Image.open(io.BytesIO(data))
            assert im.size == (W, H)
            r = C.read_jfif(data, 1, any_size=True)
            assert A.fits_16_bits(r)                     # a condition of the comparison, not a tolerance
            want = C.pixels_host(r["coef"], W, H, sr, r["qt"], 2, any_size=True)
            assert want.shape == (H, W, 3)
            assert np.array_equal(np.asarray(im.convert("RGB")), want), (W, H, kind)


# ---- the edge rule on the host -----------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_pad_edge_is_numpy_s(sr):
    rng = np.random.default_rng(5 + sr)
    for W, H in E.SIZES + E.BOTH:
        big = rng.integers(0, 256, (H + 1, W + 3, 3), dtype=np.uint8)
        for rgb in (big[:H, :W], np.ascontiguousarray(big[:H, :W])):       # a pitch of 3 W + 9, and 3 W
            got = jpgx.pad_edge(rgb, sr)
            assert got.shape == E.coded(W, H, sr)[::-1] + (3,)
            assert np.array_equal(got, E.pad_edge(rgb, sr))
    # exactly the coded frame's bytes are written
    rgb = rng.integers(0, 256, (5, 3, 3), dtype=np.uint8)
    out = np.full(8 * 8 * 3 + 16, 0x7A, np.uint8)
    assert L.jpgx_pad_edge(rgb.ctypes.data, 3, 5, 9, 8, 8, out.ctypes.data) == 0
    assert np.array_equal(out[:192].reshape(8, 8, 3), E.pad_edge(rgb, 0)) and (out[192:] == 0x7A).all()
    E_, G = jpgx.EARG, jpgx.EGEOMETRY
    assert L.jpgx_pad_edge(None, 3, 5, 9, 8, 8, out.ctypes.data) == E_
    assert L.jpgx_pad_edge(rgb.ctypes.data, 3, 5, 9, 8, 8, None) == E_
    assert L.jpgx_pad_edge(rgb.ctypes.data, 3, 5, 8, 8, 8, out.ctypes.data) == E_
    assert L.jpgx_pad_edge(rgb.ctypes.data, 0, 5, 9, 8, 8, out.ctypes.data) == G
    assert L.jpgx_pad_edge(rgb.ctypes.data, 3, 5, 9, 2, 8, out.ctypes.data) == G
    with pytest.raises(ValueError):
        jpgx.pad_edge(rgb[:, :, ::-1], 0)
    # numpy images take the padded, plain route: the argument checks are the coded frame's
    with pytest.raises(ValueError):
        jpgx.encode_blocks(np.zeros((5, 3, 3), np.uint8), 50, 3, any_size=True)


# ---- refusals, all before any device call --------------------------------------------------------------------
def _fwd(W=17, H=15, sr=0, q=50, flags=0, rows=None, nf=1, pitch=None, fstride=None, ostride=None, rgb=0x10001,
         out=0x20000, ws=0x30000, wsb=None, fr_null=False, p_null=False, size_only=False):
    cw, ch = E.coded(W, H, sr) if sr in (0, 1, 2) else (W, H)
    fr = jpgx.Frames()
    fr.width, fr.height, fr.nframes = W, H, nf
    fr.row_begin, fr.row_end = rows if rows is not None else (0, ch // 8)
    fr.in_pitch = 3 * W + 5 if pitch is None else pitch
    fr.in_frame_stride = fr.in_pitch * max(H, 1) + 3 if fstride is None else fstride
    fr.out_frame_stride = 3 * (cw // 8) * (ch // 8) * 64 if ostride is None else ostride
    p = jpgx.Params()
    p.quality, p.sample_ratio, p.flags = q, sr, flags
    frp, pp = (None if fr_null else ctypes.byref(fr)), (None if p_null else ctypes.byref(p))
    need = L.jpgx_workspace_size_any(frp, pp)
    if size_only:
        return need
    return L.jpgx_blocks_gpu_any(frp, pp, rgb, out, ws, need if wsb is None else wsb, None)


def test_forward_path_refuses_bad_arguments_without_a_device():
    E_, S, Q, G, WS = jpgx.EARG, jpgx.ESAMPLE, jpgx.EQUALITY, jpgx.EGEOMETRY, jpgx.EWORKSPACE
    assert _fwd(sr=3) == S and _fwd(sr=-1) == S and _fwd(sr=3, size_only=True) == 0
    assert _fwd(q=0) == Q and _fwd(q=98) == Q and _fwd(q=0, size_only=True) == 0 and _fwd(q=98, size_only=True) == 0
    for side in (0, 65536, -8):
        assert _fwd(W=side) == G and _fwd(H=side) == G
        assert _fwd(W=side, size_only=True) == 0 and _fwd(H=side, size_only=True) == 0
    assert _fwd(sr=3, q=0, W=0) == S and _fwd(q=0, W=0) == Q             # the order of jpgx_validate
    assert _fwd(fr_null=True) == E_ and _fwd(p_null=True) == E_
    assert _fwd(fr_null=True, size_only=True) == 0 and _fwd(p_null=True, size_only=True) == 0
    assert _fwd(rgb=None) == E_ and _fwd(out=None) == E_ and _fwd(ws=None) == E_
    # whole frames only: 17 x 15 codes 24 x 16, two block rows
    for rows in ((0, 1), (1, 2), (0, 3), (0, 0), (-1, 2)):
        assert _fwd(rows=rows) == E_ and _fwd(rows=rows, size_only=True) == 0
    assert _fwd(sr=2, H=17, rows=(0, 2)) == E_ and _fwd(sr=2, H=17, rows=(0, 3)) == E_   # 32 x 32: four
    assert _fwd(nf=0) == E_ and _fwd(nf=-1) == E_
    # 3 W = 51: no multiple-of-8 rule, so the next check is the one that refuses
    assert _fwd(pitch=50) == E_ and _fwd(pitch=51, fstride=51 * 15, wsb=0) == WS
    assert _fwd(nf=2, fstride=14 * 56 + 50) == E_ and _fwd(nf=2, fstride=14 * 56 + 51, wsb=0) == WS
    # the output follows the plain entry point's rules
    assert _fwd(out=0x20008) == E_ and _fwd(ostride=18 * 64 + 4) == E_ and _fwd(nf=2, ostride=18 * 64 - 8) == E_
    # the workspace: the padded batch (plus the plain path's, which is nothing), 16-byte aligned
    for W, H, sr, nf in ((17, 15, 0, 1), (17, 15, 2, 3), (1, 1, 1, 2), (3839, 2159, 0, 8), (65535, 3, 2, 1)):
        cw, ch = E.coded(W, H, sr)
        cfr = jpgx.frames(cw, ch, nf)
        want = (nf * ch * 3 * cw + 15) // 16 * 16 + L.jpgx_workspace_size(ctypes.byref(cfr))
        assert _fwd(W=W, H=H, sr=sr, nf=nf, size_only=True) == want > 0
    assert _fwd(wsb=24 * 16 * 3 - 1) == WS and _fwd(ws=0x30008) == WS and _fwd(wsb=0) == WS
    # flags do not change the coded size: it is sample_ratio's
    assert _fwd(sr=1, size_only=True) == _fwd(sr=1, flags=jpgx.FLAG_SUBSAMPLE, size_only=True) == 32 * 16 * 3
    assert _fwd(sr=0, flags=jpgx.FLAG_SUBSAMPLE) == S                              # as the plain entry point


def test_plain_forward_path_still_refuses():
    p = jpgx.default_params(17, 15, 50)
    assert jpgx.validate(17, 15, p) == jpgx.EGEOMETRY
    fr = jpgx.frames(16, 16)
    fr.width = 17
    assert L.jpgx_blocks_gpu(ctypes.byref(fr), ctypes.byref(p), 0x10000, 0x20000, None, 0, None) == jpgx.EGEOMETRY


def _jf(fn=None, coef=0x10000, cstride=3 * 6 * 64, nf=1, W=17, H=15, q=50, sr=0, rr=1, flags=0, out=0x20000,
        ostride=1 << 16, cap=1 << 16, lens=0x30000, ws=0x40000, wsb=None):
    if wsb is None:
        wsb = L.jpgx_jfif_gpu_any_workspace_size(W, H, sr, rr, max(nf, 1), cap, flags) or 1 << 20
    return (fn or L.jpgx_jfif_gpu_any)(coef, cstride, nf, W, H, q, sr, rr, flags, out, ostride, cap, lens, ws, wsb, None)


@pytest.mark.parametrize("flags", [0, jpgx.JFIF_OPTIMIZE])
def test_device_writer_refuses_bad_arguments_without_a_device(flags):
    def call(**kw):
        return _jf(flags=flags, **kw)
    E_ = jpgx.EARG
    size = L.jpgx_jfif_gpu_any_workspace_size
    for name in ("coef", "out", "lens", "ws"):
        assert call(**{name: None}) == E_, name
    assert call(coef=0x10008) == E_ and call(out=0x20008) == E_ and call(lens=0x30004) == E_ and call(ws=0x40008) == E_
    assert call(sr=3) == E_ and call(sr=-1) == E_ and size(17, 15, 3, 1, 1, 1 << 16, flags) == 0
    for side in (0, 65536, -8):
        assert call(W=side) == E_ and call(H=side) == E_
        assert size(side, 15, 0, 1, 1, 1 << 16, flags) == 0 and size(17, side, 0, 1, 1, 1 << 16, flags) == 0
    assert call(q=0) == jpgx.EQUALITY and call(q=98) == jpgx.EQUALITY
    assert call(rr=0) == E_ and call(rr=-2) == E_ and call(nf=0) == E_ and call(nf=65536) == E_
    # the coded frame of 17 x 15 is 24 x 16 (4:4:4: 18 blocks), 32 x 16 in 4:2:x (16 and 12 blocks)
    assert call(cstride=18 * 64 - 64) == E_ and call(cstride=18 * 64 + 32) == E_
    assert call(sr=1, cstride=16 * 64 - 64) == E_ and call(sr=2, cstride=12 * 64 - 64) == E_
    assert call(ostride=(1 << 16) - 1) == E_
    assert call(wsb=1) == jpgx.EWORKSPACE
    assert _jf(flags=2) == E_ and _jf(flags=flags | 2) == E_ and size(17, 15, 0, 1, 1, 1 << 16, 2) == 0
    # the workspace is the coded frame's; a multiple of the MCU equals the plain call's
    for W, H, sr in ((17, 15, 0), (17, 15, 1), (49, 33, 2), (1, 1, 2), (3839, 2159, 0)):
        cw, ch = E.coded(W, H, sr)
        assert size(W, H, sr, -1, 3, 40000, flags) == L.jpgx_jfif_gpu_workspace_size_ex(cw, ch, sr, -1, 3, 40000, flags) > 0
        assert size(cw, ch, sr, 2, 3, 40000, flags) == L.jpgx_jfif_gpu_workspace_size_ex(cw, ch, sr, 2, 3, 40000, flags)
    # the plain entry point still refuses the size
    assert _jf(L.jpgx_jfif_gpu_ex, flags=flags, wsb=1 << 20) == E_
    assert _jf(L.jpgx_jfif_gpu_ex, flags=flags, W=24, H=16, sr=1, cstride=12 * 64, wsb=1 << 20) == jpgx.EGEOMETRY
    assert L.jpgx_jfif_gpu_workspace_size_ex(17, 15, 0, 1, 1, 1 << 16, flags) == 0


def test_host_writer_refusals_and_the_size_needed():
    coef = P.oracle_coef("splitmix", 24, 16, 50, 0)
    n = ctypes.c_size_t()
    buf = np.empty(1 << 16, np.uint8)

    def call(coef=coef.ctypes.data, W=17, H=15, q=50, sr=0, rr=1, nt=1, flags=0, out=buf.ctypes.data, cap=buf.size):
        return L.jpgx_write_jfif_any(coef, W, H, q, sr, rr, nt, flags, out, cap, ctypes.byref(n))
    E_ = jpgx.EARG
    assert call() == 0
    full = n.value
    assert call(coef=None) == E_ and call(out=None) == E_
    assert call(sr=3) == E_ and call(sr=-1) == E_
    for side in (0, 65536, -8):
        assert call(W=side) == E_ and call(H=side) == E_
    assert call(q=0) == jpgx.EQUALITY and call(q=98) == jpgx.EQUALITY
    assert call(rr=-2) == E_ and call(nt=-1) == E_ and call(flags=2) == E_
    # a too-small buffer: JPGX_EARG and the size needed; nothing is written beyond cap
    for cap in (0, 10, 700, full - 1):
        buf[:] = 0x7A
        n.value = 0
        assert call(cap=cap) == E_ and n.value == full
        assert (buf[cap:] == 0x7A).all()
    assert call(cap=full) == 0 and n.value == full
    small = C.write_jfif_ex(coef, 17, 15, 50, 0, restart_rows=1, nthreads=1, cap=64, any_size=True)   # grown on demand
    assert len(small) == full
    with pytest.raises(ValueError):
        C.write_jfif_ex(coef[:17], 17, 15, 50, 0, any_size=True)     # 18 blocks are coded
    # the file-level entry point refuses before any work
    rgb = np.zeros((15, 17, 3), np.uint8)
    enc = L.jpgx_encode_rgb_to_jpeg_any
    path = b"/nonexistent-directory/x.jpg"
    assert enc(None, 17, 15, 51, path, 50, 0, 0, 0) == E_ and enc(rgb.ctypes.data, 17, 15, 51, None, 50, 0, 0, 0) == E_
    assert enc(rgb.ctypes.data, 17, 15, 51, path, 50, 3, 0, 0) == jpgx.ESAMPLE
    assert enc(rgb.ctypes.data, 17, 15, 51, path, 0, 0, 0, 0) == jpgx.EQUALITY
    assert enc(rgb.ctypes.data, 17, 15, 51, path, 98, 0, 0, 0) == jpgx.EQUALITY
    assert enc(rgb.ctypes.data, 0, 15, 51, path, 50, 0, 0, 0) == jpgx.EGEOMETRY
    assert enc(rgb.ctypes.data, 17, 65536, 51, path, 50, 0, 0, 0) == jpgx.EGEOMETRY
    assert enc(rgb.ctypes.data, 17, 15, 50, path, 50, 0, 0, 0) == E_
    assert _rc(C.encode_rgb_to_jpeg, rgb, "/nonexistent-directory/x.jpg", 50, 3, any_size=True) == jpgx.ESAMPLE


# ---- exports and bindings -------------------------------------------------------------------------------------
def test_exports_and_bindings():
    for name in ("jpgx_workspace_size_any", "jpgx_blocks_gpu_any", "jpgx_jfif_gpu_any_workspace_size",
                 "jpgx_jfif_gpu_any"):
        assert name in jpgx.EXPORTS and hasattr(L, name) and hasattr(jpgx.alt_library(), name)
    for name in ("jpgx_write_jfif_any", "jpgx_pad_edge", "jpgx_encode_rgb_to_jpeg_any"):
        assert name in jpgx.COMPAT_EXPORTS and hasattr(L, name) and hasattr(jpgx.alt_library(), name)
    torch = pytest.importorskip("torch")
    host = torch.zeros((15, 17, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        jpgx.encode_blocks(host, 50, any_size=True)                  # host tensors
    with pytest.raises(ValueError):
        jpgx.encode_jpeg(host, 50, any_size=True)
    with pytest.raises(ValueError):
        jpgx.jfif_gpu(torch.zeros((1, 18 * 64), dtype=torch.int16), 17, 15, 50, any_size=True)
    with pytest.raises(ValueError):
        jpgx.encode_blocks(host, 50, 3, any_size=True)
    with pytest.raises(ValueError):
        jpgx.encode_blocks(torch.zeros((0, 17, 3), dtype=torch.uint8), 50, any_size=True)


# ---- the host routines under the sanitizers ----------------------------------------------------------------
@pytest.mark.skipif(not E.san_build.HAVE_CC, reason="needs gcc and g++")
def test_host_routines_under_asan_ubsan():
    rc, out, err = E.run_san()
    assert rc == 0 and out.rstrip().endswith("encode_any_san: clean"), (out[-2000:], err[-4000:])
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-4000:]
    counts = [ln.split() for ln in out.splitlines() if ln.startswith("sizes ")][0]
    sizes, files = int(counts[1]), int(counts[3])
    assert sizes >= 3 * (40 * 40 + len(E.SIZES)) and files >= sizes      # every size, every sampling
