"""The decode at 1/2, 1/4 and 1/8 of the size on the device: jpgx_pixels_gpu_scaled and
jpgx_pixels_gpu_gray_scaled against their host twins, which tests/test_pixels_scaled.py holds to the
contract and to Pillow.  Every size, sampling and scale of tests/scaled_cases.py through a raw call into
a prefilled buffer with a wider pitch and two spare rows, so that parity and "nothing outside the image"
are one check; batches, a skipped frame, hostile frames and the frames that tell the multipliers apart;
decode_jpeg(scale=d) against Pillow's draft decode.  Every comparison is ==."""
import numpy as np
import pytest

import idct_ref_scaled as RS
import jpgx
import jpgx.compat as C
import scaled_cases as S

gpu = pytest.mark.gpu
pillow = pytest.mark.skipif(not S.have_pillow(), reason="needs Pillow")
FILL = 0x5C
SAMP_IDS = [str(s) for s in S.SAMPLINGS]


def _u16(a, cuda):
    import torch
    return torch.from_numpy(np.array(a, np.uint16).view(np.int16)).to(cuda).view(torch.uint16)


def _raw(cuda, coefs, qts, W, H, samp, d, channels=1, status=None, qstride=None, lib=None):
    """one raw call over [n] frames into a buffer of FILL: rows of bytes per pixel * ow rounded up to 8
    plus 8, two spare rows per frame.  Returns (rc, the buffer [n][oh + 2][pitch], bytes per row)"""
    import torch
    L = lib or jpgx.lib
    gray = samp == "gray"
    coefs = np.array(coefs, np.int16).reshape(len(coefs), -1)
    n, per = coefs.shape
    d_coef = torch.from_numpy(coefs).to(cuda)
    d_qt = _u16(qts, cuda)
    ow, oh = S.out_size(W, H, d)
    bpp = channels if gray else 3
    pitch = (bpp * ow + 7) // 8 * 8 + 8
    out = torch.full((n, oh + 2, pitch), FILL, dtype=torch.uint8, device=cuda)
    d_status = None if status is None else torch.tensor(status, dtype=torch.int32, device=cuda)
    sp = None if d_status is None else d_status.data_ptr()
    if qstride is None:
        qstride = 64 if gray else 128
    if gray:
        rc = L.jpgx_pixels_gpu_gray_scaled(d_coef.data_ptr(), per, n, W, H, d, d_qt.data_ptr(), qstride, sp,
                                           out.data_ptr(), pitch, (oh + 2) * pitch, channels, None)
    else:
        need = L.jpgx_pixels_gpu_scaled_workspace_size(W, H, samp, d, n)
        ws = torch.full((max(need, 16),), 0xEE, dtype=torch.uint8, device=cuda)
        rc = L.jpgx_pixels_gpu_scaled(d_coef.data_ptr(), per, n, W, H, samp, d, d_qt.data_ptr(), qstride, sp,
                                      out.data_ptr(), pitch, (oh + 2) * pitch, ws.data_ptr() if need else None, need, None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), bpp * ow


def _host(coef, qt, W, H, samp, d, channels=1):
    if samp == "gray":
        return C.pixels_host_gray(coef, W, H, qt, channels, nthreads=1, scale=d)
    return C.pixels_host(coef, W, H, samp, qt, nthreads=1, scale=d)


def _check_frames(buf, nbytes, wants, what, skipped=()):
    for k, want in enumerate(wants):
        oh = buf.shape[1] - 2
        assert (buf[k, :, nbytes:] == FILL).all() and (buf[k, oh:] == FILL).all(), (what, k)
        if k in skipped:
            assert (buf[k] == FILL).all(), (what, k)
        else:
            assert np.array_equal(buf[k, :oh, :nbytes].reshape(want.shape), want), (what, k)


@gpu
@pillow
@pytest.mark.parametrize("samp", S.SAMPLINGS, ids=SAMP_IDS)
@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: "%dx%d" % s)
def test_kernels_equal_the_host_twin_and_write_nothing_outside(cuda, size, samp):
    W, H = size
    gray = samp == "gray"
    rs = [S.read(data, gray) for data in S.files(W, H, samp)]
    coefs = np.stack([np.asarray(r["coef"]).reshape(-1, 64) for r in rs])
    qts = np.stack([r["qt"] for r in rs])
    for d in S.SCALES:
        for ch in ((1, 3) if gray else (1,)):
            rc, buf, nbytes = _raw(cuda, coefs, qts, W, H, samp, d, ch)
            assert rc == 0, rc
            _check_frames(buf, nbytes, [S.host_pixels(r, gray, d, ch) for r in rs], (W, H, samp, d, ch))


@gpu
@pillow
@pytest.mark.parametrize("samp", S.SAMPLINGS, ids=SAMP_IDS)
def test_batches_through_the_package(cuda, samp):
    import torch
    W, H = 53, 37
    gray = samp == "gray"
    rs = [S.read(data, gray) for data in S.files(W, H, samp)[:3]]
    d_coef = torch.from_numpy(np.stack([np.asarray(r["coef"]).reshape(-1, 64) for r in rs])).to(cuda)
    per_frame = _u16(np.stack([r["qt"] for r in rs]), cuda)
    one = _u16(rs[1]["qt"], cuda)
    for d in S.SCALES:
        ow, oh = jpgx.scaled_size(W, H, d)
        for ch in ((1, 3) if gray else (None,)):
            call = ((lambda qt: jpgx.pixels_gpu_gray(d_coef, W, H, qt, channels=ch, scale=d)) if gray else
                    (lambda qt: jpgx.pixels_gpu(d_coef, W, H, samp, d_qt=qt, scale=d)))
            got = call(per_frame).cpu().numpy()
            assert got.shape == (3, oh, ow) + ((3,) if ch != 1 else ())
            for k, r in enumerate(rs):
                assert np.array_equal(got[k], S.host_pixels(r, gray, d, ch or 1)), (samp, d, k)
            got = call(one).cpu().numpy()
            for k, r in enumerate(rs):
                want = _host(r["coef"], rs[1]["qt"], W, H, samp, d, ch or 1)
                assert np.array_equal(got[k], want), (samp, d, k)


@gpu
@pillow
@pytest.mark.parametrize("subinterval", (False, True))
@pytest.mark.parametrize("samp", S.SAMPLINGS, ids=SAMP_IDS)
def test_decode_jpeg_equals_pillows_draft_decode(cuda, samp, subinterval):
    gray = samp == "gray"
    for W, H in ((17, 9), (53, 37), (100, 75), (263, 21)):
        files = S.files(W, H, samp)
        for data in files:
            assert S.fits_16_bits(S.read(data, gray), gray)
        for d in S.SCALES:
            assert S.pinned(W, H, d)
            got = jpgx.decode_jpeg(files, cuda, subinterval=subinterval, gray=gray, scale=d).cpu().numpy()
            for k, data in enumerate(files):
                assert np.array_equal(got[k], S.draft_pixels(data, d, "L" if gray else "RGB")), (W, H, samp, d, k)
    one = jpgx.decode_jpeg(S.files(53, 37, samp)[0], cuda, subinterval=subinterval, gray=gray, scale=4)
    assert tuple(one.shape[:2]) == (10, 14)


@gpu
@pillow
@pytest.mark.parametrize("samp", S.SAMPLINGS, ids=SAMP_IDS)
def test_a_skipped_frame_is_untouched(cuda, samp):
    W, H = 33, 31
    gray = samp == "gray"
    rs = [S.read(data, gray) for data in S.files(W, H, samp)[:3]]
    coefs = np.stack([np.asarray(r["coef"]).reshape(-1, 64) for r in rs])
    qts = np.stack([r["qt"] for r in rs])
    for d in S.SCALES:
        rc, buf, nbytes = _raw(cuda, coefs, qts, W, H, samp, d, 3 if gray else 1, status=[0, -10, 0])
        assert rc == 0
        _check_frames(buf, nbytes, [S.host_pixels(r, gray, d, 3 if gray else 1) for r in rs], (samp, d), skipped=(1,))


@gpu
@pytest.mark.parametrize("which", ["product", "alt"])
@pytest.mark.parametrize("samp", S.SAMPLINGS, ids=SAMP_IDS)
def test_hostile_frames(cuda, samp, which):
    W, H = S.HOSTILE_SIZE
    L = jpgx.lib if which == "product" else jpgx.alt_library()
    coefs, qts = S.hostile_frames(samp)
    for d in S.SCALES:
        rc, buf, nbytes = _raw(cuda, coefs, qts, W, H, samp, d, lib=L)
        assert rc == 0
        _check_frames(buf, nbytes, [_host(coefs[k], qts[k], W, H, samp, d) for k in range(len(coefs))], (samp, d))


@gpu
@pytest.mark.parametrize("d", (2, 4))
@pytest.mark.parametrize("samp", S.SAMPLINGS, ids=SAMP_IDS)
def test_the_multiplier_is_chosen_run_by_run(cuda, samp, d):
    """pass 1 takes the 24-bit multiplier where the tables or a vote over the run allow it
    (pxs_transform): frames on which a wrong choice shows, each guarded before any device call"""
    W, H = S.MUL_SIZE
    coefs, qts = S.multiplier_frames(samp, d)
    for k in range(len(coefs)):
        assert S.multiplier_tells(samp, d, coefs[k], qts[k]), (samp, d, k)
    rc, buf, nbytes = _raw(cuda, coefs, qts, W, H, samp, d)
    assert rc == 0
    _check_frames(buf, nbytes, [_host(coefs[k], qts[k], W, H, samp, d) for k in range(len(coefs))], (samp, d))


@gpu
@pytest.mark.parametrize("samp", S.SAMPLINGS, ids=SAMP_IDS)
def test_scale_1_is_the_unscaled_call(cuda, samp):
    import torch
    W, H = 53, 37
    coefs, qts = S.hostile_frames(samp, W, H)
    coefs, qts = coefs[2:5], qts[2:5]
    rc, buf, nbytes = _raw(cuda, coefs, qts, W, H, samp, 1)
    assert rc == 0
    d_coef = torch.from_numpy(np.array(coefs)).to(cuda)
    if samp == "gray":
        want = jpgx.pixels_gpu_gray(d_coef, W, H, _u16(qts, cuda))
    else:
        want = jpgx.pixels_gpu(d_coef, W, H, samp, d_qt=_u16(qts, cuda), any_size=True)
    want = want.cpu().numpy()
    _check_frames(buf, nbytes, [want[k] for k in range(3)], samp)


@gpu
def test_raw_calls_refuse_in_the_documented_order(cuda):
    import torch
    L = jpgx.lib
    W, H = 24, 16
    coef = torch.zeros((2, 16, 64), dtype=torch.int16, device=cuda)      # 4:2:2: 4 x 2 + 2 (2 x 2) blocks
    qt = torch.ones((2, 64), dtype=torch.int16, device=cuda)
    out = torch.full((2, 10, 48), FILL, dtype=torch.uint8, device=cuda)
    need = L.jpgx_pixels_gpu_scaled_workspace_size(W, H, 1, 2, 2)
    assert need == 2 * 2 * 4 * 16
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)

    def call(coef_p=coef.data_ptr(), stride=16 * 64, n=2, w=W, h=H, sr=1, d=2, qstride=0, pitch=40, ostride=400,
             ws_p=ws.data_ptr(), ws_n=need):
        return L.jpgx_pixels_gpu_scaled(coef_p, stride, n, w, h, sr, d, qt.data_ptr(), qstride, None, out.data_ptr(),
                                        pitch, ostride, ws_p, ws_n, None)

    assert call(d=3) == jpgx.EARG and call(d=3, sr=5) == jpgx.EARG       # the scale before the geometry
    assert call(coef_p=coef.data_ptr() + 2) == jpgx.EARG and call(n=0) == jpgx.EARG
    assert call(sr=5, ws_n=0) == jpgx.ESAMPLE                            # the geometry before the workspace
    assert call(w=0, ws_n=0) == jpgx.EGEOMETRY
    assert call(stride=15 * 64, ws_n=0) == jpgx.EARG                     # strides and pitches before the workspace
    assert call(qstride=64, ws_n=0) == jpgx.EARG
    assert call(pitch=32, ws_n=0) == jpgx.EARG and call(pitch=44, ws_n=0) == jpgx.EARG
    assert call(ostride=312, ws_n=0) == jpgx.EARG
    assert call(ws_n=need - 1) == jpgx.EWORKSPACE
    assert call(ws_p=None) == jpgx.EARG and call(ws_p=ws.data_ptr() + 8) == jpgx.EARG
    torch.cuda.synchronize()
    assert (out == FILL).all()
    assert call() == 0
    assert L.jpgx_pixels_gpu_gray_scaled(coef.data_ptr(), 6 * 64, 2, W, H, 7, qt.data_ptr(), 0, None, out.data_ptr(), 8, 80,
                                         1, None) == jpgx.EARG
    assert L.jpgx_pixels_gpu_gray_scaled(coef.data_ptr(), 6 * 64, 2, W, H, 2, qt.data_ptr(), 0, None, out.data_ptr(), 8, 80,
                                         1, None) == jpgx.EARG            # ow = 12
    assert L.jpgx_pixels_gpu_gray_scaled(coef.data_ptr(), 6 * 64, 2, W, H, 2, qt.data_ptr(), 0, None, out.data_ptr(), 16,
                                         128, 1, None) == 0
    torch.cuda.synchronize()
