"""Baseline JFIF files of any width and height on the device (csrc/jpgx_jfif_dec.hip:
jpgx_jfif_decode_gpu_any; csrc/jpgx_pixels.hip: jpgx_pixels_gpu_any; jpgx.jfif_decode_gpu, pixels_gpu
and decode_jpeg with any_size=True).

The oracles are the host's _any routines on the same bytes (held to an independent decoder, to the
contract's numpy restatement and to Pillow in tests/test_any_size.py) and Pillow itself; every
comparison is ==."""
import numpy as np
import pytest

import any_cases as A
import idct_ref_any as R
import jpgx
import jpgx.compat as C
import pixels_cases as P
from gpu_files import upload as _upload

gpu = pytest.mark.gpu
pillow = pytest.mark.skipif(not A.have_pillow(), reason="needs Pillow")
L = jpgx.lib
FILL, CFILL = 0x7A, 0x5A5A
SUB = jpgx.JFIF_DECODE_SUBINTERVAL


def _host(data):
    """(status, read_jfif's dict or None) of the host reader"""
    try:
        return 0, C.read_jfif(data, 1, any_size=True)
    except jpgx.JpgxError as e:
        return e.rc, None


def _decode_and_compare(cuda, files, W, H, sr):
    """the batch through the decoder in both modes and through the pixel kernels, each against the host"""
    import torch
    d_files, lens = _upload(cuda, files)
    host = [_host(f) for f in files]
    rgb = None
    for sub in (False, True):
        coef, qt, status = jpgx.jfif_decode_gpu(d_files, lens, W, H, sr, subinterval=sub, any_size=True)
        nb, nbc = R.nblocks(W, H, sr)
        assert coef.shape == (len(files), nb + 2 * nbc, 64)
        rgb = jpgx.pixels_gpu(coef, W, H, sr, d_qt=qt, status=status, any_size=True)
        coef, status = coef.cpu().numpy(), status.cpu().numpy()
        qt = qt.view(torch.int16).cpu().numpy().view(np.uint16)
        for k, (rc, r) in enumerate(host):
            assert status[k] == rc, (k, sub)
            if rc == 0:
                assert np.array_equal(coef[k], r["coef"].reshape(-1, 64)), (k, sub)
                assert np.array_equal(qt[k], r["qt"]), (k, sub)
        assert rgb.shape == (len(files), H, W, 3)
        px = rgb.cpu().numpy()
        for k, (rc, r) in enumerate(host):
            if rc == 0:
                assert np.array_equal(px[k], C.pixels_host(r["coef"], W, H, sr, r["qt"], 2, any_size=True)), (k, sub)
    return host


# ---- basic equality ---------------------------------------------------------------------------------------
@gpu
@pillow
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_pillow_s_files(cuda, sr):
    for W, H in A.SIZES:
        files = A.pillow_files(W, H, sr)
        host = _decode_and_compare(cuda, files, W, H, sr)
        assert all(rc == 0 for rc, _ in host)
        for sub in (False, True):
            got = jpgx.decode_jpeg(files, cuda, subinterval=sub, any_size=True).cpu().numpy()
            assert got.shape == (len(files), H, W, 3)
            for k, f in enumerate(files):
                assert A.fits_16_bits(host[k][1])
                assert np.array_equal(got[k], A.pillow_pixels(f)), (W, H, k, sub)
        one = jpgx.decode_jpeg(files[0], cuda, any_size=True)
        assert one.shape == (H, W, 3) and np.array_equal(one.cpu().numpy(), A.pillow_pixels(files[0]))


@gpu
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_this_project_s_files_patched_down(cuda, sr):
    """the project's restart layout and its own Huffman tables under a smaller SOF"""
    cases = A.project_files(sr)
    for W, H in A.PATCHED[sr]:
        files = [data for w, h, _, data in cases if (w, h) == (W, H)]
        coefs = [coef for w, h, coef, _ in cases if (w, h) == (W, H)]
        host = _decode_and_compare(cuda, files, W, H, sr)
        for (rc, r), coef in zip(host, coefs):
            assert rc == 0 and np.array_equal(r["coef"].reshape(-1, 64), coef)
        d = jpgx.decode_jpeg_coefficients(files[0], cuda, any_size=True)
        assert (d["width"], d["height"], d["sample_ratio"]) == (W, H, sr)
        assert np.array_equal(d["coef"].cpu().numpy().reshape(-1, 64), coefs[0])
        with pytest.raises(jpgx.JpgxError):              # the default still refuses the size
            jpgx.decode_jpeg(files[0], cuda)


# ---- a failed frame between two good ones ---------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_truncated_middle_frame(cuda, sr, sub):
    import torch
    W, H = A.PATCHED[sr][-1]
    good = [data for w, h, _, data in A.project_files(sr) if (w, h) == (W, H)]
    scan = C.jfif_info(good[0], any_size=True)["scan_offset"]
    cut = good[0][:scan + (len(good[0]) - scan) // 2]
    files = [good[0], cut, good[2]]
    assert _host(cut)[0] == jpgx.EJFIF_SCAN
    d_files, lens = _upload(cuda, files)
    coef, qt, status = jpgx.jfif_decode_gpu(d_files, lens, W, H, sr, subinterval=sub, any_size=True)
    assert status.cpu().tolist() == [0, jpgx.EJFIF_SCAN, 0]
    pitch = (3 * W + 7) // 8 * 8
    out = torch.full((3 * H * pitch,), FILL, dtype=torch.uint8, device=cuda)
    rgb = jpgx.pixels_gpu(coef, W, H, sr, d_qt=qt, status=status, out=out, any_size=True).cpu().numpy()
    assert (out.cpu().numpy().reshape(3, -1)[1] == FILL).all()   # the failed frame's pixels are untouched
    for k in (0, 2):
        r = C.read_jfif(files[k], 1, any_size=True)
        assert np.array_equal(coef[k].cpu().numpy(), r["coef"].reshape(-1, 64))
        assert np.array_equal(rgb[k], C.pixels_host(r["coef"], W, H, sr, r["qt"], 1, any_size=True))
    with pytest.raises(jpgx.JpgxError):
        jpgx.decode_jpeg(files, cuda, subinterval=sub, any_size=True)


# ---- nothing is written that is no coefficient and no pixel --------------------------------------------------
def _raw_pixels(cuda, coefs, W, H, sr, qts, status=None, extra_pitch=8, spare_rows=2, L=L):
    """one jpgx_pixels_gpu_any call on library L; returns the prefilled buffers [n][H + spare_rows][pitch]"""
    import torch
    coefs = np.ascontiguousarray(coefs, np.int16).reshape(len(coefs), -1)
    n, per = coefs.shape
    d_coef = torch.from_numpy(coefs).to(cuda)
    qts = np.ascontiguousarray(qts, np.uint16)
    d_qt = torch.from_numpy(qts.view(np.int16)).to(cuda)
    pitch = (3 * W + 7) // 8 * 8 + extra_pitch
    ostride = (H + spare_rows) * pitch
    out = torch.full((n, ostride), FILL, dtype=torch.uint8, device=cuda)
    need = L.jpgx_pixels_gpu_any_workspace_size(W, H, sr, n)
    assert (need == 0) == (sr == 0)
    ws = torch.full((max(need, 16),), 0xEE, dtype=torch.uint8, device=cuda)      # scribbled before the call
    d_st = None if status is None else torch.tensor(status, dtype=torch.int32, device=cuda)
    rc = L.jpgx_pixels_gpu_any(d_coef.data_ptr(), per, n, W, H, sr, d_qt.data_ptr(), 0 if qts.ndim == 2 else 128,
                               d_st.data_ptr() if d_st is not None else None, out.data_ptr(), pitch, ostride,
                               ws.data_ptr() if need else None, need, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, H + spare_rows, pitch)


@gpu
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_sentinels(cuda, sr):
    import torch
    W, H = A.PATCHED[sr][-1]
    cases = [(W, H, [data for w, h, _, data in A.project_files(sr) if (w, h) == (W, H)][:2])]
    if A.have_pillow():
        cases += [(W, H, A.pillow_files(W, H, sr)[1:3]) for W, H in A.SIZES]
    for W, H, files in cases:
        nb, nbc = R.nblocks(W, H, sr)
        per = (nb + 2 * nbc) * 64
        d_files, lens = _upload(cuda, files)
        n, slack = len(files), 3 * 64
        for flags in (0, SUB):
            coef = torch.full((n, per + slack), CFILL, dtype=torch.int16, device=cuda)
            qt = torch.zeros((n, 2, 64), dtype=torch.uint16, device=cuda)
            status = torch.full((n,), 77, dtype=torch.int32, device=cuda)
            need = L.jpgx_jfif_decode_gpu_any_workspace_size(W, H, sr, n, d_files.shape[1], flags)
            ws = torch.full((need,), 0xEE, dtype=torch.uint8, device=cuda)       # scribbled before the call
            rc = L.jpgx_jfif_decode_gpu_any(d_files.data_ptr(), d_files.shape[1], lens.data_ptr(), n, W, H, sr, flags,
                                            coef.data_ptr(), per + slack, qt.data_ptr(), status.data_ptr(),
                                            ws.data_ptr(), need, None)
            assert rc == 0
            torch.cuda.synchronize()
            assert status.cpu().tolist() == [0] * n
            got = coef.cpu().numpy()
            assert (got[:, per:] == CFILL).all()                                 # the slack after each frame
            rs = [C.read_jfif(f, 1, any_size=True) for f in files]
            for k, r in enumerate(rs):
                assert np.array_equal(got[k, :per], r["coef"].reshape(-1))
        buf = _raw_pixels(cuda, [r["coef"] for r in rs], W, H, sr, np.stack([r["qt"] for r in rs]))
        for k, r in enumerate(rs):
            assert np.array_equal(buf[k, :H, :3 * W].reshape(H, W, 3),
                                  C.pixels_host(r["coef"], W, H, sr, r["qt"], 1, any_size=True)), (W, H, k)
            assert (buf[k, :H, 3 * W:] == FILL).all() and (buf[k, H:] == FILL).all(), (W, H, k)


# ---- hostile values -------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", ["product", "alt"])
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_hostile_values(cuda, sr, which):
    """tests/pixels_cases.py's extreme coefficients and tables in the coded frame of 17 x 15: they change
    values, never an address"""
    W, H = 17, 15
    cw, ch = R.coded(W, H, sr)
    coefs, qts = P.hostile_frames(cw, ch, sr)
    buf = _raw_pixels(cuda, coefs, W, H, sr, qts, L=jpgx.lib if which == "product" else jpgx.alt_library())
    for k in range(len(coefs)):
        want = C.pixels_host(coefs[k], W, H, sr, qts[k], 1, any_size=True)
        assert np.array_equal(buf[k, :H, :3 * W].reshape(H, W, 3), want), k
    assert (buf[:, :H, 3 * W:] == FILL).all() and (buf[:, H:] == FILL).all()


# ---- a size both families take ----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_mcu_multiple_equals_the_plain_call(cuda, sr):
    import torch
    W, H = 272, 32                                       # two workgroups per block row, a last run of 2 blocks
    files = [C.write_jfif_ex(P.oracle_coef("splitmix", W, H, q, sr), W, H, q, sr, restart_rows=1, nthreads=1,
                             optimize=opt) for q, opt in ((50, False), (90, True))]
    d_files, lens = _upload(cuda, files)
    for sub in (False, True):
        a = jpgx.jfif_decode_gpu(d_files, lens, W, H, sr, subinterval=sub, any_size=True)
        b = jpgx.jfif_decode_gpu(d_files, lens, W, H, sr, subinterval=sub)
        for x, y in zip(a, b):
            assert x.shape == y.shape and torch.equal(x.view(torch.int16) if x.dtype == torch.uint16 else x,
                                                      y.view(torch.int16) if y.dtype == torch.uint16 else y)
        pa = jpgx.pixels_gpu(a[0], W, H, sr, d_qt=a[1], status=a[2], any_size=True)
        pb = jpgx.pixels_gpu(b[0], W, H, sr, d_qt=b[1], status=b[2])
        assert pa.shape == pb.shape == (2, H, W, 3) and torch.equal(pa, pb)
    assert torch.equal(jpgx.decode_jpeg(files, cuda, any_size=True), jpgx.decode_jpeg(files, cuda))
