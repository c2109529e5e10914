"""One-component (grayscale) baseline files on the device (csrc/jpgx_jfif_dec.hip:
jpgx_jfif_decode_gpu_gray; csrc/jpgx_pixels.hip: jpgx_pixels_gpu_gray, k_px_gray; jpgx.jfif_decode_gpu_gray,
pixels_gpu_gray, decode_jpeg(gray=True)).

The inputs are the committed files of tests/golden/gray_fixtures/: nothing here needs Pillow.  The oracles are
the host's _gray routines on the same bytes (held to an independent decoder, to the contract's numpy
restatement and to Pillow in tests/test_gray.py); every comparison is ==."""
import numpy as np
import pytest

import any_cases as A
import gray_cases as G
import jpgx
import jpgx.compat as C
from gpu_files import upload as _upload

gpu = pytest.mark.gpu
L = jpgx.lib
FILL, CFILL = 0x7A, 0x5A5A
SUB = jpgx.JFIF_DECODE_SUBINTERVAL


def _u16(t):
    import torch
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _decode(cuda, files, W, H, sub):
    d_files, lens = _upload(cuda, files)
    coef, qt, status = jpgx.jfif_decode_gpu_gray(d_files, lens, W, H, subinterval=sub)
    assert coef.shape == (len(files), G.nblocks(W, H), 64) and qt.shape == (len(files), 64)
    return coef, qt, status


def _check_against_host(coef, qt, status, files, W, H, tag):
    """statuses, and the coefficients and tables of the status-0 frames, against the host reader"""
    coef, qt, status = coef.cpu().numpy(), _u16(qt), status.cpu().numpy()
    for k, f in enumerate(files):
        rc, r = G.host_status(f, W, H)
        assert status[k] == rc, (tag, k)
        if rc == 0:
            assert np.array_equal(coef[k], r["coef"]) and np.array_equal(qt[k], r["qt"]), (tag, k)
        elif rc == jpgx.EJFIF_HEADER:
            assert not qt[k].any(), (tag, k)


# ---- 7. decode ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sub", [False, True])
def test_every_fixture(cuda, sub):
    for W, H in G.SIZES:
        files = G.files_of(W, H) + (G.patched_files() if (W, H) == (21, 13) else [])
        coef, qt, status = _decode(cuda, files, W, H, sub)
        assert status.cpu().tolist() == [0] * len(files), (W, H)
        _check_against_host(coef, qt, status, files, W, H, (W, H, sub))
    coef, qt, status = _decode(cuda, [G.big_file()], *G.BIG, sub)
    assert status.cpu().tolist() == [0]
    _check_against_host(coef, qt, status, [G.big_file()], *G.BIG, ("big", sub))


@gpu
@pytest.mark.parametrize("flags", [0, SUB])
def test_truncated_frame_in_a_padded_batch(cuda, flags):
    """slot 1 holds a file cut in the middle of its scan: its status alone is EJFIF_SCAN, and nothing is
    written past a frame's nb * 64 elements"""
    import torch
    W, H = 263, 21
    good = G.files_of(W, H)
    scan = C.jfif_info_gray(good[1])["scan_offset"]
    files = [good[0], good[1][:scan + (len(good[1]) - scan) // 2], good[2], good[3]]
    assert G.host_status(files[1], W, H)[0] == jpgx.EJFIF_SCAN
    d_files, lens = _upload(cuda, files)
    n, per, slack = len(files), G.nblocks(W, H) * 64, 3 * 64
    coef = torch.full((n, per + slack), CFILL, dtype=torch.int16, device=cuda)
    qt = torch.zeros((n, 64), dtype=torch.uint16, device=cuda)
    status = torch.full((n,), 77, dtype=torch.int32, device=cuda)
    need = L.jpgx_jfif_decode_gpu_gray_workspace_size(W, H, n, d_files.shape[1], flags)
    ws = torch.full((need,), 0xEE, dtype=torch.uint8, device=cuda)               # scribbled before the call
    rc = L.jpgx_jfif_decode_gpu_gray(d_files.data_ptr(), d_files.shape[1], lens.data_ptr(), n, W, H, flags,
                                     coef.data_ptr(), per + slack, qt.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                     need, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, jpgx.EJFIF_SCAN, 0, 0]
    got = coef.cpu().numpy()
    assert (got[:, per:] == CFILL).all()
    for k in (0, 2, 3):
        assert np.array_equal(got[k, :per], G.host(files[k])["coef"].reshape(-1))
        assert np.array_equal(_u16(qt)[k], G.host(files[k])["qt"])


@gpu
@pytest.mark.parametrize("sub", [False, True])
def test_other_size_and_colour_files_are_header_errors(cuda, sub):
    W, H = 21, 13
    colour = A.project_files(0)[0][3]
    files = [G.files_of(W, H)[0], G.files_of(18, 10)[0], colour, G.files_of(W, H)[1]]
    coef, qt, status = _decode(cuda, files, W, H, sub)
    assert status.cpu().tolist() == [0, jpgx.EJFIF_HEADER, jpgx.EJFIF_HEADER, 0]
    assert not _u16(qt)[1:3].any()
    _check_against_host(coef, qt, status, files, W, H, sub)
    # and the colour decoder refuses the grayscale file
    d_files, lens = _upload(cuda, [files[0]])
    for any_size in (False, True):
        _, _, st = jpgx.jfif_decode_gpu(d_files, lens, 24 if not any_size else W, 16 if not any_size else H, 0,
                                        subinterval=sub, any_size=any_size)
        assert st.cpu().tolist() == [jpgx.EJFIF_HEADER]


# ---- 8. statuses of damaged files -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sub", [False, True])
def test_damaged_files_end_in_the_host_s_status(cuda, sub):
    """the decoder's contract: such bytes end in a status, the host's for the same bytes"""
    files = G.damaged_sample(256)
    W, H = 21, 13
    d_files, lens = _upload(cuda, files)
    coef, qt, status = jpgx.jfif_decode_gpu_gray(d_files, lens, W, H, subinterval=sub)
    host = [G.host_status(f, W, H) for f in files]
    assert {rc for rc, _ in host} == {0, jpgx.EJFIF_HEADER, jpgx.EJFIF_SCAN}
    got, st = coef.cpu().numpy(), status.cpu().numpy()
    for k, (rc, r) in enumerate(host):
        assert st[k] == rc, k
        if rc == 0:
            assert np.array_equal(got[k], r["coef"]), k


# ---- 9. pixels ------------------------------------------------------------------------------------------------
def _raw_pixels(cuda, coefs, W, H, qts, channels, status=None, extra_pitch=24, spare_rows=3):
    """one jpgx_pixels_gpu_gray call; returns the prefilled buffers [n][H + spare_rows][pitch]"""
    import torch
    coefs = np.ascontiguousarray(coefs, np.int16).reshape(len(coefs), -1)
    n, per = coefs.shape
    d_coef = torch.from_numpy(coefs).to(cuda)
    qts = np.ascontiguousarray(qts, np.uint16)
    d_qt = torch.from_numpy(qts.view(np.int16)).to(cuda)
    pitch = (channels * W + 7) // 8 * 8 + extra_pitch
    ostride = (H + spare_rows) * pitch
    out = torch.full((n, ostride), FILL, dtype=torch.uint8, device=cuda)
    d_st = None if status is None else torch.tensor(status, dtype=torch.int32, device=cuda)
    rc = L.jpgx_pixels_gpu_gray(d_coef.data_ptr(), per, n, W, H, d_qt.data_ptr(), 0 if qts.ndim == 1 else 64,
                                d_st.data_ptr() if d_st is not None else None, out.data_ptr(), pitch, ostride,
                                channels, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, H + spare_rows, pitch)


@gpu
@pytest.mark.parametrize("channels", [1, 3])
def test_pixels_of_every_size_in_a_padded_buffer(cuda, channels):
    for W, H in G.SIZES + (G.BIG,):
        files = G.files_of(W, H) if (W, H) != G.BIG else [G.big_file()]
        rs = [G.host(f) for f in files]
        buf = _raw_pixels(cuda, [r["coef"] for r in rs], W, H, np.stack([r["qt"] for r in rs]), channels)
        for k, r in enumerate(rs):
            want = C.pixels_host_gray(r["coef"], W, H, r["qt"], channels, nthreads=1).reshape(H, channels * W)
            assert np.array_equal(buf[k, :H, :channels * W], want), (W, H, k)
        assert (buf[:, :H, channels * W:] == FILL).all() and (buf[:, H:] == FILL).all(), (W, H)
        # one table for the batch: qt_frame_stride 0
        one = _raw_pixels(cuda, [r["coef"] for r in rs], W, H, rs[0]["qt"], channels)
        for k, r in enumerate(rs):
            want = C.pixels_host_gray(r["coef"], W, H, rs[0]["qt"], channels, nthreads=1).reshape(H, channels * W)
            assert np.array_equal(one[k, :H, :channels * W], want), (W, H, k)
        assert (one[:, :H, channels * W:] == FILL).all() and (one[:, H:] == FILL).all(), (W, H)


@gpu
@pytest.mark.parametrize("channels", [1, 3])
def test_a_failed_frame_s_pixels_are_untouched(cuda, channels):
    W, H = 65, 17
    rs = [G.host(f) for f in G.files_of(W, H)[:3]]
    buf = _raw_pixels(cuda, [r["coef"] for r in rs], W, H, np.stack([r["qt"] for r in rs]), channels,
                      status=[0, jpgx.EJFIF_SCAN, 0])
    assert (buf[1] == FILL).all()
    for k in (0, 2):
        want = C.pixels_host_gray(rs[k]["coef"], W, H, rs[k]["qt"], channels).reshape(H, channels * W)
        assert np.array_equal(buf[k, :H, :channels * W], want)


@gpu
@pytest.mark.parametrize("channels", [1, 3])
def test_hostile_values(cuda, channels):
    """tests/pixels_cases.py's extreme coefficients and tables: they change values, never an address"""
    W, H = 21, 13
    coefs, qts = G.hostile_frames(W, H)
    buf = _raw_pixels(cuda, coefs, W, H, qts, channels)
    for k in range(len(coefs)):
        want = C.pixels_host_gray(coefs[k], W, H, qts[k], channels, nthreads=1).reshape(H, channels * W)
        assert np.array_equal(buf[k, :H, :channels * W], want), k
    assert (buf[:, :H, channels * W:] == FILL).all() and (buf[:, H:] == FILL).all()


@gpu
def test_python_view_of_the_pixels(cuda):
    import torch
    W, H = 35, 18
    files = G.files_of(W, H)
    coef, qt, status = _decode(cuda, files, W, H, False)
    for channels in (1, 3):
        px = jpgx.pixels_gpu_gray(coef, W, H, qt, status=status, channels=channels)
        assert px.shape == ((4, H, W) if channels == 1 else (4, H, W, 3)) and px.dtype == torch.uint8
        for k, f in enumerate(files):
            r = G.host(f)
            assert np.array_equal(px[k].cpu().numpy(), C.pixels_host_gray(r["coef"], W, H, r["qt"], channels))
    one = jpgx.pixels_gpu_gray(coef, W, H, qt[2].contiguous(), channels=1, pitch=48)
    assert np.array_equal(one[1].cpu().numpy(), C.pixels_host_gray(G.host(files[1])["coef"], W, H, G.host(files[2])["qt"]))


# ---- 10. end to end -------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sub", [False, True])
def test_decode_jpeg_gray(cuda, sub):
    W, H = 263, 21
    files = G.files_of(W, H)
    got = jpgx.decode_jpeg(files, cuda, subinterval=sub, gray=True)
    assert got.shape == (4, H, W)
    for k, f in enumerate(files):
        r = G.host(f)
        assert np.array_equal(got[k].cpu().numpy(), C.pixels_host_gray(r["coef"], W, H, r["qt"])), k
    big, r = G.big_file(), G.host(G.big_file())
    one = jpgx.decode_jpeg(big, cuda, subinterval=sub, gray=True)
    assert one.shape == (G.BIG[1], G.BIG[0])
    assert np.array_equal(one.cpu().numpy(), C.pixels_host_gray(r["coef"], *G.BIG, r["qt"]))
    d = jpgx.decode_jpeg_coefficients(big, cuda, subinterval=sub, gray=True)
    assert (d["width"], d["height"], d["sample_ratio"], d["restart_interval"]) == G.BIG + (0, 0)
    assert np.array_equal(d["coef"].cpu().numpy(), r["coef"]) and np.array_equal(_u16(d["qt"]), r["qt"])
    for refused in (lambda: jpgx.decode_jpeg(big, cuda), lambda: jpgx.decode_jpeg(big, cuda, any_size=True),
                    lambda: jpgx.decode_jpeg(A.project_files(0)[0][3], cuda, gray=True)):
        with pytest.raises(jpgx.JpgxError) as e:
            refused()
        assert e.value.rc == jpgx.EJFIF_HEADER


@gpu
@pytest.mark.parametrize("sub", [False, True])
def test_chain_on_one_stream(cuda, sub):
    """jfif_decode_gpu_gray -> pixels_gpu_gray on a non-default stream with no host round trip in between"""
    import torch
    W, H = 263, 21
    files = G.files_of(W, H)
    d_files, lens = _upload(cuda, files)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(s):
        coef, qt, status = jpgx.jfif_decode_gpu_gray(d_files, lens, W, H, stream=s, subinterval=sub)
        px1 = jpgx.pixels_gpu_gray(coef, W, H, qt, status=status, channels=1, stream=s)
        px3 = jpgx.pixels_gpu_gray(coef, W, H, qt, status=status, channels=3, stream=s)
    s.synchronize()
    assert status.cpu().tolist() == [0] * 4
    for k, f in enumerate(files):
        r = G.host(f)
        assert np.array_equal(px1[k].cpu().numpy(), C.pixels_host_gray(r["coef"], W, H, r["qt"], 1)), k
        assert np.array_equal(px3[k].cpu().numpy(), C.pixels_host_gray(r["coef"], W, H, r["qt"], 3)), k
