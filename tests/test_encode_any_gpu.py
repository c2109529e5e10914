"""Images of any width and height on the way to a file, on the device (csrc/jpgx_pad.hip: k_pad_edge;
csrc/jpgx_device.hip: jpgx_blocks_gpu_any; csrc/jpgx_jfif.hip: jpgx_jfif_gpu_any; jpgx.encode_blocks,
jfif_gpu and encode_jpeg with any_size=True).

The oracles: the plain entry points and the CPU oracle on the image padded by numpy's edge rule, the host
writer (held to the plain writer's file in tests/test_encode_any.py), the plain decoder on the coded-size
file and Pillow; every comparison is ==."""
import ctypes

import numpy as np
import pytest

import any_cases as A
import encode_any_cases as E
import jpgx
import jpgx.compat as C

gpu = pytest.mark.gpu
pillow = pytest.mark.skipif(not E.have_pillow(), reason="needs Pillow")
SUB, EXACT = jpgx.FLAG_SUBSAMPLE, jpgx.FLAG_FORCE_EXACT
FILL, CFILL = 0x7A, 0x5A5A
# (sample_ratio, flags): 4:4:4, true 4:2:2 and 4:2:0, and parity mode at every ratio (the reference's
# 4:4:4 output on the ratio's coded frame)
MODES = ((0, 0), (1, SUB), (2, SUB), (1, 0), (2, 0))


@pytest.fixture(params=["product", "alt"])
def impl(request, monkeypatch):
    """both libraries: the MFMA kernels and the second implementation behind the same entry points"""
    if request.param == "alt":
        monkeypatch.setattr(jpgx, "lib", jpgx.alt_library())
    return request.param


def _dev(cuda, a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(cuda)          # a copy: the cached images are read-only


# ---- the coefficients -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sr,flags", MODES)
def test_coefficients_are_the_padded_image_s(cuda, impl, sr, flags):
    for W, H in E.SIZES + E.BOTH:
        for kind, q in (("splitmix", 90), ("smooth", 50)):
            rgb = E.image(kind, W, H)
            got = jpgx.encode_blocks(_dev(cuda, rgb), q, sr, flags=flags, any_size=True)
            want = jpgx.encode_blocks(_dev(cuda, E.pad_edge(rgb, sr)), q, sr, flags=flags)
            assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want.cpu().numpy()), (W, H, kind)
            assert np.array_equal(got.cpu().numpy(), E.oracle_coef(kind, W, H, q, sr, bool(flags & SUB))), (W, H, kind)
            if (W, H) == E.coded(W, H, sr):              # a size both take: the plain call on the image itself
                assert np.array_equal(got.cpu().numpy(), jpgx.encode_blocks(_dev(cuda, rgb), q, sr, flags=flags).cpu().numpy())


@gpu
def test_force_exact_underflow_bytes_and_rows_of_any_pitch(cuda, impl):
    W, H, q = 263, 21, 90
    rgb = E.image("splitmix", W, H)
    padded = _dev(cuda, E.pad_edge(rgb, 0))
    want = jpgx.encode_blocks(padded, q, flags=EXACT).cpu().numpy()
    assert np.array_equal(jpgx.encode_blocks(_dev(cuda, rgb), q, flags=EXACT, any_size=True).cpu().numpy(), want)
    assert np.array_equal(want.reshape(-1, 64), E.oracle_coef("splitmix", W, H, q, 0))
    # the caller's own underflow bytes stay
    under = bytes(range(200, 208))
    want = jpgx.encode_blocks(padded, q, underflow=under).cpu().numpy()
    assert np.array_equal(jpgx.encode_blocks(_dev(cuda, rgb), q, underflow=under, any_size=True).cpu().numpy(), want)
    assert not np.array_equal(want.reshape(-1, 64), E.oracle_coef("splitmix", W, H, q, 0))
    # a view with padded rows goes as it is; one with unpacked pixels is copied
    wide = _dev(cuda, np.pad(rgb, ((0, 0), (2, 3), (0, 0))))
    assert not wide[:, 2:2 + W].is_contiguous()
    want = jpgx.encode_blocks(padded, q).cpu().numpy()
    assert np.array_equal(jpgx.encode_blocks(wide[:, 2:2 + W], q, any_size=True).cpu().numpy(), want)
    planes = _dev(cuda, np.ascontiguousarray(rgb.transpose(2, 0, 1))).permute(1, 2, 0)
    assert np.array_equal(jpgx.encode_blocks(planes, q, any_size=True).cpu().numpy(), want)
    # numpy images take the host route
    assert np.array_equal(jpgx.encode_blocks(rgb, q, any_size=True), want)


@gpu
def test_a_launch_on_another_stream(cuda):
    import torch
    W, H, q = 667, 9, 50
    rgb = E.image("splitmix", W, H)
    d_rgb = _dev(cuda, rgb)
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(s):
        got = jpgx.encode_blocks(d_rgb, q, 2, flags=SUB, any_size=True, stream=s)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy(), E.oracle_coef("splitmix", W, H, q, 2))


# ---- the entry point itself: a batch, an odd pitch, an odd base, sentinels everywhere ------------------------------
@gpu
@pytest.mark.parametrize("which", ["product", "alt"])
@pytest.mark.parametrize("sr,flags", [(0, 0), (1, SUB), (2, SUB), (2, EXACT)])
def test_batch_with_sentinels(cuda, which, sr, flags):
    import torch
    L = jpgx.lib if which == "product" else jpgx.alt_library()
    nf, q = 3, 90
    for W, H in E.SIZES:
        cw, ch = E.coded(W, H, sr)
        nb = (cw // 8) * (ch // 8)
        per = (nb + 2 * jpgx.chroma_blocks(cw, 0, ch // 8, sr, flags)) * 64
        pitch = 3 * W + 5
        fstride = pitch * H + 11
        imgs = [np.asarray(E.image("splitmix", W, H)), np.asarray(E.image("smooth", W, H)),
                np.random.default_rng(W + H).integers(0, 256, (H, W, 3), dtype=np.uint8)]
        # the source: one byte into a buffer of sentinels, every byte outside the pixels a sentinel
        src = np.full(1 + nf * fstride + 64, FILL, np.uint8)
        for f, im in enumerate(imgs):
            rows = src[1 + f * fstride:1 + f * fstride + H * pitch].reshape(H, pitch)
            rows[:, :3 * W] = im.reshape(H, 3 * W)
        d_src = _dev(cuda, src)
        fr = jpgx.Frames()
        fr.width, fr.height, fr.row_begin, fr.row_end, fr.nframes = W, H, 0, ch // 8, nf
        fr.in_pitch, fr.in_frame_stride, fr.out_frame_stride = pitch, fstride, per + 3 * 64
        p = jpgx.default_params(W, H, q, sr, flags=flags)       # the visible size's defaults: the call takes the coded size's
        need = L.jpgx_workspace_size_any(ctypes.byref(fr), ctypes.byref(p))
        assert need == (nf * ch * 3 * cw + 15) // 16 * 16
        ws = torch.full((need + 256,), 0xEE, dtype=torch.uint8, device=cuda)        # scribbled before the call
        out = torch.full((nf, per + 3 * 64), CFILL, dtype=torch.int16, device=cuda)
        rc = L.jpgx_blocks_gpu_any(ctypes.byref(fr), ctypes.byref(p), d_src.data_ptr() + 1, out.data_ptr(),
                                   ws.data_ptr(), need, None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert np.array_equal(d_src.cpu().numpy(), src)                            # the source is only read
        wsh = ws.cpu().numpy()
        assert (wsh[need:] == 0xEE).all()                                          # nothing behind the workspace
        coded = wsh[:nf * ch * 3 * cw].reshape(nf, ch, cw, 3)
        got = out.cpu().numpy()
        assert (got[:, per:] == CFILL).all()                                       # nothing behind a frame's output
        for f, im in enumerate(imgs):
            assert np.array_equal(coded[f], E.pad_edge(im, sr)), (W, H, f)         # k_pad_edge's frames
            want = jpgx.encode_blocks(_dev(cuda, E.pad_edge(im, sr)), q, sr, flags=flags)
            assert np.array_equal(got[f, :per], want.cpu().numpy().reshape(-1)), (W, H, f)


# ---- the file ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_device_writer_equals_the_host_writer(cuda, sr, optimize):
    for W, H in E.SIZES + E.BOTH:
        q = 90 if (W + H) % 2 else 50
        coefs = [E.oracle_coef(kind, W, H, q, sr) for kind in ("splitmix", "smooth")]
        d_coef = _dev(cuda, np.stack([c.reshape(-1) for c in coefs]))
        want = [C.write_jfif_ex(c, W, H, q, sr, restart_rows=1, nthreads=1, optimize=optimize, any_size=True)
                for c in coefs]
        out, lens = jpgx.jfif_gpu(d_coef, W, H, q, sr, optimize=optimize, any_size=True)
        for k in range(2):
            assert out[k, :int(lens[k])].cpu().numpy().tobytes() == want[k], (W, H, k)
            assert C.jfif_info(want[k], any_size=True)["width"] == W
        if (W, H) == E.coded(W, H, sr):                  # a size both take
            plain, plens = jpgx.jfif_gpu(d_coef, W, H, q, sr, optimize=optimize)
            assert plens.tolist() == lens.tolist() and out[0, :int(lens[0])].equal(plain[0, :int(lens[0])])
    # two MCU rows per interval; a capacity that is too small is grown once
    W, H = 129, 65
    coef = E.oracle_coef("splitmix", W, H, 90, sr)
    want = C.write_jfif_ex(coef, W, H, 90, sr, restart_rows=2, nthreads=1, optimize=optimize, any_size=True)
    for cap in (None, 1024):
        out, lens = jpgx.jfif_gpu(_dev(cuda, coef.reshape(1, -1)), W, H, 90, sr, restart_rows=2, cap=cap,
                                  optimize=optimize, any_size=True)
        assert out[0, :int(lens[0])].cpu().numpy().tobytes() == want
    assert out.shape[1] > 1024


# ---- there and back -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_round_trip(cuda, sr):
    flags = E.flags_of(sr)
    for W, H in E.SIZES:
        for kind, q, opt in (("smooth", 90, False), ("splitmix", 50, True)):
            rgb = E.image(kind, W, H)
            data = jpgx.encode_jpeg(_dev(cuda, rgb), q, sr, flags=flags, optimize=opt, any_size=True)
            info = C.jfif_info(data, any_size=True)
            assert (info["width"], info["height"], info["sample_ratio"]) == (W, H, sr)
            assert data == C.write_jfif_ex(E.oracle_coef(kind, W, H, q, sr), W, H, q, sr, restart_rows=1, nthreads=1,
                                           optimize=opt, any_size=True)
            back = jpgx.decode_jpeg(data, cuda, any_size=True)
            assert tuple(back.shape) == (H, W, 3)
            if sr == 0:                                  # no upsampling: the visible part of the coded frame's pixels
                whole = jpgx.encode_jpeg(_dev(cuda, E.pad_edge(rgb, 0)), q, optimize=opt)
                assert whole == C.write_jfif_ex(E.oracle_coef(kind, W, H, q, 0), *E.coded(W, H, 0), q, 0, restart_rows=1,
                                                nthreads=1, optimize=opt)
                assert data == A.patch_size(whole, W, H)
                assert np.array_equal(back.cpu().numpy(), jpgx.decode_jpeg(whole, cuda).cpu().numpy()[:H, :W])
            if E.have_pillow():
                assert A.fits_16_bits(C.read_jfif(data, 1, any_size=True))      # a condition of the comparison
                assert np.array_equal(back.cpu().numpy(), A.pillow_pixels(data)), (W, H, kind)
    # without FLAG_SUBSAMPLE the file is 4:4:4 and so is the coded frame, whatever the ratio
    rgb = _dev(cuda, E.image("smooth", 17, 15))
    assert jpgx.encode_jpeg(rgb, 50, sr, any_size=True) == jpgx.encode_jpeg(rgb, 50, 0, any_size=True)
    with pytest.raises(jpgx.JpgxError):
        jpgx.encode_jpeg(rgb, 50)                        # the default still refuses the size
