"""The argument checks of the device entry points' Python binding (jpgx.jfif_decode_gpu,
jfif_decode_gpu_gray, pixels_gpu, pixels_gpu_gray, jfif_gpu): every malformed argument is refused with
ValueError and the public function's own name in front of the message, before anything is launched.
The frame is 16 x 16, 4:4:4 or one component: 4 blocks a plane."""
import pytest

import jpgx

gpu = pytest.mark.gpu
W = H = 16
NF = 2


def _refused(msg, fn, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert str(e.value) == msg


def _u16(cuda, *shape):
    import torch
    return torch.zeros(shape, dtype=torch.int16, device=cuda).view(torch.uint16)


DECODERS = {"jfif_decode_gpu": "bad geometry or sample_ratio", "jfif_decode_gpu_gray": "bad geometry"}


@gpu
@pytest.mark.parametrize("name", sorted(DECODERS))
def test_decoders_refuse_a_malformed_batch(cuda, name):
    import torch
    fn, geometry = getattr(jpgx, name), DECODERS[name]
    files = torch.zeros((NF, 64), dtype=torch.uint8, device=cuda)
    lens = torch.full((NF,), 64, dtype=torch.int64, device=cuda)
    # host tensors, and what is no tensor
    _refused(f"{name}: d_files must be a device tensor", fn, files.cpu(), lens, W, H)
    _refused(f"{name}: lens must be a device tensor", fn, files, lens.cpu(), W, H)
    _refused(f"{name}: d_files must be a device tensor", fn, bytes(64), lens, W, H)
    # wrong dtypes
    _refused(f"{name}: d_files must be torch.uint8", fn, files.to(torch.int8), lens, W, H)
    _refused(f"{name}: lens must be torch.int64", fn, files, lens.to(torch.int32), W, H)
    # shapes: lens of the wrong length, an empty batch, one dimension too few
    shape = f"{name}: d_files [nframes][cap] and lens [nframes]"
    _refused(shape, fn, files, lens[:1], W, H)
    _refused(shape, fn, files[:0], lens[:0], W, H)
    _refused(shape, fn, files[0], lens, W, H)
    # rows that are not contiguous, lens that is not, files of no bytes
    rows = f"{name}: each file must be contiguous"
    _refused(rows, fn, torch.zeros((NF, 128), dtype=torch.uint8, device=cuda)[:, ::2], lens, W, H)
    _refused(rows, fn, files, torch.zeros(2 * NF, dtype=torch.int64, device=cuda)[::2], W, H)
    _refused(rows, fn, files[:, :0], lens, W, H)
    # a stride between the files that is less than a file
    over = torch.zeros(256, dtype=torch.uint8, device=cuda).as_strided((NF, 64), (32, 1))
    _refused(f"{name}: overlapping files", fn, over, lens, W, H)
    # the geometry is refused after the batch's shape and before the overlap
    _refused(f"{name}: {geometry}", fn, over, lens, 0, H)
    _refused(shape, fn, files, lens[:1], 0, H)


# planes, a frame's table elements and their shape in the message, a pixel's bytes in the message
PIXELS = {"pixels_gpu": (3, 128, "[2][64]", "3"), "pixels_gpu_gray": (1, 64, "[64]", "channels")}


@gpu
@pytest.mark.parametrize("name", sorted(PIXELS))
def test_pixel_calls_refuse_malformed_arguments(cuda, name):
    import torch
    planes, qsize, qshape, bpp_name = PIXELS[name]
    gray = planes == 1
    bpp = 1 if gray else 3

    def call(coef, qt, **kw):
        if gray:
            return jpgx.pixels_gpu_gray(coef, W, H, qt, **kw)
        return jpgx.pixels_gpu(coef, W, H, 0, d_qt=qt, **kw)

    coef = torch.zeros((NF, planes * 4, 64), dtype=torch.int16, device=cuda)
    qt = _u16(cuda, NF, qsize)
    # d_coef: a host tensor, a wrong dtype, one dimension too few
    bad_coef = f"{name}: d_coef must be an int16 [nframes][...] device tensor"
    _refused(bad_coef, call, coef.cpu(), qt)
    _refused(bad_coef, call, coef.to(torch.int32), qt)
    _refused(bad_coef, call, coef.reshape(-1), qt)
    # d_qt: a host tensor, none, a wrong dtype, not contiguous; then neither accepted size
    bad_qt = f"{name}: d_qt must be a contiguous uint16 device tensor"
    _refused(bad_qt, call, coef, qt.cpu())
    _refused(bad_qt, call, coef, None)
    _refused(bad_qt, call, coef, qt.view(torch.int16))
    _refused(bad_qt, call, coef, _u16(cuda, NF, 2 * qsize)[:, ::2])
    _refused(f"{name}: d_qt must be {qshape} or [nframes]{qshape}", call, coef, _u16(cuda, 100))
    # a frame that holds too few blocks
    blocks = "nb blocks" if gray else "nb + 2 nbc blocks"
    _refused(f"{name}: each frame must be contiguous and hold {blocks}", call, coef[:, :planes * 4 - 1], qt)
    # status: a wrong size, a wrong dtype
    bad_status = f"{name}: status must be a contiguous int32 [nframes] tensor"
    _refused(bad_status, call, coef, qt, status=torch.zeros(NF + 1, dtype=torch.int32, device=cuda))
    _refused(bad_status, call, coef, qt, status=torch.zeros(NF, dtype=torch.int64, device=cuda))
    _refused(bad_status, call, coef, qt, status=torch.zeros(2 * NF, dtype=torch.int32, device=cuda)[::2])
    # pitch: no multiple of 8, too small
    bad_pitch = f"{name}: pitch must be a multiple of 8 and at least {bpp_name} * width"
    _refused(bad_pitch, call, coef, qt, pitch=bpp * W + 4)
    _refused(bad_pitch, call, coef, qt, pitch=bpp * W - 8)
    # out: a wrong size (for the default pitch and for a stated one), a wrong dtype
    bad_out = f"{name}: out must be a contiguous uint8 buffer of nframes * H * pitch bytes"
    _refused(bad_out, call, coef, qt, out=torch.zeros(NF * H * bpp * W + 8, dtype=torch.uint8, device=cuda))
    _refused(bad_out, call, coef, qt, out=torch.zeros(NF * H * bpp * W, dtype=torch.uint8, device=cuda), pitch=bpp * W + 8)
    _refused(bad_out, call, coef, qt, out=torch.zeros(NF * H * bpp * W, dtype=torch.int8, device=cuda))
    # the order: the tables' size before the status, the status before the pitch, the pitch before out
    _refused(f"{name}: d_qt must be {qshape} or [nframes]{qshape}", call, coef, _u16(cuda, 100), pitch=4)
    _refused(bad_status, call, coef, qt, status=torch.zeros(NF + 1, dtype=torch.int32, device=cuda), pitch=4)
    _refused(bad_pitch, call, coef, qt, pitch=4, out=torch.zeros(8, dtype=torch.uint8, device=cuda))


@gpu
def test_pixels_gpu_gray_refuses_channels_that_are_not_1_or_3(cuda):
    import torch
    coef = torch.zeros((NF, 4, 64), dtype=torch.int16, device=cuda)
    qt = _u16(cuda, NF, 64)
    for channels in (0, 2, 4):
        _refused("pixels_gpu_gray: channels must be 1 or 3", jpgx.pixels_gpu_gray, coef, W, H, qt, channels=channels)
    # before the geometry, after the tables' dtype
    _refused("pixels_gpu_gray: channels must be 1 or 3", jpgx.pixels_gpu_gray, coef, 0, H, qt, channels=2)
    _refused("pixels_gpu_gray: d_qt must be a contiguous uint16 device tensor", jpgx.pixels_gpu_gray, coef, W, H,
             qt.view(torch.int16), channels=2)
    _refused("pixels_gpu_gray: bad geometry", jpgx.pixels_gpu_gray, coef, 0, H, qt)


@gpu
def test_jfif_gpu_refuses_malformed_coefficients(cuda):
    import torch
    coef = torch.zeros((NF, 12 * 64), dtype=torch.int16, device=cuda)
    _refused("jfif_gpu: d_coef must be a device tensor", jpgx.jfif_gpu, coef.cpu(), W, H, 50)
    _refused("jfif_gpu: d_coef must be a device tensor", jpgx.jfif_gpu, coef.cpu().numpy(), W, H, 50)
    shape = "jfif_gpu: d_coef must be an int16 [nframes][...] tensor"
    _refused(shape, jpgx.jfif_gpu, coef.to(torch.int32), W, H, 50)
    _refused(shape, jpgx.jfif_gpu, coef.reshape(-1), W, H, 50)
    _refused("jfif_gpu: bad geometry or sample_ratio", jpgx.jfif_gpu, coef, W + 1, H, 50)
    _refused("jfif_gpu: each frame must be contiguous and hold nb + 2 nbc blocks", jpgx.jfif_gpu, coef[:, :-64], W, H, 50)
    _refused("jfif_gpu: 16-byte aligned frames, a stride of whole blocks", jpgx.jfif_gpu,
             torch.zeros((NF, 12 * 64 + 8), dtype=torch.int16, device=cuda)[:, :12 * 64], W, H, 50)
