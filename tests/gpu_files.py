"""Test helper of the GPU tests that decode files: the one upload of host files into a device batch, and
what tests/test_jfif_decode_gpu.py and tests/test_jfif_decode_sub_gpu.py share -- the host decoder
(jpgx.compat.read_jfif) as the oracle of a batch and of a round trip through the device coder."""
import numpy as np

import jpgx
import jpgx.compat as C

SLOT_FILL = 0xA5        # what the two decoder test files put behind a file in its slot


def upload(cuda, files, stride=None, fill=0):
    """host files -> (d_files uint8 [n][stride], lens int64 [n]) on cuda: file k at the start of row k,
    `fill` behind it; stride: bytes per row (default: the longest file's length)"""
    import torch
    stride = stride or max(len(f) for f in files)
    buf = np.full((len(files), stride), fill, np.uint8)
    for k, f in enumerate(files):
        buf[k, :len(f)] = np.frombuffer(f, np.uint8)
    return torch.from_numpy(buf).to(cuda), torch.tensor([len(f) for f in files], dtype=torch.int64, device=cuda)


def host(data):
    """(status, coef [nblk][64] or None, qt or None) of the host decoder"""
    try:
        r = C.read_jfif(data, 1)
    except jpgx.JpgxError as e:
        return e.rc, None, None
    return 0, r["coef"].reshape(-1, 64), r["qt"]


def check_batch(cuda, files, W, H, sr, stride=None, subinterval=False):
    """decodes the files as one batch and compares every frame with the host decoder"""
    d_files, lens = upload(cuda, files, stride, SLOT_FILL)
    coef, qt, status = jpgx.jfif_decode_gpu(d_files, lens, W, H, sr, subinterval=subinterval)
    coef, qt, status = coef.cpu().numpy(), qt.cpu().numpy(), status.cpu().numpy()
    for k, f in enumerate(files):
        rc, want, wqt = host(f)
        assert status[k] == rc, (k, status[k], rc)
        if rc == 0:
            assert np.array_equal(coef[k], want), k
            assert np.array_equal(qt[k], wqt), k
    return status


def roundtrip(cuda, coef, W, H, q, sr, rr, optimize=False, subinterval=False):
    """jfif_decode_gpu(*jfif_gpu(coef)): the coder's outputs passed on unchanged"""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(coef, np.int16)).to(cuda).reshape(1, -1)
    out, lens = jpgx.jfif_gpu(d, W, H, q, sr, rr, optimize=optimize)
    got, qt, status = jpgx.jfif_decode_gpu(out, lens, W, H, sr, subinterval=subinterval)
    data = out[0, :int(lens[0])].cpu().numpy().tobytes()
    rc, want, wqt = host(data)
    assert rc == 0 and int(status[0]) == 0
    assert np.array_equal(got[0].cpu().numpy(), want)
    assert np.array_equal(qt[0].cpu().numpy(), wqt)
    return got[0].cpu().numpy()
