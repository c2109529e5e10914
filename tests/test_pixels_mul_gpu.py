"""The pixel kernels' choice of multiplier (csrc/jpgx_pixels.hip: px_lane, px_lane_gray, px_transform;
DESIGN.md 4.9): pass 1 runs on the 24-bit multiplier where no table entry is above 63 and otherwise, run
by run, where a vote over the wave finds every dequantised value inside 16 bits.  The host twin computes
the contract whichever multiplier a kernel would choose, so these are frames on which a wrong choice
shows (tests/pixels_cases.py): tables just above the threshold and split at it, and under a table of 1024
one large coefficient over a small background -- in every load lane, in every channel of every kernel, in
every run of rows of 33 and 66 blocks, the tail runs included.  Every frame's guard, that a model of the
24-bit multiplier gives other pixels than the contract in the block that holds the large value, is
checked before any device call.  Raw calls on both libraries; everything is == the host twin, and the
prefill around the frames stays."""
import numpy as np
import pytest

import jpgx
import pixels_cases as P

gpu = pytest.mark.gpu
FILL = 0x7A
MUL = P.multiplier_cases()


def _call(L, cuda, case, channels):
    """one raw call over the case's frames: the whole prefilled output [n][H * pitch + 64] and the pitch"""
    import torch
    kind, W, H, sr = case["kind"], case["W"], case["H"], case["sr"]
    coefs = np.ascontiguousarray(case["coefs"], np.int16).reshape(len(case["coefs"]), -1)
    n, per = coefs.shape
    d_coef = torch.from_numpy(coefs).to(cuda)
    qts = np.ascontiguousarray(case["qts"], np.uint16)
    d_qt = torch.from_numpy(qts.view(np.int16)).to(cuda)
    bpp = channels if kind == "gray" else 3
    pitch = (bpp * W + 7) // 8 * 8 + 8
    ostride = H * pitch + 64
    out = torch.full((n, ostride), FILL, dtype=torch.uint8, device=cuda)
    if kind == "gray":
        rc = L.jpgx_pixels_gpu_gray(d_coef.data_ptr(), per, n, W, H, d_qt.data_ptr(), 64, None, out.data_ptr(), pitch,
                                    ostride, channels, None)
    else:
        size, run = ((L.jpgx_pixels_gpu_any_workspace_size, L.jpgx_pixels_gpu_any) if kind == "any" else
                     (L.jpgx_pixels_gpu_workspace_size, L.jpgx_pixels_gpu))
        need = size(W, H, sr, n)
        assert (need == 0) == (sr == 0)
        ws = torch.full((max(need, 16),), 0xEE, dtype=torch.uint8, device=cuda)
        rc = run(d_coef.data_ptr(), per, n, W, H, sr, d_qt.data_ptr(), 128, None, out.data_ptr(), pitch, ostride,
                 ws.data_ptr() if need else None, need, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy(), pitch, bpp


@gpu
@pytest.mark.parametrize("which", ["product", "alt"])
@pytest.mark.parametrize("name", [m[0] for m in MUL])
def test_the_multiplier_is_chosen_block_by_block(cuda, which, name):
    case, channels = next(m[1:] for m in MUL if m[0] == name)
    L = jpgx.lib if which == "product" else jpgx.alt_library()
    W, H = case["W"], case["H"]
    for k in range(len(case["names"])):                  # before any device call
        assert P.tells(case, k), (name, case["names"][k])
    buf, pitch, bpp = _call(L, cuda, case, channels)
    for k, what in enumerate(case["names"]):
        rows = buf[k, :H * pitch].reshape(H, pitch)
        assert (rows[:, bpp * W:] == FILL).all() and (buf[k, H * pitch:] == FILL).all(), (name, what)
        want = P.host_pixels(case, k, channels)
        assert np.array_equal(rows[:, :bpp * W].reshape(want.shape), want), (name, what)
