"""The seams of the device JFIF decoder (csrc/jpgx_jfif_dec.hip, csrc/jx_jd_sub_body.h, csrc/jx_jfif_sub.h;
DESIGN.md 6, "The device decoder's seams"): what k_jd_sub / k_jd_sub_gray carry from one tile of 8,192
bytes to the next (the true state, cz, the block ordinal), the 16 halo bytes, the bare-FF check at a
tile's last byte, the load's 16 alignments, the rounds' bound, the DC predictors' chunks of 256 blocks,
k_jd_frame's passes of 256 chunks and the gray kernel's grid stride.

Every input is a case of tests/jfif_dec_seams.py, built and guarded there on the CPU before the device
is called (tests/test_jfif_dec_seams.py runs the same guards without a GPU, and holds the host twin to
the reader on the same bytes).  The oracle is the host reader, jpgx.compat.read_jfif / read_jfif_gray,
for status, coefficients and tables; every comparison is ==.  Every case goes through both scan kernels
(k_jd_scan and k_jd_sub, or their _gray forms), through the C entry points, with sentinels behind every
frame's coefficients.  The refusals are the decoder's ordinary error path with the host's status, no
faults.  Nothing here needs Pillow."""
import numpy as np
import pytest

import gray_cases as G
import jfif_dec_seams as D
import jpgx
from gpu_files import upload
from jfif_inputs import nblocks

gpu = pytest.mark.gpu
SCAN = jpgx.EJFIF_SCAN
CFILL, SLACK = 0x5A5A, 3 * 64
KERNELS = pytest.mark.parametrize("sub", [False, True], ids=["lanes", "subinterval"])
# what lies behind `len` in a file's slot: a read past the end that influences a decode shows as a difference
FILLS = pytest.mark.parametrize("fill", [0x00, 0xFF], ids=["00", "ff"])


def _decode(cuda, files, W, H, sr, sub, fill=0xA5, stride=None, before=None):
    """one call of jpgx_jfif_decode_gpu_ex (sr None: jpgx_jfif_decode_gpu_gray) on the files, the slots
    filled with `fill` behind them -> (coef [n][blocks][64], qt, status), the sentinels checked"""
    import torch
    L, n = jpgx.lib, len(files)
    stride = stride or max(len(f) for f in files) + 3 * D.HALO     # `fill` behind every file, the longest too
    d_files, lens = upload(cuda, files, stride, fill)
    if before:
        before(d_files.data_ptr())
    gray = sr is None
    per = 64 * (G.nblocks(W, H) if gray else nblocks(W, H, sr)[0] + 2 * nblocks(W, H, sr)[1])
    coef = torch.full((n, per + SLACK), CFILL, dtype=torch.int16, device=cuda)
    qt = torch.zeros((n, 64) if gray else (n, 2, 64), dtype=torch.uint16, device=cuda)
    status = torch.full((n,), 77, dtype=torch.int32, device=cuda)
    flags = jpgx.JFIF_DECODE_SUBINTERVAL if sub else 0
    if gray:
        need = L.jpgx_jfif_decode_gpu_gray_workspace_size(W, H, n, stride, flags)
    else:
        need = L.jpgx_jfif_decode_gpu_workspace_size_ex(W, H, sr, n, stride, flags)
    assert need > 0
    ws = torch.full((need,), 0xEE, dtype=torch.uint8, device=cuda)
    args = (coef.data_ptr(), per + SLACK, qt.data_ptr(), status.data_ptr(), ws.data_ptr(), need, None)
    if gray:
        rc = L.jpgx_jfif_decode_gpu_gray(d_files.data_ptr(), stride, lens.data_ptr(), n, W, H, flags, *args)
    else:
        rc = L.jpgx_jfif_decode_gpu_ex(d_files.data_ptr(), stride, lens.data_ptr(), n, W, H, sr, flags, *args)
    assert rc == 0
    torch.cuda.synchronize()
    got = coef.cpu().numpy()
    assert (got[:, per:] == CFILL).all()             # nothing behind a frame's coefficients
    return got[:, :per].reshape(n, -1, 64), qt.view(torch.int16).cpu().numpy().view(np.uint16), status.cpu().numpy()


def _host(c):
    if not hasattr(c, "_host"):
        c._host = D.host(c)
    return c._host


def _check(cuda, cases, sub, **kw):
    """the cases, all of one geometry, as one batch: every status, and every accepted frame's coefficients
    and tables, == the host reader's"""
    c0 = cases[0]
    assert all((c.W, c.H, c.sr) == (c0.W, c0.H, c0.sr) for c in cases)
    coef, qt, status = _decode(cuda, [c.data for c in cases], c0.W, c0.H, c0.sr, sub, **kw)
    for k, c in enumerate(cases):
        rc, want, wqt = _host(c)
        assert rc == c.rc and status[k] == rc, (k, c.note, status[k], rc)
        if rc == 0:
            assert np.array_equal(coef[k], want), (k, c.note)
            assert np.array_equal(qt[k], wqt), (k, c.note)
            if c.want is not None:
                assert np.array_equal(coef[k], c.want), (k, c.note)
    return status


# ---- 1, 2, 3, 5: stuffing on a seam, the halo, the carried states, interval lengths ------------------------------
@gpu
@KERNELS
@FILLS
@pytest.mark.parametrize("name", sorted(D.SEAM_CASES))
def test_seam_case(cuda, name, fill, sub):
    c = D.guarded(D.SEAM_CASES[name]())
    assert _check(cuda, [c], sub, fill=fill).tolist() == [0]


# ---- 4, 5: refusals on a seam, between two good files --------------------------------------------------------------
@gpu
@KERNELS
@FILLS
@pytest.mark.parametrize("name", D.REFUSALS)
def test_refusal_between_two_good_files(cuda, name, fill, sub):
    bad, good = D.refusals()[name]
    D.guarded(bad)
    D.guarded(good)
    assert _check(cuda, [good, bad, good], sub, fill=fill).tolist() == [0, SCAN, 0]


# ---- 6: all 16 load alignments -------------------------------------------------------------------------------------
@gpu
@KERNELS
@pytest.mark.parametrize("which", ["three tiles", "short intervals"])
def test_sixteen_alignments(cuda, which, sub):
    c = D.guarded(D.ff_case("ff_then_seam") if which == "three tiles" else D.short_case())
    stride = D.odd_stride(len(c.data))
    status = _check(cuda, [c] * D.COPIES, sub, stride=stride, before=lambda base: D.guard_residues(base, stride, c))
    assert not status.any()


# ---- 7: most rounds --------------------------------------------------------------------------------------------------
@gpu
@KERNELS
def test_most_rounds(cuda, sub):
    c = D.guarded(D.rounds_case())
    assert _check(cuda, [c], sub).tolist() == [0]
    assert np.array_equal(_host(c)[1], D.maximal(c.W, c.H))


# ---- 8: the DC predictors' chunks ------------------------------------------------------------------------------------
@gpu
@KERNELS
@pytest.mark.parametrize("sr,n", D.DC_SHAPES)
def test_dc_chunks(cuda, sr, n, sub):
    """per shape one batch: differences nonzero throughout; every component held at 32767 and at -32768
    over its block 255 | 256; per component and sign the step that only the carry takes out of int16"""
    cases = [D.guarded(D.dc_case(sr, n, v)) for v in D.dc_variants(sr)]
    want = [0, 0, 0] + [SCAN] * (len(cases) - 3)
    assert [c.rc for c in cases] == want
    assert _check(cuda, cases, sub).tolist() == want


# ---- 9: k_jd_frame's passes --------------------------------------------------------------------------------------------
@gpu
@KERNELS
def test_markers_behind_the_first_and_second_pass_of_chunks(cuda, sub):
    c = D.guarded(D.passes_case())
    assert _check(cuda, [c, c.small], sub, stride=c.stride).tolist() == [0, 0]


# ---- 10: the gray kernel's grid stride -----------------------------------------------------------------------------------
@gpu
@KERNELS
def test_more_gray_intervals_than_workgroups(cuda, sub):
    c = D.guarded(D.grid_case())
    assert _check(cuda, [c], sub).tolist() == [0]
