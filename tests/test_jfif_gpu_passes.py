"""The device JFIF coder's multi-pass paths (csrc/jpgx_jfif.hip).  Its kernels work in passes of 256
lanes and carry state from one pass to the next: a running bit offset over an interval's blocks and
the word two passes share (k_jf_len, k_jf_count, k_jf_pack), the 0xFF bytes already stuffed over an
interval's bytes, 4,096 to a pass (k_jf_stuff), 64-bit places over a frame's intervals (k_jf_place,
k_jf_frame).  The inputs here put something at every such seam: more than 512 blocks, more than
4,096 bytes and more than 256 intervals, with the content that strains the carry at the seam itself.

Every input is a case of tests/jfif_bits.py: built and guarded there, on the CPU, before the device is
called (tests/test_jfif_bits.py runs the same guards without a GPU).  The oracle is the host writer on
one thread, == on bytes; the bytes are then decoded by tests/jfif_decode.py back to the clamped
coefficients, so that a mistake in the walk host and device share cannot cancel out.  No tolerances."""
import numpy as np
import pytest

import jfif_bits as B
import jpgx
import jpgx.compat as C
from jfif_decode import decode

gpu = pytest.mark.gpu
MODES = pytest.mark.parametrize("optimize", [False, True], ids=["std", "opt"])
SENTINEL = 0xA5


def _flat(planes):
    return np.concatenate([np.asarray(x).reshape(-1, 64) for x in planes])


def _dev(cuda, a):
    import torch
    return torch.from_numpy(np.array(a)).to(cuda)       # a copy: the cases' arrays are read-only


# ---- one frame: the binding ----------------------------------------------------------------------
@gpu
@MODES
@pytest.mark.parametrize("name", sorted(B.PASS_CASES))
def test_bytes_equal_host_writer_and_decode_back(cuda, name, optimize):
    c = B.pass_case(name, optimize)                      # guarded
    out, lens = jpgx.jfif_gpu(_dev(cuda, c.coef).reshape(1, -1), c.W, c.H, 50, c.sr, c.rr, optimize=optimize)
    n = int(lens[0])
    assert 0 < n <= out.shape[1]
    got = out[0, :n].cpu().numpy().tobytes()
    assert got == c.data
    back = _flat(C.read_jfif(got)["coef"]).astype(np.int32)
    if name.startswith("both"):
        # 68,112 blocks take the independent decoder 14 s: the host reader alone (held to that decoder
        # in tests/test_jfif_read.py); Laplacian content lies inside the clamps and comes back as it is
        assert np.array_equal(back, c.coef)
        return
    want = B.coded_values(c.coef, c.W, c.H, c.sr, c.rr)
    assert np.array_equal(_flat(decode(got)["coef"]), want)
    assert np.array_equal(back, want)


# ---- batches: the entry points themselves --------------------------------------------------------
def _raw(entry, d_coef, fstride, nf, W, H, sr, rr, flags, out, ostride, cap, lens, ws=None, ws_cap=0):
    """jpgx_jfif_gpu_ex / jpgx_jfif_gpu_any on torch tensors; returns the workspace, prefilled when new
    (ws_cap: the largest capacity it is going to serve)"""
    import torch
    size_fn = {"ex": jpgx.lib.jpgx_jfif_gpu_workspace_size_ex, "any": jpgx.lib.jpgx_jfif_gpu_any_workspace_size}[entry]
    code_fn = {"ex": jpgx.lib.jpgx_jfif_gpu_ex, "any": jpgx.lib.jpgx_jfif_gpu_any}[entry]
    need = size_fn(W, H, sr, rr, nf, cap, flags)
    assert need > 0
    if ws is None:
        ws = torch.full((max(need, size_fn(W, H, sr, rr, nf, ws_cap, flags)),), 0xEE, dtype=torch.uint8, device=out.device)     # never cleared, and no zeros
    assert ws.numel() >= need
    assert code_fn(d_coef.data_ptr(), fstride, nf, W, H, 50, sr, rr, flags, out.data_ptr(), ostride, cap,
                   lens.data_ptr(), ws.data_ptr(), ws.numel(), None) == 0
    torch.cuda.synchronize()
    return ws


def _batch(cuda, frames, pad=5 * 64):
    """the frames' coefficients at a padded frame stride, the gaps full of another frame's values"""
    import torch
    per = frames[0].size
    d = torch.full((len(frames), per + pad), 32767, dtype=torch.int16, device=cuda)
    for k, f in enumerate(frames):
        assert f.size == per
        d[k, :per] = _dev(cuda, f.reshape(-1))
    return d, per + pad


def _outputs(cuda, nf, cap):
    import torch
    ostride = B.r16(cap) + 48
    out = torch.full((nf, ostride), SENTINEL, dtype=torch.uint8, device=cuda)
    lens = torch.zeros(nf, dtype=torch.int64, device=cuda)
    return out, ostride, lens


KINDS = ("tall_lap_8x2064", "tall_stuffing_8x2064", "tall_zeros_8x2064")


@gpu
@pytest.mark.parametrize("entry,optimize", [("ex", False), ("ex", True), ("any", False)])
def test_batch_of_frames_of_258_intervals(cuda, entry, optimize):
    """three frames of 8 x 2064 (through jpgx_jfif_gpu_any once, stated as 7 x 2061), padded strides,
    sentinels, one never-cleared workspace used twice, the second time with the frames in other slots"""
    cases = [B.pass_case(k, optimize) for k in KINDS]
    W, H = (8, 2064) if entry == "ex" else (7, 2061)
    flags = jpgx.JFIF_OPTIMIZE if optimize else 0
    refs = [c.data for c in cases]
    if entry == "any":
        assert jpgx.coded_size(W, H, 0) == (8, 2064)
        refs = [C.write_jfif_ex(c.coef, W, H, 50, 0, restart_rows=1, nthreads=1, any_size=True) for c in cases]
        assert all(len(a) == len(b) and a != b for a, b in zip(refs, (c.data for c in cases)))
    cap = max(len(r) for r in refs) + 7
    ws = None
    for order in ((0, 1, 2), (2, 0, 1)):
        d, fstride = _batch(cuda, [cases[k].coef for k in order])
        out, ostride, lens = _outputs(cuda, 3, cap)
        ws = _raw(entry, d, fstride, 3, W, H, 0, 1, flags, out, ostride, cap, lens, ws)
        got, n = out.cpu().numpy(), lens.cpu().numpy()
        for slot, k in enumerate(order):
            assert n[slot] == len(refs[k]), (order, slot)
            assert got[slot, :n[slot]].tobytes() == refs[k], (order, slot)
            assert (got[slot, n[slot]:] == SENTINEL).all()


LATE = ("tall_stuffing_8x2064", "lap_64x48_rr1")


def _bound(c):
    """the largest capacity an overflow may report: headers, twice the unstuffed bytes, markers, EOI"""
    hdrlen = B.file_header(c.data)[1]
    return hdrlen + 2 * sum(len(s) for s in c.streams) + 2 * (len(c.streams) - 1) + 2


@gpu
@MODES
@pytest.mark.parametrize("name", LATE)
def test_exact_fit_and_late_overflow(cuda, name, optimize):
    """cap = the file's length fits; one byte less is refused by k_jf_frame, after the packing"""
    c = B.pass_case(name, optimize)
    ref = c.data
    B.guard_late_overflow(c, len(ref) - 1)
    flags = jpgx.JFIF_OPTIMIZE if optimize else 0
    d, fstride = _batch(cuda, [c.coef])
    # the exact fit
    out, ostride, lens = _outputs(cuda, 1, len(ref))
    ws = _raw("ex", d, fstride, 1, c.W, c.H, c.sr, c.rr, flags, out, ostride, len(ref), lens, ws_cap=_bound(c))
    got = out[0].cpu().numpy()
    assert int(lens[0]) == len(ref) and got[:len(ref)].tobytes() == ref and (got[len(ref):] == SENTINEL).all()
    # one byte short
    out, ostride, lens = _outputs(cuda, 1, len(ref) - 1)
    ws = _raw("ex", d, fstride, 1, c.W, c.H, c.sr, c.rr, flags, out, ostride, len(ref) - 1, lens, ws)
    n = int(lens[0])
    assert n < 0                                         # bit 63
    need = n & ((1 << 62) - 1)
    print("file bytes", len(ref), "reported capacity", need, "bound", _bound(c))
    assert len(ref) <= need <= _bound(c)
    assert (out == SENTINEL).all()                       # the whole row
    # the reported capacity suffices
    out, ostride, lens = _outputs(cuda, 1, need)
    _raw("ex", d, fstride, 1, c.W, c.H, c.sr, c.rr, flags, out, ostride, need, lens, ws)
    got = out[0].cpu().numpy()
    assert int(lens[0]) == len(ref) and got[:len(ref)].tobytes() == ref and (got[len(ref):] == SENTINEL).all()


@gpu
@MODES
@pytest.mark.parametrize("name", LATE)
def test_late_overflow_between_two_frames_that_fit(cuda, name, optimize):
    c = B.pass_case(name, optimize)
    if name.startswith("tall"):
        sides = [B.pass_case("tall_lap_8x2064", optimize), B.pass_case("tall_zeros_8x2064", optimize)]
    else:
        from jfif_inputs import lap
        sides = [B.Case(c.W, c.H, c.sr, c.rr, lap(c.W, c.H, c.sr, seed, scale=2.0), optimize) for seed in (31, 33)]
    cases = [sides[0], c, sides[1]]
    cap = len(c.data) - 1
    B.guard_late_overflow(c, cap)
    assert all(len(s.data) < cap for s in sides)
    flags = jpgx.JFIF_OPTIMIZE if optimize else 0
    d, fstride = _batch(cuda, [x.coef for x in cases])
    out, ostride, lens = _outputs(cuda, 3, cap)
    _raw("ex", d, fstride, 3, c.W, c.H, c.sr, c.rr, flags, out, ostride, cap, lens)
    got, n = out.cpu().numpy(), lens.cpu().numpy()
    for k in (0, 2):
        assert n[k] == len(cases[k].data) and got[k, :n[k]].tobytes() == cases[k].data
        assert (got[k, n[k]:] == SENTINEL).all()
    assert n[1] < 0 and len(c.data) <= (int(n[1]) & ((1 << 62) - 1)) <= _bound(c)
    assert (got[1] == SENTINEL).all()


# ---- there and back on the device ----------------------------------------------------------------
@gpu
@MODES
@pytest.mark.parametrize("subinterval", [False, True], ids=["lanes", "subinterval"])
@pytest.mark.parametrize("name", ["seam_stuffing_444", "tall_stuffing_8x4112"])
def test_device_decoder_reads_the_device_coder_s_file(cuda, name, subinterval, optimize):
    """one interval of 528 blocks and tens of thousands of stuffed bytes; 514 intervals"""
    c = B.pass_case(name, optimize)
    out, lens = jpgx.jfif_gpu(_dev(cuda, c.coef).reshape(1, -1), c.W, c.H, 50, c.sr, c.rr, optimize=optimize)
    coef, qt, status = jpgx.jfif_decode_gpu(out, lens, c.W, c.H, c.sr, subinterval=subinterval)
    assert status.cpu().tolist() == [0]
    want = C.read_jfif(c.data)
    assert np.array_equal(coef[0].cpu().numpy(), _flat(want["coef"]))
    assert np.array_equal(qt[0].cpu().numpy(), want["qt"])
