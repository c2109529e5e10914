"""The device decoder that works inside a restart interval (csrc/jpgx_jfif_dec.hip: k_jd_sub behind
JPGX_JFIF_DECODE_SUBINTERVAL; jpgx.jfif_decode_gpu(..., subinterval=True)).

The oracle everywhere is the host decoder on the same bytes, jpgx.compat.read_jfif, for the
coefficients, the tables and the status alike, as in tests/test_jfif_decode_gpu.py; every comparison
is ==.  The inputs that make the mechanism work are those of tests/test_jfif_read_sub.py
(tests/jfif_sub_cases.py), uploaded as they are."""
import functools

import numpy as np
import pytest

import gpu_files
import jfif_san_cases as S
import jfif_sub_cases as K
import jpgx
import jpgx.compat as C
from gpu_files import host as _host
from jfif_inputs import hand_made, lap as _lap, nblocks as _nblocks, stuffing_heavy

gpu = pytest.mark.gpu
HEADER, SCAN = jpgx.EJFIF_HEADER, jpgx.EJFIF_SCAN
SUB = jpgx.JFIF_DECODE_SUBINTERVAL


_upload = functools.partial(gpu_files.upload, fill=gpu_files.SLOT_FILL)
_check_batch = functools.partial(gpu_files.check_batch, subinterval=True)
_roundtrip = functools.partial(gpu_files.roundtrip, subinterval=True)


# ---- round trips ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_round_trip(cuda, sr, optimize):
    for H in (64, 80 if sr == 2 else 72):
        for rr in (-1, 1, 2, 3):
            coef = _lap(64, H, sr, 100 * sr + H + rr)
            got = _roundtrip(cuda, coef, 64, H, 75, sr, rr, optimize)
            assert np.array_equal(got, coef)         # inside the coder's clamps: the input comes back


@gpu
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_hand_made_blocks(cuda, sr):
    for rr, opt in ((1, False), (2, True)):
        _roundtrip(cuda, hand_made(sr, 64, 32)[2], 64, 32, 50, sr, rr, opt)


@gpu
@pytest.mark.parametrize("sr", [0, 2])
def test_stuffing_heavy_frame(cuda, sr):
    _roundtrip(cuda, stuffing_heavy(sr, 64, 96)[3], 64, 96, 50, sr, 1)


@gpu
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257])
def test_interval_counts(cuda, rows):
    W, H = 16, 8 * rows
    coef = _lap(W, H, 0, rows)
    assert np.array_equal(_roundtrip(cuda, coef, W, H, 60, 0, 1), coef)


@gpu
def test_two_thousand_intervals_of_a_subsequence_or_two(cuda):
    """tests/test_jfif_decode_gpu.py's 8 x 16000 frame of 2,000 one-MCU intervals as its 16-frame batch:
    more intervals than workgroups stride over, one or two subsequences each"""
    from test_jfif_decode_gpu import _boundary_case
    W, H, coef, files, _ = _boundary_case()
    lengths = [e - b for b, e in K.intervals(files[0])]
    assert len(lengths) == 2000 and 0 < min(lengths) < K.SUB and max(lengths) < 2 * K.SUB
    status = _check_batch(cuda, files, W, H, 0)
    assert not status.any()
    assert np.array_equal(_host(files[7])[1], coef)


# ---- the inputs that make the mechanism work, as the host twin decoded them ----------------------------
@gpu
def test_mechanism_inputs(cuda):
    inputs = K.mechanism_inputs()
    assert {"stuffing, no intervals", "three tiles", "short intervals", "a whole multiple"} <= set(inputs)
    stats = C.read_jfif_sub(inputs["three tiles"][3])["stats"]
    assert stats["tiles"] >= 3 and stats["units_across_tile"] > 0 and stats["rounds_max"] >= 3
    for name, (W, H, sr, data) in inputs.items():
        status = _check_batch(cuda, [data], W, H, sr)
        assert status.tolist() == [0], name
    # a batch of files without restart intervals: the three-tile file, a corruption in its third tile
    # between two good copies, and one cut short
    big, pos, val = K.late_tile_flip()
    status = _check_batch(cuda, [big, S.flipped(big, pos, val), big, big[:30000] + b"\xff\xd9"], K.BIG_W, K.BIG_H, 0)
    assert status.tolist() == [0, SCAN, 0, SCAN]


# ---- batches ----------------------------------------------------------------------------------------
def _raw(d_files, fstride, lens, nf, W, H, sr, coef, cstride, qt, status, flags=SUB):
    import torch
    need = jpgx.lib.jpgx_jfif_decode_gpu_workspace_size_ex(W, H, sr, nf, fstride, flags)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=coef.device)
    rc = jpgx.lib.jpgx_jfif_decode_gpu_ex(d_files.data_ptr(), fstride, lens.data_ptr(), nf, W, H, sr, flags,
                                          coef.data_ptr(), cstride, qt.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                          need, None)
    torch.cuda.synchronize()
    return rc


@gpu
def test_batch_with_padded_strides_and_a_bad_frame(cuda):
    import torch
    W, H, sr = 96, 64, 1
    nb, nbc = _nblocks(W, H, sr)
    per = (nb + 2 * nbc) * 64
    frames = [_lap(W, H, sr, 200 + k, scale=4.0 + 3 * k) for k in range(4)]
    files = [C.write_jfif_ex(c, W, H, 60, sr, restart_rows=2, nthreads=1) for c in frames]
    scan = C.jfif_info(files[1])["scan_offset"]
    good = files[1]                                  # the frame in the middle: the first bit flip from
    for at in range(scan + 40, len(good) - 2):       # here on that the host decoder refuses
        files[1] = S.flipped(good, at, good[at] ^ 0x10)
        if _host(files[1])[0] != 0:
            break
    bad_rc = _host(files[1])[0]
    assert bad_rc == SCAN
    fstride = max(len(f) for f in files) + 37
    d_files, lens = _upload(cuda, files, fstride)
    lens = torch.tensor([len(f) for f in files[:3]] + [len(files[3]) - (1 << 63)], dtype=torch.int64).to(cuda)
    assert int(lens[3]) < 0                          # bit 63: an overflow report of the coder, passed on
    cstride = per + 5 * 64
    coef = torch.full((4, cstride), 0x5A5A, dtype=torch.int16, device=cuda)
    qt = torch.zeros((4, 2, 64), dtype=torch.uint16, device=cuda)
    status = torch.full((4,), 77, dtype=torch.int32, device=cuda)
    assert _raw(d_files, fstride, lens, 4, W, H, sr, coef, cstride, qt, status) == 0
    got, st = coef.cpu().numpy(), status.cpu().numpy()
    assert st.tolist() == [0, bad_rc, 0, HEADER]
    for k in (0, 2):
        assert np.array_equal(got[k, :per].reshape(-1, 64), frames[k])
        assert np.array_equal(qt[k].cpu().numpy(), _host(files[k])[2])
    assert (got[:, per:] == 0x5A5A).all()            # nothing outside a frame's coefficients
    assert (got[3, :per] == 0x5A5A).all()            # a refused header decodes nothing


@gpu
def test_flags_zero_is_the_plain_call(cuda):
    import torch
    W, H, sr = 64, 64, 2
    nb, nbc = _nblocks(W, H, sr)
    per = (nb + 2 * nbc) * 64
    files = [C.write_jfif_ex(_lap(W, H, sr, 400 + k), W, H, 70, sr, restart_rows=1, nthreads=1) for k in range(3)]
    files[1] = files[1][:len(files[1]) // 2]
    stride = max(len(f) for f in files)
    d_files, lens = _upload(cuda, files, stride)
    outs = []
    for which in ("plain", 0, SUB):
        coef = torch.zeros((3, per), dtype=torch.int16, device=cuda)
        qt = torch.zeros((3, 2, 64), dtype=torch.uint16, device=cuda)
        status = torch.full((3,), 77, dtype=torch.int32, device=cuda)
        if which == "plain":
            need = jpgx.lib.jpgx_jfif_decode_gpu_workspace_size(W, H, sr, 3, stride)
            assert need == jpgx.lib.jpgx_jfif_decode_gpu_workspace_size_ex(W, H, sr, 3, stride, 0)
            ws = torch.empty(need, dtype=torch.uint8, device=cuda)
            assert jpgx.lib.jpgx_jfif_decode_gpu(d_files.data_ptr(), stride, lens.data_ptr(), 3, W, H, sr, coef.data_ptr(),
                                                 per, qt.data_ptr(), status.data_ptr(), ws.data_ptr(), need, None) == 0
            torch.cuda.synchronize()
        else:
            assert _raw(d_files, stride, lens, 3, W, H, sr, coef, per, qt, status, flags=which) == 0
        outs.append((coef.cpu().numpy(), qt.cpu().numpy(), status.cpu().tolist()))
    assert outs[0][2] == outs[1][2] == outs[2][2] == [0, SCAN, 0]
    for k in (0, 2):
        for o in outs[1:]:
            assert np.array_equal(o[0][k], outs[0][0][k]) and np.array_equal(o[1][k], outs[0][1][k])
        assert np.array_equal(outs[0][0][k].reshape(-1, 64), _host(files[k])[1])
    assert np.array_equal(outs[1][1], outs[0][1])    # the tables of all three frames, the refused one's too


@gpu
def test_graph_capture(cuda):
    """the call captured once on a single stream, replayed over two sets of files swapped in place"""
    import torch
    W, H, sr = 64, 64, 2
    nb, nbc = _nblocks(W, H, sr)
    per = (nb + 2 * nbc) * 64
    sets = [[C.write_jfif_ex(_lap(W, H, sr, 300 + 2 * s + k), W, H, 70, sr, restart_rows=k, nthreads=1,
                             optimize=bool(k)) for k in range(2)] for s in range(2)]
    stride = max(len(f) for fs in sets for f in fs)
    ups = [_upload(cuda, fs, stride) for fs in sets]
    d_files, lens = ups[0][0].clone(), ups[0][1].clone()
    coef = torch.zeros((2, per), dtype=torch.int16, device=cuda)
    qt = torch.zeros((2, 2, 64), dtype=torch.uint16, device=cuda)
    status = torch.full((2,), 77, dtype=torch.int32, device=cuda)
    need = jpgx.lib.jpgx_jfif_decode_gpu_workspace_size_ex(W, H, sr, 2, stride, SUB)
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    st = torch.cuda.Stream()

    def call():
        rc = jpgx.lib.jpgx_jfif_decode_gpu_ex(d_files.data_ptr(), stride, lens.data_ptr(), 2, W, H, sr, SUB,
                                              coef.data_ptr(), per, qt.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                              need, st.cuda_stream)
        assert rc == 0

    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        call()                                       # once eagerly: nothing is left to initialise
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        call()
    torch.cuda.synchronize()
    for s in (1, 0):
        d_files.copy_(ups[s][0])
        lens.copy_(ups[s][1])
        coef.fill_(0x5A5A)                           # the call zeroes what it does not write
        status.fill_(77)
        ws.fill_(0xEE)                               # the call initialises what it reads of the workspace
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0, 0]
        for k in range(2):
            assert np.array_equal(coef[k].cpu().numpy().reshape(-1, 64), _host(sets[s][k])[1])


# ---- refusals on the device: inputs of the two sanitizer sweeps ------------------------------------------
@gpu
def test_corrupt_inputs_of_the_sanitizer_sweeps(cuda):
    """tests/test_jfif_decode_gpu.py's three corrupt inputs (a truncation inside the scan, an undefined
    code, a dropped RSTm of tests/c/jfif_read_san.c's 16x16 file, which tests/c/jfif_sub_san.c sweeps
    too) and one corruption of jfif_sub_san.c's three-tile file that lies in its third tile.  The gates
    are the CPU tests test_jfif_read.py::test_decoder_under_asan_ubsan and
    test_jfif_read_sub.py::test_twin_under_asan_ubsan, which hold the programs' files and corruptions
    to the constants checked here: the shared routines have decoded these very bytes under
    AddressSanitizer where those tests have passed on the same tree.  No sanitizer runs here.  This is
    the refusal path, not a fault: the device's status is the host's."""
    idx = S.GPU_FILE[0]
    data, W, H, sr, _ = S.file_of(idx)
    assert (W, H, sr) == (16, 16, 0) and (len(data), S.fnv1a(data)) == S.GPU_FILE[1:]
    scan = C.jfif_info(data)["scan_offset"]
    pos, val = S.GPU_FLIP
    assert (pos, val) in S.flips(idx, data, S.FLIPS) and scan <= pos < len(data) - 2
    files = [data, data[:scan + (len(data) - scan) // 2], S.flipped(data, pos, val), S.drop_first_rst(data)]
    assert [_host(f)[0] for f in files] == [0, SCAN, SCAN, SCAN]
    assert _check_batch(cuda, files, W, H, sr).tolist() == [0, SCAN, SCAN, SCAN]
    big, _ = K.big_file()
    assert (len(big), S.fnv1a(big)) == K.BIG_FILE
    pos, val = K.BIG_FLIP
    first = K.intervals(big)[0][0]
    assert (pos, val) in S.flips(K.BIG, big, K.BIG_FLIPS) and first + 2 * 64 * 256 <= pos < len(big) - 2
    files = [big, S.flipped(big, pos, val)]
    assert [_host(f)[0] for f in files] == [0, SCAN]
    assert _check_batch(cuda, files, K.BIG_W, K.BIG_H, 0).tolist() == [0, SCAN]


# ---- other routes in ---------------------------------------------------------------------------------
@gpu
def test_decode_jpeg_of_a_pillow_file(cuda):
    Image = pytest.importorskip("PIL.Image")
    import io
    data = K.pillow_tiger(2, 90)
    want = jpgx.decode_jpeg(data, cuda).cpu().numpy()
    got = jpgx.decode_jpeg(data, cuda, subinterval=True).cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(got, np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
    a = jpgx.decode_jpeg_coefficients(data, cuda, subinterval=True)
    b = jpgx.decode_jpeg_coefficients(data, cuda)
    assert np.array_equal(a["coef"].cpu().numpy(), b["coef"].cpu().numpy())
    assert np.array_equal(a["coef"].cpu().numpy(), C.read_jfif(data)["coef"])
    with pytest.raises(jpgx.JpgxError) as e:
        jpgx.decode_jpeg_coefficients(data[:-2], cuda, subinterval=True)
    assert e.value.rc == SCAN
