"""The device JFIF decoder (csrc/jpgx_jfif_dec.hip: jpgx_jfif_decode_gpu, jpgx.jfif_decode_gpu,
jpgx.decode_jpeg_coefficients).

The oracle everywhere is the host decoder on the same bytes, jpgx.compat.read_jfif (itself checked
against the independent decoder in tests/test_jfif_read.py), for the coefficients, the tables and
the status alike; every comparison is ==.  (4:2:0 cases use 64x80 where the others use 64x72: a
4:2:0 MCU is 16 rows high.)"""
import functools

import numpy as np
import pytest

import gpu_files
import jfif_san_cases as S
import jpgx
import jpgx.compat as C
from gpu_files import check_batch as _check_batch, host as _host, roundtrip as _roundtrip
from jfif_decode import decode
from jfif_inputs import hand_made, lap as _lap, nblocks as _nblocks, stuffing_heavy

gpu = pytest.mark.gpu
HEADER, SCAN = jpgx.EJFIF_HEADER, jpgx.EJFIF_SCAN
# csrc/jpgx_jfif_dec.hip: a lane of the marker search takes PIECE bytes, a workgroup CHUNK bytes
PIECE, CHUNK = 16, 4096


_upload = functools.partial(gpu_files.upload, fill=gpu_files.SLOT_FILL)


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
    import torch
    coef = stuffing_heavy(sr, 64, 96)[3]
    d = torch.from_numpy(coef).to(cuda).reshape(1, -1)
    out, lens = jpgx.jfif_gpu(d, 64, 96, 50, sr, 1)
    data = out[0, :int(lens[0])].cpu().numpy().tobytes()
    scan = data[C.jfif_info(data)["scan_offset"]:-2]
    endings = sum(scan.count(b"\xff\x00\xff" + bytes([0xd0 + m])) for m in range(8))
    assert scan.count(b"\xff\x00") >= 1000 and endings >= 1      # stuffed FF 00 next to markers
    _roundtrip(cuda, coef, 64, 96, 50, sr, 1)


@gpu
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257])
def test_interval_counts_around_the_wave_size(cuda, rows):
    """one-wave workgroups of the scan kernel: 1, 63, 64, 65 and 257 intervals (lanes)"""
    W, H = 16, 8 * rows
    coef = _lap(W, H, 0, rows)
    got = _roundtrip(cuda, coef, W, H, 60, 0, 1)
    assert np.array_equal(got, coef)


# ---- batches ----------------------------------------------------------------------------------------
def _raw(d_files, fstride, lens, nf, W, H, sr, coef, cstride, qt, status):
    import torch
    need = jpgx.lib.jpgx_jfif_decode_gpu_workspace_size(W, H, sr, nf, fstride)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=coef.device)
    rc = jpgx.lib.jpgx_jfif_decode_gpu(d_files.data_ptr(), fstride, lens.data_ptr(), nf, W, H, sr, coef.data_ptr(),
                                       cstride, qt.data_ptr(), status.data_ptr(), ws.data_ptr(), need, None)
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
def test_stated_geometry_must_be_the_file_s(cuda):
    f = C.write_jfif_ex(_lap(64, 64, 0, 1), 64, 64, 50, 0, restart_rows=1, nthreads=1)
    g = C.write_jfif_ex(_lap(64, 64, 1, 1), 64, 64, 50, 1, restart_rows=1, nthreads=1)
    d_files, lens = _upload(cuda, [f, g, f[:100]])
    for W, H, sr, want in ((64, 64, 0, [0, HEADER, HEADER]), (64, 64, 1, [HEADER, 0, HEADER]),
                           (64, 72, 0, [HEADER] * 3), (128, 64, 0, [HEADER] * 3)):
        _, _, status = jpgx.jfif_decode_gpu(d_files, lens, W, H, sr)
        assert status.cpu().tolist() == want, (W, H, sr)


# ---- the marker search's boundaries ------------------------------------------------------------------
def _boundary_case():
    """an 8-pixel-wide frame of 2000 one-MCU intervals and its 16 files whose COM segment grows by
    0 .. 15 bytes, for the first seed at which, somewhere in the batch: a restart marker's FF is the
    last byte of a lane's piece, one is the last byte of a chunk, and a stuffed FF 00 straddles each
    of the two boundaries"""
    W, H = 8, 16000
    for seed in range(64):
        rng = np.random.default_rng(seed)
        coef = rng.laplace(0, 0.4, size=(3 * 2000, 64)).astype(np.int16)
        big = rng.random(coef.shape) < 0.004
        coef[big] = rng.choice(np.array([1023, -1023, 511, -1, 255], np.int16), int(big.sum()))
        coef[:, 0] = rng.integers(-300, 300, size=coef.shape[0])
        base = C.write_jfif_ex(coef, W, H, 50, 0, restart_rows=1, nthreads=1)
        files = [base[:2] + b"\xff\xfe" + (3 + k).to_bytes(2, "big") + b"c" * (1 + k) + base[2:] for k in range(16)]
        scan = C.jfif_info(base)["scan_offset"]
        b = np.frombuffer(base, np.uint8)
        ff = np.flatnonzero(b[scan:-2] == 0xFF) + scan
        marks = ff[(b[ff + 1] & 0xF8) == 0xD0]
        stuffed = ff[b[ff + 1] == 0]
        assert marks.size == 1999
        hit = {"marker, piece": 0, "marker, chunk": 0, "stuffed, piece": 0, "stuffed, chunk": 0}
        for k in range(16):
            shift = 5 + k                            # the COM segment's bytes in front
            for name, pos in (("marker", marks), ("stuffed", stuffed)):
                hit[name + ", piece"] += int(((pos + shift) % PIECE == PIECE - 1).sum())
                hit[name + ", chunk"] += int(((pos + shift) % CHUNK == CHUNK - 1).sum())
        if all(hit.values()):
            return W, H, coef, files, hit
    raise AssertionError("no seed puts a marker and a stuffed byte on every boundary")


@gpu
def test_markers_on_piece_and_chunk_boundaries(cuda):
    W, H, coef, files, hit = _boundary_case()
    print("boundary hits:", hit, "file bytes:", len(files[0]))
    assert all(hit.values()) and 20000 < len(files[0]) < 100000      # tens of KiB of scan
    assert C.jfif_info(files[15])["scan_offset"] == C.jfif_info(files[0])["scan_offset"] + 15
    status = _check_batch(cuda, files, W, H, 0)
    assert not status.any()
    assert np.array_equal(_host(files[7])[1], coef)


# ---- other routes in ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sr", [0, 2])
def test_file_without_restart_intervals(cuda, sr):
    coef = _lap(64, 48, sr, 9)
    data = C.write_jfif(coef.reshape(3, -1, 64), 64, 48, 50) if sr == 0 else C.write_jfif_sub(coef, 64, 48, 50, sr)
    assert C.jfif_info(data)["restart_interval"] == 0
    _check_batch(cuda, [data], 64, 48, sr)
    assert np.array_equal(_host(data)[1], coef)


@gpu
def test_encode_then_decode(cuda):
    import torch
    import oracle
    rgb = torch.from_numpy(oracle.gen_splitmix(3, 64, 64)).to(cuda)
    data = jpgx.encode_jpeg(rgb, 90)
    got = jpgx.decode_jpeg_coefficients(data, cuda)
    ref = decode(data)
    assert got["coef"].is_cuda and got["coef"].shape == (3, 64, 64)
    assert np.array_equal(got["coef"].cpu().numpy().astype(np.int32), ref["coef"])
    assert got["qt"].cpu().numpy().tolist() == [ref["dqt"][ref["qsel"][0]], ref["dqt"][ref["qsel"][1]]]
    assert (got["width"], got["height"], got["sample_ratio"]) == (64, 64, 0)
    assert np.array_equal(got["coef"].cpu().numpy(), jpgx.encode_blocks(rgb, 90).cpu().numpy())
    with pytest.raises(jpgx.JpgxError) as e:
        jpgx.decode_jpeg_coefficients(data[:-2], cuda)
    assert e.value.rc == SCAN


@gpu
def test_graph_capture(cuda):
    """the call captured once on a single stream, replayed over two sets of files swapped in place"""
    import torch
    W, H, sr = 64, 64, 2
    nb, nbc = _nblocks(W, H, sr)
    per = (nb + 2 * nbc) * 64
    sets = [[C.write_jfif_ex(_lap(W, H, sr, 300 + 2 * s + k), W, H, 70, sr, restart_rows=1, nthreads=1,
                             optimize=bool(k)) for k in range(2)] for s in range(2)]
    stride = max(len(f) for fs in sets for f in fs)
    ups = [_upload(cuda, fs, stride) for fs in sets]
    d_files, lens = ups[0][0].clone(), ups[0][1].clone()
    coef = torch.zeros((2, per), dtype=torch.int16, device=cuda)
    qt = torch.zeros((2, 2, 64), dtype=torch.uint16, device=cuda)
    status = torch.full((2,), 77, dtype=torch.int32, device=cuda)
    need = jpgx.lib.jpgx_jfif_decode_gpu_workspace_size(W, H, sr, 2, stride)
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    st = torch.cuda.Stream()

    def call():
        rc = jpgx.lib.jpgx_jfif_decode_gpu(d_files.data_ptr(), stride, lens.data_ptr(), 2, W, H, sr, coef.data_ptr(),
                                           per, qt.data_ptr(), status.data_ptr(), ws.data_ptr(), need, st.cuda_stream)
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
        coef.zero_()
        status.fill_(77)
        ws.fill_(0xEE)                               # the call initialises what it reads of the workspace
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0, 0]
        for k in range(2):
            assert np.array_equal(coef[k].cpu().numpy().reshape(-1, 64), _host(sets[s][k])[1])


# ---- refusals on the device: three inputs of the sanitizer sweep ----------------------------------
@gpu
def test_three_corrupt_inputs_of_the_sanitizer_sweep(cuda):
    """A truncation inside the scan, a corruption that makes an undefined code and a dropped RSTm
    of the sanitizer program's 16x16 4:4:4 file (tests/c/jfif_read_san.c decodes every truncation,
    every dropped marker and this corruption of that file).  The gate is the CPU test
    test_jfif_read.py::test_decoder_under_asan_ubsan, which holds the program's file and the
    corruption to the constants checked here: the shared routines have decoded these very bytes
    under AddressSanitizer where that test has passed on the same tree.  No sanitizer runs here.
    This is the refusal path, not a fault: the device's status is the host's."""
    idx = S.GPU_FILE[0]
    data, W, H, sr, _ = S.file_of(idx)
    assert (W, H, sr) == (16, 16, 0) and (len(data), S.fnv1a(data)) == S.GPU_FILE[1:]
    scan = C.jfif_info(data)["scan_offset"]
    pos, val = S.GPU_FLIP
    assert (pos, val) in S.flips(idx, data, S.FLIPS) and scan <= pos < len(data) - 2
    files = [data, data[:scan + (len(data) - scan) // 2], S.flipped(data, pos, val), S.drop_first_rst(data)]
    assert [_host(f)[0] for f in files] == [0, SCAN, SCAN, SCAN]
    status = _check_batch(cuda, files, W, H, sr)
    assert status.tolist() == [0, SCAN, SCAN, SCAN]
