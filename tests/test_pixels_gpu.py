"""The pixel kernels (csrc/jpgx_pixels.hip: jpgx_pixels_gpu, jpgx.pixels_gpu, jpgx.decode_jpeg;
DESIGN.md 4.9).

The oracle everywhere is the host twin on the same coefficients and tables, jpgx.compat.pixels_host
(itself held to the contract's numpy restatement and to libjpeg in tests/test_pixels.py); every
comparison is ==.  Both libraries link the kernels, so the raw-call tests run on both."""
import hashlib
import io

import numpy as np
import pytest

import jfif_san_cases as S
import jpgx
import jpgx.compat as C
import pixels_cases as P
from gpu_files import upload
from jfif_decode import decode

gpu = pytest.mark.gpu
FILL = 0x7A


def _lib(which):
    return jpgx.lib if which == "product" else jpgx.alt_library()


def _raw(L, cuda, coefs, W, H, sr, qts, status=None, cpad=0, pitch=None, opad=0, stream=None):
    """one jpgx_pixels_gpu call on library L: coefs [n][nblk * 64] int16, qts [n][2][64] (a pair per
    frame) or [2][64] (one pair); returns the whole prefilled output buffer [n][H * pitch + opad]"""
    import torch
    coefs = np.ascontiguousarray(coefs, np.int16).reshape(len(coefs), -1)
    n, per = coefs.shape
    cstride = per + cpad
    host = np.full((n, cstride), 0x5A5A, np.int16)
    host[:, :per] = coefs
    d_coef = torch.from_numpy(host).to(cuda)
    qts = np.ascontiguousarray(qts, np.uint16)
    d_qt = torch.from_numpy(qts.view(np.int16)).to(cuda)
    qstride = 0 if qts.ndim == 2 else 128
    pitch = pitch or 3 * W
    ostride = H * pitch + opad
    out = torch.full((n, ostride), FILL, dtype=torch.uint8, device=cuda)
    need = L.jpgx_pixels_gpu_workspace_size(W, H, sr, n)
    assert (need == 0) == (sr == 0)
    ws = torch.full((max(need, 16),), 0xEE, dtype=torch.uint8, device=cuda)
    d_st = None if status is None else torch.tensor(status, dtype=torch.int32, device=cuda)
    rc = L.jpgx_pixels_gpu(d_coef.data_ptr(), cstride, n, W, H, sr, d_qt.data_ptr(), qstride,
                           d_st.data_ptr() if d_st is not None else None, out.data_ptr(), pitch, ostride,
                           ws.data_ptr() if need else None, need, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _frame(buf, k, W, H, pitch=None):
    pitch = pitch or 3 * W
    return buf[k, :H * pitch].reshape(H, pitch)[:, :3 * W].reshape(H, W, 3)


# ---- the grid ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", ["product", "alt"])
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_grid_equals_the_host(cuda, sr, which):
    L = _lib(which)
    for W, H in P.SIZES[sr]:
        cases = [(kind, q) for kind in ("splitmix", "tie") for q in P.QUALITIES]
        coefs = np.stack([P.oracle_coef(kind, W, H, q, sr) for kind, q in cases])
        qts = np.stack([P.qt_of(q) for _, q in cases])
        buf = _raw(L, cuda, coefs, W, H, sr, qts)
        for k, (kind, q) in enumerate(cases):
            want = C.pixels_host(coefs[k], W, H, sr, qts[k], 2)
            assert np.array_equal(_frame(buf, k, W, H), want), (W, H, kind, q)


@gpu
@pytest.mark.parametrize("which", ["product", "alt"])
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_hostile_values(cuda, sr, which):
    """extreme coefficients and tables change values, never an address: the wrap arithmetic on the device"""
    L = _lib(which)
    for W, H in ((16, 16), (48, 32)):
        coefs, qts = P.hostile_frames(W, H, sr)
        buf = _raw(L, cuda, coefs, W, H, sr, qts)
        for k in range(len(coefs)):
            assert np.array_equal(_frame(buf, k, W, H), C.pixels_host(coefs[k], W, H, sr, qts[k], 1)), (W, H, k)


# ---- batches and layouts -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", ["product", "alt"])
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_batch_with_padded_layouts_and_a_skipped_frame(cuda, sr, which):
    L = _lib(which)
    W, H = 136 if sr == 0 else 144, 32
    qs = (1, 30, 50, 90, 97)
    coefs = np.stack([P.oracle_coef("splitmix", W, H, q, sr) for q in qs])
    per_frame = np.stack([P.qt_of(q) for q in qs])
    for pitch, qts in ((3 * W + 8, per_frame), (3 * W + 40, per_frame[3])):
        buf = _raw(L, cuda, coefs, W, H, sr, qts, status=[0, 0, -10, 0, 0], cpad=3 * 64, pitch=pitch, opad=4096)
        for k in range(5):
            rows = buf[k, :H * pitch].reshape(H, pitch)
            assert (rows[:, 3 * W:] == FILL).all() and (buf[k, H * pitch:] == FILL).all()   # no byte that is no pixel
            if k == 2:
                assert (buf[k] == FILL).all()            # the skipped frame's whole slot
            else:
                qt = qts[k] if qts.ndim == 3 else qts
                assert np.array_equal(_frame(buf, k, W, H, pitch), C.pixels_host(coefs[k], W, H, sr, qt, 2)), k


@gpu
def test_python_view(cuda):
    import torch
    W, H, sr = 48, 32, 2
    coefs = np.stack([P.oracle_coef("splitmix", W, H, q, sr) for q in (50, 90)])
    qts = np.stack([P.qt_of(q) for q in (50, 90)])
    d_coef = torch.from_numpy(coefs).to(cuda)
    d_qt = torch.from_numpy(qts.view(np.int16)).to(cuda).view(torch.uint16)
    got = jpgx.pixels_gpu(d_coef, W, H, sr, d_qt=d_qt)
    assert got.shape == (2, H, W, 3) and got.dtype == torch.uint8 and got.is_cuda and got.is_contiguous()
    pad = jpgx.pixels_gpu(d_coef, W, H, sr, d_qt=d_qt[1], pitch=3 * W + 16,
                          status=torch.tensor([0, 0], dtype=torch.int32, device=cuda))
    assert pad.shape == (2, H, W, 3) and pad.stride() == (H * (3 * W + 16), 3 * W + 16, 3, 1)
    for k in range(2):
        assert np.array_equal(got[k].cpu().numpy(), C.pixels_host(coefs[k], W, H, sr, qts[k], 1))
        assert np.array_equal(pad[k].cpu().numpy(), C.pixels_host(coefs[k], W, H, sr, qts[1], 1))


# ---- the chain: coder -> decoder -> pixels, nothing on the host in between ------------------------------
@gpu
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_chain_on_one_stream(cuda, sr):
    import torch
    W, H, q = 96, 64, 75
    coefs = np.stack([P.oracle_coef(kind, W, H, q, sr) for kind in ("splitmix", "tie", "splitmix")])
    st = torch.cuda.Stream()
    d = torch.from_numpy(coefs).to(cuda).reshape(3, -1)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        files, lens = jpgx.jfif_gpu(d, W, H, q, sr, 1, stream=st)
        coef, qt, status = jpgx.jfif_decode_gpu(files, lens, W, H, sr, stream=st)
        rgb = jpgx.pixels_gpu(coef, W, H, sr, d_qt=qt, status=status, stream=st)
    st.synchronize()
    assert status.cpu().tolist() == [0, 0, 0]
    for k in range(3):
        assert np.array_equal(rgb[k].cpu().numpy(), C.pixels_host(coefs[k], W, H, sr, P.qt_of(q), 2)), k


@gpu
def test_chain_with_a_corrupt_file_in_the_middle(cuda):
    """the sanitizer sweep's 16x16 4:4:4 file and its undefined-code corruption (the constants of
    tests/test_jfif_decode_gpu.py): the decoder's status makes the pixel kernels skip the frame"""
    import torch
    idx = S.GPU_FILE[0]
    data, W, H, sr, _ = S.file_of(idx)
    assert (W, H, sr) == (16, 16, 0) and (len(data), S.fnv1a(data)) == S.GPU_FILE[1:]
    pos, val = S.GPU_FLIP
    files = [data, S.flipped(data, pos, val), data]
    d_files, lens = upload(cuda, files)
    out = torch.full((3 * H * 3 * W,), FILL, dtype=torch.uint8, device=cuda)
    coef, qt, status = jpgx.jfif_decode_gpu(d_files, lens, W, H, sr)
    rgb = jpgx.pixels_gpu(coef, W, H, sr, d_qt=qt, status=status, out=out)
    assert status.cpu().tolist() == [0, jpgx.EJFIF_SCAN, 0]
    r = C.read_jfif(data, 1)
    want = C.pixels_host(r["coef"], W, H, sr, r["qt"], 1)
    got = rgb.cpu().numpy()
    assert np.array_equal(got[0], want) and np.array_equal(got[2], want)
    assert (got[1] == FILL).all()                        # the corrupt frame's slot is untouched


# ---- files in, pixels out --------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_decode_jpeg(cuda, sr):
    import torch
    import oracle
    imgs = [oracle.gen_splitmix(11 + k, 64, 48) for k in range(2)]
    imgs[1] = (imgs[1] // 4 + np.arange(64, dtype=np.uint8)[None, :, None] * 2).astype(np.uint8)
    files = [jpgx.encode_jpeg(torch.from_numpy(im).to(cuda), 90, sample_ratio=sr, flags=jpgx.FLAG_SUBSAMPLE if sr else 0)
             for im in imgs]
    for data in files:
        got = jpgx.decode_jpeg(data, "cuda:0")
        assert got.shape == (48, 64, 3) and got.dtype == torch.uint8 and got.is_cuda
        r = C.read_jfif(data, 1)
        assert r["sample_ratio"] == sr
        assert np.array_equal(got.cpu().numpy(), C.pixels_host(r["coef"], 64, 48, sr, r["qt"], 2))
        try:
            from PIL import Image
        except ImportError:
            continue
        if P.fits_16_bits(r["coef"], r["qt"], 48):       # libjpeg-turbo's 16-bit multiply: a condition
            assert np.array_equal(got.cpu().numpy(), np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
    batch = jpgx.decode_jpeg(files, cuda)                # a list: files of one geometry
    assert batch.shape == (2, 48, 64, 3)
    for k in range(2):
        assert np.array_equal(batch[k].cpu().numpy(), jpgx.decode_jpeg(files[k], cuda).cpu().numpy())
    with pytest.raises(jpgx.JpgxError) as e:
        jpgx.decode_jpeg(files[0][:-2], cuda)
    assert e.value.rc == jpgx.EJFIF_SCAN


@gpu
def test_frames_wider_than_high_and_higher_than_wide(cuda):
    """48x16 and 16x48, 4:2:2 and 4:2:0, through encode_jpeg and decode_jpeg: the smallest frames whose
    blocks per row and block rows differ for Y and for chroma alike, so that a frame field taken
    for its neighbour (csrc/jx_frame.h: bw / bh, cbw / cbh) shows in the bytes or in the pixels"""
    import torch
    import oracle
    for W, H in ((48, 16), (16, 48)):
        rgb = torch.from_numpy(oracle.gen_splitmix(7 * W + H, W, H)).to(cuda)
        for sr in (1, 2):
            data = jpgx.encode_jpeg(rgb, 90, sample_ratio=sr, flags=jpgx.FLAG_SUBSAMPLE, restart_rows=1)
            coef = jpgx.encode_blocks(rgb, 90, sr, flags=jpgx.FLAG_SUBSAMPLE).cpu().numpy()
            assert data == C.write_jfif_ex(coef, W, H, 90, sr, restart_rows=1, nthreads=1), (W, H, sr)
            r = C.read_jfif(data, 1)
            assert (r["width"], r["height"], r["sample_ratio"]) == (W, H, sr)
            # tests/jfif_decode.py places the blocks by its own reading of T.81, not by jx_frame.h
            ind = decode(data)
            assert (ind["width"], ind["height"], ind["sampling"]) == (W, H, (2, sr))
            assert np.array_equal(np.concatenate([np.asarray(c).reshape(-1, 64) for c in ind["coef"]]), r["coef"])
            got = jpgx.decode_jpeg(data, cuda)
            assert got.shape == (H, W, 3)
            assert np.array_equal(got.cpu().numpy(), C.pixels_host(r["coef"], W, H, sr, r["qt"], 2)), (W, H, sr)


# ---- a captured graph ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sr", [0, 2])
def test_graph_capture_of_decode_and_pixels(cuda, sr):
    """decode + pixels captured once on a single stream, replayed over two sets of files swapped in
    place and scribbled workspaces"""
    import torch
    W, H, q = 64, 64, 70
    nb, nbc = P.nblocks(W, H, sr)
    per = (nb + 2 * nbc) * 64
    sets = [[C.write_jfif_ex(P.oracle_coef(kind, W, H, q, sr) if s == 0 else -P.oracle_coef(kind, W, H, q, sr),
                             W, H, q, sr, restart_rows=1, nthreads=1) for kind in ("splitmix", "tie")] for s in range(2)]
    stride = max(len(f) for fs in sets for f in fs)
    ups = [upload(cuda, fs, stride, 0xA5) for fs in sets]
    d_files, lens = ups[0][0].clone(), ups[0][1].clone()
    coef = torch.zeros((2, per), dtype=torch.int16, device=cuda)
    qt = torch.zeros((2, 2, 64), dtype=torch.int16, device=cuda)
    status = torch.full((2,), 77, dtype=torch.int32, device=cuda)
    rgb = torch.zeros((2, H, W, 3), dtype=torch.uint8, device=cuda)
    need_d = jpgx.lib.jpgx_jfif_decode_gpu_workspace_size(W, H, sr, 2, stride)
    need_p = jpgx.lib.jpgx_pixels_gpu_workspace_size(W, H, sr, 2)
    ws_d = torch.empty(need_d, dtype=torch.uint8, device=cuda)
    ws_p = torch.empty(max(need_p, 16), dtype=torch.uint8, device=cuda)
    st = torch.cuda.Stream()

    def call():
        assert jpgx.lib.jpgx_jfif_decode_gpu(d_files.data_ptr(), stride, lens.data_ptr(), 2, W, H, sr, coef.data_ptr(),
                                             per, qt.data_ptr(), status.data_ptr(), ws_d.data_ptr(), need_d,
                                             st.cuda_stream) == 0
        assert jpgx.lib.jpgx_pixels_gpu(coef.data_ptr(), per, 2, W, H, sr, qt.data_ptr(), 128, status.data_ptr(),
                                        rgb.data_ptr(), 3 * W, 3 * W * H, ws_p.data_ptr() if need_p else None, need_p,
                                        st.cuda_stream) == 0

    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        call()                                           # once eagerly: nothing is left to initialise
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        call()
    torch.cuda.synchronize()
    for s in (1, 0):
        d_files.copy_(ups[s][0])
        lens.copy_(ups[s][1])
        rgb.fill_(FILL)
        status.fill_(77)
        ws_d.fill_(0xEE)
        ws_p.fill_(0xEE)                                 # the call writes what it reads of the workspace
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0, 0]
        for k in range(2):
            r = C.read_jfif(sets[s][k], 1)
            assert np.array_equal(rgb[k].cpu().numpy(), C.pixels_host(r["coef"], W, H, sr, r["qt"], 2)), (s, k)


# ---- full size ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_one_4k_frame(cuda, sr):
    """3840 x 2160: 480 blocks per row (60 whole runs), 270 block rows; the only full-size case"""
    import torch
    W, H = 3840, 2160
    nb, nbc = P.nblocks(W, H, sr)
    rng = np.random.default_rng(40 + sr)
    coef = rng.laplace(0, 3.0, size=(nb + 2 * nbc, 64)).astype(np.int16)
    coef[:, 0] = rng.integers(-100, 100, size=nb + 2 * nbc)
    qt = P.qt_of(90)
    want = C.pixels_host(coef, W, H, sr, qt, 0)
    d_qt = torch.from_numpy(qt.view(np.int16)).to(cuda).view(torch.uint16)
    got = jpgx.pixels_gpu(torch.from_numpy(coef).to(cuda).reshape(1, -1), W, H, sr, d_qt=d_qt)
    got = got[0].cpu().numpy()
    assert len(np.unique(want)) > 200
    assert hashlib.sha256(got.tobytes()).hexdigest() == hashlib.sha256(np.ascontiguousarray(want).tobytes()).hexdigest()
