"""The device JFIF coder (csrc/jpgx_jfif.hip: jpgx_jfif_gpu, jpgx.jfif_gpu, jpgx.encode_jpeg).

The oracle everywhere is the host writer on the same coefficients,
jpgx.compat.write_jfif_ex(coef, W, H, q, sr, restart_rows=rr, nthreads=1), and the comparison is
== on bytes: no golden data, no tolerance.  (The device's restart_rows = -1 means one MCU row per
interval; the host writer's -1 depends on its thread count, so its equivalent call passes 1.)"""
import io
import os

import numpy as np
import pytest

import jpgx
import jpgx.compat as C
import san_build
from conftest import GOLDEN
from jfif_decode import decode
from jfif_inputs import CASES, hand_made, stuffing_guard, stuffing_heavy
from jfif_inputs import lap as _lap, nblocks as _nblocks, scan_of as _scan

gpu = pytest.mark.gpu


def _host(coef, W, H, q, sr, rr):
    return C.write_jfif_ex(coef, W, H, q, sr, restart_rows=1 if rr == -1 else rr, nthreads=1)


def _device(cuda, coef, W, H, q, sr, rr, cap=None):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(coef, np.int16)).to(cuda).reshape(1, -1)
    out, lens = jpgx.jfif_gpu(d, W, H, q, sr, rr, cap=cap)
    n = int(lens[0])
    assert 0 < n <= out.shape[1]
    return out[0, :n].cpu().numpy().tobytes()


def _raw(d_coef, fstride, nf, W, H, q, sr, rr, out, ostride, cap, lens, ws=None):
    """jpgx_jfif_gpu itself on torch tensors (a workspace of the size the library asks for)"""
    import torch
    need = jpgx.lib.jpgx_jfif_gpu_workspace_size(W, H, sr, rr, nf, cap)
    assert need > 0
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=out.device)
    rc = jpgx.lib.jpgx_jfif_gpu(d_coef.data_ptr(), fstride, nf, W, H, q, sr, rr, out.data_ptr(), ostride, cap,
                                lens.data_ptr(), ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    return rc


# ---- CPU: argument checks happen before any device call ------------------------------------------
def _call(coef=0x10000, fstride=3 * 64 * 64, nf=1, W=64, H=64, q=50, sr=0, rr=1, out=0x20000, ostride=1 << 16,
          cap=1 << 16, lens=0x30000, ws=0x40000, wsb=None):
    if wsb is None:
        wsb = jpgx.lib.jpgx_jfif_gpu_workspace_size(W, H, sr, rr, max(nf, 1), cap) or 1 << 20
    return jpgx.lib.jpgx_jfif_gpu(coef, fstride, nf, W, H, q, sr, rr, out, ostride, cap, lens, ws, wsb, None)


def test_bad_arguments_are_refused_without_a_device():
    assert _call(rr=0) == jpgx.EARG
    assert _call(rr=-2) == jpgx.EARG
    assert _call(rr=8192) == jpgx.EARG               # 8192 rows x 8 MCUs: Ri would not fit 16 bits
    assert _call(fstride=3 * 64 * 64 + 32) == jpgx.EARG
    assert _call(fstride=3 * 64 * 64 - 64) == jpgx.EARG
    assert _call(nf=0) == jpgx.EARG
    assert _call(nf=65536) == jpgx.EARG
    for name in ("coef", "out", "lens", "ws"):
        assert _call(**{name: None}) == jpgx.EARG, name
    assert _call(coef=0x10008) == jpgx.EARG          # 16-byte alignment
    assert _call(ostride=(1 << 16) - 1) == jpgx.EARG
    assert _call(q=0) == jpgx.EQUALITY and _call(q=98) == jpgx.EQUALITY
    assert _call(W=72, sr=1) == jpgx.EGEOMETRY
    assert _call(sr=3) == jpgx.EARG
    for bad in (dict(rr=0), dict(rr=-2), dict(rr=8192), dict(nf=0), dict(nf=65536), dict(sr=3)):
        a = dict(W=64, H=64, sr=0, rr=1, nf=1)
        a.update(bad)
        assert jpgx.lib.jpgx_jfif_gpu_workspace_size(a["W"], a["H"], a["sr"], a["rr"], a["nf"], 1 << 16) == 0


def test_workspace_one_byte_short():
    for sr, rr, nf in ((0, 1, 1), (2, -1, 3), (1, 4, 2)):
        need = jpgx.lib.jpgx_jfif_gpu_workspace_size(64, 64, sr, rr, nf, 1 << 16)
        # out_cap bytes of unstuffed stream per frame and 4 bytes of offset per block, at least
        nb, nbc = _nblocks(64, 64, sr)
        assert need >= nf * ((1 << 16) + 4 * (nb + 2 * nbc))
        assert _call(sr=sr, rr=rr, nf=nf, fstride=(nb + 2 * nbc) * 64, wsb=need - 1) == jpgx.EWORKSPACE


def test_binding_refuses_host_tensors():
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError):
        jpgx.jfif_gpu(torch.zeros((1, 3 * 64 * 64), dtype=torch.int16), 64, 64, 50)
    with pytest.raises(ValueError):
        jpgx.jfif_gpu(np.zeros((1, 3 * 64 * 64), np.int16), 64, 64, 50)
    with pytest.raises(ValueError):
        jpgx.encode_jpeg(torch.zeros((64, 64, 3), dtype=torch.uint8), 50)


@pytest.mark.skipif(not san_build.HAVE_CC, reason="needs gcc/g++ with libasan/libubsan")
def test_header_and_tables_under_asan_ubsan():
    """tests/c/jfif_header_san.c, a program of its own, with host/*.c and the host plan under
    AddressSanitizer + UndefinedBehaviorSanitizer (nothing is preloaded)."""
    rc, out, err = san_build.run("jfif_header_san")
    assert rc == 0 and "jfif_header_san: clean" in out, (out[-2000:], err[-4000:])
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-4000:]


# ---- GPU: byte equality with the host writer ------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_bytes_equal_host_writer(cuda, name):
    W, H, q, sr, rr, seed = CASES[name]
    coef = _lap(W, H, sr, seed)
    ref = _host(coef, W, H, q, sr, rr)
    if name == "rst_wraps":
        assert ref.count(b"\xff\xd7") >= 1 and decode(ref)["restarts"] == 11
    if name == "single_interval":
        assert decode(ref)["restart_interval"] == 100 * (W // 8) and decode(ref)["restarts"] == 0
    assert _device(cuda, coef, W, H, q, sr, rr) == ref


@gpu
def test_all_zero_frame(cuda):
    """14 bits per MCU: eight and more blocks share a 32-bit word of the stream"""
    W, H = 64, 96
    coef = np.zeros((3 * 96, 64), np.int16)
    ref = _host(coef, W, H, 50, 0, 1)
    scan = _scan(ref)
    assert len(scan) == 190 and scan[:6] == bytes.fromhex("2800a002800a")
    assert _device(cuda, coef, W, H, 50, 0, 1) == ref


@gpu
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_hand_made_blocks(cuda, sr):
    W, H, coef = hand_made(sr)
    for rr in (1, 2):
        assert _device(cuda, coef, W, H, 50, sr, rr) == _host(coef, W, H, 50, sr, rr)


@gpu
@pytest.mark.parametrize("sr", [0, 2])
def test_stuffing_heavy_frame(cuda, sr):
    W, H, q, coef = stuffing_heavy(sr)
    ref = _host(coef, W, H, q, sr, 1)
    pairs, endings = stuffing_guard(ref)
    assert pairs >= 1000 and endings >= 1          # a different numpy must not empty the case
    assert _device(cuda, coef, W, H, q, sr, 1) == ref


@gpu
@pytest.mark.parametrize("sr,W,H", [(0, 1920, 1080), (2, 1920, 1088)])
def test_full_hd_from_the_transform(cuda, sr, W, H):
    """an interval has 720 blocks: lanes loop; coefficients from encode_blocks on the device"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(5)
    small = torch.randint(0, 256, (H // 8, W // 8, 3), generator=g, dtype=torch.uint8)
    rgb = small.repeat_interleave(8, 0).repeat_interleave(8, 1)
    rgb = (rgb.to(torch.int16) + torch.randint(-6, 7, rgb.shape, generator=g, dtype=torch.int16)).clamp(0, 255)
    rgb = rgb.to(torch.uint8).to(cuda)
    flags = jpgx.FLAG_SUBSAMPLE if sr else 0
    coef = jpgx.encode_blocks(rgb, 75, sr, flags=flags)
    out, lens = jpgx.jfif_gpu(coef.reshape(1, -1), W, H, 75, sr, 1)
    n = int(lens[0])
    ref = _host(coef.cpu().numpy().reshape(-1, 64), W, H, 75, sr, 1)
    assert 0 < n == len(ref)
    assert out[0, :n].cpu().numpy().tobytes() == ref


@gpu
def test_batch_with_padded_strides(cuda):
    import torch
    W, H, q, sr, rr = 96, 64, 60, 0, 2
    per = 3 * (W // 8) * (H // 8) * 64
    fstride, cap, ostride = per + 5 * 64, 40000, 40000 + 48
    frames = [_lap(W, H, sr, 100 + k, scale=4.0 + 3 * k) for k in range(3)]
    d = torch.zeros((3, fstride), dtype=torch.int16, device=cuda)
    for k in range(3):
        d[k, :per] = torch.from_numpy(frames[k].reshape(-1)).to(cuda)
    out = torch.full((3, ostride), 0xA5, dtype=torch.uint8, device=cuda)
    lens = torch.zeros(3, dtype=torch.int64, device=cuda)
    assert _raw(d, fstride, 3, W, H, q, sr, rr, out, ostride, cap, lens) == 0
    got, n = out.cpu().numpy(), lens.cpu().numpy()
    for k in range(3):
        single = _device(cuda, frames[k], W, H, q, sr, rr)
        assert single == _host(frames[k], W, H, q, sr, rr)
        assert got[k, :n[k]].tobytes() == single
        assert (got[k, n[k]:] == 0xA5).all()


@gpu
def test_overflow_reports_a_sufficient_capacity(cuda):
    import torch
    W, H, q, sr, rr = 64, 48, 50, 0, 1
    coef = _lap(W, H, sr, 21)
    ref = _host(coef, W, H, q, sr, rr)
    hdrlen = ref.index(b"\xff\xda") + 14
    cap = hdrlen + 16
    d = torch.from_numpy(coef).to(cuda).reshape(1, -1)
    out = torch.full((1, 1 << 16), 0xA5, dtype=torch.uint8, device=cuda)
    lens = torch.zeros(1, dtype=torch.int64, device=cuda)
    assert _raw(d, d.shape[1], 1, W, H, q, sr, rr, out, out.shape[1], cap, lens) == 0
    n = int(lens[0])
    assert n < 0                                     # bit 63
    need = n & ((1 << 62) - 1)
    assert len(ref) <= need <= hdrlen + 2 * len(_scan(ref)) + 2
    assert (out[0, cap:] == 0xA5).all()
    assert _raw(d, d.shape[1], 1, W, H, q, sr, rr, out, out.shape[1], need, lens) == 0
    assert int(lens[0]) == len(ref) and out[0, :len(ref)].cpu().numpy().tobytes() == ref
    # the binding retries once with the reported capacity
    assert _device(cuda, coef, W, H, q, sr, rr, cap=cap) == ref


@gpu
def test_overflow_of_one_frame_leaves_its_neighbours(cuda):
    import torch
    W, H, q, sr, rr = 64, 48, 50, 0, 1
    frames = [_lap(W, H, sr, 31, scale=2.0), _lap(W, H, sr, 32, scale=60.0), _lap(W, H, sr, 33, scale=2.0)]
    refs = [_host(c, W, H, q, sr, rr) for c in frames]
    cap = (max(len(refs[0]), len(refs[2])) + 15) // 16 * 16
    assert len(refs[1]) > cap + 64
    d = torch.stack([torch.from_numpy(c.reshape(-1)) for c in frames]).to(cuda)
    ostride = cap + 4096
    out = torch.full((3, ostride), 0xA5, dtype=torch.uint8, device=cuda)
    lens = torch.zeros(3, dtype=torch.int64, device=cuda)
    assert _raw(d, d.shape[1], 3, W, H, q, sr, rr, out, ostride, cap, lens) == 0
    got, n = out.cpu().numpy(), lens.cpu().numpy()
    for k in (0, 2):
        assert n[k] == len(refs[k]) and got[k, :n[k]].tobytes() == refs[k]
        assert (got[k, n[k]:] == 0xA5).all()
    assert n[1] < 0 and (int(n[1]) & ((1 << 62) - 1)) >= len(refs[1])
    assert (got[1, cap:] == 0xA5).all()


@gpu
def test_encode_jpeg_end_to_end(cuda):
    import torch
    rgb, _ = C.bmp_read(os.path.join(GOLDEN, "images", "cam.bmp"))
    H, W = rgb.shape[:2]
    d_rgb = torch.from_numpy(rgb).to(cuda)
    data = jpgx.encode_jpeg(d_rgb, 75)
    coef = jpgx.encode_blocks(d_rgb, 75).cpu().numpy()
    assert data == _host(coef, W, H, 75, 0, 1)
    dec = decode(data)
    assert (dec["width"], dec["height"]) == (W, H)
    got = np.concatenate([np.asarray(x).reshape(-1, 64) for x in dec["coef"]])
    assert np.array_equal(got, coef.reshape(-1, 64).astype(np.int32))
    if W % 16 == 0 and H % 16 == 0:
        sub = jpgx.encode_jpeg(d_rgb, 75, 2, flags=jpgx.FLAG_SUBSAMPLE)
        csub = jpgx.encode_blocks(d_rgb, 75, 2, flags=jpgx.FLAG_SUBSAMPLE).cpu().numpy()
        assert sub == _host(csub, W, H, 75, 2, 1)


@gpu
def test_encode_jpeg_opens_in_pil(cuda):
    Image = pytest.importorskip("PIL.Image")
    import torch
    rgb, _ = C.bmp_read(os.path.join(GOLDEN, "images", "cam.bmp"))
    data = jpgx.encode_jpeg(torch.from_numpy(rgb).to(cuda), 90)
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.size == (rgb.shape[1], rgb.shape[0])


@gpu
def test_same_call_twice_gives_the_same_bytes(cuda):
    W, H, q, sr, rr = 128, 96, 80, 1, 2
    coef = _lap(W, H, sr, 77)
    a = _device(cuda, coef, W, H, q, sr, rr)
    b = _device(cuda, coef, W, H, q, sr, rr)
    assert a == b == _host(coef, W, H, q, sr, rr)
