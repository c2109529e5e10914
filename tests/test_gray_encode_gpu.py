"""The encode side of the one-component family on the device: k_gray
(jpgx_blocks_gpu_gray) against the oracle of tests/gray_enc_cases.py at the seams of its tiles, frames and
load paths, jpgx_jfif_gpu_gray against the host writer byte for byte, and the round trips through the
device decoder and the pixel path.  Every comparison is ==."""
import numpy as np
import pytest

import gray_enc_cases as G
import jpgx
import jpgx.compat as C

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A
# blocks per frame 1, 63, 64, 65, 256, 257: a tile that is not full, exactly one, one block more, four, a fifth
SEAM_WIDTHS = (8, 504, 512, 520, 2048, 2056)


def _torch():
    import torch
    return torch


def _dev(a, cuda):
    return _torch().from_numpy(np.array(a)).to(cuda)           # a copy: the helper's arrays are read-only


def _inputs(q):
    for W, H in G.SIZES:
        yield "noise %dx%d" % (W, H), G.noise(W, H)
        yield "ramp %dx%d" % (W, H), G.ramp(W, H)
    for W in SEAM_WIDTHS:
        yield "noise %dx8" % W, G.noise(W, 8)
    yield "flat", G.flat()
    if q == 97:
        yield "extremes", G.extremes()
    if q == 90:
        yield "ties", G.ties4_image()


@pytest.mark.parametrize("q", G.QUALITIES)
def test_forward_is_the_oracle(cuda, q):
    for name, img in _inputs(q):
        want = G.gray_oracle(img, q)
        got = jpgx.encode_blocks_gray(_dev(img, cuda), q)
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want), (name, q)
        forced = jpgx.encode_blocks_gray(_dev(img, cuda), q, flags=jpgx.FLAG_FORCE_EXACT)
        assert np.array_equal(forced.cpu().numpy(), want), (name, q, "force")


def test_every_width_mod_8(cuda):
    for W in range(17, 25):                                          # W mod 8 = 1 .. 7, 0
        img = G.noise(W, 11)
        assert np.array_equal(jpgx.encode_blocks_gray(_dev(img, cuda), 90).cpu().numpy(), G.gray_oracle(img, 90)), W


def test_a_frame_boundary_inside_a_wave(cuda):
    """11 frames of 24 x 16, 6 blocks each: 66 blocks, so frames end inside the first tile and the second
    tile has two blocks"""
    frames = np.stack([G.noise(24, 16, seed=10 + k) for k in range(11)])
    got = jpgx.encode_blocks_gray(_dev(frames, cuda), 90).cpu().numpy()
    assert got.shape == (11, 6, 64)
    for k in range(11):
        assert np.array_equal(got[k], G.gray_oracle(frames[k], 90)), k


@pytest.mark.parametrize("W,H", [(21, 13), (65, 17), (263, 21), (64, 16)])
def test_layouts(cuda, W, H):
    """rows exactly W + 1 and W + 13 bytes apart, the first pixel at offsets 0 .. 3 of a flat buffer (views made
    with as_strided, their strides asserted), 7 bytes of gap between a frame's last pixel and the next frame,
    and the buffer ending with the last frame's last pixel; one frame expanded to three (frame stride 0);
    an output stride above nb * 64 with sentinels after every frame and around the buffer"""
    torch = _torch()
    nf, nb = 3, G.nblocks(W, H)
    imgs = np.stack([G.noise(W, H, seed=20 + k) for k in range(nf)])
    want = np.stack([G.gray_oracle(imgs[k], 90) for k in range(nf)])
    d_imgs = _dev(imgs, cuda)
    for pitch in (W + 1, W + 13):
        for off in range(4):
            fstride = pitch * (H - 1) + W + 7
            flat = torch.full((off + fstride * (nf - 1) + pitch * (H - 1) + W,), 0xEE, dtype=torch.uint8, device=cuda)
            assert flat.data_ptr() % 8 == 0
            view = torch.as_strided(flat, (nf, H, W), (fstride, pitch, 1), off)
            view.copy_(d_imgs)
            assert view.stride() == (fstride, pitch, 1) and view.data_ptr() == flat.data_ptr() + off
            got = jpgx.encode_blocks_gray(view, 90)
            assert np.array_equal(got.cpu().numpy(), want), (pitch, off)
            one = jpgx.encode_blocks_gray(view[1], 90)
            assert view[1].stride() == (pitch, 1) and np.array_equal(one.cpu().numpy(), want[1]), (pitch, off)
    same = jpgx.encode_blocks_gray(d_imgs[2].expand(nf, H, W), 90)      # the input is only read: frames may coincide
    assert np.array_equal(same.cpu().numpy(), np.stack([want[2]] * nf))
    # the output: frames (nb + 3) * 64 apart inside a buffer with a margin of 64 elements each side
    ostride = (nb + 3) * 64
    buf = torch.full((64 + nf * ostride + 64,), SENTINEL, dtype=torch.int16, device=cuda)
    rc = jpgx.lib.jpgx_blocks_gpu_gray(d_imgs.data_ptr(), W, W * H, nf, W, H, 90, 0, buf.data_ptr() + 128, ostride,
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    host = buf.cpu().numpy()
    body = host[64:64 + nf * ostride].reshape(nf, nb + 3, 64)
    assert np.array_equal(body[:, :nb], want)
    assert (body[:, nb:] == SENTINEL).all() and (host[:64] == SENTINEL).all() and (host[-64:] == SENTINEL).all()


def test_repeated_launches_agree(cuda):
    """64 launches into fresh buffers all equal the first (the exact pass's queue and the stage are the
    wave's own: nothing depends on what another launch left)"""
    torch = _torch()
    img = _dev(G.ties4_image(), cuda)
    outs = [jpgx.encode_blocks_gray(img, 90) for _ in range(64)]
    torch.cuda.synchronize()
    first = outs[0].cpu().numpy()
    assert np.array_equal(first, G.gray_oracle(G.ties4_image(), 90))
    for k, o in enumerate(outs[1:]):
        assert torch.equal(o, outs[0]), k + 1


# ---- the coder --------------------------------------------------------------------------------------------
def _files(out, lens):
    host, n = out.cpu().numpy(), lens.cpu().numpy()
    assert (n > 0).all(), n
    return [host[k, :int(n[k])].tobytes() for k in range(len(n))]


@pytest.mark.parametrize("optimize", [False, True])
def test_coder_is_the_host_writer_s(cuda, optimize):
    for W, H, q in ((21, 13, 90), (65, 17, 50), (263, 29, 97), (2056, 24, 90), (8, 8, 50), (1, 1, 90)):
        coefs = np.stack([G.gray_oracle(G.noise(W, H, seed=30 + k) if k != 1 else G.ramp(W, H), q) for k in range(3)])
        d = _dev(coefs, cuda)
        for rr in (-1, 1, 2, 3):
            out, lens = jpgx.jfif_gpu_gray(d, W, H, q, restart_rows=rr, optimize=optimize)
            for k, data in enumerate(_files(out, lens)):
                want = C.write_jfif_gray(coefs[k], W, H, q, restart_rows=abs(rr), nthreads=1, optimize=optimize)
                assert data == want, (W, H, q, rr, k)


def test_coder_small_capacity(cuda):
    W, H, q = 263, 21, 97
    coef = G.gray_oracle(G.noise(W, H), q)
    want = C.write_jfif_gray(coef, W, H, q, restart_rows=1, nthreads=1)
    torch = _torch()
    d = _dev(coef[None], cuda)
    cap = 512
    out = torch.empty((1, cap), dtype=torch.uint8, device=cuda)
    lens = torch.empty(1, dtype=torch.int64, device=cuda)
    need = int(jpgx.lib.jpgx_jfif_gpu_gray_workspace_size(W, H, 1, 1, cap, 0))
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    rc = jpgx.lib.jpgx_jfif_gpu_gray(d.data_ptr(), coef.size, 1, W, H, q, 1, 0, out.data_ptr(), cap, cap, lens.data_ptr(),
                                     ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    n = int(lens[0])
    assert n < 0                                                     # bit 63: the frame does not fit
    enough = n & ((1 << 62) - 1)
    assert len(want) <= enough <= 4 * len(want)
    out, lens = jpgx.jfif_gpu_gray(d, W, H, q, restart_rows=1, cap=enough)
    assert _files(out, lens) == [want]
    out, lens = jpgx.jfif_gpu_gray(d, W, H, q, restart_rows=1, cap=cap)      # the retry inside
    assert _files(out, lens) == [want]


def test_round_trips_on_the_device(cuda):
    for W, H, q in ((21, 13, 90), (263, 21, 50), (2056, 8, 97)):
        imgs = np.stack([G.noise(W, H, seed=40), G.ramp(W, H)])
        coef = jpgx.encode_blocks_gray(_dev(imgs, cuda), q)
        for optimize in (False, True):
            back, qt, status = jpgx.jfif_decode_gpu_gray(*jpgx.jfif_gpu_gray(coef, W, H, q, optimize=optimize), W, H)
            assert status.cpu().tolist() == [0, 0] and _torch().equal(back, coef), (W, H, q, optimize)
            assert np.array_equal(qt.cpu().numpy(), np.stack([jpgx.jfif_qt(q)[0]] * 2))
    for W, H in ((21, 13), (65, 17), (8, 8)):
        img = G.ramp(W, H)
        data = jpgx.encode_jpeg(_dev(img, cuda), 90, gray=True)
        px = jpgx.decode_jpeg(data, cuda, gray=True).cpu().numpy()
        want = C.pixels_host_gray(G.gray_oracle(img, 90), W, H, jpgx.jfif_qt(90)[0], 1)
        assert px.shape == (H, W) and np.array_equal(px, want), (W, H)
        assert data == C.write_jfif_gray(G.gray_oracle(img, 90), W, H, 90, restart_rows=1, nthreads=1)


def test_python_refusals(cuda):
    torch = _torch()
    img = _dev(G.noise(21, 13), cuda)
    with pytest.raises(ValueError):
        jpgx.encode_blocks_gray(img.cpu(), 90)                       # a host tensor
    with pytest.raises(ValueError):
        jpgx.encode_blocks_gray(img.to(torch.int16), 90)             # the wrong dtype
    with pytest.raises(ValueError):
        jpgx.encode_blocks_gray(img[None, None], 90)                 # 4-D
    with pytest.raises(ValueError):
        jpgx.encode_jpeg(img[None], 90, gray=True)                   # 3-D with gray
    with pytest.raises(ValueError):
        jpgx.encode_jpeg(img, 90)                                    # 2-D without gray
    with pytest.raises(ValueError):
        jpgx.encode_blocks_gray(img.t(), 90)                         # pixels of a row not adjacent
    with pytest.raises(ValueError):
        jpgx.encode_blocks_gray(torch.as_strided(img, (13, 21), (20, 1)), 90)    # pitch < W
    for q in (0, 98):
        with pytest.raises(jpgx.JpgxError) as e:
            jpgx.encode_blocks_gray(img, q)
        assert e.value.rc == jpgx.EQUALITY
    with pytest.raises(jpgx.JpgxError) as e:
        jpgx.encode_blocks_gray(img, 90, flags=jpgx.FLAG_SUBSAMPLE)
    assert e.value.rc == jpgx.EARG
    coef = jpgx.encode_blocks_gray(img, 90)
    with pytest.raises(ValueError):
        jpgx.jfif_gpu_gray(coef.cpu()[None], 21, 13, 90)
    with pytest.raises(ValueError):
        jpgx.jfif_gpu_gray(coef[None, :5], 21, 13, 90)               # too few blocks
    with pytest.raises(jpgx.JpgxError) as e:
        jpgx.jfif_gpu_gray(coef[None], 21, 13, 90, restart_rows=0)
    assert e.value.rc == jpgx.EARG
