"""k_mxs's Cr tile from four full-width products (csrc/jpgx_mx.hip, mxs_cr_rows): one operand tile
[Cr hi | Cr lo] per block set and row half, the hi and lo halves merged by a DPP add inside the
16-lane row, lanes j < 8 from the set-0 tile and lanes j >= 8 from the set-1 tile.

Every coefficient of all three channels must equal the oracle's, with JPGX_FLAG_FORCE_EXACT off and
on, at q 1, 50, 90 and 97, on the smallest launches that reach every path of the tile:
  128 x 8             one simple step and one general step (a block row's last)
  72 x 8              a launch ending in a one-block step
  256 x 16, 2 frames  all three slots of a wave, both row halves, a frame crossing
  832 x 8             13 steps: a second workgroup
Inputs: splitmix noise, all 0, all 255, pure red / green / blue (Cr at both ends of its range), and
frames whose blocks 0..3 of every step are black and 4..7 white, and the reverse -- a set-0 / set-1
mix-up in the merge cannot cancel there."""
import functools

import numpy as np
import pytest

import jpgx
import oracle as O

gpu = pytest.mark.gpu

SHAPES = {"128x8": (128, 8, 1), "72x8": (72, 8, 1), "256x16x2": (256, 16, 2), "832x8": (832, 8, 1)}
INPUTS = ["noise", "all0", "all255", "red", "green", "blue", "black_white", "white_black"]
QUALITIES = (1, 50, 90, 97)


@functools.lru_cache(maxsize=None)
def frames_of(shape, name):
    """uint8 [F][H][W][3], read-only"""
    W, H, F = SHAPES[shape]
    a = np.zeros((F, H, W, 3), np.uint8)
    if name == "noise":
        for f in range(F):
            a[f] = O.gen_splitmix(0x43725F74 + f, W, H)
    elif name == "all255":
        a[:] = 255
    elif name in ("red", "green", "blue"):
        a[..., ("red", "green", "blue").index(name)] = 255
    elif name in ("black_white", "white_black"):
        bpr, nb = W // 8, (W // 8) * (H // 8)
        for f in range(F):
            for by in range(H // 8):
                for bx in range(bpr):
                    right = (f * nb + by * bpr + bx) % 8 >= 4      # the step's block set 1
                    if right == (name == "black_white"):
                        a[f, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = 255
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(shape, name, q):
    """the oracle's int16 [F][3][nb][64], computed once per case"""
    w = np.stack([O.blocks(fr, q) for fr in frames_of(shape, name)])
    w.setflags(write=False)
    return w


def test_step_halves_differ_in_the_split_frames():
    """the generator: in every whole step, blocks 0..3 are one constant and 4..7 the other"""
    for shape, (W, H, F) in SHAPES.items():
        a = frames_of(shape, "black_white")
        b = frames_of(shape, "white_black")
        assert np.array_equal(a, 255 - b)
        blk = a.reshape(F, H // 8, 8, W // 8, 8, 3).transpose(0, 1, 3, 2, 4, 5).reshape(-1, 192)
        assert (blk.min(axis=1) == blk.max(axis=1)).all()
        assert np.array_equal(blk[:, 0] == 255, np.arange(len(blk)) % 8 >= 4)


@gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_cr_tile_matches_the_oracle(cuda, shape):
    import torch
    W, H, F = SHAPES[shape]
    nb = (W // 8) * (H // 8)
    fr = jpgx.frames(W, H, nframes=F)
    ws = torch.empty(max(jpgx.workspace_size(fr), 16), dtype=torch.uint8, device=cuda)
    for name in INPUTS:
        d_in = torch.from_numpy(frames_of(shape, name).copy()).to(cuda)
        for q in QUALITIES:
            ref = want(shape, name, q)
            for flags in (0, jpgx.FLAG_FORCE_EXACT):
                out = torch.full((F, 3, nb, 64), 0x5A5A, dtype=torch.int16, device=cuda)
                jpgx.blocks_gpu(fr, jpgx.default_params(W, H, q, 0, flags=flags), d_in, out, ws)
                got = out.cpu().numpy()
                bad = np.argwhere(got != ref)
                assert len(bad) == 0, (f"{shape} {name} q{q} flags {flags}: {len(bad)} mismatches, first (frame, "
                                       f"channel, block, k, got, want) "
                                       f"{[tuple(int(x) for x in b) + (int(got[tuple(b)]), int(ref[tuple(b)])) for b in bad[:4]]}")
                if F == 1 and flags == 0:           # the one-image entry point reaches the same kernel
                    one = jpgx.encode_blocks(d_in[0], q).cpu().numpy()
                    assert np.array_equal(one, ref[0]), f"{shape} {name} q{q}: encode_blocks"
