"""Saturated inputs: blocks whose pixels are 0 or 255 by the sign of one coefficient's basis
function, the inputs that drive that coefficient as far as 8-bit pixels can (about twice what
noise reaches, half of DESIGN.md section 3's |coef| <= 2728), and all-0 / all-255 frames.  Three
parts of the kernels depend on magnitude: the f16-subnormal A operands at byte 255, the
fma(F, w, 1.5 * 2^23) low-16-bit quantiser, and the band table at its largest magnitudes.

The corpus is pinned on the CPU (the oracle's maximum |coef| per channel); on the GPU every
coefficient must equal the oracle's, on both libraries and in all three sample modes."""
import functools
import math

import numpy as np
import pytest

import jpgx
import oracle as O

gpu = pytest.mark.gpu

# the reference's colour rows (src/preprocess.c), the Cb row with its sign bug
COL = ((0.299, 0.587, 0.114), (-0.168736, 0.331264, -0.5), (0.5, -0.418688, -0.081312))
NPAT = 3 * 8 * 8 * 2
BLOCK_ROWS, BLOCKS_PER_ROW = 9, NPAT + 8


def saturated_blocks():
    """uint8 [384][8][8][3] (y, x, byte): channel c, (u, v), sign s; byte k of pixel (x, y) is 255
    where s * COL[c][k] * cos_u[x] * cos_v[y] > 0, else 0."""
    cos = [[math.cos((2 * x + 1) * u * math.pi / 16) for x in range(8)] for u in range(8)]
    out = np.zeros((NPAT, 8, 8, 3), np.uint8)
    i = 0
    for c in range(3):
        for u in range(8):
            for v in range(8):
                for s in (1.0, -1.0):
                    for y in range(8):
                        for x in range(8):
                            for k in range(3):
                                if s * COL[c][k] * cos[u][x] * cos[v][y] > 0:
                                    out[i, y, x, k] = 255
                    i += 1
    return out


@functools.lru_cache(maxsize=None)
def corpus_frame(rep_x=1, rep_y=1):
    """9 block rows of 392 blocks: row 0 blank; row 1 + s holds s blank blocks, the 384 patterns,
    then blank blocks -- every pattern at every position 0..7 of an 8-block step, none the last
    block of its row.  rep_x / rep_y repeat every pixel (for 4:2:2 / 4:2:0: every chroma sample is
    then the saturated value itself)."""
    pats = saturated_blocks()
    rgb = np.zeros((8 * BLOCK_ROWS, 8 * BLOCKS_PER_ROW, 3), np.uint8)
    for s in range(8):
        for i in range(NPAT):
            rgb[8 * (1 + s):8 * (2 + s), 8 * (s + i):8 * (s + i + 1)] = pats[i]
    rgb = np.repeat(np.repeat(rgb, rep_x, axis=1), rep_y, axis=0)
    rgb.setflags(write=False)
    return rgb


def _frame(name, sr):
    if name == "corpus":
        return corpus_frame(2 if sr else 1, 2 if sr == 2 else 1)
    a = np.full((32, 64, 3), 0 if name == "all0" else 255, np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _want(name, sr, q):
    rgb = _frame(name, sr)
    if sr == 0:
        return O.blocks(rgb, q).reshape(-1, 64)
    return np.concatenate([O.blocks(rgb, q, sr)[0], O.chroma_sub(rgb, q, sr).reshape(-1, 64)])


def test_corpus_reaches_the_recorded_maxima():
    """Recorded from the oracle: the generator must not silently weaken."""
    rgb = corpus_frame()
    assert rgb.shape == (72, 3136, 3)
    assert len({b.tobytes() for b in saturated_blocks()}) == NPAT
    for q, want in ((97, (1024, 1364, 1020)), (90, (471, 455, 340))):
        coef = O.blocks(rgb, q).astype(np.int64)
        assert tuple(int(np.abs(coef[c]).max()) for c in range(3)) == want, q


@pytest.fixture(params=["alt", "product"])
def impl(request, monkeypatch):
    """product: libjpgx.so (k_mxs, k_mx422, k_mx420).  alt: libjpgx_alt.so (k_xform, k_chroma)."""
    if request.param == "alt":
        monkeypatch.setattr(jpgx, "lib", jpgx.alt_library())
    return request.param


RUNS = [(1, 0), (50, 0), (90, 0), (97, 0), (97, jpgx.FLAG_FORCE_EXACT)]


def _check(cuda, name, sr):
    import torch
    d = torch.from_numpy(_frame(name, sr)).to(cuda)
    S = jpgx.FLAG_SUBSAMPLE if sr else 0
    for q, flags in RUNS:
        got = jpgx.encode_blocks(d, q, sr, flags=S | flags).cpu().numpy().reshape(-1, 64)
        want = _want(name, sr, q)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (f"{name} sr{sr} q{q} flags {flags}: {len(bad)} mismatches, first "
                               f"{[(b, k, int(got[b, k]), int(want[b, k])) for b, k in bad[:4]]}")


@gpu
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_saturated_blocks(cuda, impl, sr):
    _check(cuda, "corpus", sr)


@gpu
@pytest.mark.parametrize("sr", [0, 1, 2])
@pytest.mark.parametrize("name", ["all0", "all255"])
def test_constant_extreme_frames(cuda, impl, sr, name):
    _check(cuda, name, sr)
