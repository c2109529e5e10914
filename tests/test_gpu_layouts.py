"""The device ABI's layout fields and the launch residues on the GPU (include/jpgx.h:
jpgx_frames.in_pitch, in_frame_stride, out_frame_stride).

Layouts: the input rows lie `in_pitch` apart, the frames `in_frame_stride` apart, frame 0 starts 8
bytes into its allocation, and every byte that is no pixel is noise of another seed, so a read
through the wrong pitch or stride, or of padding, changes coefficients.  The output is prefilled
with 0x7A7A (no coefficient has that value), the frames' outputs lie `out_frame_stride` apart, and
the gaps between them and a guard region behind the last must come back untouched.

Residues: k_mxs / k_mx422 / k_mx420 work in steps of 8 blocks, 3 steps per wave and 4 waves per
workgroup with no loop, so every total modulo 8, 24 and 96 is a tail case of its own (clamped
copies in the last step, idle steps in the last wave, idle waves in the last workgroup).

Expected values are the oracle's on the unpadded frames, compared with np.array_equal; every GPU
test runs on the product library (k_mxs, and k_mx422 / k_mx420 for true 4:2:2 / 4:2:0: "mx" /
"fused" elsewhere in the suite) and on the test-only cross-check library (k_xform, with k_chroma
for 4:2:x: "xform" / "two-pass")."""
import ctypes
import functools

import numpy as np
import pytest

import jpgx
import oracle as O

gpu = pytest.mark.gpu
SENTINEL = 0x7A7A
GUARD = 4096
UF = np.arange(24, dtype=np.uint8).reshape(3, 8) * 7 + 3    # distinct per plane (test_edge_geometries)


@pytest.fixture(params=["alt", "product"])
def impl(request, monkeypatch):
    """product: libjpgx.so (k_mxs, k_mx422, k_mx420).  alt: libjpgx_alt.so (k_xform, k_chroma)."""
    if request.param == "alt":
        monkeypatch.setattr(jpgx, "lib", jpgx.alt_library())
    return request.param


# ---- frames and their oracle outputs (computed once, shared by both libraries) -------------------
@functools.lru_cache(maxsize=None)
def _source(kind, seed, W, H):
    a = O.gen_tie(W, H) if kind == "T" else O.gen_splitmix(seed, W, H)
    a.setflags(write=False)
    return a


def _cut(kind, seed, W, H, F, across):
    """F frames of W x H cut from one F-fold frame: side by side (`across`, the wide frame of a
    sweep cut into its blocks / MCUs) or stacked.  Tie frames cut this way differ from one another
    (gen_tie's block value depends on the block index), so a mixed-up frame shows."""
    big = _source(kind, seed, W * F, H) if across else _source(kind, seed, W, H * F)
    return [np.ascontiguousarray(big[:, f * W:(f + 1) * W] if across else big[f * H:(f + 1) * H])
            for f in range(F)]


@functools.lru_cache(maxsize=None)
def _want(kind, seed, W, H, F, across, f, q, sr, rows, uf):
    """One frame's expected output, flat: [3][nb][64] for sr 0, else Y | Cb | Cr.  (One oracle
    thread: the frames are small, and a thread team per call costs more than the work.)"""
    rgb = _cut(kind, seed, W, H, F, across)[f]
    under = UF if uf else None
    if sr == 0:
        out = O.blocks(rgb, q, underflow=under, rows=rows, nthreads=1).reshape(-1)
    else:
        crows = None if rows is None else ((rows[0], rows[1]) if sr == 1 else (rows[0] // 2, rows[1] // 2))
        out = np.concatenate([O.blocks(rgb, q, sr, underflow=under, rows=rows, nthreads=1)[0].reshape(-1),
                              O.chroma_sub(rgb, q, sr, crows=crows, nthreads=1).reshape(-1)])
    out.setflags(write=False)
    return out


def _poison(n, seed):
    return O.gen_splitmix(seed, 64, (n + 191) // 192).reshape(-1)[:n].copy()


def padded_input(frames, in_pitch, in_frame_stride, seed=0xBAD):
    """The host image of a device input buffer: frame f's pixel row y at 8 + f * in_frame_stride +
    y * in_pitch, every other byte (the 8-byte lead-in, row and frame padding) splitmix noise."""
    H, W = frames[0].shape[:2]
    assert in_pitch >= 3 * W and in_frame_stride >= in_pitch * (H - 1) + 3 * W
    buf = _poison(8 + len(frames) * in_frame_stride, seed)
    for f, fr in enumerate(frames):
        for y in range(H):
            o = 8 + f * in_frame_stride + y * in_pitch
            buf[o:o + 3 * W] = fr[y].reshape(-1)
    return buf


def _launch(cuda, frames, q, sr, flags=0, pitch=None, fstride=None, ostride=None, rows=None,
            underflow=None):
    """One jpgx_blocks_gpu launch over `frames` in the given layout -> (host copy of the whole
    output buffer, elements per frame, out_frame_stride)."""
    import torch
    H, W = frames[0].shape[:2]
    F = len(frames)
    S = jpgx.FLAG_SUBSAMPLE if sr else 0
    r0, r1 = rows if rows is not None else (0, H // 8)
    nb = (r1 - r0) * (W // 8)
    per = (nb + 2 * jpgx.chroma_blocks(W, r0, r1, sr, S)) * 64
    pitch = 3 * W if pitch is None else pitch
    fstride = pitch * H if fstride is None else fstride
    ostride = per if ostride is None else ostride
    d_in = torch.from_numpy(padded_input(frames, pitch, fstride)).to(cuda)
    assert d_in.data_ptr() % 16 == 0
    buf = torch.full((F * ostride + GUARD,), SENTINEL, dtype=torch.int16, device=cuda)
    fr = jpgx.frames(W, H, nframes=F, rows=rows, in_pitch=pitch, in_frame_stride=fstride,
                     out_frame_stride=ostride)
    ws = torch.empty(max(jpgx.workspace_size(fr), 16), dtype=torch.uint8, device=cuda)
    jpgx.blocks_gpu(fr, jpgx.default_params(W, H, q, sr, underflow, flags | S),
                    d_in.data_ptr() + 8 + 8 * r0 * pitch, buf, ws)
    got = buf.cpu().numpy()
    del d_in
    return got, per, ostride


def _compare(got, per, ostride, wants, what):
    F = len(wants)
    assert (got[F * ostride:] == SENTINEL).all(), f"{what}: write into the guard region"
    for f, want in enumerate(wants):
        seg = got[f * ostride:(f + 1) * ostride]
        assert want.size == per
        bad = np.flatnonzero(seg[:per] != want)
        assert bad.size == 0, f"{what} frame {f}: {bad.size} mismatches, first {bad[:6].tolist()}"
        assert (seg[per:] == SENTINEL).all(), f"{what} frame {f}: write into the gap behind it"


# ---- A. strides, alignment, gaps -----------------------------------------------------------------
DATA = {"random": ("G", 85, 0), "tie": ("T", 50, 0), "exact": ("G", 85, jpgx.FLAG_FORCE_EXACT)}


def _geometries(sr):
    """17 blocks per block row (sr 0) or 17 MCUs per MCU row (4:2:x needs W % 16 == 0, so 272
    there, not 136): simple steps, a step with the quirk block inside, steps across rows and
    frames.  48 wide: every step is general."""
    return [(136 if sr == 0 else 272, 32, 3), (48, 16, 5)]


@gpu
@pytest.mark.parametrize("data", sorted(DATA))
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_padded_strides_and_output_gaps(cuda, impl, sr, data):
    kind, q, flags = DATA[data]
    for W, H, F in _geometries(sr):
        frames = _cut(kind, 4000 + W, W, H, F, False)
        wants = [_want(kind, 4000 + W, W, H, F, False, f, q, sr, None, False) for f in range(F)]
        for pitch in (3 * W + 8, 3 * W + 40, 2 * 3 * W):
            for gap in (8, 72):          # + 8: frame bases 16-byte but not 128-byte aligned
                got, per, ostride = _launch(cuda, frames, q, sr, flags, pitch, pitch * H + 24,
                                            wants[0].size + gap)
                _compare(got, per, ostride, wants, f"{W}x{H}x{F} pitch {pitch} gap {gap}")


@gpu
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_padded_stripe_reads_its_halo_through_the_pitch(cuda, impl, sr):
    """A stripe that starts below block row 0: the pointer is at pixel row 8 * row_begin and the
    quirk block's first pixel row is the row above it, at the padded pitch."""
    rows = (2, 4) if sr == 2 else (1, 3)
    for data in sorted(DATA):
        kind, q, flags = DATA[data]
        for W, H, F in _geometries(sr):
            H = max(H, 8 * rows[1])
            frames = _cut(kind, 4100 + W, W, H, F, False)
            wants = [_want(kind, 4100 + W, W, H, F, False, f, q, sr, rows, False) for f in range(F)]
            for pitch in (3 * W + 8, 3 * W + 40, 2 * 3 * W):
                got, per, ostride = _launch(cuda, frames, q, sr, flags, pitch, pitch * H + 24,
                                            wants[0].size + 8, rows=rows)
                _compare(got, per, ostride, wants, f"{data} {W}x{H}x{F} rows {rows} pitch {pitch}")


@pytest.mark.parametrize("sr", [0, 1, 2])
def test_layout_argument_codes(sr):
    """Validation happens before any device work (the pointers are never dereferenced)."""
    W, H = 48, 16
    S = jpgx.FLAG_SUBSAMPLE if sr else 0
    per = (12 + 2 * jpgx.chroma_blocks(W, 0, 2, sr, S)) * 64
    p = jpgx.default_params(W, H, 85, sr, flags=S)
    fake = 1 << 20

    def rc(F=1, **kw):
        kw.setdefault("out_frame_stride", per)
        fr = jpgx.frames(W, H, nframes=F, **kw)
        return jpgx.lib.jpgx_blocks_gpu(ctypes.byref(fr), ctypes.byref(p), fake, fake, fake, 1 << 20, None)

    assert rc(in_pitch=3 * W + 4) == jpgx.EARG                       # not a multiple of 8
    assert rc(in_pitch=3 * W - 8) == jpgx.EARG                       # rows overlap
    assert rc(F=2, in_pitch=3 * W + 8, in_frame_stride=(3 * W + 8) * (H - 1)) == jpgx.EARG
    assert rc(F=2, out_frame_stride=per - 64) == jpgx.EARG           # frames' outputs overlap
    assert rc(out_frame_stride=per + 4) == jpgx.EARG                 # 8-byte aligned frame bases
    assert rc(F=2, in_pitch=3 * W + 4, in_frame_stride=(3 * W + 8) * H) == jpgx.EARG


# ---- B. launch residues --------------------------------------------------------------------------
SWEEP_444 = list(range(1, 51)) + list(range(94, 99)) + list(range(190, 195))
SWEEP_SUB = list(range(1, 27)) + list(range(47, 50))


def _sweep(cuda, sr, counts, unit_w, H):
    """Every count n as (W = unit_w * n, F = 1) and as (W = unit_w, F = n): the second from the
    same pixels cut into n frames, each block / MCU the last of its row (x0 = -8 quirk at block
    row 0: the underflow table).  Returns the counts that ran."""
    done = []
    for n in counts:
        kind, q = ("T", 50) if n % 2 else ("G", 85)
        flags = jpgx.FLAG_FORCE_EXACT if n % 5 == 0 else 0
        for W, F, across, uf in ((unit_w * n, 1, False, False), (unit_w, n, True, True)):
            seed = 5000 + n
            frames = _cut(kind, seed, W, H, F, across)
            wants = [_want(kind, seed, W, H, F, across, f, q, sr, None, uf) for f in range(F)]
            got, per, ostride = _launch(cuda, frames, q, sr, flags, underflow=UF if uf else None)
            _compare(got, per, ostride, wants, f"n {n} as {W}x{H}x{F}")
        done.append(n)
    return done


def _required_444():
    return set(range(1, 51)) | {94, 95, 96, 97, 98} | {190, 191, 192, 193, 194}


def _required_sub():
    return set(range(1, 27)) | {47, 48, 49}


def test_sweeps_cover_every_residue():
    """The lists the sweeps loop over, against the counts they must reach, and what those counts
    are for: every residue modulo 8 (blocks of a step), 24 (of a wave) and, for 4:4:4, the wave
    counts 1..4 and 5 (a second workgroup) and 8, 9."""
    assert set(SWEEP_444) >= _required_444() and set(SWEEP_SUB) >= _required_sub()
    assert {t % 8 for t in SWEEP_444} == set(range(8)) and {t % 24 for t in SWEEP_444} == set(range(24))
    assert {-(-t // 24) for t in SWEEP_444} >= {1, 2, 3, 4, 5, 8, 9}
    for blocks_per_mcu in (2, 4):
        assert {(m * blocks_per_mcu) % 8 for m in SWEEP_SUB} == set(range(0, 8, blocks_per_mcu))
        assert {(m * blocks_per_mcu) % 24 for m in SWEEP_SUB} == set(range(0, 24, blocks_per_mcu))


@gpu
def test_launch_residues_444(cuda, impl):
    assert set(_sweep(cuda, 0, SWEEP_444, 8, 8)) >= _required_444()


@gpu
def test_launch_residues_422(cuda, impl):
    assert set(_sweep(cuda, 1, SWEEP_SUB, 16, 8)) >= _required_sub()


@gpu
def test_launch_residues_420(cuda, impl):
    assert set(_sweep(cuda, 2, SWEEP_SUB, 16, 16)) >= _required_sub()
