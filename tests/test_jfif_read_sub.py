"""The decoder that works inside a restart interval, on the host (csrc/jx_jfif_sub.h through
jpgx_read_jfif_sub of csrc/jpgx_jfif_read.cpp, the twin of the kernel k_jd_sub), and
the argument checks of jpgx_jfif_decode_gpu_ex.

The oracle is the host decoder jpgx_read_jfif on the same bytes (itself checked against an
independent decoder in tests/test_jfif_read.py), for the status, the coefficients and the tables;
every comparison is ==, for the shapes (16, 2), (16, 4), (32, 3) and the kernel's own."""
import numpy as np
import pytest

import jfif_san_cases as S
import jfif_sub_cases as K
import jpgx
import jpgx.compat as C
from jfif_inputs import hand_made, lap as _lap, stuffing_heavy

HEADER, SCAN = jpgx.EJFIF_HEADER, jpgx.EJFIF_SCAN
SUB = jpgx.JFIF_DECODE_SUBINTERVAL


def _rc(fn, *args):
    try:
        fn(*args)
    except jpgx.JpgxError as e:
        return e.rc
    return 0


def _same(data, shapes=K.SHAPES):
    """read_jfif_sub == read_jfif in every shape; the kernel's shape's counters"""
    ref = C.read_jfif(data, 1)
    stats = None
    for sub_bytes, tile_subs in shapes:
        got = C.read_jfif_sub(data, sub_bytes, tile_subs)
        assert got["coef"].dtype == np.int16 and got["coef"].shape == ref["coef"].shape
        assert np.array_equal(got["coef"], ref["coef"]), (sub_bytes, tile_subs)
        assert np.array_equal(got["qt"], ref["qt"])
        for key in ("width", "height", "sample_ratio", "restart_interval"):
            assert got[key] == ref[key]
        stats = got["stats"]
    return stats


def test_shape_and_exports():
    assert K.SUB >= 16 and K.SUB % 16 == 0 and K.TILE >= 2
    for name in ("jpgx_jfif_decode_gpu_workspace_size_ex", "jpgx_jfif_decode_gpu_ex", "jpgx_jfif_decode_sub_shape"):
        assert name in jpgx.EXPORTS and hasattr(jpgx.lib, name) and hasattr(jpgx.alt_library(), name)
    assert "jpgx_read_jfif_sub" in jpgx.COMPAT_EXPORTS and hasattr(jpgx.lib, "jpgx_read_jfif_sub")
    assert C.read_jfif_sub(K.big_file()[0], K.SUB, K.TILE)["stats"] == C.read_jfif_sub(K.big_file()[0])["stats"]


# ---- the inputs make the mechanism work, then parity ------------------------------------------------
def test_the_inputs_exercise_the_mechanism():
    inputs = K.mechanism_inputs()
    stats = {name: C.read_jfif_sub(data)["stats"] for name, (_, _, _, data) in inputs.items()}
    for name, st in stats.items():
        print(name, st)
    total = {k: sum(st[k] for st in stats.values()) for k in next(iter(stats.values()))}
    assert total["wrong_first_guesses"] > 0 and total["redecodes"] > 0
    assert max(st["rounds_max"] for st in stats.values()) >= 3
    assert total["starts_on_stuffing"] > 0 and total["units_across_sub"] > 0 and total["units_across_tile"] > 0
    # by the stuffing-heavy frame and Pillow's file alone, as the kernel's design was checked
    for name in ("stuffing, one row per interval", "pillow 4:2:0"):
        if name not in stats:                        # no Pillow here
            continue
        assert stats[name]["wrong_first_guesses"] > 0 and stats[name]["rounds_max"] >= 3
        assert stats[name]["starts_on_stuffing"] > 0 and stats[name]["units_across_sub"] > 0
    # a file of at least three tiles in one interval
    big = inputs["three tiles"][3]
    assert C.jfif_info(big)["restart_interval"] == 0 and stats["three tiles"]["tiles"] >= 3
    assert stats["three tiles"]["units_across_tile"] > 0
    assert K.intervals(big)[0][1] - K.intervals(big)[0][0] > 2 * K.SUB * K.TILE
    # intervals shorter than one subsequence, and one that is a whole number of subsequences
    short = K.intervals(inputs["short intervals"][3])
    assert len(short) == 250 and 0 < max(e - b for b, e in short) < K.SUB
    W, H, sr, _, data, k = K.whole_multiple()
    b, e = K.intervals(data)[k]
    assert e > b and (e - b) % K.SUB == 0
    for name, (_, _, _, data) in inputs.items():
        _same(data)


# ---- parity over tests/test_jfif_read.py's grid -------------------------------------------------------
@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("rr", [0, 1, 2, 3])
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_files_of_every_writer(sr, rr, optimize):
    W, H = (64, 80) if sr == 2 else (64, 72)         # 9 (5) MCU rows: a short last interval for rr 2, 3
    coef = _lap(W, H, sr, 10 * sr + rr)
    data = K.write(coef, W, H, 50, sr, rr, optimize)
    _same(data)
    assert np.array_equal(C.read_jfif_sub(data)["coef"].reshape(-1, 64), coef)


@pytest.mark.parametrize("q", [1, 50, 97])
def test_qualities(q):
    coef = _lap(64, 48, 0, 40 + q)
    _same(K.write(coef, 64, 48, q, 0, 2))


@pytest.mark.parametrize("W,H,sr", [(8, 8, 0), (16, 16, 2)])
def test_one_block_and_one_mcu(W, H, sr):
    coef = _lap(W, H, sr, 3)
    for rr in (0, 1):
        data = K.write(coef, W, H, 50, sr, rr)
        _same(data)
        assert np.array_equal(C.read_jfif_sub(data, 16, 2)["coef"].reshape(-1, 64), coef)


@pytest.mark.parametrize("sr", [0, 1, 2])
def test_hand_made_blocks_and_clamped_input(sr):
    coef = hand_made(sr, 64, 32)[2]
    for rr, opt in ((0, False), (1, False), (2, True)):
        _same(K.write(coef, 64, 32, 50, sr, rr, opt))


@pytest.mark.parametrize("sr", [0, 2])
def test_stuffing_heavy_frame(sr):
    for rr in (0, 1):
        data = K.write(stuffing_heavy(sr, 64, 96)[3], 64, 96, 50, sr, rr)
        assert data.count(b"\xff\x00") >= 1000
        assert _same(data)["starts_on_stuffing"] > 0


@pytest.mark.parametrize("subsampling,quality", [(2, 90), (2, 50), (0, 90)])
def test_pil_written_tiger(subsampling, quality):
    pytest.importorskip("PIL.Image")
    data = K.pillow_tiger(subsampling, quality)
    assert C.jfif_info(data)["restart_interval"] == 0 and C.jfif_info(data)["sample_ratio"] == subsampling
    _same(data)


# ---- refusals: the status is the host decoder's --------------------------------------------------------
def test_refusals_are_the_host_decoder_s():
    data = K.write(_lap(64, 48, 0, 21), 64, 48, 50, 0, 1)
    scan = C.jfif_info(data)["scan_offset"]
    marks = [i for i in range(scan, len(data) - 1) if data[i] == 0xFF and data[i + 1] & 0xF8 == 0xD0]
    single = K.write(_lap(64, 48, 2, 4), 64, 48, 50, 2, 0)
    big, pos, val = K.late_tile_flip()
    small, spos, sval = S.undefined_code_flip()
    bad = {
        "cut in the header": (data[:scan - 1], HEADER),
        "cut in the scan": (data[:scan + (len(data) - scan) // 2], SCAN),
        "cut at a marker": (data[:marks[2]], SCAN),
        "RST removed": (data[:marks[1]] + data[marks[1] + 2:], SCAN),
        "RST renumbered": (data[:marks[1] + 1] + b"\xd2" + data[marks[1] + 2:], SCAN),
        "no EOI": (data[:-2], SCAN),
        "a byte too many in an interval": (data[:marks[0]] + b"\x00" + data[marks[0]:], SCAN),
        "eight bits too many at the end": (data[:-2] + b"\x7f" + data[-2:], SCAN),
        "a byte too few in an interval": (data[:marks[0] - 1] + data[marks[0]:], SCAN),
        "a marker in an interval": (data[:marks[0] - 1] + b"\xff\xe0" + data[marks[0]:], SCAN),
        "an FF that ends an interval": (data[:marks[0]] + b"\xff" + data[marks[0]:], SCAN),
        "an FF without its 00 early in a long interval": (S.flipped(big, K.intervals(big)[0][0] + 70, 0xFF), SCAN),
        "the one interval running out": (single[:-40] + b"\xff\xd9", SCAN),
        "an undefined code": (S.flipped(small, spos, sval), SCAN),
        "a corruption in the third tile": (S.flipped(big, pos, val), SCAN),
    }
    for name, (b, want) in bad.items():
        assert _rc(C.read_jfif, b, 1) == want, name
        for shape in K.SHAPES:
            assert _rc(C.read_jfif_sub, b, *shape) == want, (name, shape)


def test_dc_out_of_int16_is_refused():
    """DC differences of +2047 that sum past 32767: every unit decodes, the running sum does not fit.
    A hand-written scan, since the writers clamp"""
    coef = np.zeros((3 * 40, 64), np.int16)
    data = bytearray(K.write(coef, 320, 8, 50, 0, 0))
    scan = C.jfif_info(bytes(data))["scan_offset"]
    # Annex K.3 luminance DC: size 11 is 111111110; chrominance DC size 0 is 00; EOB is 1010 / 00
    bits = ""
    for _ in range(40):
        bits += "111111110" + "1" * 11 + "1010" + "00" + "00" + "00" + "00"
    bits += "1" * (-len(bits) % 8)
    raw = int(bits, 2).to_bytes(len(bits) // 8, "big").replace(b"\xff", b"\xff\x00")
    bad = bytes(data[:scan]) + raw + b"\xff\xd9"
    assert _rc(C.read_jfif, bad, 1) == SCAN
    for shape in K.SHAPES:
        assert _rc(C.read_jfif_sub, bad, *shape) == SCAN
    ok_bits = ""                                     # 16 blocks of +2047: 32752 fits
    for k in range(40):
        ok_bits += ("111111110" + "1" * 11 if k < 16 else "00") + "1010" + "00" + "00" + "00" + "00"
    ok_bits += "1" * (-len(ok_bits) % 8)
    raw = int(ok_bits, 2).to_bytes(len(ok_bits) // 8, "big").replace(b"\xff", b"\xff\x00")
    good = bytes(data[:scan]) + raw + b"\xff\xd9"
    ref = C.read_jfif(good, 1)
    assert int(ref["coef"][0, 15, 0]) == 32752 and int(ref["coef"][0, 39, 0]) == 32752
    _same(good)


def test_capacity_and_arguments():
    data = K.write(_lap(64, 48, 0, 21), 64, 48, 50, 0, 1)
    buf = np.frombuffer(data, np.uint8)
    coef = np.zeros(3 * 48 * 64, np.int16)
    info = C.JfifInfo()
    call = jpgx.lib.jpgx_read_jfif_sub
    assert call(buf.ctypes.data, len(buf), 0, 0, coef.ctypes.data, coef.size - 1, None, info, None) == jpgx.EARG
    assert (info.width, info.height, info.nb_y, info.nb_c) == (64, 48, 48, 48)
    assert call(buf.ctypes.data, len(buf), 0, 0, coef.ctypes.data, coef.size, None, None, None) == 0
    assert call(None, len(buf), 0, 0, coef.ctypes.data, coef.size, None, None, None) == jpgx.EARG
    assert call(buf.ctypes.data, len(buf), 0, 0, None, coef.size, None, None, None) == jpgx.EARG
    for shape in ((15, 2), (16, 1), (0, 2), (64, 0), (1 << 16, 1 << 16)):
        assert call(buf.ctypes.data, len(buf), *shape, coef.ctypes.data, coef.size, None, None, None) == jpgx.EARG, shape


# ---- the routines under the sanitizers ------------------------------------------------------------------
@pytest.mark.skipif(not S.HAVE_CC, reason="needs gcc/g++ with libasan/libubsan")
def test_twin_under_asan_ubsan():
    """tests/c/jfif_sub_san.c, a program of its own, with host/*.c, the host plan and the host decoders
    under AddressSanitizer + UndefinedBehaviorSanitizer (nothing is preloaded): tests/c/jfif_read_san.c's
    sweep in the shapes (16, 2), (64, 256) and the kernel's own, every status and every status-0 frame's coefficients
    equal to jpgx_read_jfif's, and a three-tile file's corruptions, whose line and results are what
    jfif_sub_cases regenerates"""
    rc, out, err = K.run_program()
    assert rc == 0 and "jfif_sub_san: clean" in out, (out[-2000:], err[-4000:])
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-4000:]
    files = [ln.split() for ln in out.splitlines() if ln.startswith("file ")]
    shown = [ln.split() for ln in out.splitlines() if ln.startswith("flip ")]
    cases = [ln.split() for ln in out.splitlines() if ln.startswith("cases ")]
    assert int(cases[0][1]) >= 50000 and len(files) == 1 and len(shown) == K.BIG_FLIPS
    idx, W, H, sr, opt, n = (int(x) for x in files[0][1:7])
    assert (idx, W, H, sr, opt) == (K.BIG, K.BIG_W, K.BIG_H, 0, 0) and (n, int(files[0][7], 16)) == K.BIG_FILE
    data, _ = K.big_file()
    assert (len(data), S.fnv1a(data)) == K.BIG_FILE
    mine = S.flips(K.BIG, data, K.BIG_FLIPS)
    theirs = [(int(r[3]), int(r[4]), int(r[5])) for r in shown]
    assert [(p, v) for p, v, _ in theirs] == mine
    for (pos, val), (_, _, rc) in list(zip(mine, theirs))[:60]:
        assert rc == _rc(C.read_jfif, S.flipped(data, pos, val), 1), (pos, val)
    # the corruption the GPU test uploads is one of these, refused here under the sanitizers
    _, pos, val = K.late_tile_flip()
    assert (pos, val) == K.BIG_FLIP and (pos, val, SCAN) in theirs


# ---- jpgx_jfif_decode_gpu_ex's argument checks happen before any device call ---------------------------
def _call(files=0x10000, fstride=1 << 16, lens=0x20000, nf=1, W=64, H=64, sr=0, flags=SUB, coef=0x30000,
          cstride=3 * 64 * 64, qt=0x40000, status=0x50000, ws=0x60000, wsb=None):
    if wsb is None:
        wsb = jpgx.lib.jpgx_jfif_decode_gpu_workspace_size(W, H, sr, max(nf, 1), fstride) or 1 << 20
    return jpgx.lib.jpgx_jfif_decode_gpu_ex(files, fstride, lens, nf, W, H, sr, flags, coef, cstride, qt, status, ws,
                                            wsb, None)


@pytest.mark.parametrize("flags", [0, SUB])
def test_ex_refuses_bad_arguments_without_a_device(flags):
    def call(**kw):
        return _call(flags=flags, **kw)
    for name in ("files", "lens", "coef", "status", "ws"):
        assert call(**{name: None}) == jpgx.EARG, name
    assert call(lens=0x20004) == jpgx.EARG and call(coef=0x30008) == jpgx.EARG and call(status=0x50002) == jpgx.EARG
    assert call(qt=0x40001) == jpgx.EARG and call(ws=0x60008) == jpgx.EARG
    assert call(nf=0) == jpgx.EARG and call(nf=65536) == jpgx.EARG
    assert call(fstride=0) == jpgx.EARG and call(fstride=1 << 32) == jpgx.EARG
    assert call(cstride=3 * 64 * 64 + 32) == jpgx.EARG and call(cstride=3 * 64 * 64 - 64) == jpgx.EARG
    assert call(sr=3) == jpgx.EARG and call(sr=-1) == jpgx.EARG
    assert call(W=0) == jpgx.EARG and call(H=-8) == jpgx.EARG and call(W=65536) == jpgx.EARG
    assert call(W=60) == jpgx.EGEOMETRY and call(W=72, sr=1, cstride=1 << 20) == jpgx.EGEOMETRY
    assert call(H=72, sr=2, cstride=1 << 20) == jpgx.EGEOMETRY
    # the order: EARG before EGEOMETRY before EWORKSPACE, as jpgx_jfif_decode_gpu
    assert call(W=60, cstride=32) == jpgx.EGEOMETRY and call(W=60, nf=0) == jpgx.EARG
    assert call(cstride=32, wsb=1) == jpgx.EARG and call(wsb=1) == jpgx.EWORKSPACE


def test_ex_flags_and_sizes():
    size, size_ex = jpgx.lib.jpgx_jfif_decode_gpu_workspace_size, jpgx.lib.jpgx_jfif_decode_gpu_workspace_size_ex
    for unknown in (2, 3, 4, 1 << 31):
        assert _call(flags=unknown) == jpgx.EARG
        assert _call(flags=unknown, W=60) == jpgx.EARG          # before the geometry
        assert size_ex(64, 64, 0, 1, 1 << 16, unknown) == 0
    for sr, nf, cap in ((0, 1, 1 << 16), (2, 3, 40000), (1, 2, 4097)):
        need = size(64, 64, sr, nf, cap)
        assert need > 0 and size_ex(64, 64, sr, nf, cap, 0) == need
        assert 0 < size_ex(64, 64, sr, nf, cap, SUB) and size_ex(64, 64, sr, nf, cap, SUB) % 16 == 0
        nbc = (64, 32, 16)[sr]
        for flags in (0, SUB):
            want = size_ex(64, 64, sr, nf, cap, flags)
            assert _call(sr=sr, nf=nf, fstride=cap, cstride=(64 + 2 * nbc) * 64, flags=flags, wsb=want - 1) == jpgx.EWORKSPACE
    for bad in (dict(nf=0), dict(nf=65536), dict(sr=3), dict(W=60), dict(H=0), dict(cap=0), dict(cap=1 << 32)):
        a = dict(W=64, H=64, sr=0, nf=1, cap=1 << 16)
        a.update(bad)
        for flags in (0, SUB):
            assert size_ex(a["W"], a["H"], a["sr"], a["nf"], a["cap"], flags) == 0, bad


def test_bindings_refuse_host_tensors():
    torch = pytest.importorskip("torch")
    files, lens = torch.zeros((1, 4096), dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError):
        jpgx.jfif_decode_gpu(files, lens, 64, 64, subinterval=True)
    with pytest.raises(ValueError):
        jpgx.decode_jpeg_coefficients(K.big_file()[0], "cpu", subinterval=True)
    with pytest.raises(ValueError):
        jpgx.decode_jpeg(K.big_file()[0], "cpu", subinterval=True)
