"""The host JFIF decoder (csrc/jpgx_jfif_read.cpp over csrc/jx_jfif_dec.h: jpgx_read_jfif,
jpgx_jfif_info_of) and the device entry point's argument checks.

Oracles: the independent T.81 decoder tests/jfif_decode.py on the same bytes, and the coefficients
the files were written from.  Every comparison is ==.  (4:2:0 cases that ask for a short last
interval use 64x80 instead of 64x72: a 4:2:0 MCU is 16 rows high.)"""
import io
import os

import numpy as np
import pytest

import jfif_san_cases as S
import jpgx
import jpgx.compat as C
from conftest import GOLDEN, coef_sha
from jfif_decode import decode
from jfif_inputs import hand_made, lap as _lap, nblocks as _nblocks, stuffing_heavy

HEADER, SCAN = jpgx.EJFIF_HEADER, jpgx.EJFIF_SCAN


def _write(coef, W, H, q, sr, rr, optimize=False):
    """rr 0: the writers without restart intervals (write_jfif, write_jfif_sub), else write_jfif_ex"""
    if rr == 0 and not optimize:
        return C.write_jfif(coef.reshape(3, -1, 64), W, H, q) if sr == 0 else C.write_jfif_sub(coef, W, H, q, sr)
    return C.write_jfif_ex(coef, W, H, q, sr, restart_rows=rr, nthreads=1, optimize=optimize)


def _flat(x):
    return np.concatenate([np.asarray(c).reshape(-1, 64) for c in x])


def _check_against_independent(data, nthreads=1):
    ref = decode(data)
    got = C.read_jfif(data, nthreads)
    assert got["coef"].dtype == np.int16 and got["qt"].dtype == np.uint16
    assert np.array_equal(_flat(got["coef"]).astype(np.int32), _flat(ref["coef"]))
    assert (got["width"], got["height"]) == (ref["width"], ref["height"])
    assert got["sample_ratio"] == {(1, 1): 0, (2, 1): 1, (2, 2): 2}[ref["sampling"]]
    assert got["restart_interval"] == ref["restart_interval"]
    assert got["qt"][0].tolist() == ref["dqt"][ref["qsel"][0]]
    assert got["qt"][1].tolist() == ref["dqt"][ref["qsel"][1]] == ref["dqt"][ref["qsel"][2]]
    return got


def _rc(data, nthreads=1):
    try:
        C.read_jfif(data, nthreads)
    except jpgx.JpgxError as e:
        return e.rc
    return 0


def _independent_fails(data):
    try:
        decode(data)
    except (AssertionError, ValueError, IndexError, KeyError):
        return True
    return False


# ---- parity with the independent decoder and with the coefficients coded --------------------------
@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("rr", [0, 1, 2, 3])
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_files_of_every_writer(sr, rr, optimize):
    W, H = (64, 80) if sr == 2 else (64, 72)         # 9 (5) MCU rows: a short last interval for rr 2, 3
    coef = _lap(W, H, sr, 10 * sr + rr)
    data = _write(coef, W, H, 50, sr, rr, optimize)
    got = _check_against_independent(data)
    assert np.array_equal(_flat(got["coef"]), coef)  # inside the writers' clamps: the input comes back
    assert got["coef"].shape == ((3, coef.shape[0] // 3, 64) if sr == 0 else coef.shape)
    assert got["restart_interval"] == rr * (W // (16 if sr else 8))


@pytest.mark.parametrize("q", [1, 50, 97])
def test_qualities(q):
    coef = _lap(64, 48, 0, 40 + q)
    data = _write(coef, 64, 48, q, 0, 2)
    got = _check_against_independent(data)
    assert np.array_equal(_flat(got["coef"]), coef)
    if q == 1:
        assert decode(data)["sof"] == 0xC1 and int(got["qt"].max()) > 255      # 16-bit DQT entries


@pytest.mark.parametrize("W,H,sr", [(8, 8, 0), (16, 16, 2)])
def test_one_block_and_one_mcu(W, H, sr):
    coef = _lap(W, H, sr, 3)
    for rr in (0, 1):
        got = _check_against_independent(_write(coef, W, H, 50, sr, rr))
        assert np.array_equal(_flat(got["coef"]), coef)


@pytest.mark.parametrize("sr", [0, 1, 2])
def test_hand_made_blocks_and_clamped_input(sr):
    coef = hand_made(sr, 64, 32)[2]
    for rr, opt in ((0, False), (1, False), (2, True)):
        _check_against_independent(_write(coef, 64, 32, 50, sr, rr, opt))


@pytest.mark.parametrize("sr", [0, 2])
def test_stuffing_heavy_frame(sr):
    data = _write(stuffing_heavy(sr, 64, 96)[3], 64, 96, 50, sr, 1)
    assert data.count(b"\xff\x00") >= 1000
    _check_against_independent(data, nthreads=3)


def test_thread_count_does_not_show():
    coef = _lap(64, 72, 1, 77)
    data = _write(coef, 64, 72, 60, 1, 1)
    first = C.read_jfif(data, 1)
    assert np.array_equal(first["coef"], coef)
    for n in (2, 5, 64):
        got = C.read_jfif(data, n)
        assert np.array_equal(got["coef"], first["coef"]) and np.array_equal(got["qt"], first["qt"])


def test_golden_photo(golden):
    ref = np.load(os.path.join(GOLDEN, "cam_q75_ref.npy"))
    rgb, _ = C.bmp_read(os.path.join(GOLDEN, "images", "cam.bmp"))
    H, W = rgb.shape[:2]
    for opt in (False, True):
        data = C.write_jfif_ex(ref, W, H, 75, 0, restart_rows=1, nthreads=2, optimize=opt)
        got = C.read_jfif(data, 4)
        assert np.array_equal(got["coef"], ref)
        assert coef_sha(got["coef"]) == golden["images"]["cam"]["coef_sha256"]["75"]


# ---- other writers' files --------------------------------------------------------------------------
def _segments(data):
    """[(marker, offset, length with the marker)] from SOI to SOS"""
    out, i = [], 2
    while True:
        ln = data[i + 2] << 8 | data[i + 3]
        out.append((data[i + 1], i, 2 + ln))
        if data[i + 1] == 0xDA:
            return out
        i += 2 + ln


def _segment(data, marker, first=None):
    for m, at, n in _segments(data):
        if m == marker and (first is None or data[at + 4] == first):
            return at, n
    raise KeyError(marker)


def test_com_and_app1_segments_are_skipped():
    coef = _lap(64, 48, 2, 5)
    data = _write(coef, 64, 48, 50, 2, 1)
    at, _ = _segment(data, 0xDB)
    text = b"hello\xff\xd0\xff\xd9x"                                              # marker-like bytes in a comment
    com = b"\xff\xfe" + (2 + len(text)).to_bytes(2, "big") + text
    app1 = b"\xff\xe1" + (2 + 6).to_bytes(2, "big") + b"Exif\0\0"
    more = data[:at] + com + app1 + data[at:]
    a, b = C.read_jfif(data), _check_against_independent(more)
    assert np.array_equal(a["coef"], b["coef"]) and np.array_equal(a["qt"], b["qt"])
    assert C.jfif_info(more)["scan_offset"] == C.jfif_info(data)["scan_offset"] + len(com) + len(app1)


@pytest.mark.parametrize("subsampling", [0, 2])
def test_pil_written_file(subsampling):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(9)
    small = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    rgb = np.clip(small.repeat(8, 0).repeat(8, 1).astype(np.int16) + rng.integers(-9, 10, (48, 64, 3)), 0, 255)
    buf = io.BytesIO()
    Image.fromarray(rgb.astype(np.uint8)).save(buf, "JPEG", quality=85, optimize=False, subsampling=subsampling)
    got = _check_against_independent(buf.getvalue())
    assert got["sample_ratio"] == subsampling and got["restart_interval"] == 0


# ---- refusals --------------------------------------------------------------------------------------
def _base():
    coef = _lap(64, 48, 0, 21)
    return _write(coef, 64, 48, 50, 0, 1)


def _patched(data, at, new):
    return data[:at] + bytes(new) + data[at + len(new):]


def test_header_refusals():
    data = _base()
    assert _rc(data) == 0
    sof, n = _segment(data, 0xC0)
    bad = {
        "progressive": _patched(data, sof + 1, [0xC2]),
        "12 bit": _patched(data, sof + 4, [12]),
        "lossless": _patched(data, sof + 1, [0xC3]),
        "arithmetic": _patched(data, sof + 1, [0xC9]),
    }
    seg = data[sof:sof + n]
    one = seg[:2] + (8 + 3).to_bytes(2, "big") + seg[4:9] + b"\x01" + seg[10:13]
    four = seg[:2] + (8 + 12).to_bytes(2, "big") + seg[4:9] + b"\x04" + seg[10:19] + b"\x04\x11\x01"
    bad["1 component"] = data[:sof] + one + data[sof + n:]
    bad["4 components"] = data[:sof] + four + data[sof + n:]
    dht, _ = _segment(data, 0xC4, 0x00)              # DC luminance: bits 0 1 5 1 1 1 1 1 1 0 ...
    assert list(data[dht + 5:dht + 9]) == [0, 1, 5, 1]
    bad["over-subscribed"] = _patched(data, dht + 5, [3, 1, 2])                # three 1-bit codes, the same total
    at, n = _segment(data, 0xC4, 0x11)
    bad["undefined table"] = data[:at] + data[at + n:]
    scan = C.jfif_info(data)["scan_offset"]
    for cut in (0, 1, 3, 10, sof + 5, dht + 9, scan - 1):
        bad[f"cut {cut}"] = data[:cut]
    bad["chroma 2x1"] = _patched(data, sof + 4 + 10, [0x21])
    bad["luma 4x1"] = _patched(data, sof + 4 + 7, [0x41])
    bad["no SOI"] = b"\xff\xd9" + data[2:]
    bad["DAC"] = data[:sof] + b"\xff\xcc\x00\x04\x00\x11" + data[sof:]
    for name, b in bad.items():
        assert _rc(b) == HEADER, name
        with pytest.raises(jpgx.JpgxError):
            C.jfif_info(b)
    # a width that is no multiple of the 4:2:2 MCU
    sub = _write(_lap(64, 48, 1, 2), 64, 48, 50, 1, 1)
    sof, _ = _segment(sub, 0xC0)
    assert _rc(_patched(sub, sof + 4 + 3, (72).to_bytes(2, "big"))) == HEADER


def test_scan_refusals():
    data = _base()
    scan = C.jfif_info(data)["scan_offset"]
    marks = [i for i in range(scan, len(data) - 1) if data[i] == 0xFF and data[i + 1] & 0xF8 == 0xD0]
    assert len(marks) == 5 and [data[i + 1] & 7 for i in marks] == [0, 1, 2, 3, 4]
    bad = {
        "cut in the scan": data[:scan + (len(data) - scan) // 2],
        "cut at a marker": data[:marks[2]],
        "cut after a marker": data[:marks[2] + 2],
        "RST removed": data[:marks[1]] + data[marks[1] + 2:],
        "last RST removed": data[:marks[4]] + data[marks[4] + 2:],
        "RST renumbered": _patched(data, marks[1] + 1, [0xD2]),
        "RST added": data[:marks[1]] + b"\xff\xd1" + data[marks[1]:],
        "no EOI": data[:-2],
        "EOI damaged": data[:-1] + b"\xd8",
        "bytes after EOI": data + b"\0",
        "a byte too many in an interval": data[:marks[0]] + b"\x00" + data[marks[0]:],
        "a byte too few in an interval": data[:marks[0] - 1] + data[marks[0]:],
        "a marker in an interval": data[:marks[0] - 1] + b"\xff\xe0" + data[marks[0]:],
    }
    for name, b in bad.items():
        assert _rc(b) == SCAN, name
        assert C.jfif_info(b)["width"] == 64          # the header is still fine
    for name in ("cut in the scan", "RST removed", "RST renumbered", "no EOI"):
        assert _independent_fails(bad[name]), name
    small, pos, val = S.undefined_code_flip()
    assert _rc(small) == 0 and _rc(S.flipped(small, pos, val)) == SCAN
    # without restart intervals a dropped tail is the one interval running out
    single = _write(_lap(64, 48, 2, 4), 64, 48, 50, 2, 0)
    assert _rc(single) == 0 and _rc(single[:-40] + b"\xff\xd9") == SCAN


def test_results_do_not_depend_on_threads_when_refused():
    data = _base()
    scan = C.jfif_info(data)["scan_offset"]
    b = S.flipped(data, scan + 100, data[scan + 100] ^ 0x55)
    assert len({_rc(b, n) for n in (1, 2, 5, 64)}) == 1


def test_capacity_and_arguments():
    data = _base()
    buf = np.frombuffer(data, np.uint8)
    coef = np.zeros(3 * 48 * 64, np.int16)
    info = C.JfifInfo()
    call = jpgx.lib.jpgx_read_jfif
    assert call(buf.ctypes.data, len(buf), 1, coef.ctypes.data, coef.size - 1, None, info) == jpgx.EARG
    assert (info.width, info.height, info.nb_y, info.nb_c) == (64, 48, 48, 48)
    assert call(buf.ctypes.data, len(buf), 1, coef.ctypes.data, coef.size, None, None) == 0
    assert call(None, len(buf), 1, coef.ctypes.data, coef.size, None, None) == jpgx.EARG
    assert call(buf.ctypes.data, len(buf), 1, None, coef.size, None, None) == jpgx.EARG
    assert call(buf.ctypes.data, len(buf), -1, coef.ctypes.data, coef.size, None, None) == jpgx.EARG
    assert "EJFIF_SCAN" in str(jpgx.JpgxError(SCAN, "x")) and "EJFIF_HEADER" in str(jpgx.JpgxError(HEADER, "x"))


# ---- the device entry point's argument checks happen before any device call -----------------------
def _call(files=0x10000, fstride=1 << 16, lens=0x20000, nf=1, W=64, H=64, sr=0, coef=0x30000, cstride=3 * 64 * 64,
          qt=0x40000, status=0x50000, ws=0x60000, wsb=None):
    if wsb is None:
        wsb = jpgx.lib.jpgx_jfif_decode_gpu_workspace_size(W, H, sr, max(nf, 1), fstride) or 1 << 20
    return jpgx.lib.jpgx_jfif_decode_gpu(files, fstride, lens, nf, W, H, sr, coef, cstride, qt, status, ws, wsb, None)


def test_bad_arguments_are_refused_without_a_device():
    for name in ("files", "lens", "coef", "status", "ws"):
        assert _call(**{name: None}) == jpgx.EARG, name
    assert _call(lens=0x20004) == jpgx.EARG           # 8-byte alignment
    assert _call(coef=0x30008) == jpgx.EARG           # 16
    assert _call(status=0x50002) == jpgx.EARG         # 4
    assert _call(qt=0x40001) == jpgx.EARG             # 2
    assert _call(ws=0x60008) == jpgx.EARG             # 16
    assert _call(nf=0) == jpgx.EARG and _call(nf=65536) == jpgx.EARG
    assert _call(fstride=0) == jpgx.EARG and _call(fstride=1 << 32) == jpgx.EARG
    assert _call(cstride=3 * 64 * 64 + 32) == jpgx.EARG
    assert _call(cstride=3 * 64 * 64 - 64) == jpgx.EARG
    assert _call(sr=3) == jpgx.EARG and _call(sr=-1) == jpgx.EARG
    assert _call(W=0) == jpgx.EARG and _call(H=-8) == jpgx.EARG and _call(W=65536) == jpgx.EARG
    assert _call(W=60) == jpgx.EGEOMETRY and _call(W=72, sr=1, cstride=1 << 20) == jpgx.EGEOMETRY
    assert _call(H=72, sr=2, cstride=1 << 20) == jpgx.EGEOMETRY
    size = jpgx.lib.jpgx_jfif_decode_gpu_workspace_size
    for bad in (dict(nf=0), dict(nf=65536), dict(sr=3), dict(W=60), dict(H=0), dict(cap=0), dict(cap=1 << 32)):
        a = dict(W=64, H=64, sr=0, nf=1, cap=1 << 16)
        a.update(bad)
        assert size(a["W"], a["H"], a["sr"], a["nf"], a["cap"]) == 0, bad


def test_workspace_one_byte_short():
    size = jpgx.lib.jpgx_jfif_decode_gpu_workspace_size
    for sr, nf, cap in ((0, 1, 1 << 16), (2, 3, 40000), (1, 2, 4097)):
        need = size(64, 64, sr, nf, cap)
        nb, nbc = _nblocks(64, 64, sr)
        # a place per MCU for its restart marker and four decode tables per frame, at least
        assert need >= nf * (4 * nbc + 4 * 840) and need % 16 == 0
        assert _call(sr=sr, nf=nf, fstride=cap, cstride=(nb + 2 * nbc) * 64, wsb=need - 1) == jpgx.EWORKSPACE
        assert size(64, 64, sr, nf, cap + 4096) > need


def test_bindings_refuse_host_tensors():
    torch = pytest.importorskip("torch")
    files, lens = torch.zeros((1, 4096), dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError):
        jpgx.jfif_decode_gpu(files, lens, 64, 64)
    with pytest.raises(ValueError):
        jpgx.jfif_decode_gpu(files.numpy(), lens.numpy(), 64, 64)
    with pytest.raises(ValueError):
        jpgx.decode_jpeg_coefficients(_base(), "cpu")


# ---- the shared routines under the sanitizers ------------------------------------------------------
@pytest.mark.skipif(not S.HAVE_CC, reason="needs gcc/g++ with libasan/libubsan")
def test_decoder_under_asan_ubsan():
    """tests/c/jfif_read_san.c, a program of its own, with host/*.c, the host plan and the host
    decoder under AddressSanitizer + UndefinedBehaviorSanitizer (nothing is preloaded): every
    truncation, every dropped restart marker and 2000 corruptions of each of 12 files.  What it
    prints is what jfif_san_cases regenerates: the 16x16 files' bytes and every file's first
    corruptions, with the result the library gives here."""
    out = S.assert_clean()
    files = [ln.split() for ln in out.splitlines() if ln.startswith("file ")]
    shown = [ln.split() for ln in out.splitlines() if ln.startswith("flip ")]
    cases = [ln.split() for ln in out.splitlines() if ln.startswith("cases ")]
    assert len(files) == 12 and len(shown) == 12 * S.SHOWN and int(cases[0][1]) >= 20000
    for rec in files:
        idx, W, H, sr, opt, n = (int(x) for x in rec[1:7])
        assert S.FILES[idx] == (W, H, sr, opt)
        if idx == S.GPU_FILE[0]:
            assert (n, int(rec[7], 16)) == S.GPU_FILE[1:]
        if W != 16:
            continue
        data, _, _, _, _ = S.file_of(idx)
        assert len(data) == n and S.fnv1a(data) == int(rec[7], 16), idx
        mine = S.flips(idx, data)
        theirs = [(int(r[3]), int(r[4]), int(r[5])) for r in shown if int(r[1]) == idx]
        assert [(p, v) for p, v, _ in theirs] == mine, idx
        for (pos, val), (_, _, rc) in zip(mine, theirs):
            b = S.flipped(data, pos, val)
            try:                                      # the program's caller states the geometry
                i = C.jfif_info(b)
                same = (i["width"], i["height"], i["sample_ratio"]) == (W, H, sr)
                want = _rc(b) if same else HEADER
            except jpgx.JpgxError as e:
                want = e.rc
            assert rc == want, (idx, pos, val)
    # the corruption the GPU test uses is one of the sweep's 2000 for that file, all decoded above
    data, pos, val = S.undefined_code_flip(S.GPU_FILE[0])
    assert (pos, val) == S.GPU_FLIP and (pos, val) in S.flips(S.GPU_FILE[0], data, S.FLIPS)
