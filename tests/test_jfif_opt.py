"""Per-image Huffman tables (JPGX_JFIF_OPTIMIZE): the table builder jx_jfif_optimal, the host writer
jpgx_write_jfif_opt and the device coder jpgx_jfif_gpu_ex.

The builder is checked against a restatement of ITU-T T.81 Annex K.2 written from the standard
(annex_k2, tests/jfif_opt_common.py); the host files against that restatement applied to symbol
counts the tests compute themselves from the coefficients, and by decoding them; the device against
the host writer on one thread, == on bytes."""
import ctypes
import io
import itertools
import os
import subprocess

import numpy as np
import pytest

import jpgx
import jpgx.compat as C
import san_build
from conftest import GOLDEN, REPO
from jfif_decode import decode
from jfif_inputs import CASES, hand_made, stuffing_heavy          # the geometries of tests/test_jfif_gpu.py
from jfif_inputs import lap as _lap, nblocks as _nblocks
from jfif_opt_common import (_check_table, _device, _dht_bytes, _flat, _host, _raw, annex_k2, dht_tables, fib_vector,
                             segments, symbol_counts)   # shared with tests/test_jfif_tables*.py

gpu = pytest.mark.gpu
OPT = jpgx.JFIF_OPTIMIZE


def _optimal(counts):
    c = np.ascontiguousarray(counts, np.uint64)
    assert c.shape == (256,)
    bits, vals = np.zeros(16, np.uint8), np.zeros(256, np.uint8)
    fn = jpgx.lib.jx_jfif_optimal
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    n = fn(c.ctypes.data, bits.ctypes.data, vals.ctypes.data)
    return [int(b) for b in bits], [int(v) for v in vals[:n]]


def _vectors():
    rng = np.random.default_rng(11)
    v = {}
    c = np.zeros(256, np.uint64); c[0x21] = 7; v["one_symbol"] = c
    c = np.zeros(256, np.uint64); c[3] = c[200] = 5; v["two_equal"] = c
    v["all_256_equal"] = np.full(256, 9, np.uint64)
    c = np.zeros(256, np.uint64); c[::3] = rng.integers(1, 4, size=c[::3].size); v["many_ties"] = c
    c = rng.integers(0, 50, size=256).astype(np.uint64); c[17] = (1 << 32) + 12345; c[0] = 1 << 40
    v["above_2_32"] = c
    for k in range(4):
        c = (rng.integers(0, 1 << int(rng.integers(2, 30)), size=256) * (rng.random(256) < 0.6)).astype(np.uint64)
        v[f"random{k}"] = c
    c = rng.integers(0, 3, size=256).astype(np.uint64); v["small_random"] = c
    for n in (18, 19):
        c = np.zeros(256, np.uint64)
        c[rng.permutation(256)[:n]] = fib_vector(n)
        v[f"fibonacci{n}"] = c
    return v


VECTORS = _vectors()


@pytest.mark.parametrize("name", sorted(VECTORS))
def test_builder_matches_restatement(name):
    counts = VECTORS[name]
    bits, vals, depth = annex_k2(counts)
    if name.startswith("fibonacci"):
        n = int(name[9:])
        print(name, "depth", depth, "sum", int(counts.sum()), "bits", bits)
        assert depth > 16 and depth == n and int(counts.sum()) == {18: 10944, 19: 17709}[n]
        assert bits[-3:] == {18: [0, 2, 3], 19: [0, 1, 5]}[n]
    got_bits, got_vals = _optimal(counts)
    assert got_bits == bits and got_vals == vals
    _check_table(counts, got_bits, got_vals)


def test_builder_all_zero_counts():
    bits, vals = _optimal(np.zeros(256, np.uint64))
    assert bits == [0] * 16 and vals == []
    assert annex_k2(np.zeros(256, np.uint64))[:2] == (bits, vals)


# ---- coefficients, symbol counts and file parsing ------------------------------------------------
@pytest.fixture(scope="module")
def jfd():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "c"), "jfd"], check=True)
    lib = ctypes.CDLL(os.path.join(REPO, "tests", "c", "_build", "libjfd.so"))
    lib.jfd_decode.restype = ctypes.c_int
    lib.jfd_decode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                               ctypes.c_int, ctypes.c_void_p]
    return lib


def _jfd_decode(lib, data, nelems):
    buf = np.frombuffer(data, np.uint8)
    out = np.zeros(nelems, np.int16)
    info = np.zeros(6, np.int32)
    rc = lib.jfd_decode(buf.ctypes.data, buf.size, out.ctypes.data, out.size, 2, info.ctypes.data)
    assert rc == 0, f"jfif_dec.c check at line {-rc}"
    return out.reshape(-1, 64)


# ---- CPU: the host writer ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_file_is_legal_and_faithful(jfd, name):
    W, H, q, sr, rr, seed = CASES[name]
    coef = _lap(W, H, sr, seed)
    data = _host(coef, W, H, q, sr, rr)
    std = _host(coef, W, H, q, sr, rr, optimize=False)
    dec = decode(data)
    assert (dec["width"], dec["height"]) == (W, H)
    assert np.array_equal(_flat(dec["coef"]), coef.astype(np.int32))
    assert np.array_equal(_jfd_decode(jfd, data, coef.size), coef)
    cnt = symbol_counts(coef, W, H, sr, rr)
    tabs = dht_tables(data)
    for k, key in enumerate((0x00, 0x10, 0x01, 0x11)):
        bits, vals, _ = annex_k2(cnt[k])
        assert tabs[key] == (bits, vals), hex(key)
        _check_table(cnt[k], *tabs[key])
    # the segments around the tables are the standard file's
    a, b = segments(data)[0], segments(std)[0]
    assert [x for x in a if x[0] != 0xc4] == [x for x in b if x[0] != 0xc4]
    print(name, "file bytes", len(std), "->", len(data), "DHT", len(_dht_bytes(std)), "->", len(_dht_bytes(data)))
    assert len(_dht_bytes(data)) <= len(_dht_bytes(std))
    assert len(data) < len(std)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_file_opens_in_pil(name):
    Image = pytest.importorskip("PIL.Image")
    W, H, q, sr, rr, seed = CASES[name]
    coef = _lap(W, H, sr, seed)
    a = Image.open(io.BytesIO(_host(coef, W, H, q, sr, rr)))
    a.load()
    assert a.size == (W, H)
    b = Image.open(io.BytesIO(_host(coef, W, H, q, sr, rr, optimize=False)))
    assert np.array_equal(np.asarray(a.convert("RGB")), np.asarray(b.convert("RGB")))


@pytest.mark.parametrize("sr", [0, 2])
def test_host_all_zero_frame(jfd, sr):
    W, H = 64, 96
    nb, nbc = _nblocks(W, H, sr)
    coef = np.zeros((nb + 2 * nbc, 64), np.int16)
    data = _host(coef, W, H, 50, sr, 1)
    for key, (bits, vals) in dht_tables(data).items():
        assert bits == [1] + [0] * 15 and vals == [0], hex(key)
    assert not _flat(decode(data)["coef"]).any()
    assert not _jfd_decode(jfd, data, coef.size).any()
    assert len(data) < len(_host(coef, W, H, 50, sr, 1, optimize=False))


def test_host_threads_and_flags():
    W, H, q = 128, 96, 75
    for sr, rr in ((0, 1), (2, 2), (1, 0)):
        coef = _lap(W, H, sr, 90 + sr)
        one = _host(coef, W, H, q, sr, rr, nthreads=1)
        for nt in (4, 16):
            assert _host(coef, W, H, q, sr, rr, nthreads=nt) == one
        n = ctypes.c_size_t()
        buf = np.empty(1 << 20, np.uint8)
        fn = C.lib.jpgx_write_jfif_opt
        assert fn(coef.ctypes.data, W, H, q, sr, rr, 2, 0, buf.ctypes.data, buf.size, ctypes.byref(n)) == 0
        assert buf[:n.value].tobytes() == C.write_jfif_ex(coef, W, H, q, sr, restart_rows=rr, nthreads=2)
        for bad in (2, 3, 0x80000000):
            assert fn(coef.ctypes.data, W, H, q, sr, rr, 2, bad, buf.ctypes.data, buf.size,
                      ctypes.byref(n)) == jpgx.EARG
        # cap too small: EARG and the size needed
        assert fn(coef.ctypes.data, W, H, q, sr, rr, 2, OPT, buf.ctypes.data, 100, ctypes.byref(n)) == jpgx.EARG
        assert n.value == len(one)


# ---- CPU: the device entry's argument checks come before any device call -------------------------
def _call(flags=OPT, coef=0x10000, fstride=3 * 64 * 64, nf=1, W=64, H=64, q=50, sr=0, rr=1, out=0x20000,
          ostride=1 << 16, cap=1 << 16, lens=0x30000, ws=0x40000, wsb=None):
    if wsb is None:
        wsb = jpgx.lib.jpgx_jfif_gpu_workspace_size_ex(W, H, sr, rr, max(nf, 1), cap, OPT) or 1 << 20
    return jpgx.lib.jpgx_jfif_gpu_ex(coef, fstride, nf, W, H, q, sr, rr, flags, out, ostride, cap, lens, ws, wsb,
                                     None)


def test_device_entry_argument_checks():
    size_ex, size = jpgx.lib.jpgx_jfif_gpu_workspace_size_ex, jpgx.lib.jpgx_jfif_gpu_workspace_size
    for bad in (2, 3, 0x80000000):
        assert _call(flags=bad) == jpgx.EARG
        assert size_ex(64, 64, 0, 1, 1, 1 << 16, bad) == 0
    assert _call(rr=0) == jpgx.EARG and _call(nf=0) == jpgx.EARG and _call(coef=None) == jpgx.EARG
    assert _call(q=0) == jpgx.EQUALITY and _call(W=72, sr=1) == jpgx.EGEOMETRY
    assert size_ex(64, 64, 0, 0, 1, 1 << 16, OPT) == 0
    for sr, rr, nf in ((0, 1, 1), (2, -1, 3), (1, 4, 2)):
        old = size(64, 64, sr, rr, nf, 1 << 16)
        assert old > 0 and size_ex(64, 64, sr, rr, nf, 1 << 16, 0) == old
        need = size_ex(64, 64, sr, rr, nf, 1 << 16, OPT)
        assert need >= old + nf * 4 * 256 * 8 and need % 16 == 0
        nb, nbc = _nblocks(64, 64, sr)
        for flags, n in ((OPT, need), (0, old)):
            assert _call(flags=flags, sr=sr, rr=rr, nf=nf, fstride=(nb + 2 * nbc) * 64, wsb=n - 1) == jpgx.EWORKSPACE


@pytest.mark.skipif(not san_build.HAVE_CC, reason="needs gcc/g++ with libasan/libubsan")
def test_builder_and_writer_under_asan_ubsan():
    """tests/c/jfif_opt_san.c, a program of its own, with host/*.c and the host plan under
    AddressSanitizer + UndefinedBehaviorSanitizer (nothing is preloaded)."""
    rc, out, err = san_build.run("jfif_opt_san")
    assert rc == 0 and "jfif_opt_san: clean" in out, (out[-2000:], err[-4000:])
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-4000:]


# ---- GPU: byte equality with the host writer -----------------------------------------------------
@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_bytes_equal_host_writer(cuda, name):
    W, H, q, sr, rr, seed = CASES[name]
    coef = _lap(W, H, sr, seed)
    ref = _host(coef, W, H, q, sr, rr)
    assert ref != _host(coef, W, H, q, sr, rr, optimize=False)
    assert _device(cuda, coef, W, H, q, sr, rr) == ref


@gpu
@pytest.mark.parametrize("sr", [0, 2])
def test_all_zero_frame(cuda, sr):
    """one symbol per table; at 4:2:0 the chroma tables count half as many blocks as the luma ones"""
    W, H = 64, 96
    nb, nbc = _nblocks(W, H, sr)
    coef = np.zeros((nb + 2 * nbc, 64), np.int16)
    ref = _host(coef, W, H, 50, sr, 1)
    assert all(t == ([1] + [0] * 15, [0]) for t in dht_tables(ref).values())
    assert _device(cuda, coef, W, H, 50, sr, 1) == ref


@gpu
@pytest.mark.parametrize("sr", [0, 2])
def test_hand_made_blocks(cuda, sr):
    W, H, coef = hand_made(sr)
    for rr in (1, 2):
        ref = _host(coef, W, H, 50, sr, rr)
        cnt = symbol_counts(coef, W, H, sr, rr)
        assert cnt[1, 0xf0] >= 5 and cnt[3, 0xf0] >= 3 and cnt[0, 11] >= 2     # ZRLs and clamped DC steps
        assert dht_tables(ref)[0x10] == annex_k2(cnt[1])[:2]
        assert _device(cuda, coef, W, H, 50, sr, rr) == ref


@gpu
@pytest.mark.parametrize("sr", [0, 2])
def test_stuffing_heavy_frame(cuda, sr):
    W, H, q, coef = stuffing_heavy(sr)
    ref = _host(coef, W, H, q, sr, 1)
    at = ref.index(b"\xff\xda")
    pairs = ref[at + 14:-2].count(b"\xff\x00")
    print("stuffed pairs", pairs)
    assert pairs >= 1000                             # a different numpy must not empty the case
    assert _device(cuda, coef, W, H, q, sr, 1) == ref


def length_limiting_frame():
    """192 x 128, 4:4:4: luma AC symbol counts are the Fibonacci vector on 18 symbols.  EOB counts
    the untouched luma blocks (an entry e of the vector); the other 17 entries go to run 0 and run 1
    symbols so that the tokens fill whole blocks up to position 63 (no EOB in a used block):
    tokens + run-1 tokens = 63 x (384 - e) positions."""
    W, H = 192, 128
    nb = (W // 8) * (H // 8)
    vec = fib_vector(18)
    for e in vec:
        rest = [x for x in vec if x != e]
        n1 = 63 * (nb - e) - sum(rest)               # tokens of run 1
        if n1 < 0:
            continue
        for k in range(7, 11):                       # at most 10 sizes per run
            for pick in itertools.combinations(rest, k):
                if sum(pick) == n1:
                    break
            else:
                continue
            break
        else:
            continue
        break
    else:
        raise AssertionError("no placement")
    run0 = [x for x in rest if x not in pick]
    assert len(run0) <= 10 and len(pick) <= 10
    tok1 = [(1, s + 1) for s, c in enumerate(pick) for _ in range(c)]
    tok0 = [(0, s + 1) for s, c in enumerate(run0) for _ in range(c)]
    coef = np.zeros((3 * nb, 64), np.int16)
    b = 0
    while tok1 or tok0:
        k = 1
        take = min(31, len(tok1))                    # 31 pairs and one single, or what is left
        for run, size in [tok1.pop() for _ in range(take)] + [tok0.pop() for _ in range(63 - 2 * take)]:
            k += run
            coef[b, k] = (1 << (size - 1)) * (1 if (b + k) & 1 else -1)
            k += 1
        assert k == 64
        b += 1
    assert b == nb - e
    return W, H, coef, e


@gpu
def test_length_limited_table(cuda):
    W, H, coef, e = length_limiting_frame()
    cnt = symbol_counts(coef, W, H, 0, 2)
    assert sorted(int(c) for c in cnt[1] if c) == fib_vector(18) and int(cnt[1, 0]) == e
    bits, vals, depth = annex_k2(cnt[1])
    print("luma AC depth", depth, "bits", bits)
    assert depth > 16
    ref = _host(coef, W, H, 50, 0, 2)
    assert dht_tables(ref)[0x10] == (bits, vals)
    assert np.array_equal(_flat(decode(ref)["coef"]), coef.astype(np.int32))
    assert _device(cuda, coef, W, H, 50, 0, 2) == ref


@gpu
def test_batch_with_padded_strides(cuda):
    import torch
    W, H, q, sr, rr = 96, 64, 60, 0, 2
    per = 3 * (W // 8) * (H // 8) * 64
    fstride, cap, ostride = per + 5 * 64, 40000, 40000 + 48
    frames = [_lap(W, H, sr, 100 + k, scale=s) for k, s in enumerate((4.0, 7.0, 60.0))]
    d = torch.zeros((3, fstride), dtype=torch.int16, device=cuda)
    for k in range(3):
        d[k, :per] = torch.from_numpy(frames[k].reshape(-1)).to(cuda)
    out = torch.full((3, ostride), 0xA5, dtype=torch.uint8, device=cuda)
    lens = torch.zeros(3, dtype=torch.int64, device=cuda)
    assert _raw(d, fstride, 3, W, H, q, sr, rr, OPT, out, ostride, cap, lens) == 0
    got, n = out.cpu().numpy(), lens.cpu().numpy()
    files = []
    for k in range(3):
        single = _device(cuda, frames[k], W, H, q, sr, rr)
        assert single == _host(frames[k], W, H, q, sr, rr)
        assert got[k, :n[k]].tobytes() == single
        assert (got[k, n[k]:] == 0xA5).all()
        files.append(single)
    dhts = [_dht_bytes(x) for x in files]
    assert dhts[0] != dhts[1] and dhts[1] != dhts[2] and dhts[0] != dhts[2]


@gpu
def test_one_workspace_reused_without_clearing(cuda):
    import torch
    W, H, q, sr, rr, cap = 96, 64, 70, 0, 1, 40000
    a, b = _lap(W, H, sr, 201, scale=5.0), _lap(W, H, sr, 202, scale=20.0)
    need = jpgx.lib.jpgx_jfif_gpu_workspace_size_ex(W, H, sr, rr, 1, cap, OPT)
    ws = torch.full((need,), 0xEE, dtype=torch.uint8, device=cuda)     # never cleared: not zeros either
    out = torch.empty((1, cap), dtype=torch.uint8, device=cuda)
    lens = torch.zeros(1, dtype=torch.int64, device=cuda)
    for coef, flags in ((a, OPT), (a, 0), (b, OPT), (a, OPT)):
        d = torch.from_numpy(coef).to(cuda).reshape(1, -1)
        assert _raw(d, d.shape[1], 1, W, H, q, sr, rr, flags, out, cap, cap, lens, ws=ws) == 0
        n = int(lens[0])
        assert out[0, :n].cpu().numpy().tobytes() == _host(coef, W, H, q, sr, rr, optimize=bool(flags))


@gpu
def test_overflow_of_one_frame(cuda):
    import torch
    W, H, q, sr, rr = 64, 48, 50, 0, 1
    frames = [_lap(W, H, sr, 31, scale=2.0), _lap(W, H, sr, 32, scale=60.0), _lap(W, H, sr, 33, scale=2.0)]
    refs = [_host(c, W, H, q, sr, rr) for c in frames]
    cap = (max(len(refs[0]), len(refs[2])) + 15) // 16 * 16
    assert len(refs[1]) > cap + 64
    d = torch.stack([torch.from_numpy(c.reshape(-1)) for c in frames]).to(cuda)
    ostride = 1 << 16
    out = torch.full((3, ostride), 0xA5, dtype=torch.uint8, device=cuda)
    lens = torch.zeros(3, dtype=torch.int64, device=cuda)
    assert _raw(d, d.shape[1], 3, W, H, q, sr, rr, OPT, out, ostride, cap, lens) == 0
    got, n = out.cpu().numpy(), lens.cpu().numpy()
    for k in (0, 2):
        assert n[k] == len(refs[k]) and got[k, :n[k]].tobytes() == refs[k]
        assert (got[k, n[k]:] == 0xA5).all()
    assert n[1] < 0
    need = int(n[1]) & ((1 << 62) - 1)
    hdrlen = refs[1].index(b"\xff\xda") + 14                # the frame's own header
    scan = len(refs[1]) - hdrlen - 2
    assert len(refs[1]) <= need <= hdrlen + 2 * scan + 2
    assert (got[1, cap:] == 0xA5).all()
    # the reported capacity suffices
    assert _raw(d, d.shape[1], 3, W, H, q, sr, rr, OPT, out, ostride, need, lens) == 0
    n = lens.cpu().numpy()
    for k in range(3):
        assert n[k] == len(refs[k]) and out[k, :n[k]].cpu().numpy().tobytes() == refs[k]
    # the binding retries once with the reported capacity
    assert _device(cuda, frames[1], W, H, q, sr, rr, cap=cap) == refs[1]


@gpu
@pytest.mark.parametrize("sr,W,H", [(0, 1920, 1080), (2, 1920, 1088)])
def test_full_hd_from_the_transform(cuda, sr, W, H):
    """an interval has 720 blocks: lanes loop in the count pass; coefficients from encode_blocks"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(5)
    small = torch.randint(0, 256, (H // 8, W // 8, 3), generator=g, dtype=torch.uint8)
    rgb = small.repeat_interleave(8, 0).repeat_interleave(8, 1)
    rgb = (rgb.to(torch.int16) + torch.randint(-6, 7, rgb.shape, generator=g, dtype=torch.int16)).clamp(0, 255)
    rgb = rgb.to(torch.uint8).to(cuda)
    flags = jpgx.FLAG_SUBSAMPLE if sr else 0
    coef = jpgx.encode_blocks(rgb, 75, sr, flags=flags)
    out, lens = jpgx.jfif_gpu(coef.reshape(1, -1), W, H, 75, sr, 1, optimize=True)
    n = int(lens[0])
    ref = _host(coef.cpu().numpy().reshape(-1, 64), W, H, 75, sr, 1)
    assert 0 < n == len(ref)
    assert out[0, :n].cpu().numpy().tobytes() == ref


@gpu
def test_encode_jpeg_end_to_end(cuda):
    import torch
    rgb, _ = C.bmp_read(os.path.join(GOLDEN, "images", "cam.bmp"))
    H, W = rgb.shape[:2]
    d_rgb = torch.from_numpy(rgb).to(cuda)
    data = jpgx.encode_jpeg(d_rgb, 75, optimize=True)
    coef = jpgx.encode_blocks(d_rgb, 75).cpu().numpy()
    assert data == _host(coef.reshape(-1, 64), W, H, 75, 0, 1)
    assert len(data) < len(jpgx.encode_jpeg(d_rgb, 75))
    dec = decode(data)
    assert (dec["width"], dec["height"]) == (W, H)
    assert np.array_equal(_flat(dec["coef"]), coef.reshape(-1, 64).astype(np.int32))


@gpu
def test_encode_jpeg_opens_in_pil(cuda):
    Image = pytest.importorskip("PIL.Image")
    import torch
    rgb, _ = C.bmp_read(os.path.join(GOLDEN, "images", "cam.bmp"))
    data = jpgx.encode_jpeg(torch.from_numpy(rgb).to(cuda), 75, optimize=True)
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
