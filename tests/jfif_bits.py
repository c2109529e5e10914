"""Test helper: the coded bits of every block of a scan, restated from ITU-T T.81 F.1.2 and
independent of the writers.

walk() is the one per-block walk of the tests (tests/jfif_opt_common.py's symbol_counts counts its
symbols, interval_bits() here adds up their lengths).  The code lengths come from the DHT segments of
the file under test, so the same helper serves the standard and the per-image tables.  From the bits
follow each block's bit offset within its restart interval, the interval's bits and the length of its
unstuffed stream; file_intervals() cuts the same intervals out of a file's bytes, so the two can be
held against each other (tests/test_jfif_bits.py) and the inputs of tests/test_jfif_gpu_passes.py can
be placed at exact bit and byte positions."""
import functools

import numpy as np

import jfif_inputs as I
from jfif_inputs import scan_rows

DC_MAX, AC_MAX = 2047, 1023


def category(v):
    return int(abs(int(v))).bit_length()


def mcu_rows(H, sr):
    return H // 8 // (1, 1, 2)[sr]


def interval_rows(H, sr, rr):
    """MCU rows per restart interval: rr 0 none (one interval), -1 one row, as the device coder's"""
    rows = mcu_rows(H, sr)
    return rows if rr == 0 else (1 if rr == -1 else min(rr, rows))


def walk(coef, W, H, sr, rr, visit):
    """visit(interval, component, row, step, diff, acs) for every block in scan order.  step is the DC
    step against the component's previous block of the interval (the true DC: predictors are reset to
    0 at every interval), diff the step clamped to +-2047, acs the AC symbols in order as
    (run << 4 | size, clamped value): ZRL (0xf0) while a run of zeros exceeds 15, EOB (0x00) unless
    coefficient 63 is nonzero (T.81 F.1.2.2)."""
    per = interval_rows(H, sr, rr) * (W // 8 // (1, 2, 2)[sr]) * (3, 4, 6)[sr]
    pred = [0, 0, 0]
    for i, (row, comp) in enumerate(scan_rows(W, H, sr)):
        if i % per == 0:
            pred = [0, 0, 0]
        z = coef[row]
        step = int(z[0]) - pred[comp]
        pred[comp] = int(z[0])
        acs, prev = [], 0
        for k in np.nonzero(z[1:])[0] + 1:
            run = int(k) - prev - 1
            prev = int(k)
            while run > 15:
                acs.append((0xf0, 0))
                run -= 16
            v = max(-AC_MAX, min(AC_MAX, int(z[k])))
            acs.append((run << 4 | category(v), v))
        if prev < 63:
            acs.append((0, 0))
        visit(i // per, comp, row, step, max(-DC_MAX, min(DC_MAX, step)), acs)


def file_header(data):
    """(code lengths {class << 4 | id: {symbol: length}}, offset of the scan's first byte) of a file"""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    at, lengths = 2, {}
    while True:
        assert data[at] == 0xff
        m, n = data[at + 1], data[at + 2] << 8 | data[at + 3]
        p = data[at + 4:at + 2 + n]
        at += 2 + n
        if m == 0xc4:
            j = 0
            while j < len(p):
                bits = list(p[j + 1:j + 17])
                vals = list(p[j + 17:j + 17 + sum(bits)])
                lens = [l for l, b in enumerate(bits, 1) for _ in range(b)]
                lengths[p[j]] = dict(zip(vals, lens))
                j += 17 + sum(bits)
        if m == 0xda:
            return lengths, at


def interval_bits(coef, W, H, sr, rr, data):
    """[[coded bits of each block in scan order] per restart interval], with the code lengths of
    `data`, the file a writer made of coef: the DC code and the category's additional bits, per AC
    symbol its code and its size's additional bits (T.81 F.1.2.1, F.1.2.2)"""
    lengths = file_header(data)[0]
    out = []

    def visit(iv, comp, row, step, diff, acs):
        t = 0 if comp == 0 else 1
        s = category(diff)
        n = lengths[t][s] + s
        for sym, _ in acs:
            n += lengths[0x10 | t][sym] + (sym & 15)
        if iv == len(out):
            out.append([])
        out[iv].append(n)

    walk(coef, W, H, sr, rr, visit)
    return out


def offsets(bits):
    """the bit offset of every block of an interval, and one more entry: the interval's bits"""
    return [0] + [int(x) for x in np.cumsum(bits)]


def unstuffed_len(bits):
    return (sum(bits) + 7) // 8


def pad_bits(bits):
    return (8 - sum(bits) % 8) % 8


def file_intervals(data):
    """the unstuffed stream of every restart interval of a file: the entropy-coded bytes between the
    RSTm markers (checked to count 0..7 round), the 00 after each FF removed"""
    data = bytes(data)
    at = file_header(data)[1]
    assert data[-2:] == b"\xff\xd9"
    scan = data[at:-2]
    out, start, i, m = [], 0, 0, 0
    while i < len(scan):
        if scan[i] == 0xff:
            assert i + 1 < len(scan)
            if scan[i + 1] != 0:
                assert scan[i + 1] == 0xd0 + m, "RSTm out of order"
                out.append(scan[start:i].replace(b"\xff\x00", b"\xff"))
                m = (m + 1) & 7
                start = i + 2
            i += 2
        else:
            i += 1
    out.append(scan[start:].replace(b"\xff\x00", b"\xff"))
    return out


def check_against_file(coef, W, H, sr, rr, data):
    """the helper held to a writer's file: per interval ceil(bits / 8) is the unstuffed length and the
    last byte ends in (8 - bits % 8) % 8 one-bits; returns (bits per block per interval, streams)"""
    bits = interval_bits(coef, W, H, sr, rr, data)
    streams = file_intervals(data)
    assert len(bits) == len(streams) == -(-mcu_rows(H, sr) // interval_rows(H, sr, rr))
    for b, s in zip(bits, streams):
        assert unstuffed_len(b) == len(s), (sum(b), len(s))
        pad = pad_bits(b)
        assert s[-1] & ((1 << pad) - 1) == (1 << pad) - 1
    return bits, streams


def coded_values(coef, W, H, sr, rr):
    """what a decoder gets back from a writer's file of coef, int32 [nb + 2 nbc][64]: the AC
    coefficients clamped to +-1023, the DC the running sum of the steps clamped to +-2047"""
    out = np.clip(np.asarray(coef, np.int32), -AC_MAX, AC_MAX)
    acc = [0, 0, 0]
    state = {"iv": -1}

    def visit(iv, comp, row, step, diff, acs):
        if iv != state["iv"]:
            state["iv"] = iv
            acc[:] = [0, 0, 0]
        acc[comp] += diff
        out[row, 0] = acc[comp]

    walk(coef, W, H, sr, rr, visit)
    return out


# ---- the cases of tests/test_jfif_gpu_passes.py and their guards ----------------------------------
# A case is an input of tests/jfif_inputs.py with the guard that holds it to its purpose: an assertion
# computed here, from the host writer's file and the walk above, before any device is called.  A
# different numpy or a changed seed fails the guard; it does not quietly empty the case.
def host(coef, W, H, sr, rr, optimize, q=50):
    import jpgx.compat as C
    return C.write_jfif_ex(coef, W, H, q, sr, restart_rows=1 if rr == -1 else rr, nthreads=1, optimize=optimize)


class Case:
    """W, H, sr, rr, coef (read-only), data (the host writer's file), bits and streams (per interval)"""

    def __init__(self, W, H, sr, rr, coef, optimize, bits=True):
        coef = np.ascontiguousarray(coef, np.int16)
        coef.setflags(write=False)
        self.W, self.H, self.sr, self.rr, self.coef, self.optimize = W, H, sr, rr, coef, optimize
        self.data = host(coef, W, H, sr, rr, optimize)
        if bits:
            self.bits, self.streams = check_against_file(coef, W, H, sr, rr, self.data)

    @property
    def pairs(self):
        return I.scan_of(self.data).count(b"\xff\x00")


def _find(build, ok, optimize):
    """the least n of 0..63 whose frame build(n) passes ok(offsets of its one interval)"""
    for n in range(64):
        W, H, coef = build(n)
        if ok(offsets(interval_bits(coef, W, H, 0, I.ONE, host(coef, W, H, 0, I.ONE, optimize))[0])):
            return n
    raise AssertionError("no frame found")


def _word(bit):
    return bit >> 5


def _aligned(off):
    return off[256] % 32 == 0


def _same_word(off):
    """blocks 254..257 lie wholly inside one word"""
    return _word(off[254]) == _word(off[258] - 1)


def _maximal(off, words=50):
    """block 255 starts mid-word, covers more than 50 words and ends mid-word, where block 256 starts"""
    return off[255] % 32 != 0 and off[256] % 32 != 0 and _word(off[256]) - _word(off[255]) + 1 > words


def _maximal_opt(off):
    """with per-image tables the block's 63 equal symbols take a two-bit code (only EOB is more
    frequent): 13 + 63 x 12 bits, 25 words; more than 20 is what is asked there"""
    return _maximal(off, 20)


def _seam_blocks(c):
    """per seam the walk's view of scan blocks seam - 2 .. seam + 1: [(step, acs, row)]"""
    seen = []
    walk(c.coef, c.W, c.H, c.sr, c.rr, lambda iv, comp, row, step, diff, acs: seen.append((step, acs, row)))
    return [seen[s - 2:s + 2] for s in I.SEAMS]


def guard_blocks(c):
    n = len(c.bits[0])
    print("blocks per interval", n, "bits", sum(c.bits[0]), "unstuffed bytes", len(c.streams[0]))
    assert len(c.bits) == 1 and n > 2 * I.PASS        # one interval, three passes over its blocks


def guard_stuffing_seam(c):
    """three passes over the blocks; and of the unstuffed bytes that end a pass of 4,096 and of those
    that begin one, at least one each is 0xFF: the stuffing pass's carry counts a byte of its last
    lane and shifts a stuffed pair of its first"""
    guard_blocks(c)
    s = c.streams[0]
    ends = [k for k in range(4096, len(s), 4096) if s[k - 1] == 0xff]
    begins = [k for k in range(4096, len(s), 4096) if s[k] == 0xff]
    print("stuffed pairs", c.pairs, "0xFF at 4096 k - 1:", ends, "at 4096 k:", begins)
    assert c.pairs >= 1000 and len(s) > 2 * 4096 and ends and begins


def guard_hand_made(c):
    """every rule of hand_made in the four blocks around each seam"""
    guard_blocks(c)
    for blocks in _seam_blocks(c):
        syms = [[sym for sym, _ in acs] for _, acs, _ in blocks]
        raw = [c.coef[row] for _, _, row in blocks]
        assert any(s.count(0xf0) == 3 and s[-1] != 0 for s in syms)            # three ZRLs, no EOB
        assert any(len(s) == 63 and 0 not in s and 0xf0 not in s for s in syms)  # 63 codes
        assert any(0xf0 in s and s[s.index(0xf0) + 1] >> 4 == 0 for s in syms)   # a run of exactly 16
        assert any((np.abs(z[1:].astype(np.int32)) > AC_MAX).any() for z in raw)  # the AC clamp
        assert any(abs(step) > DC_MAX for step, _, _ in blocks)                # the DC clamp
        assert any(int(z[0]) in (32767, -32768) and abs(step) > 65000 for (step, _, _), z in zip(blocks, raw))


def guard_aligned(c):
    off = offsets(c.bits[0])
    print("block 256 starts at bit", off[256])
    guard_blocks(c)
    assert _aligned(off)


def guard_same_word(c):
    off = offsets(c.bits[0])
    print("blocks 254..258 start at bits", off[254:259])
    guard_blocks(c)
    assert _same_word(off)


def guard_maximal(c):
    off = offsets(c.bits[0])
    print("block 255 covers bits", off[255], "..", off[256], "=", _word(off[256]) - _word(off[255]) + 1, "words")
    guard_blocks(c)
    assert (_maximal_opt if c.optimize else _maximal)(off) and c.bits[0][255] == max(c.bits[0])
    step, acs, _ = _seam_blocks(c)[0][1]
    assert step == DC_MAX and len(acs) == 63 and all(abs(v) == AC_MAX for _, v in acs)


def guard_trimmed(target):
    def guard(c):
        print("unstuffed bytes", len(c.streams[0]), "bits", sum(c.bits[0]), "stuffed pairs", c.pairs)
        assert len(c.bits) == 1 and len(c.streams[0]) == unstuffed_len(c.bits[0]) == target
    return guard


def guard_tall(c):
    """more than one pass over the intervals (but for the 256-interval frame, the last that takes
    one); some intervals need no padding, some fill their 16-byte place exactly"""
    ni = len(c.bits)
    nopad = sum(1 for b in c.bits if sum(b) % 8 == 0)
    full = sum(1 for s in c.streams if len(s) % 16 == 0)
    print("intervals", ni, "without padding", nopad, "of a multiple of 16 bytes", full, "file bytes", len(c.data),
          "stuffed pairs", c.pairs)
    assert ni == mcu_rows(c.H, c.sr) >= I.PASS and nopad and full
    assert ni > I.PASS or c.H == 2048


def guard_intervals(ni):
    def guard(c):
        print("intervals", len(c.bits), "unstuffed bytes", sum(len(s) for s in c.streams), "file bytes", len(c.data))
        assert len(c.bits) == ni
    return guard


def r16(n):
    return (n + 15) // 16 * 16


def guard_late_overflow(c, cap):
    """a capacity the frame does not fit, but its unstuffed stream fits the area the coder keeps for
    it (cap rounded up to 16, and 16 bytes per interval), every interval at a 16-byte place: the
    kernel that places the intervals accepts the frame, and the refusal is the later kernel's, which
    knows the stuffed sizes"""
    places = sum(r16(len(s)) for s in c.streams)
    print("file bytes", len(c.data), "capacity", cap, "places", places, "area", r16(cap) + 16 * len(c.streams))
    assert cap < len(c.data) and places <= r16(cap) + 16 * len(c.streams)


def guard_both(c):
    W, H = I.BOTH
    assert (W // 8) * 3 > I.PASS and H // 8 > I.PASS and c.data.count(b"\xff\xd0") >= H // 64 - 1


def _cases():
    """{name: (build(optimize) -> Case, guard)}"""
    out = {}
    for sr, tag in ((0, "444"), (1, "422"), (2, "420")):
        W, H = I.SEAM_FRAMES[sr]
        out[f"seam_stuffing_{tag}"] = (lambda o, sr=sr, W=W, H=H: Case(
            W, H, sr, I.ONE, I.stuffing_heavy(sr, W, H, I.STUFF_SEEDS[sr])[3], o), guard_stuffing_seam)
        out[f"seam_zeros_{tag}"] = (lambda o, sr=sr, W=W, H=H: Case(W, H, sr, I.ONE, I.zeros(W, H, sr), o), guard_blocks)
        out[f"seam_hand_made_{tag}"] = (lambda o, sr=sr: Case(*I.seam_hand_made(sr)[:2], sr, I.ONE,
                                                              I.seam_hand_made(sr)[2], o), guard_hand_made)
    for tag, frame, ok, guard in (("aligned", I.seam_shifted, _aligned, guard_aligned),
                                  ("same_word", I.seam_shifted, _same_word, guard_same_word),
                                  ("maximal", I.seam_maximal, _maximal, guard_maximal)):
        out[f"seam_{tag}"] = (lambda o, frame=frame, ok=ok: Case(
            *I.SEAM_FRAMES[0], 0, I.ONE,
            frame(_find(frame, _maximal_opt if o and ok is _maximal else ok, o))[2], o), guard)
    for target in (4096, 4097):
        out[f"trimmed_{target}"] = (lambda o, t=target: Case(64, 48, 0, I.ONE, I.trimmed(t, o)[2], o),
                                    guard_trimmed(target))
    for W, H, sr in I.TALL:
        for kind in ("lap", "stuffing"):
            out[f"tall_{kind}_{W}x{H}"] = (lambda o, W=W, H=H, sr=sr, kind=kind: Case(
                W, H, sr, 1, I.tall(W, H, sr, kind), o), guard_tall)
    out["tall_zeros_8x2064"] = (lambda o: Case(8, 2064, 0, 1, I.tall(8, 2064, 0, "zeros"), o), guard_intervals(258))
    out["lap_64x48_rr1"] = (lambda o: Case(64, 48, 0, 1, I.lap(64, 48, 0, 21), o), guard_intervals(6))
    out["both_704x2064"] = (lambda o: Case(*I.BOTH, 0, 1, I.lap(*I.BOTH, 0, 704), o, bits=False), guard_both)
    return out


PASS_CASES = _cases()


@functools.lru_cache(maxsize=None)
def pass_case(name, optimize):
    """the case, built once and guarded: tests share it and leave it unchanged"""
    build, guard = PASS_CASES[name]
    c = build(optimize)
    guard(c)
    return c
