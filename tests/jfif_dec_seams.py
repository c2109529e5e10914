"""Test helper: the cases of tests/test_jfif_dec_seams.py and tests/test_jfif_decode_gpu_seams.py, which
put content on the seams of the device JFIF decoder (csrc/jpgx_jfif_dec.hip, csrc/jx_jd_sub_body.h,
csrc/jx_jfif_sub.h): the tiles of S x T = 8,192 bytes that k_jd_sub walks an
interval in and what it carries between them, the 16 halo bytes, the load's 16 alignments, the DC
predictors' chunks of 256 blocks, k_jd_frame's passes of 256 chunks and the gray kernel's grid stride.

Most seams need exact byte positions.  Scan below is a bit-level writer of scans, independent of the
project's writers: it takes its Huffman codes from the DHT segments of the header it is given, emits DC
differences and AC units of any value (nothing is clamped), stuffs FF, pads with one-bits, inserts RSTm
and is spliced behind a header.  Positions are counted as csrc/jx_jfif_sub.h counts them: r is a byte of
the interval counted from its first, p = 8 r + the bit's index from the top, and a stuffed 00 is never
a unit's place.

A case is a file with its guard: an assertion computed from the file's own bytes (K.intervals, the
twin's counters), run before a device is called and again by the CPU tests, so that a changed seed or
another numpy fails the guard and does not quietly empty the case."""
import functools

import numpy as np

import any_cases as A
import gray_cases as G
import jfif_bits as B
import jfif_sub_cases as K
import jpgx
import jpgx.compat as C
from jfif_decode import _table
from jfif_inputs import lap, nblocks, scan_rows

SUB, TILE = K.SUB, K.TILE
SEAM = SUB * TILE                   # bytes of a tile: a seam is r = SEAM k
HALO = 16                           # JXS_HALO of csrc/jx_jfif_sub.h
CHUNK = 4096                        # bytes per workgroup of k_jd_count; k_jd_frame scans 256 chunks a pass
SUB_GRID = 1024                     # kSubGrid of csrc/jpgx_jfif_dec.hip
SCAN = jpgx.EJFIF_SCAN
I16 = (-32768, 32767)


# ---- headers ---------------------------------------------------------------------------------------------
class Header:
    """what the builder needs of a file's header: per DHT table {symbol: (code, length)} (canonical codes,
    T.81 Annex C), the scan's table selectors, the luma sampling, the scan's offset"""

    def __init__(self, data):
        data = bytes(data)
        assert data[:2] == b"\xff\xd8"
        at, self.codes, self.dri_at = 2, {}, None
        while True:
            assert data[at] == 0xff
            m, n = data[at + 1], data[at + 2] << 8 | data[at + 3]
            p = data[at + 4:at + 2 + n]
            if m == 0xc4:
                j = 0
                while j < len(p):
                    bits = list(p[j + 1:j + 17])
                    vals = list(p[j + 17:j + 17 + sum(bits)])
                    self.codes[p[j]] = {sym: (code, ln) for (ln, code), sym in _table(bits, vals).items()}
                    j += 17 + sum(bits)
            elif m in (0xc0, 0xc1):
                self.hs, self.vs = p[7] >> 4, p[7] & 15
            elif m == 0xdd:
                self.dri_at = at + 4
            elif m == 0xda:
                self.sos_at = at
                self.sel = [(p[2 + 2 * k] >> 4, p[2 + 2 * k] & 15) for k in range(p[0])]
                self.scan = at + 2 + n
                return
            at += 2 + n


def with_dri(head, dri):
    """the header (a file's bytes up to its scan) with DRI set to `dri`: its value replaced, or the
    segment inserted before SOS"""
    h = Header(head)
    v = bytes([dri >> 8, dri & 255])
    if h.dri_at is not None:
        return head[:h.dri_at] + v + head[h.dri_at + 2:]
    return head[:h.sos_at] + b"\xff\xdd\x00\x04" + v + head[h.sos_at:]


def with_table(head, tc_th, bits, vals):
    """the header with the DHT segment of the one table tc_th replaced (the host writer writes a
    segment per table)"""
    at = 2
    while True:
        m, n = head[at + 1], head[at + 2] << 8 | head[at + 3]
        if m == 0xc4 and head[at + 4] == tc_th:
            assert n == 2 + 17 + sum(head[at + 5:at + 21])       # the segment holds this table alone
            seg = bytes([tc_th]) + bytes(bits) + bytes(vals)
            return head[:at] + b"\xff\xc4" + (len(seg) + 2).to_bytes(2, "big") + seg + head[at + 2 + n:]
        assert m != 0xda
        at += 2 + n


@functools.lru_cache(maxsize=None)
def _base(sr):
    """the header of the host writer's 16 x 16 file without restart intervals: Annex K.3's tables"""
    nb, nbc = nblocks(16, 16, sr)
    data = K.write(np.zeros((nb + 2 * nbc, 64), np.int16), 16, 16, 50, sr, 0)
    return data[:Header(data).scan]


def colour_header(sr, W, H, dri=0, table=None):
    head = A.patch_size(_base(sr), W, H)
    if table:
        head = with_table(head, *table)
    return with_dri(head, dri) if dri else head


def gray_header(W, H, dri):
    """the header of the committed 8 x 8 one-component file (Pillow's, Annex K.3's luminance tables),
    its size and its DRI replaced"""
    data = G.files_of(8, 8)[0]
    return with_dri(A.patch_size(data[:Header(data).scan], W, H), dri)


# A luminance AC table whose 16-bit code of run 0 / size 10 is a zero and fifteen ones: one code each of
# 2 .. 15 bits (00, 010, 0110, ..) and two of 16 bits, 0x7FFE and 0x7FFF.  Annex K.3's 16-bit codes all
# have a zero among their bits 9 .. 15, which leaves a unit's second byte behind a seam unstuffed.
DEEP_TABLE = (0x10, [0] + [1] * 14 + [2],
              [0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0xf0, 0x11, 0x12, 0x21, 0x13, 0x0a])


# ---- the scan builder ------------------------------------------------------------------------------------
class Scan:
    """a scan, unit by unit.  `blocks`: per interval the blocks written, (component, DC difference,
    {zig-zag index: value}) in scan order"""

    def __init__(self, head):
        h = Header(head)
        self.dc = [h.codes[td] for td, _ in h.sel]
        self.ac = [h.codes[0x10 | ta] for _, ta in h.sel]
        self.ncomp = len(h.sel)
        self.lum = h.hs * h.vs if self.ncomp == 3 else 1
        self.out, self.begin, self.acc, self.n = bytearray(), 0, 0, 0
        self.blocks = [[]]
        self._dc_sum = 0

    @property
    def p(self):
        """where the next bit goes, seen from the interval's first byte"""
        return 8 * (len(self.out) - self.begin) + self.n

    @property
    def nmcu(self):
        return len(self.blocks[-1]) // (self.lum + self.ncomp - 1)

    def bits(self, code, ln):
        self.acc = self.acc << ln | code
        self.n += ln
        while self.n >= 8:
            self.n -= 8
            x = self.acc >> self.n
            self.acc &= (1 << self.n) - 1
            self.out.append(x)
            if x == 0xff:
                self.out.append(0)

    def _value(self, code, v):
        s = B.category(v)
        self.bits(*code(s))
        self.bits(v if v >= 0 else v + (1 << s) - 1, s)

    def block(self, comp, diff=0, acs=()):
        """a DC difference and AC units (run, value), (15, 0) for ZRL; EOB unless index 63 is written"""
        self._value(lambda s: self.dc[comp][s], diff)
        k, vals = 0, {}
        for run, v in acs:
            if v == 0:
                assert run == 15
                self.bits(*self.ac[comp][0xf0])
                k += 16
            else:
                self._value(lambda s: self.ac[comp][run << 4 | s], v)
                k += run + 1
                vals[k] = v
            assert k <= 63
        if k < 63:
            self.bits(*self.ac[comp][0])
        self.blocks[-1].append((comp, diff, vals))

    def mcu(self, y=(), cb=(0, ()), cr=(0, ())):
        """y: (diff, acs) of the first luma blocks, the others all zero"""
        for j in range(self.lum):
            self.block(0, *(y[j] if j < len(y) else (0, ())))
        if self.ncomp == 3:
            self.block(1, *cb)
            self.block(2, *cr)

    def block_bits(self, comp, diff=0):
        s = B.category(diff)
        return self.dc[comp][s][1] + s + self.ac[comp][0][1]

    @property
    def zero_mcu(self):
        return self.lum * self.block_bits(0) + (self.block_bits(1) + self.block_bits(2) if self.ncomp == 3 else 0)

    def _plan(self, nbits):
        """(DC difference, units of 0/1, units of 0/2) of an MCU of nbits bits: the first luma block holds
        them, every other block is zero"""
        a, b = self.ac[0][1][1] + 1, self.ac[0][2][1] + 2
        odd = -2 if self._dc_sum > 0 else 2
        for diff in (0, odd):
            rest = nbits - self.zero_mcu - (self.block_bits(0, diff) - self.block_bits(0))
            for j in range(63):
                if rest - b * j >= 0 and (rest - b * j) % a == 0 and (rest - b * j) // a + j <= 62:
                    return diff, (rest - b * j) // a, j
        raise AssertionError("no filler MCU of %d bits" % nbits)

    def filler(self, nbits):
        """an MCU of exactly nbits bits without an FF: units of -1 and -3, whose bits are zeros"""
        diff, k, j = self._plan(nbits)
        self._dc_sum += diff
        self.mcu([(diff, [(0, -1)] * k + [(0, -3)] * j)])

    def fill_to(self, p):
        """filler MCUs up to the bit p of the interval"""
        fat = self.zero_mcu + 62 * (self.ac[0][1][1] + 1)
        while self.p < p:
            n = p - self.p
            self.filler(fat if n >= 2 * fat else n // 2 if n > fat else n)
        assert self.p == p

    def pad(self):
        if self.n:
            self.bits((1 << (8 - self.n)) - 1, 8 - self.n)

    def restart(self):
        self.pad()
        self.out += bytes([0xff, 0xd0 + (len(self.blocks) - 1 & 7)])
        self.begin = len(self.out)
        self.blocks.append([])

    def file(self, head):
        self.pad()
        return bytes(head) + bytes(self.out) + b"\xff\xd9"


def expected(scan, W, H, sr):
    """int64 [blocks][64]: what a decoder owes for the builder's blocks, the running sums unclamped.
    sr None: a one-component frame, its blocks in raster order"""
    rows = scan_rows(W, H, sr) if sr is not None else [(i, 0) for i in range(G.nblocks(W, H))]
    blocks = [(iv, b) for iv, bs in enumerate(scan.blocks) for b in bs]
    assert len(rows) == len(blocks), (len(rows), len(blocks))
    out = np.zeros((len(rows), 64), np.int64)
    pred, cur = [0, 0, 0], 0
    for (row, comp), (iv, (c, diff, vals)) in zip(rows, blocks):
        assert comp == c
        if iv != cur:
            pred, cur = [0, 0, 0], iv
        pred[c] += diff
        out[row, 0] = pred[c]
        for k, v in vals.items():
            out[row, k] = v
    return out


def from_coef(data, coef, W, H, sr, mpi=0):
    """the builder's file for a frame's coefficients, behind the header and with the tables of `data`, a
    writer's file of them: the control that holds the builder to the host writer.  mpi: MCUs per interval"""
    head = data[:Header(data).scan]
    s = Scan(head)
    pred = [0, 0, 0]
    per = (s.lum + 2) * mpi
    for i, (row, comp) in enumerate(scan_rows(W, H, sr)):
        if per and i and i % per == 0:
            s.restart()
            pred = [0, 0, 0]
        z = coef[row].astype(np.int64)
        acs, prev = [], 0
        for k in np.flatnonzero(z[1:]) + 1:
            run = int(k) - prev - 1
            prev = int(k)
            acs += [(15, 0)] * (run // 16) + [(run % 16, int(z[k]))]
        s.block(comp, int(z[0]) - pred[comp], acs)
        pred[comp] = int(z[0])
    return s.file(head), s


# ---- cases -----------------------------------------------------------------------------------------------
class Case:
    """data; W, H, sr (None: one component); want: the builder's int64 coefficients or None; rc: what the
    host reader must say; guard(case)"""

    def __init__(self, data, W, H, sr, want=None, rc=0, guard=None, note=""):
        self.data, self.W, self.H, self.sr, self.want, self.rc, self.guard, self.note = data, W, H, sr, want, rc, guard, note
        if want is not None:
            want.setflags(write=False)

    @property
    def gray(self):
        return self.sr is None


def host(c):
    """(status, coef int16 [blocks][64] or None, qt or None) of the host reader for a case"""
    try:
        r = C.read_jfif_gray(c.data, 1) if c.gray else C.read_jfif(c.data, 1)
    except jpgx.JpgxError as e:
        return e.rc, None, None
    return 0, r["coef"].reshape(-1, 64), r["qt"]


def raw_interval(data, k=-1):
    b, e = K.intervals(data)[k]
    return data[b:e]


def stats(c):
    return (C.read_jfif_sub_gray if c.gray else C.read_jfif_sub)(c.data)["stats"]


def _one_row(s, head_kw=None, two=False):
    """the 4:4:4 file of the builder's one interval, 8 n x 8; two: 8 n x 16 with an interval of n zero
    MCUs in front (DRI = n)"""
    n = s.nmcu
    assert len(s.blocks) == 1 and 0 < n < 8192
    kw = head_kw or {}
    if not two:
        return s.file(colour_header(0, 8 * n, 8, **kw)), 8 * n, 8
    t = Scan(colour_header(0, 16, 16, **kw))
    for _ in range(n):
        t.mcu()
    t.restart()
    t.out += s.out
    t.acc, t.n = s.acc, s.n
    t.blocks[-1] = s.blocks[0]
    s.out, s.blocks = t.out, t.blocks
    return s.file(colour_header(0, 8 * n, 16, dri=n, **kw)), 8 * n, 16


# 1. stuffing on a tile seam.  Annex K.3's luminance AC code of 0/7 is the byte F8; its seven one-bits of
# +127 and the first bit of the EOB behind them (1010) make an FF of the next byte, X
FF_OFFSETS = {"ff_then_seam": -1, "ff00_before_seam": -2, "ff00_behind_seam": 0}


def guard_ff(off):
    def guard(c):
        raw = raw_interval(c.data)
        around = [raw[k * SEAM - 2:k * SEAM + 2].hex() for k in (1, 2)]
        print("bytes around the seams", around, "interval bytes", len(raw))
        assert len(raw) > 2 * SEAM + HALO
        for k in (1, 2):
            x = k * SEAM + off
            assert raw[x] == 0xff and raw[x + 1] == 0 and raw[x - 1] != 0xff
        st = stats(c)
        assert st["tiles"] == 3 and st["units_across_tile"] >= 2
    return guard


@functools.lru_cache(maxsize=None)
def ff_case(name):
    off = FF_OFFSETS[name]
    s = Scan(_base(0))
    assert s.ac[0][7] == (0xf8, 8) and s.ac[0][0] == (0b1010, 4)
    for k in (1, 2):
        s.fill_to(8 * (k * SEAM + off - 2) + 6)      # DC 00, then F8 fills byte X - 1
        s.mcu([(0, [(0, 127)])], cb=(3 * k, ()), cr=(-5 * k, ()))
    s.fill_to(s.p + 8 * 40 + 3)
    data, W, H = _one_row(s)
    return Case(data, W, H, 0, expected(s, W, H, 0), guard=guard_ff(off))


# 2. the deepest reach into the halo, and the carried states (0, .) and (., next block, z = 0)
def unit_reach(raw, r, bit, nbits):
    """the last byte a unit of nbits bits needs that begins at bit `bit` of byte r: the byte that holds its
    last bit, or the 00 behind that byte where it is an FF"""
    while True:
        nbits -= min(8 - bit, nbits)
        last, bit = r, 0
        if raw[r] == 0xff:
            assert raw[r + 1] == 0
            last, r = r + 1, r + 2
        else:
            r += 1
        if not nbits:
            return last


def unit_bits(raw, r, bit, nbits):
    """the unit's bits as an int"""
    data, k = 0, 0
    while 8 * k < bit + nbits:
        data = data << 8 | raw[r]
        r += 2 if raw[r] == 0xff else 1
        k += 1
    return data >> (8 * k - bit - nbits) & ((1 << nbits) - 1)


def guard_deep(c):
    raw = raw_interval(c.data)
    assert len(raw) > 3 * SEAM + HALO
    h = Header(c.data)
    assert h.codes[0x10][0x0a] == (0x7fff, 16)
    # seam 1: a unit of 16 + 10 bits from the tile's last bit on: a zero and 25 ones
    assert unit_bits(raw, SEAM - 1, 7, 26) == (1 << 25) - 1 and raw[SEAM - 1] != 0xff
    need = unit_reach(raw, SEAM - 1, 7, 26)
    print("halo bytes", raw[SEAM:SEAM + HALO].hex(), "the unit needs byte", need - SEAM, "behind the seam")
    assert raw[SEAM:SEAM + 8] == b"\xff\x00" * 4
    assert need == SEAM + 7 and need - SEAM + 1 >= 8 and need - SEAM < HALO      # the halo's first eight bytes, all of them
    # seam 2: a unit (0/1, the code 010 and a zero bit) ends with the tile's last bit and the next begins
    # behind it; seam 3: a luma block (DC 00, EOB 00) ends there
    assert raw[2 * SEAM - 1] & 15 == 0b0100 and raw[3 * SEAM - 1] & 15 == 0
    for name, p in c.marks.items():
        print(name, "begins at r", p >> 3, "bit", p & 7)
    assert c.marks["unit behind seam 2"] == 8 * 2 * SEAM and c.marks["block behind seam 3"] == 8 * 3 * SEAM
    st = stats(c)
    assert st["tiles"] == 4 and st["units_across_tile"] >= 1


@functools.lru_cache(maxsize=None)
def deep_case():
    kw = dict(table=DEEP_TABLE)
    s = Scan(colour_header(0, 16, 16, **kw))
    marks = {}
    ones = [(0, -1)] * 62
    assert s.ac[0][1] == (0b010, 3) and s.block_bits(0) == 4
    s.fill_to(8 * (SEAM - 1) + 7 - (2 + 4 * 62))
    # 62 units of four bits, then 0/10 = +1023 at index 63 from the tile's last bit on: no EOB, and Cb's DC
    # code of size 11 (1111 1111 110) goes on with ones
    s.mcu([(0, ones + [(0, 1023)])], cb=(2047, ()), cr=(-2047, ()))
    s.fill_to(8 * 2 * SEAM - 4 - 2)
    marks["unit before seam 2"] = s.p + 2
    marks["unit behind seam 2"] = s.p + 6
    s.mcu([(0, [(0, -1), (0, -3)])], cb=(-2047, ()), cr=(2047, ()))
    s.fill_to(8 * 3 * SEAM - 4)
    marks["block behind seam 3"] = s.p + 4
    s.mcu(cb=(-7, [(0, 1)]), cr=(9, [(1, -2)]))
    s.fill_to(s.p + 8 * 40 + 5)
    data, W, H = _one_row(s, kw)
    c = Case(data, W, H, 0, expected(s, W, H, 0), guard=guard_deep)
    c.marks = marks
    return c


# 3. interval lengths around the tile and the halo
LENGTHS = [(k, d, two) for two in (False, True) for k in (1, 2) for d in (0, 1, 15, 16, 17)]


def guard_length(k, d):
    def guard(c):
        raw = raw_interval(c.data)
        print("interval bytes", len(raw), "its last", raw[-2:].hex())
        assert len(raw) == k * SEAM + d
        # Cr's block of the last MCU (DC 00, EOB 00) begins with the last byte, four one-bits pad it:
        # where d > 0 a unit begins in the last tile, and for d = 1 that tile is one byte that holds two
        assert raw[-1] == 0x0f and c.last_unit == 8 * (len(raw) - 1)
        assert d == 0 or c.last_unit >= 8 * k * SEAM
        assert stats(c)["tiles"] == (k if d == 0 else k + 1) + (1 if len(K.intervals(c.data)) == 2 else 0)
    return guard


@functools.lru_cache(maxsize=None)
def length_case(k, d, two):
    s = Scan(_base(0))
    L = k * SEAM + d
    s.fill_to(8 * (L - 1) - s.block_bits(0) - s.block_bits(1))
    s.mcu()
    last = s.p - s.block_bits(2)
    assert (s.block_bits(0), s.block_bits(1), s.block_bits(2)) == (6, 4, 4)
    data, W, H = _one_row(s, two=two)
    c = Case(data, W, H, 0, expected(s, W, H, 0), guard=guard_length(k, d))
    c.last_unit = last
    return c


# 4. refusals on a seam, each with the good file it was made of (its neighbours in a batch)
def guard_refused(c):
    rc = host(c)[0]
    print(c.note, "->", rc)
    assert rc == SCAN


def _sub(data, at, new):
    return data[:at] + new + data[at + len(new):]


@functools.lru_cache(maxsize=None)
def refusals():
    """{name: (the refused case, the good case)}"""
    out = {}

    def add(name, good, data):
        out[name] = (Case(data, good.W, good.H, good.sr, rc=SCAN, guard=guard_refused, note=name), good)

    good = ff_case("ff_then_seam")
    b, e = K.intervals(good.data)[0]
    for k in (1, 2):
        assert good.data[b + k * SEAM - 1:b + k * SEAM + 1] == b"\xff\x00"
        add("01 for the 00 behind seam %d" % k, good, _sub(good.data, b + k * SEAM, b"\x01"))
        for more in (0, 1):
            add("cut at seam %d + %d" % (k, more), good, good.data[:b + k * SEAM + more] + b"\xff\xd9")
    for k, two in ((1, False), (2, False), (1, True)):
        good = length_case(k, 0, two)
        b, e = K.intervals(good.data)[-1]
        assert e - b == k * SEAM and e == len(good.data) - 2
        add("an FF ends the interval of %d tiles%s" % (k, ", the second" if two else ""), good, _sub(good.data, e - 1, b"\xff"))
    good = deep_case()
    b, e = K.intervals(good.data)[0]
    # sixteen one-bits where the third tile's first unit begins: a code in no table
    add("an undefined code behind seam 2", good, _sub(good.data, b + 2 * SEAM, b"\xff\x00\xff\x00"))
    return out


# 6. all 16 load alignments: 16 copies of a file at a stride that is 1 modulo 16
COPIES = 16


def odd_stride(n):
    return n + (1 - n) % 16


def guard_residues(base, stride, c):
    """file k's scan begins at every residue of the address modulo 16 (base: the batch's address)"""
    scan = K.intervals(c.data)[0][0]
    res = sorted((base + k * stride + scan) % 16 for k in range(COPIES))
    print("residues", res)
    assert res == list(range(16))


def guard_short(c):
    iv = K.intervals(c.data)
    assert len(iv) == 250 and 0 < max(e - b for b, e in iv) < SUB


@functools.lru_cache(maxsize=None)
def short_case():
    """K.short_intervals: every interval shorter than a subsequence, both pieces of its load ragged"""
    W, H, sr, _, data = K.short_intervals()
    return Case(data, W, H, sr, guard=guard_short)


# 7. most rounds: a frame of maximal blocks without restart intervals
ROUNDS_FRAME = (48, 16)            # 36 blocks, 9,484 bytes: the smallest whose scan fills a tile (33 blocks do not)


def maximal(W, H):
    coef = np.zeros((3 * (W // 8) * (H // 8), 64), np.int16)
    coef[:, 1::2] = 1023
    coef[:, 2::2] = -1023
    coef[:, 0] = np.where(np.arange(coef.shape[0]) & 1, 1023, -1024)
    return coef


def guard_rounds(c):
    st = stats(c)
    print("file bytes", len(c.data), st)
    assert st["rounds_max"] == TILE - 1 and st["starts_on_stuffing"] > 0 and st["units_across_tile"] > 0
    assert C.jfif_info(c.data)["restart_interval"] == 0


@functools.lru_cache(maxsize=None)
def rounds_case():
    W, H = ROUNDS_FRAME
    return Case(K.write(maximal(W, H), W, H, 50, 0, 0), W, H, 0, guard=guard_rounds)


# 8. the DC predictors' chunks of 256 blocks
DC_SHAPES = [(0, 255), (0, 256), (0, 257), (0, 513), (2, 64), (2, 65), (1, 128), (1, 129), (None, 257)]
DC_CHUNK = 256


def dc_geometry(sr, n):
    """(W, H, blocks per component) of a frame of n MCUs in one row"""
    if sr is None:
        return 8 * n, 8, [n]
    return (8, 16, 16)[sr] * n, (8, 8, 16)[sr], [n * (1, 2, 4)[sr], n, n]


def _ramp(count, top, sign):
    """DC differences of one sign whose running sum reaches sign * top (or -top - 1) exactly at block
    `count - 1` and not before"""
    total = top if sign > 0 else top + 1
    q = total // count
    d = [q] * (count - 1) + [total - q * (count - 1)]
    assert max(d) <= B.DC_MAX and count >= 17
    return [sign * x for x in d]


def dc_diffs(sr, n, kind, comp=0, sign=1):
    """per component the DC differences of its blocks in decode order.
    random: nonzero throughout, a seeded walk inside +-2047 a step and inside int16 in sum
    hold:   every component reaches 32767 (-32768) at its block 255 (its last but one where it has fewer
            than 257) and stays there
    over:   component `comp` as hold and one more step of `sign` at the next block; the others random"""
    _, _, counts = dc_geometry(sr, n)
    rng = np.random.default_rng(1000 * n + 10 * (3 if sr is None else sr) + 1)
    out = []
    for c, cnt in enumerate(counts):
        walk, acc = [], 0
        for _ in range(cnt):
            while True:
                d = int(rng.integers(-B.DC_MAX, B.DC_MAX + 1))
                if d and I16[0] <= acc + d <= I16[1]:
                    break
            acc += d
            walk.append(d)
        at = DC_CHUNK - 1 if cnt > DC_CHUNK else cnt - 2
        if kind == "hold" or (kind == "over" and c == comp):
            walk = _ramp(at + 1, I16[1], sign) + [0] * (cnt - at - 1)
            if kind == "over":
                walk[at + 1] = sign
        out.append(walk)
    return out


def dc_variants(sr):
    comps = (0,) if sr is None else (0, 1, 2)
    return [("random", 0, 1), ("hold", 0, 1), ("hold", 0, -1)] + [("over", c, s) for c in comps for s in (1, -1)]


def guard_dc(c):
    sums = [np.cumsum(d) for d in c.diffs]
    ok = all(I16[0] <= int(s.min()) and int(s.max()) <= I16[1] for s in sums)
    assert c.rc == (0 if ok else SCAN)
    kind, comp, sign = c.variant
    for k, s in enumerate(sums):
        at = DC_CHUNK - 1 if len(s) > DC_CHUNK else len(s) - 2
        if kind == "random":
            assert all(c.diffs[k])
        if kind == "hold" or (kind == "over" and k == comp):
            edge = I16[1] if sign > 0 else I16[0]
            assert s[at] == edge and abs(int(s[at - 1])) < abs(edge) and s[at + 1] == edge + (sign if kind == "over" else 0)
            if kind == "over":                       # the next chunk's own partial sums stay inside int16
                assert all(abs(int(x)) <= 1 for x in np.cumsum(c.diffs[k][at + 1:]))
            else:
                assert (s[at:] == edge).all()
    rc, coef, _ = host(c)
    assert rc == c.rc
    if rc == 0:
        assert np.array_equal(coef, c.want)


@functools.lru_cache(maxsize=None)
def dc_case(sr, n, variant):
    kind, comp, sign = variant
    W, H, counts = dc_geometry(sr, n)
    diffs = dc_diffs(sr, n, kind, comp, sign)
    head = gray_header(W, H, 0) if sr is None else colour_header(sr, W, H)
    s = Scan(head)
    at = [0, 0, 0]

    def take(c):
        at[c] += 1
        return diffs[c][at[c] - 1]

    for _ in range(n):
        s.mcu([(take(0), ()) for _ in range(s.lum)], *([(take(1), ()), (take(2), ())] if sr is not None else []))
    assert at[:len(counts)] == counts
    c = Case(s.file(head), W, H, sr, expected(s, W, H, sr), rc=SCAN if kind == "over" else 0, guard=guard_dc)
    c.diffs, c.variant = diffs, variant
    return c


# 9. k_jd_frame's passes of 256 chunks
PASSES_FRAME = (512, 1024, 60.0)


def guard_passes(c):
    n = len(c.data)
    marks = np.array([b - 2 for b, _ in K.intervals(c.data)[1:]])
    second = int(((marks >= 256 * CHUNK) & (marks < 512 * CHUNK)).sum())
    third = int((marks >= 512 * CHUNK).sum())
    nchunk = -(-c.stride // CHUNK)
    print("file bytes", n, "markers", len(marks), "in chunks 256 .. 511:", second, "from chunk 512 on:", third, "chunks", nchunk)
    assert n > 512 * CHUNK and second >= 2 and third >= 2 and nchunk >= 514 and c.stride >= n
    # the neighbour ends inside the first pass: every chunk of the later passes lies behind its len
    assert len(c.small.data) < 256 * CHUNK and (c.small.W, c.small.H) == (c.W, c.H)


@functools.lru_cache(maxsize=None)
def passes_case():
    W, H, scale = PASSES_FRAME
    data = K.write(lap(W, H, 0, 7, scale=scale), W, H, 50, 0, 1)
    c = Case(data, W, H, 0, guard=guard_passes)
    c.stride = max(len(data), 513 * CHUNK + 1)
    c.small = Case(K.write(np.zeros((3 * (W // 8) * (H // 8), 64), np.int16), W, H, 50, 0, 1), W, H, 0)
    return c


# 10. the gray kernel's grid stride
GRID_BLOCKS = 1100


def guard_grid(c):
    iv = gray_intervals(c.data)
    print("intervals", len(iv), "bytes", len(c.data))
    assert len(iv) == GRID_BLOCKS > SUB_GRID and C.jfif_info_gray(c.data)["restart_interval"] == 1


def gray_intervals(data):
    """K.intervals for a one-component file"""
    scan = C.jfif_info_gray(data)["scan_offset"]
    b = np.frombuffer(data, np.uint8)
    ff = np.flatnonzero(b[scan:-2] == 0xff) + scan
    marks = ff[(b[ff + 1] & 0xf8) == 0xd0].tolist()
    return list(zip([scan] + [m + 2 for m in marks], marks + [len(data) - 2]))


@functools.lru_cache(maxsize=None)
def grid_case():
    W, H = 8, 8 * GRID_BLOCKS
    head = gray_header(W, H, 1)
    s = Scan(head)
    rng = np.random.default_rng(10)
    for i in range(GRID_BLOCKS):
        if i:
            s.restart()
        acs = [(int(rng.integers(0, 4)), int(rng.integers(1, 200)) * (1, -1)[i & 1]) for _ in range(i % 5)]
        s.mcu([(int(rng.integers(-B.DC_MAX, B.DC_MAX + 1)), acs)])
    return Case(s.file(head), W, H, None, expected(s, W, H, None), guard=guard_grid)


# ---- the lists the two test files run ---------------------------------------------------------------------
def seam_cases():
    """{name: build() -> Case} of the cases 1 .. 3, one-interval and two-interval files of tiles"""
    out = {name: functools.partial(ff_case, name) for name in FF_OFFSETS}
    out["deep_halo"] = deep_case
    for k, d, two in LENGTHS:
        out["length_%dx8192+%d%s" % (k, d, "_second" if two else "")] = functools.partial(length_case, k, d, two)
    return out


SEAM_CASES = seam_cases()
REFUSALS = ["01 for the 00 behind seam 1", "01 for the 00 behind seam 2", "cut at seam 1 + 0", "cut at seam 1 + 1",
            "cut at seam 2 + 0", "cut at seam 2 + 1", "an FF ends the interval of 1 tiles", "an FF ends the interval of 2 tiles",
            "an FF ends the interval of 1 tiles, the second", "an undefined code behind seam 2"]


def guarded(c):
    """the case with its guard run (once per case object)"""
    if c.guard and not getattr(c, "_guarded", False):
        c.guard(c)
        c._guarded = True
    return c
