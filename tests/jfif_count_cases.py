"""Test helper of tests/test_jfif_tables.py and tests/test_jfif_tables_gpu.py: coefficient frames
made from prescribed symbol counts, so that the per-image Huffman table builders (jx_jfif_optimal on
the host, k_jf_tables and k_jf_count on the device) meet the counts at which a
restatement of Annex K.2 can go wrong: ties inside one lane of the device's wave, ties between a
merged tree and a leaf and with the reserved point, the symbols of runs 12-15, all 162 AC symbols at
once, trees far deeper than 16 and the deepest DC tree.

frame_from_counts() is never trusted.  A case is the frame, the counts that symbol_counts (the walk
of tests/jfif_bits.py) finds in it, an instrumented copy of annex_k2 run on those counts, and a guard:
an assertion on those figures, computed on the CPU before any device is called.  A changed seed or a
different numpy fails the guard; it does not quietly empty the case.  Quality 50 throughout."""
import functools
import itertools

import numpy as np

from jfif_inputs import nblocks, scan_rows
from jfif_bits import interval_rows
from jfif_opt_common import _host, annex_k2, dht_tables, fib_vector, symbol_counts

Q = 50
MAX_BLOCKS = 6000                                          # per frame: the walk is Python
ZRL, EOB = 0xf0, 0x00
AC_SYMS = [r << 4 | s for r in range(16) for s in range(1, 11)]      # the 160 run/size symbols
LUMA, CHROMA = 1, 3                                        # the AC tables among symbol_counts' four
DC_LUMA, DC_CHROMA = 0, 2


# ---- Annex K.2 with counters ---------------------------------------------------------------------
def k2_figures(counts):
    """annex_k2 (tests/jfif_opt_common.py) with counters: a dict of its bits, vals and depth, the
    merges [(v1, v2)], `ties` (merges at which a third live frequency equals freq[v1] or freq[v2]),
    `moves` (passes of Figure K.3's inner loop), `skipped` (its steps of j over empty levels) and
    `levels` (the codes of each length before the reserved point leaves the deepest one)"""
    freq = [int(c) for c in counts] + [1]
    codesize, others = [0] * 257, [-1] * 257
    merges, ties = [], 0

    def least(skip):
        best = -1
        for i in range(257):
            if freq[i] and i != skip and (best < 0 or freq[i] <= freq[best]):
                best = i
        return best

    while True:
        v1 = least(-1)
        v2 = least(v1)
        if v2 < 0:
            break
        merges.append((v1, v2))
        ties += any(freq[i] in (freq[v1], freq[v2]) for i in range(257) if freq[i] and i not in (v1, v2))
        freq[v1] += freq[v2]
        freq[v2] = 0
        while True:
            codesize[v1] += 1
            if others[v1] < 0:
                break
            v1 = others[v1]
        others[v1] = v2
        while True:
            codesize[v2] += 1
            if others[v2] < 0:
                break
            v2 = others[v2]
    depth = max(codesize)
    bits = [0] * (max(depth, 16) + 1)
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    moves = skipped = 0
    i = depth
    while i > 16:
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
                skipped += 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
            moves += 1
        i -= 1
    levels = bits[1:17]                                    # the reserved point still among them
    i = 16
    while i > 0 and bits[i] == 0:
        i -= 1
    if i:
        bits[i] -= 1
    vals = [s for _, s in sorted((codesize[s], s) for s in range(256) if codesize[s])]
    return dict(bits=bits[1:17], levels=levels, vals=vals, depth=depth, merges=merges, ties=ties, moves=moves,
                skipped=skipped, used=len(vals), total=int(sum(int(c) for c in counts)))


# ---- frames from counts --------------------------------------------------------------------------
def _pack(ac, n):
    """n blocks' tokens [[(zeros before the coefficient, size)]] with the AC symbol counts `ac`
    ({run << 4 | size: count}, ZRL 0xf0 included).  A token of run r takes r + 1 of a block's 63
    positions; a ZRL is put in front of a token of the least run, which then takes 16 more.  The
    largest tokens go first.  With ac[EOB] given that many blocks end before position 63 and all the
    others at it exactly (the whole-block trick of test_jfif_opt.py's length_limiting_frame);
    without it the blocks are filled as far as the tokens go, and EOB comes out as it may."""
    ac = {int(k): int(v) for k, v in (ac or {}).items()}
    eob, zrl = ac.pop(EOB, None), ac.pop(ZRL, 0)
    ac = {s: c for s, c in ac.items() if c}
    assert all(s in AC_SYMS for s in ac), "no such symbol"
    kinds = [[s >> 4, s & 15, c] for s, c in ac.items()]    # zeros, size, tokens left
    if zrl:
        kinds.sort()
        assert kinds and kinds[0][2] >= zrl, "a ZRL needs a coded coefficient behind it"
        kinds[0][2] -= zrl
        kinds.append([kinds[0][0] + 16, kinds[0][1], zrl])
    kinds = sorted((k for k in kinds if k[2]), reverse=True)
    full = n if eob is None else n - eob
    assert full >= 0
    blocks = []
    for b in range(n):
        room = 63 if b < full else 62
        toks = []
        for k in kinds:
            take = min(k[2], room // (k[0] + 1))
            k[2] -= take
            room -= take * (k[0] + 1)
            toks += [(k[0], k[1])] * take
        assert eob is None or b >= full or room == 0, "a block that must end at position 63 does not"
        blocks.append(toks)
    assert not any(k[2] for k in kinds), "the tokens do not fit the frame"
    return blocks


def _dc_steps(hist, n, rng):
    """n DC steps' magnitudes with the category histogram {category: count}: one category alone
    gives +d, -d, ... with d the category's largest value, several a seeded order and seeded values"""
    hist = {int(k): int(v) for k, v in (hist or {0: n}).items() if v}
    assert sum(hist.values()) == n, (sum(hist.values()), n)
    cats = [c for c, k in sorted(hist.items()) for _ in range(k)]
    if len(hist) == 1:
        return [(1 << c) - 1 for c in cats]
    cats = [cats[i] for i in rng.permutation(n)]
    return [int(rng.integers(1 << (c - 1), 1 << c)) if c else 0 for c in cats]


def frame_from_counts(W, H, sr, ac_luma=None, ac_chroma=None, dc_luma=None, dc_chroma=None, rr=1, seed=0):
    """int16 [nb + 2 nbc][64]: a frame whose scan has the AC symbol counts ac_* ({run << 4 | size:
    count}; Cb and Cr share ac_chroma) and the DC category counts dc_* ({category: count} over every
    block of the table; None: all DC zero), coded with rr MCU rows per restart interval.  A
    coefficient of size s is +-2^(s - 1), the signs alternating.  A DC step goes against the sign of
    the predictor, which is 0 at every interval's start, so the values stay inside +-2047 and the
    writer's clamp never acts."""
    rng = np.random.default_rng(seed)
    nb, nbc = nblocks(W, H, sr)
    assert nb + 2 * nbc <= MAX_BLOCKS
    coef = np.zeros((nb + 2 * nbc, 64), np.int16)
    sign = 1
    for first, n, ac in ((0, nb, ac_luma), (nb, 2 * nbc, ac_chroma)):
        blocks = _pack(ac, n)
        for row, b in zip(first + rng.permutation(n), blocks):
            k = 1
            for zeros, size in b:
                k += zeros
                coef[row, k] = sign << (size - 1)
                sign = -sign
                k += 1
            assert k <= 64
    order = scan_rows(W, H, sr)
    per = interval_rows(H, sr, rr) * (W // 8 // (1, 2, 2)[sr]) * (3, 4, 6)[sr]
    steps = _dc_steps(dc_chroma, 2 * nbc, rng)
    steps = {0: iter(_dc_steps(dc_luma, nb, rng)), 1: iter(steps[:nbc]), 2: iter(steps[nbc:])}
    pred = [0, 0, 0]
    for i, (row, comp) in enumerate(order):
        if i % per == 0:
            pred = [0, 0, 0]
        d = next(steps[comp])
        pred[comp] += -d if pred[comp] > 0 else d
        assert abs(pred[comp]) <= 2047
        coef[row, 0] = pred[comp]
    return coef


# ---- a case: the frame, what the walk counts in it, and the guard ---------------------------------
class Case:
    """W, H, sr, rr, coef (read-only), cnt (symbol_counts), k2 (k2_figures per table), data (the host
    writer's file with per-image tables), table (the table the case is about)"""

    def __init__(self, W, H, sr, rr, coef, table):
        coef = np.ascontiguousarray(coef, np.int16)
        coef.setflags(write=False)
        self.W, self.H, self.sr, self.rr, self.coef, self.table = W, H, sr, rr, coef, table
        self.cnt = symbol_counts(coef, W, H, sr, rr)
        self.k2 = [k2_figures(c) for c in self.cnt]
        for c, k in zip(self.cnt, self.k2):
            assert (k["bits"], k["vals"], k["depth"]) == annex_k2(c)      # the counters changed nothing
        self.data = _host(coef, W, H, Q, sr, rr)

    @property
    def fig(self):
        return self.k2[self.table]

    @property
    def counts(self):
        return self.cnt[self.table]

    def show(self, name):
        f = self.fig
        nb, nbc = nblocks(self.W, self.H, self.sr)
        print(f"{name}: {self.W}x{self.H} sr {self.sr} rr {self.rr}, {nb + 2 * nbc} blocks, table {self.table}: "
              f"used {f['used']}, symbols {f['total']}, EOB {int(self.cnt[self.table][0])}, depth {f['depth']}, "
              f"moves {f['moves']}, skipped {f['skipped']}, tie merges {f['ties']} of {len(f['merges'])}, "
              f"bits {f['bits']}, DHT bytes {4 + 17 + f['used']}, file bytes {len(self.data)}")


def _same_lane(m):
    """both symbols proper, and of one lane of k_jf_tables' wave (lane l owns l, l + 64, l + 128, l + 192)"""
    return m[0] < 256 and m[1] < 256 and m[0] % 64 == m[1] % 64


def _only(table, ac):
    """the frame's arguments with `ac` in the table the case is about and nothing in the other"""
    return dict(ac_luma=ac) if table == LUMA else dict(ac_chroma=ac)


# A: all 162 AC symbols, 7 of each; EOB as the packing leaves it
A_FRAMES = {LUMA: (128, 88), CHROMA: (64, 88)}             # 176 blocks of the table's


def _build_a(table, W=None, H=None):
    W, H = (W, H) if W else A_FRAMES[table]
    ac = {s: 7 for s in AC_SYMS + [ZRL]}
    return Case(W, H, 0, 2, frame_from_counts(W, H, 0, **_only(table, ac), rr=2), table)


def guard_a(c):
    f = c.fig
    assert f["used"] == 162 and 4 + 17 + f["used"] == 2 + 181
    assert all(int(c.counts[s]) == 7 for s in AC_SYMS + [ZRL]) and c.counts[EOB] > 0
    assert f["ties"] >= 150
    assert len(dht_tables(c.data)[0x10 | c.table >> 1][1]) == 162


# B: 150 symbols of count 1 under a chain of twelve, 151 x fib_vector(12); EOB is one of the twelve
CHAIN = [151 * x for x in fib_vector(12)]


def _chain_counts(n):
    """the counts of case B for n blocks of the table: the crowd, and the chain on EOB, the ten run 0
    symbols and 0x11, placed so that n - EOB blocks are filled to position 63 exactly"""
    crowd = [s for s in AC_SYMS if s >> 4 >= 1 and s != 0x11] + [ZRL]
    assert len(crowd) == 150
    base = sum((s >> 4) + 1 for s in crowd if s != ZRL) + 16
    for e in CHAIN:
        rest = [x for x in CHAIN if x != e]
        for one in rest:                                   # the chain count that goes to 0x11 (two positions)
            p = base + sum(rest) + one
            if 63 * (n - e) <= p <= 63 * (n - e) + 62 * e and n >= e:
                ac = {s: 1 for s in crowd}
                ac[EOB], ac[0x11] = e, one
                ac.update(zip(range(0x01, 0x0b), [x for x in rest if x != one]))
                return ac
    raise AssertionError("no placement")


B_FRAMES = {                                               # name: (W, H, sr, table, rr)
    "B_luma_444": (352, 352, 0, LUMA, 2),                  # 1,936 luma blocks
    "B_luma_422": (352, 352, 1, LUMA, 2),
    "B_chroma_444": (352, 352, 0, CHROMA, 2),              # 2 x 1,936 chroma blocks
    "B_chroma_420": (704, 352, 2, CHROMA, 2),              # 2 x 968 chroma blocks under 3,872 luma blocks
    "H_rr1": (352, 352, 0, LUMA, 1),                       # 44 intervals of 132 blocks
    "H_one_interval": (352, 352, 0, LUMA, 1000),           # one interval of 5,808 blocks
}


def _build_b(name):
    W, H, sr, table, rr = B_FRAMES[name]
    nb, nbc = nblocks(W, H, sr)
    ac = _chain_counts(nb if table == LUMA else 2 * nbc)
    return Case(W, H, sr, rr, frame_from_counts(W, H, sr, **_only(table, ac), rr=rr), table)


def guard_b(c):
    f = c.fig
    assert f["used"] == 162 and f["depth"] >= 19 and f["moves"] >= 100 and f["skipped"] >= 100
    assert f["bits"][15] >= 140
    ones = [s for s in range(256) if c.counts[s] == 1]
    assert len(ones) == 150 and ZRL in ones and all(r << 4 | s in ones for r in range(12, 16) for s in range(1, 11))
    assert sorted(int(x) for x in c.counts if x > 1) == CHAIN


# C: the Fibonacci vector on 22 symbols, EOB one of them
FIB22 = fib_vector(22)
C_SMALL = [0xc1, 0xd1, 0xe1, 0xf1, 0xc2, 0xd2]             # the six smallest counts: symbols >= 192
C_PAIR = (0x01, 0x41)                                      # the two largest: one lane
C_FRAMES = {LUMA: (512, 320, 2), CHROMA: (320, 256, 0)}    # 2,560 blocks of the table's, 3,840 in all


def _build_c(table):
    W, H, sr = C_FRAMES[table]
    nb, nbc = nblocks(W, H, sr)
    n = nb if table == LUMA else 2 * nbc
    ac = dict(zip(C_SMALL, FIB22[:6]))
    ac[C_PAIR[0]], ac[C_PAIR[1]] = FIB22[21], FIB22[20]
    base = sum(((s >> 4) + 1) * k for s, k in ac.items())
    mid = FIB22[6:20]
    for e in mid:
        rest = [x for x in mid if x != e]
        for k in range(4, 11):                             # the counts on run 1; the others, at most 9, on run 0
            for pick in itertools.combinations(rest, k):
                p = base + sum(rest) + sum(pick)
                if 63 * (n - e) <= p <= 63 * (n - e) + 62 * e:
                    ac[EOB] = e
                    ac.update(zip(range(0x11, 0x1b), pick))
                    ac.update(zip(range(0x02, 0x0b), [x for x in rest if x not in pick]))
                    return Case(W, H, sr, 4, frame_from_counts(W, H, sr, **_only(table, ac), rr=4), table)
    raise AssertionError("no placement")


def guard_c(c):
    f = c.fig
    assert sorted(int(x) for x in c.counts if x) == FIB22 and f["total"] == 75023
    assert f["depth"] == 22 and f["moves"] >= 16 and f["skipped"] >= 9
    assert sorted(int(c.counts[s]) for s in C_SMALL) == FIB22[:6] and min(C_SMALL) >= 192
    assert C_PAIR[1] == C_PAIR[0] + 64 and [int(c.counts[s]) for s in C_PAIR] == [FIB22[21], FIB22[20]]


# D: the four symbols of one lane; and four symbols of four rows of 16 lanes as the whole table
D_LANE = (0x11, 0x51, 0x91, 0xd1)                          # 17, 17 + 64, 17 + 128, 17 + 192
D_ROWS = (3, 16 + 3, 32 + 3, 48 + 3)
D_COUNTS = {"D_equal": (5, 5, 5, 5), "D_1122": (1, 1, 2, 2)}
D_FRAMES = {LUMA: (32, 32), CHROMA: (32, 16)}              # 16 blocks of the table's
D_ROWS_FRAMES = {LUMA: (80, 8), CHROMA: (40, 8)}           # 10 blocks, each filled to position 63


def _build_d(kind, table):
    if kind == "D_rows":
        W, H = D_ROWS_FRAMES[table]
        ac = dict(zip(D_ROWS, (63,) * 4))
        ac[EOB] = 0
    else:
        W, H = D_FRAMES[table]
        ac = dict(zip(D_LANE, D_COUNTS[kind]))
    return Case(W, H, 0, 1, frame_from_counts(W, H, 0, **_only(table, ac)), table)


def guard_d(kind):
    def guard(c):
        f = c.fig
        m = f["merges"]
        if kind == "D_rows":
            assert sorted(f["vals"]) == list(D_ROWS) and f["ties"] >= 2
            assert len({s % 64 // 16 for s in D_ROWS}) == 4
            return
        assert [int(c.counts[s]) for s in D_LANE] == list(D_COUNTS[kind]) and f["used"] == 5
        assert c.counts[EOB] > 2 * max(D_COUNTS[kind])
        # the reserved point has the least frequency there is and the largest index: it is v1 of every
        # table's first merge.  The first merge of two symbols proper takes two of one lane
        assert m[0][0] == 256 and m[0][1] in D_LANE
        assert _same_lane(next(x for x in m if 256 not in x))
        if kind == "D_equal":
            assert _same_lane(m[1])
        else:                                              # the reserved point ties with two symbols,
            assert m[0][1] == 0x51 and f["ties"] >= 2      # its tree of 2 with the two leaves of 2
            assert m[1] == (0x11, 256)
    return guard


# E: counts 1..3 on about 100 seeded symbols
E_SEEDS = (1, 2, 3)
E_FRAMES = {LUMA: (64, 48), CHROMA: (32, 48)}              # 48 blocks of the table's


def _build_e(seed, table):
    rng = np.random.default_rng(seed)
    syms = AC_SYMS + [ZRL]
    ac = {syms[i]: int(rng.integers(1, 4)) for i in rng.permutation(len(syms))[:100]}
    if ZRL in ac:                                          # no more ZRLs than tokens of the least symbol
        ac[ZRL] = min(ac[ZRL], ac[min(ac)])
    W, H = E_FRAMES[table]
    return Case(W, H, 0, 1, frame_from_counts(W, H, 0, **_only(table, ac), seed=seed), table)


def guard_e(c):
    f = c.fig
    assert f["used"] >= 95 and max(int(x) for x in c.counts[1:]) <= 3 and f["ties"] >= 60


# F: DC
FIB12 = fib_vector(12)


def _build_f(kind):
    if kind == "F_fib_luma":                               # 608 luma blocks
        W, H, table, dc = 256, 152, DC_LUMA, dict(dc_luma=dict(enumerate(FIB12)), dc_chroma={3: 2 * 608})
    elif kind == "F_fib_chroma":                           # 2 x 304 chroma blocks
        W, H, table, dc = 128, 152, DC_CHROMA, dict(dc_chroma=dict(enumerate(FIB12)), dc_luma={9: 304})
    elif kind == "F_equal":                                # 24 luma blocks, 48 chroma blocks
        W, H, table = 48, 32, DC_LUMA
        dc = dict(dc_luma={c: 2 for c in range(12)}, dc_chroma={c: 4 for c in range(12)})
    else:                                                  # one category in each table
        W, H, table, dc = 48, 32, DC_LUMA, dict(dc_luma={11: 24}, dc_chroma={6: 48})
    return Case(W, H, 0, 2, frame_from_counts(W, H, 0, **dc, rr=2, seed=12), table)


def guard_f(kind):
    def guard(c):
        f = c.fig
        if kind.startswith("F_fib"):
            assert [int(x) for x in c.counts[:12]] == FIB12 and f["depth"] == 12
            assert f["levels"][:12] == [1] * 11 + [2] and f["bits"] == [1] * 12 + [0] * 4      # the deepest DC tree
        elif kind == "F_equal":
            for t, k in ((DC_LUMA, 2), (DC_CHROMA, 4)):
                assert [int(x) for x in c.cnt[t][:12]] == [k] * 12 and c.k2[t]["used"] == 12
            # the reserved point's merge with eleven leaves tied for v2, then five merges of two equal
            # leaves beside a third (11, 9, 7, 5, 3 equal leaves live)
            assert f["ties"] >= 6
        else:
            for t, cat, k in ((DC_LUMA, 11, 24), (DC_CHROMA, 6, 48)):
                assert int(c.cnt[t][cat]) == k == int(c.cnt[t].sum())
                assert c.k2[t]["bits"] == [1] + [0] * 15 and c.k2[t]["vals"] == [cat]
    return guard


def _cases():
    """{name: (build() -> Case, guard)}"""
    out = {}
    for t, tag in ((LUMA, "luma"), (CHROMA, "chroma")):
        out[f"A_{tag}"] = (lambda t=t: _build_a(t), guard_a)
        out[f"C_{tag}"] = (lambda t=t: _build_c(t), guard_c)
        for kind in ("D_equal", "D_1122", "D_rows"):
            out[f"{kind}_{tag}"] = (lambda kind=kind, t=t: _build_d(kind, t), guard_d(kind))
        for seed in E_SEEDS:
            out[f"E{seed}_{tag}"] = (lambda seed=seed, t=t: _build_e(seed, t), guard_e)
    for name in B_FRAMES:
        out[name] = (lambda name=name: _build_b(name), guard_b)
    for kind in ("F_fib_luma", "F_fib_chroma", "F_equal", "F_one_category"):
        out[kind] = (lambda kind=kind: _build_f(kind), guard_f(kind))
    return out


COUNT_CASES = _cases()
WIDE = ("A_luma", "A_chroma", "B_luma_444", "B_luma_422", "B_chroma_444", "B_chroma_420", "C_luma", "C_chroma")


@functools.lru_cache(maxsize=None)
def count_case(name):
    """the case, built once and guarded: tests share it and leave it unchanged"""
    build, guard = COUNT_CASES[name]
    c = build()
    c.show(name)
    guard(c)
    return c


# G: a batch of four frames of one geometry
G_FRAME = (352, 352, 0, 2)                                 # W, H, sr, rr: B_luma_444's


@functools.lru_cache(maxsize=None)
def batch_cases():
    """[deep table as luma AC, deep table as chroma AC, case A in both AC tables, all zero], guarded"""
    W, H, sr, rr = G_FRAME
    nb, nbc = nblocks(W, H, sr)
    assert B_FRAMES["B_luma_444"][:3] == B_FRAMES["B_chroma_444"][:3] == G_FRAME[:3]
    ac = {s: 7 for s in AC_SYMS + [ZRL]}
    a = Case(W, H, sr, rr, frame_from_counts(W, H, sr, ac_luma=ac, ac_chroma=ac, rr=rr), LUMA)
    guard_a(a)
    zero = Case(W, H, sr, rr, np.zeros((nb + 2 * nbc, 64), np.int16), LUMA)
    cases = [count_case("B_luma_444"), count_case("B_chroma_444"), a, zero]
    for name, c in zip(("G_all_162", "G_zero"), cases[2:]):
        c.show(name)
    segs = [[(key, tuple(b), tuple(v)) for key, (b, v) in sorted(dht_tables(c.data).items())] for c in cases]
    every = [s for f in segs for s in f]
    assert len(every) == 16 and len(set(every)) < 16       # not all pairwise distinct,
    assert all(segs[i] != segs[j] for i in range(4) for j in range(i))      # but no two frames share all four
    return cases
