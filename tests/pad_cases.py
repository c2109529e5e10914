"""Test helper shared by tests/test_pad_rule.py and tests/test_pad_rule_gpu.py: the
sweep of source layouts that k_pad_edge's chunk rule (csrc/jx_pad.h) is held to, on the host twin with
every load checked (csrc/jpgx_pad_host.cpp, jpgx.compat.pad_host) and on the device, and the guards
that say which of the rule's paths a sweep reached.

A case is (W, H, slack): a batch of NFRAMES frames of W x H pixels in one buffer, rows 3 W + slack bytes
apart, frames a stride apart that is 1 (mod 4), so that the four frames begin on the four residues of an
address modulo 4, and with them, row by row, sh, the residue of a row's start.  Frame 0 begins with the
buffer, (W + H) % 4 bytes past a multiple of 16, and the buffer ends with the last frame's last pixel: a
load in front of the first row or behind the last one is a load outside the buffer.  Pixels are noise of
one seed, every other byte noise of another."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np

import encode_any_cases as E
import jpgx.compat as C
import san_build
from conftest import PKG, REPO

# every width up to three chunks of a row; 681 .. 696: coded widths 688 and 696 in 4:4:4, 688 and 704 in
# 4:2:x -- 258, 261 and 264 chunks of a row pair, a second workgroup of k_pad_edge with (cw / 8 odd) and
# without a chunk that straddles the pair's two rows
WIDTHS = tuple(range(1, 49)) + tuple(range(681, 697))
HEIGHTS = (1, 2, 7, 8, 9)
SLACKS = (0, 1, 2, 3)                   # in_pitch - 3 W
SAMPLINGS = (0, 1, 2)
NFRAMES = 4
FAST, FIRST, SHORT, FIFTH, STRADDLE, HIGH, EXACT, OVER = (slice(0, 4), 4, 5, 6, 7, 8, slice(9, 13), slice(13, 17))


def sweep(widths=WIDTHS, heights=HEIGHTS, slacks=SLACKS):
    return [(W, H, s) for W in widths for H in heights for s in slacks]


def layout(W, H, slack):
    """(in_pitch, frame stride, buffer length)"""
    pitch = 3 * W + slack
    extent = pitch * (H - 1) + 3 * W
    fstride = extent + (1 - extent) % 4
    return pitch, fstride, (NFRAMES - 1) * fstride + extent


@functools.lru_cache(maxsize=8)
def batch(W, H, slack):
    """(buf uint8 [len], (W + H) % 4 bytes past a multiple of 16 and read-only; images: NFRAMES read-only
    views (H, W, 3) of it; pixel: bool [len], the bytes that are pixels)"""
    pitch, fstride, n = layout(W, H, slack)
    raw = np.zeros(n + 20, np.uint8)
    at = -raw.ctypes.data % 16 + (W + H) % 4
    buf = raw[at:at + n]
    key = (W * 131 + H) * 4 + slack
    buf[:] = np.random.default_rng(2000003 + key).integers(0, 256, n, dtype=np.uint8)
    pixel = np.zeros(n, bool)
    rows = np.lib.stride_tricks.as_strided(pixel, (NFRAMES, H, 3 * W), (fstride, pitch, 1))
    rows[:] = True
    buf[pixel] = np.random.default_rng(1000003 + key).integers(0, 256, int(pixel.sum()), dtype=np.uint8)
    buf.setflags(write=False)
    images = [np.lib.stride_tricks.as_strided(buf[f * fstride:], (H, W, 3), (pitch, 3, 1), writeable=False)
              for f in range(NFRAMES)]
    assert buf.ctypes.data % 16 == (W + H) % 4 and {(f * fstride) % 4 for f in range(NFRAMES)} == {0, 1, 2, 3}
    return buf, images, pixel


def want(images, sr):
    """the coded frames by numpy's edge rule: uint8 [NFRAMES][ch][cw][3]"""
    return np.stack([E.pad_edge(im, sr) for im in images])


def twin(W, H, slack, sr, trace=True, library=None):
    """the host twin over a case's batch: (bad, coded, touched, stats)"""
    buf, _, _ = batch(W, H, slack)
    pitch, fstride, _ = layout(W, H, slack)
    return C.pad_host(buf, 0, W, H, pitch, fstride, NFRAMES, *E.coded(W, H, sr), trace=trace, library=library)


class Reached:
    """what a sweep reached, summed from the twin's counters call by call"""

    def __init__(self):
        self.total = np.zeros(C.PAD_STATS, np.uint64)
        self.high_with_straddle = self.high_without_straddle = 0
        self.calls = 0

    def add(self, stats):
        self.total += stats
        self.calls += 1
        self.high_with_straddle += bool(stats[HIGH] and stats[STRADDLE])
        self.high_without_straddle += bool(stats[HIGH] and not stats[STRADDLE])

    def check(self, straddle=True):
        """a sweep that no longer reaches one of the rule's paths fails here, not silently.  straddle: whether
        the sweep has coded widths with cw / 8 odd -- 4:4:4 only: 4:2:x codes multiples of 16"""
        t = self.total
        assert self.calls > 0
        assert (t[FAST] > 0).all(), t[FAST]                                # the funnel ran at every sh
        assert t[FIRST] and t[SHORT] and t[FIFTH], t[4:8]                  # every reason for the byte path
        assert self.high_without_straddle                                  # a second workgroup's chunks
        assert bool(t[STRADDLE]) == bool(self.high_with_straddle) == straddle, (t[STRADDLE], self.high_with_straddle)
        # the fifth dword's bound from both sides: the last chunk it lets through, the first it does not
        assert (t[EXACT][1:] > 0).all() and (t[OVER][1:] > 0).all(), (t[EXACT], t[OVER])


# the rule's line in csrc/jx_pad.h and two ways of getting it wrong that no output byte shows: the fifth
# dword supplies sh bytes only, the dword in front of a row none
RULE = "fast = k.whole && k.xb >= sh && (sh == 0u || k.xb - sh + 20u <= w3);"
WRONG_RULES = {"+ 16 for + 20": RULE.replace("+ 20u", "+ 16u"), "xb >= sh dropped": RULE.replace(" && k.xb >= sh", "")}


def wrong_twin(tmpdir, rule):
    """the host twin built from a copy of csrc/jx_pad.h whose rule is `rule`: a library of its own"""
    csrc = os.path.join(PKG, "csrc")
    text = open(os.path.join(csrc, "jx_pad.h")).read()
    assert text.count(RULE) == 1 and rule != RULE
    with open(os.path.join(tmpdir, "jx_pad.h"), "w") as f:
        f.write(text.replace(RULE, rule))
    shutil.copy(os.path.join(csrc, "jpgx_pad_host.cpp"), tmpdir)
    so = os.path.join(tmpdir, "libpadwrong.so")
    b = subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-I" + csrc, "-I" + os.path.join(REPO, "include"),
                        os.path.join(tmpdir, "jpgx_pad_host.cpp"), "-o", so], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    return ctypes.CDLL(so)


def run_san():
    """tests/c/pad_rule_san.c with the twin and host/jpgx_pad.c under the sanitizers; (returncode, stdout,
    stderr)"""
    return san_build.run("pad_rule_san", [os.path.join(PKG, "csrc", "jpgx_pad_host.cpp"),
                                          os.path.join(PKG, "host", "jpgx_pad.c")], timeout=900)
