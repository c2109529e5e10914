#!/usr/bin/env python3
"""Writes tests/golden/gray_fixtures/: the one-component (grayscale) baseline JPEG files of the grayscale
tests (tests/gray_cases.py lists them by the same rules).  Needs Pillow; the inputs are deterministic,
so a run with the same Pillow and libjpeg writes the same bytes.  The files are committed: the GPU
tests must not need Pillow where they run.

Per size four files:
  0  smooth, q 50, one block row per restart interval
  1  noise,  q 90, no DRI
  2  noise,  q 50, per-image Huffman tables, a restart interval of 2 blocks (at 21 x 13 the intervals
     straddle block rows; at 263 x 21 there are 50 of them, so RSTn wraps six times)
  3  smooth, q 90, a restart interval of 1 block (99 intervals at 263 x 21)
One 263 x 200 noise file without DRI (a scan of about 41 KB: the sub-interval kernel's 8 KiB tile is
crossed five times), and file 2 of 21 x 13 with SOF's sampling byte patched to 0x22, 0x12 and 0x41."""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "gray_fixtures")
SIZES = ((1, 1), (7, 9), (8, 8), (12, 30), (21, 13), (35, 18), (64, 8), (65, 17), (129, 65), (263, 21),
         (18, 10), (30, 22))
WRITERS = (("smooth", 50, dict(restart_marker_rows=1)), ("noise", 90, dict()),
           ("noise", 50, dict(optimize=True, restart_marker_blocks=2)), ("smooth", 90, dict(restart_marker_blocks=1)))
BIG = (263, 200)
PATCHED = (0x22, 0x12, 0x41)


def image(kind, W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "smooth":
        return ((2 * xx + 3 * yy + xx * yy // 16) % 256).astype(np.uint8)
    return np.random.default_rng(1000 * W + H).integers(0, 256, (H, W), dtype=np.uint8)


def encode(kind, W, H, q, **kw):
    b = io.BytesIO()
    Image.fromarray(image(kind, W, H), "L").save(b, "JPEG", quality=q, **kw)
    return b.getvalue()


def patch_sampling(data, byte):
    """the file with the sampling byte of SOF's one component replaced"""
    b = bytearray(data)
    i = 2
    while b[i + 1] not in (0xC0, 0xC1):
        i += 2 + (b[i + 2] << 8 | b[i + 3])
    assert b[i + 9] == 1 and b[i + 11] == 0x11
    b[i + 11] = byte
    return bytes(b)


def main():
    os.makedirs(OUT, exist_ok=True)
    total = 0
    files = {}
    for W, H in SIZES:
        for k, (kind, q, kw) in enumerate(WRITERS):
            files["g_%dx%d_%d.jpg" % (W, H, k)] = encode(kind, W, H, q, **kw)
    files["g_%dx%d_noise.jpg" % BIG] = encode("noise", BIG[0], BIG[1], 90)
    for s in PATCHED:
        files["g_21x13_2_s%02x.jpg" % s] = patch_sampling(files["g_21x13_2.jpg"], s)
    for name, data in sorted(files.items()):
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(data)
        total += len(data)
    print("%d files, %d bytes" % (len(files), total))
    return 0


if __name__ == "__main__":
    sys.exit(main())
