"""Regenerate tests/golden/mx_plan_pins.json from the built library (lib/libjpgx.so, or $JPGX_LIB).

The pins are SHA-256 hashes of everything the host hands the three MFMA kernels (k_mxs, k_mxs422,
k_mxs420), per kernel:
  tables    w | lim | q of jx_plan_tables_mx* concatenated over quality 1..97
  operands  the f16 B operands of jx_mx*_operands
  images    the workgroup images of jx_mx_image concatenated over force 0, 1 and quality 1..97
  selftest  the (return, flagged, ratio) triples of the jx_selftest_mx* calls tests/test_host.py
            makes (600 blocks, the same seeds and qualities)
tests/test_mx_pins.py recomputes them with pins() below and compares.  Regenerate only when a
change is MEANT to alter what a kernel receives, and say so in that change.

Run:  python tests/golden/make_mx_pins.py        (a few seconds)
"""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
PINS = os.path.join(HERE, "mx_plan_pins.json")

QUALITIES = range(1, 98)
# kernel -> (suffix of the entry points, operand shape per JX_MX_PARTS, selftest seed base)
KERNELS = {"k_mxs": ("mx", lambda p: (3 * p, 64, 8), 77),
           "k_mxs422": ("mx422", lambda p: (p, 4, 64, 8), 91),
           "k_mxs420": ("mx420", lambda p: (p, 5, 64, 8), 53)}
SELFTEST_BLOCKS, SELFTEST_QUALITIES = 600, (10, 50, 75, 90, 97)


def _ptr(a: np.ndarray) -> ctypes.c_void_p:
    return a.ctypes.data_as(ctypes.c_void_p)


def pins(lib: ctypes.CDLL) -> dict:
    out: dict = {}
    parts = lib.jx_mx_parts()
    lib.jx_mx_image.restype = ctypes.c_longlong
    lib.jx_mx_image.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_longlong]
    for sr, (kernel, (sfx, shape, seed0)) in enumerate(KERNELS.items()):
        ent: dict = {}
        plan = getattr(lib, f"jx_plan_tables_{sfx}")
        plan.restype = ctypes.c_int
        h = hashlib.sha256()
        w, lim = np.zeros((24, 8), np.float32), np.zeros((24, 8), np.float32)
        q = np.zeros((2, 64), np.int16)
        for quality in QUALITIES:
            assert plan(quality, _ptr(w), _ptr(lim), _ptr(q)) == 0, (kernel, quality)
            h.update(w.tobytes() + lim.tobytes() + q.tobytes())
        ent["tables"] = h.hexdigest()

        ops = np.zeros(shape(parts), np.uint16)
        f = getattr(lib, f"jx_{sfx}_operands")
        f.restype = ctypes.c_int
        assert f(_ptr(ops)) == 0, kernel
        ent["operands"] = hashlib.sha256(ops.tobytes()).hexdigest()

        buf = np.zeros(1 << 16, np.uint8)
        size = lib.jx_mx_image(sr, 0, 1, _ptr(buf), buf.size)
        assert 0 < size <= buf.size, (kernel, size)
        h = hashlib.sha256()
        for force in (0, 1):
            for quality in QUALITIES:
                assert lib.jx_mx_image(sr, force, quality, _ptr(buf), buf.size) == size
                h.update(buf[:size].tobytes())
        ent["image_bytes"] = int(size)
        ent["images"] = h.hexdigest()

        st = getattr(lib, f"jx_selftest_{sfx}")
        st.restype = ctypes.c_longlong
        st.argtypes = [ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_int,
                       ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_double)]
        ent["selftest"] = []
        for quality in SELFTEST_QUALITIES:
            flagged, ratio = ctypes.c_longlong(), ctypes.c_double()
            rc = st(SELFTEST_BLOCKS, seed0 + quality, quality, ctypes.byref(flagged), ctypes.byref(ratio))
            ent["selftest"].append([int(rc), int(flagged.value), float(ratio.value).hex()])
        out[kernel] = ent
    return out


def main() -> None:
    sys.path.insert(0, os.path.join(REPO, "jpeg-encoder-and-decoder_amd"))
    import jpgx
    g = {"generator": "tests/golden/make_mx_pins.py", "mx_parts": jpgx.lib.jx_mx_parts(),
         "mx_loexp": jpgx.lib.jx_mx_loexp(), "kernels": pins(jpgx.lib)}
    with open(PINS, "w") as f:
        json.dump(g, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
