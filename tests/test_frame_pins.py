"""Pins on what the JFIF coder, the device decoder and the pixel path answer for a grid of frame
sizes and sample ratios: their workspace sizes and the code each refuses with, recorded in
tests/golden/frame_pins.json (tests/golden/make_frame_pins.py) from the library as it was before
the three shared one frame geometry (csrc/jx_frame.h).  The three map one rule to three
conventions of refusal; a moved boundary or a swapped code shows here.  No GPU: a size query and a
refused call return before any device call."""
import importlib.util
import json
import os

import pytest

import jpgx
import jpgx.compat  # noqa: F401  (declares jpgx_pixels_host's arguments)
from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_frame_pins", os.path.join(GOLDEN, "make_frame_pins.py"))
make_frame_pins = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_frame_pins)


def test_sizes_and_refusals_are_pinned():
    with open(make_frame_pins.PINS) as f:
        pinned = json.load(f)["points"]
    computed = make_frame_pins.pins(jpgx.lib)
    assert list(computed) == list(pinned)
    # the grid has frames that all three take and frames that all three refuse
    kinds = {(bool(p["jfif"][0]), bool(p["decode"][0]), p["host"] == jpgx.EARG) for p in pinned.values()}
    assert {(True, True, True), (False, False, False)} <= kinds
    wrong = [key for key in pinned if computed[key] != pinned[key]]
    assert not wrong, [(key, computed[key], pinned[key]) for key in wrong[:8]]


def test_file_entry_point_refuses_a_side_above_65535_before_the_transform(tmp_path):
    """jpgx_encode_rgb_to_jpeg sizes its coefficients from the frame (csrc/jx_frame.h), so a side that
    SOF's 16-bit field cannot hold is refused with the coder's EARG before anything runs on a device
    and before a file is opened; the forward path's own multiples are checked first, with their codes"""
    import numpy as np
    dst = tmp_path / "wide.jpg"
    for sr, flags in ((0, 0), (1, jpgx.FLAG_SUBSAMPLE), (2, jpgx.FLAG_SUBSAMPLE)):
        with pytest.raises(jpgx.JpgxError) as e:
            jpgx.compat.encode_rgb_to_jpeg(np.zeros((16, 65552, 3), np.uint8), str(dst), 50, sr, flags)
        assert e.value.rc == jpgx.EARG and not dst.exists()
    with pytest.raises(jpgx.JpgxError) as e:
        jpgx.compat.encode_rgb_to_jpeg(np.zeros((16, 65548, 3), np.uint8), str(dst), 50)
    assert e.value.rc == jpgx.EGEOMETRY
