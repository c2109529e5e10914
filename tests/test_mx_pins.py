"""Pins on everything the host hands the three MFMA kernels (k_mxs, k_mxs422, k_mxs420): the
per-quality scale / band-limit / divisor tables, the f16 B operands, the workgroup images
(jx_mx_image: host only, no GPU) and the band self-tests' results, as SHA-256 hashes in
tests/golden/mx_plan_pins.json (tests/golden/make_mx_pins.py).  A parity test cannot see a wrong
band limit in one mode's image; a changed byte here can."""
import importlib.util
import json
import os

import pytest

import jpgx
from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_mx_pins", os.path.join(GOLDEN, "make_mx_pins.py"))
make_mx_pins = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_mx_pins)

LIBM_NOTE = ("the pinned values are float32 / f16 roundings of long-double libm results (cosl, sqrtl): "
             "on a host whose libm differs from glibc's in a last ulp such a rounding could flip; "
             "otherwise the plan, the operands or the image builder changed what a kernel receives")


@pytest.fixture(scope="module")
def pinned():
    with open(make_mx_pins.PINS) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def computed():
    return make_mx_pins.pins(jpgx.lib)


def test_split_configuration_is_the_pinned_one(pinned):
    assert jpgx.lib.jx_mx_parts() == pinned["mx_parts"]
    assert jpgx.lib.jx_mx_loexp() == pinned["mx_loexp"]


@pytest.mark.parametrize("kernel", list(make_mx_pins.KERNELS))
@pytest.mark.parametrize("what", ["tables", "operands", "image_bytes", "images", "selftest"])
def test_host_products_are_pinned(pinned, computed, kernel, what):
    assert computed[kernel][what] == pinned["kernels"][kernel][what], f"{kernel} {what}: {LIBM_NOTE}"


def test_image_hook_refuses_bad_arguments():
    import ctypes
    f = jpgx.lib.jx_mx_image
    f.restype = ctypes.c_longlong
    f.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_longlong]
    buf = ctypes.create_string_buffer(1 << 16)
    for sr in range(3):
        size = f(sr, 0, 50, buf, len(buf))
        assert size > 0 and size % 16 == 0
        assert f(sr, 0, 50, buf, size - 1) == jpgx.EARG
        assert f(sr, 0, 50, None, len(buf)) == jpgx.EARG
        assert f(sr, 2, 50, buf, len(buf)) == jpgx.EARG
        assert f(sr, 0, 0, buf, len(buf)) == jpgx.EQUALITY
        assert f(sr, 0, 98, buf, len(buf)) == jpgx.EQUALITY
    assert f(3, 0, 50, buf, len(buf)) == jpgx.ESAMPLE
    assert f(-1, 0, 50, buf, len(buf)) == jpgx.ESAMPLE
