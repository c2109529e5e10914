"""The host JFIF writer's bytes, pinned.

The host writer and the device coder share the block walk, the clamps and the scan order
(csrc/jx_jfif_enc.h), so "device == host" cannot catch an error in those; nor can the decoders,
since a clamped value does not come back.  PINNED holds the SHA-256 of what the writer of commit
6f7195d -- the last with a walk of its own in host/jpgx_jfif.c -- wrote for the inputs that
exercise every rule of the walk: the shared routines must write the very same bytes."""
import hashlib

import pytest

import jpgx.compat as C
from jfif_inputs import hand_made, stuffing_guard, stuffing_heavy

# (input, sample_ratio, restart_rows, optimize) -> SHA-256 of write_jfif_ex(..., nthreads=1)
PINNED = {
    ("hand_made", 0, 1, False): "2166b008556dbc6073e1e65b79a2b08b7fd3a627ac9d1c648cd190141c67c73f",
    ("hand_made", 0, 1, True): "d82de1c1f5a9e4f68ff7c160c5e03447ce7f5f16d2f0247c4894986ade802c5a",
    ("hand_made", 0, 2, False): "5bd39fc0fa7474be28797a7f7a0abc4a4a452f7398c5a410bf1b95de25153214",
    ("hand_made", 0, 2, True): "b7e34051a509e45d0ea6e7db9c44bfcd04de8e6b79c23481734b201f3e6543c0",
    ("hand_made", 1, 1, False): "d0b52fb8bd0f05be8b31cc44ef988890a2e143071448afc1387f41febad3627d",
    ("hand_made", 1, 1, True): "ed13ddb20aa89fc3f7b4eb0a68070fda8ae01bbb2b96583bb8f8c09846f62c80",
    ("hand_made", 1, 2, False): "6950e6d24eaaa37152e36be57536416178b0becd107dc1b6ce58e85d40b86ea8",
    ("hand_made", 1, 2, True): "e6dd9d838fe3f4277c8763f02ad5f60e17f4d77a3335da8f9f3ad0e5cc0995e6",
    ("hand_made", 2, 1, False): "e038f603dc74297f95ec7229144c19d13a86bb4f710a45338228484411b56276",
    ("hand_made", 2, 1, True): "de5233ad99f7efd726d3e53f406ecc1a868cec611b3f6b812cf8155df28f9459",
    ("hand_made", 2, 2, False): "f2f7f9c1ced992fed5018cca6d52f9ef2bab23cd66ce84e434be3fac8eefecc6",
    ("hand_made", 2, 2, True): "f3225498f589e07de24f1237bcae663c788753479972c191dabcafeecb47a15b",
    ("stuffing", 0, 1, False): "70fc7c23322010f87c435959a7a6a0ef80b4482b308a5d98111acc44000b42f2",
    ("stuffing", 0, 1, True): "fff791e14adfd40ab7bcc8a46a99b38c085cf73346ed7563e3a8a65136286c8a",
    ("stuffing", 2, 1, False): "e95a0ea46f064aff48b096534f81ef705ea5800d6eaba0d9df0ec968868a51cf",
    ("stuffing", 2, 1, True): "005960ab62bddf5bf326dffd92a165b1fbbb7f138b469d81fdab2a8b192d9860",
}


def _input(kind, sr):
    if kind == "hand_made":
        W, H, coef = hand_made(sr)
        return W, H, 50, coef
    return stuffing_heavy(sr)


@pytest.mark.parametrize("key", sorted(PINNED))
def test_bytes_equal_the_separate_writer(key):
    kind, sr, rr, opt = key
    W, H, q, coef = _input(kind, sr)
    data = C.write_jfif_ex(coef, W, H, q, sr, restart_rows=rr, nthreads=1, optimize=opt)
    if kind == "stuffing":
        pairs, endings = stuffing_guard(data)
        assert pairs >= 1000 and endings >= 1          # a different numpy must not empty the case
    assert hashlib.sha256(data).hexdigest() == PINNED[key]
