"""k_mxs's three device operand tiles (jx_mxs_device_operands, csrc/jpgx_plan.cpp; what
MxsK::upload_operands puts into g_mxs_B) against the plan's six (jx_mx_operands, pinned by
tests/test_mx_pins.py): Y|Cb hi, Y|Cb lo, and the Cr tile Bc = [Cr hi | Cr lo].  No GPU: the hook
is host code, and the products are emulated in float32 through the B layout of
v_mfma_f32_16x16x32_f16 (lane l holds B[k = 8 (l >> 4) + e][column l & 15])."""
import ctypes

import numpy as np
import pytest

import jpgx
import san_build


@pytest.fixture(scope="module")
def plan_ops():
    ops = np.full((6, 64, 8), 0xA5A5, np.uint16)
    assert jpgx.lib.jx_mx_parts() == 2
    assert jpgx.lib.jx_mx_operands(ctypes.c_void_p(ops.ctypes.data)) == 0
    return ops


@pytest.fixture(scope="module")
def dev_ops():
    dev = np.full((3, 64, 8), 0xA5A5, np.uint16)
    assert jpgx.lib.jx_mxs_device_operands(ctypes.c_void_p(dev.ctypes.data)) == 0
    return dev


def test_ycb_tiles_are_the_plans(plan_ops, dev_ops):
    assert np.array_equal(dev_ops[0], plan_ops[0])
    assert np.array_equal(dev_ops[1], plan_ops[3])


def test_cr_tile_is_hi_left_lo_right(plan_ops, dev_ops):
    left = (np.arange(64) % 16 < 8)[:, None]
    assert np.array_equal(dev_ops[2], np.where(left, plan_ops[3 * 0 + 1], plan_ops[3 * 1 + 2]))
    # what the tile leaves out is the plan's stored zeros and the Cr matrix's second copy
    for t in (1, 4):
        assert not plan_ops[t][~left[:, 0]].any()
    for t in (2, 5):
        assert not plan_ops[t][left[:, 0]].any()
    roll = np.arange(64) // 16 * 16 + (np.arange(64) + 8) % 16           # lane with column j +- 8
    assert np.array_equal(plan_ops[2], plan_ops[1][roll]) and np.array_equal(plan_ops[5], plan_ops[4][roll])


def b_matrix(tile):
    """float32 [k = 32][column = 16] of one operand tile"""
    B = np.zeros((32, 16), np.float32)
    f = tile.view(np.float16).astype(np.float32)
    for l in range(64):
        B[8 * (l >> 4):8 * (l >> 4) + 8, l & 15] = f[l]
    return B


def a_rows(rows):
    """float32 [n][32] A operands of byte rows [n][24]: byte b is the f16 subnormal b 2^-24, k = 24
    the bias 1.0, the rest zero (jpgx_mx.hip, mx_aop)"""
    A = np.zeros((len(rows), 32), np.float32)
    A[:, :24] = rows.astype(np.uint16).view(np.float16).astype(np.float32)
    A[:, 24] = 1.0
    return A


def product(A, B):
    """float32 [n][16], every product and partial sum rounded to float32, k ascending"""
    acc = np.zeros((A.shape[0], 16), np.float32)
    for k in range(32):
        acc = (acc + (A[:, k:k + 1] * B[k:k + 1, :]).astype(np.float32)).astype(np.float32)
    return acc


def test_cr_tile_reproduces_the_six_tile_sums(plan_ops, dev_ops):
    rng = np.random.default_rng(0x4372)
    rows = np.concatenate([rng.integers(0, 256, (256, 24)).astype(np.uint8), np.zeros((1, 24), np.uint8),
                           np.full((1, 24), 255, np.uint8)])
    A = a_rows(rows)
    assert np.array_equal(A[:, :24], rows.astype(np.float32) * np.float32(2.0 ** -24))
    new = product(A, b_matrix(dev_ops[2]))
    hi0, lo0 = product(A, b_matrix(plan_ops[1])), product(A, b_matrix(plan_ops[4]))      # set 0: columns 0..7
    hi1, lo1 = product(A, b_matrix(plan_ops[2])), product(A, b_matrix(plan_ops[5]))      # set 1: columns 8..15
    assert np.array_equal(new[:, :8], hi0[:, :8]) and np.array_equal(new[:, :8], hi1[:, 8:])
    assert np.array_equal(new[:, 8:], lo0[:, :8]) and np.array_equal(new[:, 8:], lo1[:, 8:])
    assert new[:-2].any(axis=0).all()                                 # every column carries something
    # the rows R = fl(acc_h + acc_l) of both sets from the one tile, as the kernel merges them
    R = (new[:, :8] + new[:, 8:]).astype(np.float32)
    assert np.array_equal(R, (hi0 + lo0).astype(np.float32)[:, :8])
    assert np.array_equal(R, (hi1 + lo1).astype(np.float32)[:, 8:])
    # acc_h is exact in any order: the float32 sum is the float64 sum
    exact = A.astype(np.float64) @ b_matrix(dev_ops[2]).astype(np.float64)
    assert np.array_equal(new[:, :8].astype(np.float64), exact[:, :8])


@pytest.mark.skipif(not san_build.HAVE_CC, reason="needs gcc/g++ with libasan/libubsan")
def test_hook_under_asan_ubsan():
    """tests/c/mxs_operands_san.c, a program of its own, with the host layer under AddressSanitizer +
    UndefinedBehaviorSanitizer (nothing is preloaded): the hook on an exact-size heap buffer"""
    rc, out, err = san_build.run("mxs_operands_san")
    assert rc == 0 and "mxs_operands_san: clean" in out, (out[-2000:], err[-4000:])
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-4000:]
