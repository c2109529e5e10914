"""tests/jfif_bits.py, the per-block bit counts restated from T.81 F.1.2, held to the host writer's
files; and the guards of the inputs of tests/test_jfif_gpu_passes.py, which that file asserts again
before it calls the device (no GPU here)."""
import numpy as np
import pytest

import jfif_bits as B
import jpgx.compat as C
from jfif_decode import decode
from jfif_inputs import CASES, hand_made, lap, scan_rows, stuffing_heavy, zeros

MODES = pytest.mark.parametrize("optimize", [False, True], ids=["std", "opt"])


def _flat(planes):
    return np.concatenate([np.asarray(x).reshape(-1, 64) for x in planes])


def test_one_all_zero_mcu_by_hand():
    """standard tables: luma DC category 0 is 00 and EOB 1010, chroma 00 and 00 -- 6 + 4 + 4 bits,
    then two 1-bits of padding: 0010 1000 0000 0011"""
    coef = zeros(8, 8, 0)
    data = B.host(coef, 8, 8, 0, 1, False)
    assert B.interval_bits(coef, 8, 8, 0, 1, data) == [[6, 4, 4]]
    assert B.file_intervals(data) == [b"\x28\x03"]
    assert B.offsets([6, 4, 4]) == [0, 6, 10, 14] and B.unstuffed_len([6, 4, 4]) == 2 and B.pad_bits([6, 4, 4]) == 2
    assert B.pad_bits([8, 8]) == 0 and B.unstuffed_len([8, 8]) == 2


def test_one_coded_block_by_hand():
    """luma DC 3 (category 2: 011, then 11), AC 1 = -2 (0/2: 01, then 01), AC 18 = 1 after 16 zeros (ZRL
    11111111001, 0/1: 00, then 1), EOB 1010: 5 + 4 + 14 + 4 = 27 bits"""
    coef = zeros(8, 8, 0)
    coef[0, 0], coef[0, 1], coef[0, 18] = 3, -2, 1
    data = B.host(coef, 8, 8, 0, 1, False)
    assert B.interval_bits(coef, 8, 8, 0, 1, data) == [[27, 4, 4]]
    bits = "011" "11" "01" "01" "11111111001" "00" "1" "1010" + "00" "00" + "00" "00" + "11111"
    assert B.file_intervals(data) == [int(bits, 2).to_bytes(5, "big")]


def test_scan_order():
    assert [r for r, _ in scan_rows(32, 16, 2)] == [0, 1, 4, 5, 8, 10, 2, 3, 6, 7, 9, 11]
    assert [c for _, c in scan_rows(32, 8, 1)] == [0, 0, 1, 2, 0, 0, 1, 2]
    assert scan_rows(16, 16, 0) == [(0, 0), (4, 1), (8, 2), (1, 0), (5, 1), (9, 2), (2, 0), (6, 1), (10, 2), (3, 0),
                                    (7, 1), (11, 2)]


@MODES
@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_of_the_shared_cases(name, optimize):
    """ceil(bits / 8) is every interval's unstuffed length, and the pad is (8 - bits % 8) % 8 one-bits"""
    W, H, q, sr, rr, seed = CASES[name]
    coef = lap(W, H, sr, seed)
    bits, streams = B.check_against_file(coef, W, H, sr, rr, B.host(coef, W, H, sr, rr, optimize, q))
    assert sum(len(b) for b in bits) == coef.shape[0]


@MODES
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_bits_of_the_hand_made_and_stuffing_heavy_frames(sr, optimize):
    W, H, coef = hand_made(sr)
    for rr in (1, 2):
        B.check_against_file(coef, W, H, sr, rr, B.host(coef, W, H, sr, rr, optimize))
    W, H, q, coef = stuffing_heavy(sr)
    _, streams = B.check_against_file(coef, W, H, sr, 1, B.host(coef, W, H, sr, 1, optimize))
    assert sum(s.count(b"\xff") for s in streams) >= 1000


@MODES
@pytest.mark.parametrize("name", sorted(B.PASS_CASES))
def test_guard(name, optimize):
    """the new inputs: the helper held to the file (Case), and the input's own guard.  The walk over
    the 68,112 blocks of the largest takes seconds: that one is held to the helper once, with the
    standard tables"""
    c = B.pass_case(name, optimize)
    if name.startswith("both") and not optimize:
        B.check_against_file(c.coef, c.W, c.H, c.sr, c.rr, c.data)


def test_the_plain_all_zero_frame_is_the_same_word_case():
    """standard tables: blocks 254..257 of the all-zero 4:4:4 frame share word 37, the seam at bit 1,196;
    per-image tables: every block is 2 bits and block 256 starts word 16"""
    c = B.pass_case("seam_same_word", False)
    assert not c.coef.any() and B.offsets(c.bits[0])[254:259] == [1186, 1190, 1196, 1200, 1204]
    c = B.pass_case("seam_aligned", True)
    assert not c.coef.any() and B.offsets(c.bits[0])[256] == 512
    assert B.offsets(B.pass_case("seam_aligned", False).bits[0])[256] == 1196 + 20 + 64


@MODES
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_decoded_values_of_clamped_input(sr, optimize):
    """coded_values is what the independent decoder and the host reader give back"""
    for name in ("seam_hand_made", "seam_stuffing"):
        c = B.pass_case(f"{name}_{('444', '422', '420')[sr]}", optimize)
        want = B.coded_values(c.coef, c.W, c.H, c.sr, c.rr)
        assert not np.array_equal(want, c.coef)              # the clamps show
        assert np.array_equal(_flat(decode(c.data)["coef"]), want)
        assert np.array_equal(_flat(C.read_jfif(c.data)["coef"]).astype(np.int32), want)


@MODES
@pytest.mark.parametrize("name", ["tall_stuffing_8x2064", "lap_64x48_rr1"])
def test_late_overflow_guard(name, optimize):
    c = B.pass_case(name, optimize)
    B.guard_late_overflow(c, len(c.data) - 1)
    with pytest.raises(AssertionError):                      # the capacities of the older overflow tests: refused early
        B.guard_late_overflow(c, B.file_header(c.data)[1] + 16)
