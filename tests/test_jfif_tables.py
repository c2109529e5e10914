"""The per-image Huffman table builder held to T.81 Annex K.2 by symbol counts, on the CPU: the cases
of tests/jfif_count_cases.py (frames made from prescribed counts), their guards, and the host writer
on them.  tests/test_jfif_tables_gpu.py puts the same guarded cases in front of the device's
k_jf_count and k_jf_tables, whose oracle the host writer is; here the host writer
itself is held to the restatement (annex_k2), applied to counts the independent walk of
tests/jfif_bits.py finds, and its files are decoded back by two decoders."""
import io

import numpy as np
import pytest

import jfif_count_cases as K
import jpgx.compat as C
from jfif_bits import coded_values
from jfif_decode import decode
from jfif_opt_common import _check_table, _flat, annex_k2, dht_tables

KEYS = (0x00, 0x10, 0x01, 0x11)                            # symbol_counts' four tables as DHT class << 4 | id


def _check_case(c):
    tabs = dht_tables(c.data)
    for k, key in enumerate(KEYS):
        bits, vals, _ = annex_k2(c.cnt[k])
        assert tabs[key] == (bits, vals), hex(key)
        _check_table(c.cnt[k], *tabs[key])
    want = coded_values(c.coef, c.W, c.H, c.sr, c.rr)
    assert np.array_equal(want, c.coef)                    # no clamp acted: the counts are the frame's
    dec = decode(c.data)
    assert (dec["width"], dec["height"]) == (c.W, c.H)
    assert np.array_equal(_flat(dec["coef"]), want)
    assert np.array_equal(_flat(C.read_jfif(c.data)["coef"]), c.coef)


@pytest.mark.parametrize("name", sorted(K.COUNT_CASES))
def test_case_is_guarded_and_the_host_file_is_the_restatement_s(name):
    _check_case(K.count_case(name))                        # built, its figures printed, guarded


@pytest.mark.parametrize("name", sorted(K.COUNT_CASES))
def test_host_file_opens_in_pil(name):
    Image = pytest.importorskip("PIL.Image")
    c = K.count_case(name)
    im = Image.open(io.BytesIO(c.data))
    im.load()
    assert im.size == (c.W, c.H)


def test_batch_frames_are_guarded():
    """case G: the deep table as luma AC, as chroma AC, all 162 symbols in both AC tables, all zero"""
    cases = K.batch_cases()
    for c in cases[2:]:
        _check_case(c)
    assert [c.k2[K.LUMA]["depth"] > 16 for c in cases] == [True, False, False, False]
    assert [c.k2[K.CHROMA]["depth"] > 16 for c in cases] == [False, True, False, False]


def test_intervals_move_no_ac_symbol():
    """case H: one frame coded with 1, 2 and all its MCU rows per interval has the same AC tables"""
    cases = [K.count_case(n) for n in ("B_luma_444", "H_rr1", "H_one_interval")]
    assert all(np.array_equal(c.coef, cases[0].coef) for c in cases)
    assert sorted(c.data.count(b"\xff\xd0") > 0 for c in cases) == [False, True, True]
    for c in cases[1:]:
        for t in (K.LUMA, K.CHROMA):
            assert np.array_equal(c.cnt[t], cases[0].cnt[t])
        for key in (0x10, 0x11):
            assert dht_tables(c.data)[key] == dht_tables(cases[0].data)[key]


def test_packer_refuses_what_it_cannot_place():
    """the synthesiser's own refusals: a ZRL with nothing behind it, tokens beyond the frame, a
    block that cannot end at position 63"""
    for ac in ({K.ZRL: 1}, {0xf1: 5 * 4}, {0x11: 31, K.EOB: 0}):
        with pytest.raises(AssertionError):
            K.frame_from_counts(8, 8, 0, ac_luma=ac)
    with pytest.raises(AssertionError):
        K.frame_from_counts(8, 8, 0, dc_luma={3: 2})
