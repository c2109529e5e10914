"""The device's Huffman table builder (k_jf_count and k_jf_tables, csrc/jpgx_jfif.hip)
held to T.81 Annex K.2 by symbol counts.  It is the one piece of the device JFIF coder that shares no
source with the host: a restatement of jx_jfif_optimal on one wave.  The inputs are the guarded cases
of tests/jfif_count_cases.py, each built for one place where that restatement can go wrong
(tests/test_jfif_tables.py runs the same guards, and holds the host writer to them, without a GPU).

Two oracles, so that a misreading of K.2 that host and device share cannot hide: the device's bytes
== the host writer's on one thread, and the DHT segments cut from the device's file == annex_k2
applied to the counts of the independent walk.  Then the device decoder, with both scan kernels, reads
the device coder's own file back.  No tolerances."""
import numpy as np
import pytest

import jfif_count_cases as K
import jpgx
import jpgx.compat as C
from any_cases import patch_size
from jfif_opt_common import _flat, _raw, annex_k2, dht_tables

gpu = pytest.mark.gpu
OPT = jpgx.JFIF_OPTIMIZE
KEYS = (0x00, 0x10, 0x01, 0x11)
SENTINEL = 0xA5


def _dev(cuda, a):
    import torch
    return torch.from_numpy(np.array(a)).to(cuda)           # a copy: the cases' arrays are read-only


def _code(cuda, c, W=None, H=None, any_size=False):
    out, lens = jpgx.jfif_gpu(_dev(cuda, c.coef).reshape(1, -1), W or c.W, H or c.H, K.Q, c.sr, c.rr, optimize=True,
                              any_size=any_size)
    n = int(lens[0])
    assert 0 < n <= out.shape[1]
    return out, lens, out[0, :n].cpu().numpy().tobytes()


def _check_tables(got, c):
    tabs = dht_tables(got)
    for k, key in enumerate(KEYS):
        assert tabs[key] == annex_k2(c.cnt[k])[:2], hex(key)


@gpu
@pytest.mark.parametrize("name", sorted(K.COUNT_CASES))
def test_device_file_is_the_host_writer_s_and_its_tables_the_restatement_s(cuda, name):
    c = K.count_case(name)                                  # guarded
    _, _, got = _code(cuda, c)
    _check_tables(got, c)
    assert got == c.data


@gpu
@pytest.mark.parametrize("subinterval", [False, True], ids=["lanes", "subinterval"])
@pytest.mark.parametrize("name", sorted(K.COUNT_CASES))
def test_device_decoder_reads_the_device_coder_s_file(cuda, name, subinterval):
    """the files of case B put 151 codes of 16 bits in front of the device decoder's table build"""
    c = K.count_case(name)
    out, lens, _ = _code(cuda, c)
    coef, qt, status = jpgx.jfif_decode_gpu(out, lens, c.W, c.H, c.sr, subinterval=subinterval)
    assert status.cpu().tolist() == [0]
    want = C.read_jfif(c.data)
    assert np.array_equal(_flat(want["coef"]), c.coef)
    assert np.array_equal(coef[0].cpu().numpy(), c.coef)
    assert np.array_equal(qt[0].cpu().numpy(), want["qt"])


@gpu
@pytest.mark.parametrize("name", K.WIDE)
def test_wide_cases_through_the_any_size_entry(cuda, name):
    """the frame stated a few pixels smaller: the same scan under another SOF"""
    c = K.count_case(name)
    W, H = c.W - 3, c.H - 5
    assert jpgx.coded_size(W, H, c.sr) == (c.W, c.H)
    _, _, got = _code(cuda, c, W, H, any_size=True)
    _check_tables(got, c)
    assert got == patch_size(c.data, W, H)
    assert got == C.write_jfif_ex(c.coef, W, H, K.Q, c.sr, restart_rows=c.rr, nthreads=1, optimize=True, any_size=True)


@gpu
def test_batch_of_four_frames_in_one_uncleared_workspace(cuda):
    """case G: the deep table is luma AC in one frame and chroma AC in the next, beside all 162 symbols
    and the all-zero frame; padded strides, sentinels, a workspace that never held zeros, used twice
    with the frames in other slots"""
    import torch
    cases = K.batch_cases()                                 # guarded
    W, H, sr, rr = K.G_FRAME
    per = cases[0].coef.size
    fstride = per + 5 * 64
    cap = max(len(c.data) for c in cases) + 7
    ostride = (cap + 15) // 16 * 16 + 48
    need = jpgx.lib.jpgx_jfif_gpu_workspace_size_ex(W, H, sr, rr, 4, cap, OPT)
    ws = torch.full((need,), 0xEE, dtype=torch.uint8, device=cuda)
    for order in ((0, 1, 2, 3), (3, 2, 0, 1)):
        d = torch.full((4, fstride), 32767, dtype=torch.int16, device=cuda)
        for slot, k in enumerate(order):
            d[slot, :per] = _dev(cuda, cases[k].coef.reshape(-1))
        out = torch.full((4, ostride), SENTINEL, dtype=torch.uint8, device=cuda)
        lens = torch.zeros(4, dtype=torch.int64, device=cuda)
        assert _raw(d, fstride, 4, W, H, K.Q, sr, rr, OPT, out, ostride, cap, lens, ws=ws) == 0
        got, n = out.cpu().numpy(), lens.cpu().numpy()
        for slot, k in enumerate(order):
            assert n[slot] == len(cases[k].data), (order, slot)
            data = got[slot, :n[slot]].tobytes()
            _check_tables(data, cases[k])
            assert data == cases[k].data, (order, slot)
            assert (got[slot, n[slot]:] == SENTINEL).all()


@gpu
def test_intervals_move_no_ac_table(cuda):
    """case H: 44 workgroups' atomic adds, 22, and one workgroup whose lanes loop over 5,808 blocks
    build the same two AC tables"""
    files = []
    for name in ("B_luma_444", "H_rr1", "H_one_interval"):
        c = K.count_case(name)
        _, _, got = _code(cuda, c)
        assert got == c.data
        files.append(dht_tables(got))
    for f in files[1:]:
        assert f[0x10] == files[0][0x10] and f[0x11] == files[0][0x11]
