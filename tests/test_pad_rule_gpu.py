"""k_pad_edge (csrc/jpgx_pad.hip) on the device over the sweep of tests/pad_cases.py, the one
its host twin is held to with every load checked (tests/test_pad_rule.py): every width 1 .. 48 and
681 .. 696 (a second workgroup per row pair, with and without a chunk that straddles the pair's rows),
rows 3 W + 0 .. 3 bytes apart, four frames per launch on the four residues of an address modulo 4.  The
frames are read from jpgx_blocks_gpu_any's workspace, as tests/test_encode_any_gpu.py reads them, and are
== numpy's edge rule and == the twin's bytes; the source stays as it was and nothing is written behind
the workspace.  What the device cannot show, a load outside a row that supplies no byte, is the twin's
part."""
import ctypes

import numpy as np
import pytest

import encode_any_cases as E
import jpgx
import pad_cases as P

gpu = pytest.mark.gpu
SUB = jpgx.FLAG_SUBSAMPLE
FILL, WFILL, CFILL = 0x7A, 0xEE, 0x5A5A
Q = 90


@gpu
@pytest.mark.parametrize("which", ["product", "alt"])
@pytest.mark.parametrize("sr", P.SAMPLINGS)
def test_the_sweep_on_the_device(cuda, which, sr):
    import torch
    L = jpgx.lib if which == "product" else jpgx.alt_library()
    flags = SUB if sr else 0
    cases = P.sweep()
    nf = P.NFRAMES
    cw, ch = E.coded(max(P.WIDTHS), max(P.HEIGHTS), sr)
    src_all = torch.empty(16 + max(P.layout(W, H, s)[2] for W, H, s in cases) + 16, dtype=torch.uint8, device=cuda)
    ws_all = torch.empty(nf * ch * 3 * cw + 16 + 256, dtype=torch.uint8, device=cuda)
    out_all = torch.empty(nf * (3 * (cw // 8) * (ch // 8) + 3) * 64, dtype=torch.int16, device=cuda)
    reached = P.Reached()
    widest = max(cases)
    for W, H, slack in cases:
        buf, images, _ = P.batch(W, H, slack)
        pitch, fstride, n = P.layout(W, H, slack)
        cw, ch = E.coded(W, H, sr)
        per = ((cw // 8) * (ch // 8) + 2 * jpgx.chroma_blocks(cw, 0, ch // 8, sr, flags)) * 64
        what = (W, H, slack)
        # the source: the case's buffer on its own residue modulo 16, sentinels in front of it and behind
        at = buf.ctypes.data % 16
        host = np.full(at + n + 16, FILL, np.uint8)
        host[at:at + n] = buf
        d_src = src_all[:len(host)]
        d_src.copy_(torch.from_numpy(host))
        assert d_src.data_ptr() % 16 == 0
        fr = jpgx.Frames()
        fr.width, fr.height, fr.row_begin, fr.row_end, fr.nframes = W, H, 0, ch // 8, nf
        fr.in_pitch, fr.in_frame_stride, fr.out_frame_stride = pitch, fstride, per + 3 * 64
        p = jpgx.default_params(W, H, Q, sr, flags=flags)
        need = L.jpgx_workspace_size_any(ctypes.byref(fr), ctypes.byref(p))
        assert need == (nf * ch * 3 * cw + 15) // 16 * 16, what
        ws = ws_all[:need + 256].fill_(WFILL)                                       # scribbled before the call
        out = out_all[:nf * (per + 3 * 64)].fill_(CFILL).view(nf, per + 3 * 64)
        rc = L.jpgx_blocks_gpu_any(ctypes.byref(fr), ctypes.byref(p), d_src.data_ptr() + at, out.data_ptr(),
                                   ws.data_ptr(), need, None)
        assert rc == 0, (rc, what)
        wsh = ws.cpu().numpy()
        assert np.array_equal(d_src.cpu().numpy(), host), what                     # the source is only read
        assert (wsh[need:] == WFILL).all(), what                                   # nothing behind the workspace
        coded = wsh[:nf * ch * 3 * cw].reshape(nf, ch, cw, 3)
        assert np.array_equal(coded, P.want(images, sr)), what                     # k_pad_edge's frames
        bad, twin, _, stats = P.twin(W, H, slack, sr, trace=False)
        assert bad == 0 and np.array_equal(coded, twin), what
        reached.add(stats)
        if (W, H, slack) == widest:                                                 # the frames are what is coded
            got = out.cpu().numpy()
            assert (got[:, per:] == CFILL).all()
            for f, im in enumerate(images):
                padded = torch.from_numpy(E.pad_edge(im, sr)).to(cuda)
                want = jpgx.encode_blocks(padded, Q, sr, flags=flags)
                assert np.array_equal(got[f, :per], want.cpu().numpy().reshape(-1)), (what, f)
    reached.check(straddle=sr == 0)
    assert reached.calls == len(cases) and widest == (696, 9, 3)
