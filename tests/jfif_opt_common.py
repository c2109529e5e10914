"""Test helper shared by tests/test_jfif_opt.py, tests/test_jfif_tables.py and
tests/test_jfif_tables_gpu.py: T.81 Annex K.2 restated from the standard (annex_k2),
the symbol counts of a frame by the walk of tests/jfif_bits.py, the DHT segments of a file, and the
two ways to a file: the host writer on one thread (_host) and the device coder (_device, _raw)."""
import numpy as np

import jpgx
import jpgx.compat as C
from jfif_bits import category, walk


# ---- T.81 Annex K.2, restated -------------------------------------------------------------------
def annex_k2(counts):
    """(bits[16], vals, depth of the unlimited tree) for 256 symbol counts: Figures K.1 - K.4 with
    the reserved point 256 of frequency 1; of equal frequencies the largest index is taken."""
    freq = [int(c) for c in counts] + [1]
    codesize, others = [0] * 257, [-1] * 257

    def least(skip):
        best = -1
        for i in range(257):
            if freq[i] and i != skip and (best < 0 or freq[i] <= freq[best]):
                best = i
        return best

    while True:
        v1 = least(-1)
        v2 = least(v1)
        if v2 < 0:
            break
        freq[v1] += freq[v2]
        freq[v2] = 0
        while True:
            codesize[v1] += 1
            if others[v1] < 0:
                break
            v1 = others[v1]
        others[v1] = v2
        while True:
            codesize[v2] += 1
            if others[v2] < 0:
                break
            v2 = others[v2]
    depth = max(codesize)
    bits = [0] * (max(depth, 16) + 1)
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    i = depth
    while i > 16:
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        i -= 1
    i = 16
    while i > 0 and bits[i] == 0:
        i -= 1
    if i:
        bits[i] -= 1
    vals = [s for _, s in sorted((codesize[s], s) for s in range(256) if codesize[s])]
    return bits[1:17], vals, depth


def fib_vector(n):
    """1, 2, 3, 5, 8, ...: n distinct counts, each the sum of the two before it"""
    v = [1, 2]
    while len(v) < n:
        v.append(v[-1] + v[-2])
    return v[:n]


def _check_table(counts, bits, vals):
    assert len(bits) == 16 and sum(bits) == len(vals)              # no length above 16
    assert sum(b << (16 - l) for l, b in enumerate(bits, 1)) <= (1 << 16) - 1   # Kraft, all ones free
    assert sorted(vals) == [s for s in range(256) if counts[s]]


def _host(coef, W, H, q, sr, rr, optimize=True, nthreads=1):
    """the oracle: the host writer (the device's restart_rows -1 is one MCU row per interval)"""
    return C.write_jfif_ex(coef, W, H, q, sr, restart_rows=1 if rr == -1 else rr, nthreads=nthreads,
                           optimize=optimize)


def symbol_counts(coef, W, H, sr, rr):
    """[4][256]: DC luma, AC luma, DC chroma, AC chroma symbols of the scan, in MCU order with the
    predictors reset at every interval of rr MCU rows (0: never) and the writer's clamps; the walk is
    tests/jfif_bits.py's"""
    cnt = np.zeros((4, 256), np.uint64)

    def visit(iv, comp, row, step, diff, acs):
        t = 0 if comp == 0 else 2
        cnt[t, category(diff)] += 1
        for sym, _ in acs:
            cnt[t + 1, sym] += 1

    walk(coef, W, H, sr, rr, visit)
    return cnt


def segments(data):
    """[(marker, payload)] of the segments before the scan"""
    assert data[:2] == b"\xff\xd8"
    at, out = 2, []
    while True:
        assert data[at] == 0xff
        m, n = data[at + 1], data[at + 2] << 8 | data[at + 3]
        out.append((m, data[at + 4:at + 2 + n]))
        at += 2 + n
        if m == 0xda:
            return out, at


def dht_tables(data):
    """{class << 4 | id: (bits, vals)} and the segments' bytes in file order"""
    tabs, order = {}, []
    for m, p in segments(data)[0]:
        if m == 0xc4:
            bits = list(p[1:17])
            assert len(p) == 17 + sum(bits)                    # one table per segment
            tabs[p[0]] = (bits, list(p[17:]))
            order.append(p[0])
    assert order == [0x00, 0x10, 0x01, 0x11]
    return tabs


def _dht_bytes(data):
    return b"".join(bytes([m]) + p for m, p in segments(data)[0] if m == 0xc4)


def _flat(planes):
    return np.concatenate([np.asarray(x).reshape(-1, 64) for x in planes])


def _device(cuda, coef, W, H, q, sr, rr, cap=None, optimize=True):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(coef, np.int16)).to(cuda).reshape(1, -1)
    out, lens = jpgx.jfif_gpu(d, W, H, q, sr, rr, cap=cap, optimize=optimize)
    n = int(lens[0])
    assert 0 < n <= out.shape[1]
    return out[0, :n].cpu().numpy().tobytes()


def _raw(d_coef, fstride, nf, W, H, q, sr, rr, flags, out, ostride, cap, lens, ws=None):
    """jpgx_jfif_gpu_ex itself on torch tensors (a workspace of the size the library asks for)"""
    import torch
    need = jpgx.lib.jpgx_jfif_gpu_workspace_size_ex(W, H, sr, rr, nf, cap, flags)
    assert need > 0
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=out.device)
    assert ws.numel() >= need
    rc = jpgx.lib.jpgx_jfif_gpu_ex(d_coef.data_ptr(), fstride, nf, W, H, q, sr, rr, flags, out.data_ptr(), ostride,
                                   cap, lens.data_ptr(), ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    return rc


