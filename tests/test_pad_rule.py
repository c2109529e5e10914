"""k_pad_edge's chunk rule (csrc/jx_pad.h) on the host: the text the kernel runs, chunk by
chunk over the sweep of tests/pad_cases.py with every load checked against the buffer and recorded
(csrc/jpgx_pad_host.cpp).  A fifth dword that supplies sh bytes only, or a dword in front of a row, read
outside the row changes no output byte, on the device or here: only the trace shows it.  The guards say
which of the rule's paths the sweep reached; two deliberately wrong rules show that the trace, and no
output comparison, catches them.  Every comparison is ==."""
import numpy as np
import pytest

import jpgx
import pad_cases as P


def _held(W, H, slack, sr, reached):
    buf, images, pixel = P.batch(W, H, slack)
    bad, coded, touched, stats = P.twin(W, H, slack, sr)
    what = (W, H, slack, sr)
    assert bad == 0, what
    assert not touched[~pixel].any(), what                     # nothing outside [0, 3 W) of rows 0 .. H - 1
    assert touched[pixel].all(), what                          # and every pixel byte is read
    assert np.array_equal(coded, P.want(images, sr)), what
    for f, im in enumerate(images):
        assert np.array_equal(coded[f], jpgx.pad_edge(im, sr)), what + (f,)        # host/jpgx_pad.c
    plain = P.twin(W, H, slack, sr, trace=False)
    assert plain[0] == 0 and np.array_equal(plain[1], coded) and np.array_equal(plain[3], stats), what
    reached.add(stats)
    return stats


@pytest.mark.parametrize("sr", P.SAMPLINGS)
def test_the_rule_stays_inside_the_rows(sr):
    reached = P.Reached()
    for W, H, slack in P.sweep():
        _held(W, H, slack, sr, reached)
    reached.check(straddle=sr == 0)
    t = reached.total
    print("sr %d: calls %d fast %s slow %s high %d exact %s over %s" % (
        sr, reached.calls, t[P.FAST].tolist(), t[4:8].tolist(), int(t[P.HIGH]), t[P.EXACT].tolist(), t[P.OVER].tolist()))
    # the counters are the grid's: every chunk of every row pair of every frame is one of them
    chunks = sum(P.NFRAMES * (P.E.coded(W, H, sr)[1] // 2) * (3 * P.E.coded(W, H, sr)[0] // 8) for W, H, _ in P.sweep())
    assert int(t[0:8].sum()) == chunks


def test_the_sweep_is_the_one_the_guards_were_written_for():
    s = P.sweep()
    assert len(s) == 64 * 5 * 4 and len(set(s)) == len(s)
    assert {W for W, _, _ in s} == set(range(1, 49)) | set(range(681, 697))
    assert {P.E.coded(W, 8, 0)[0] for W in range(681, 697)} == {688, 696}
    assert {P.E.coded(W, 8, 1)[0] for W in range(681, 697)} == {688, 704}
    # 3 cw / 8 chunks of a row pair: a second workgroup from cw = 688, none in 1 .. 48
    assert 3 * 688 // 8 == 258 and all(3 * P.E.coded(W, 8, 2)[0] // 8 <= 256 for W in range(1, 49))


def test_a_thinned_sweep_fails_a_guard():
    """the guards are no formality: without the wide frames, or with one width, they do not hold"""
    def reached(cases, srs=P.SAMPLINGS):
        r = P.Reached()
        for W, H, slack in cases:
            for sr in srs:
                r.add(P.twin(W, H, slack, sr)[3])
        return r
    with pytest.raises(AssertionError):
        reached(P.sweep(widths=range(1, 49), heights=(8,))).check()             # no second workgroup
    with pytest.raises(AssertionError):
        reached(P.sweep(widths=(688,), heights=(8,), slacks=(0,)), (0,)).check()  # cw / 8 even: no straddling chunk
    with pytest.raises(AssertionError):
        P.Reached().check()


@pytest.mark.skipif(not P.san_build.HAVE_CC, reason="needs g++")
@pytest.mark.parametrize("name", sorted(P.WRONG_RULES))
def test_a_rule_that_reads_past_a_row_shows_in_the_trace_only(tmp_path, name):
    """the case that only the twin can see: the wrong rule's frames are the right ones, byte for byte"""
    L = P.wrong_twin(str(tmp_path), P.WRONG_RULES[name])
    refused = outside = 0
    for W, H, slack in P.sweep(heights=(2, 9)):
        _, images, pixel = P.batch(W, H, slack)
        bad, coded, touched, _ = P.twin(W, H, slack, 0, library=L)
        assert np.array_equal(coded, P.want(images, 0)), (W, H, slack)
        refused += bad
        outside += int(touched[~pixel].any())
    print("%s: refused loads %d, cases with a byte read outside the rows %d" % (name, refused, outside))
    assert refused > 0 and outside > 0


def test_argument_checks():
    buf = np.zeros(64, np.uint8)
    for bad in (dict(width=0), dict(height=0), dict(nframes=0), dict(coded_width=9), dict(coded_height=4),
                dict(coded_width=0), dict(in_pitch=8)):
        a = dict(width=3, height=5, in_pitch=9, in_frame_stride=45, nframes=1, coded_width=8, coded_height=8)
        a.update(bad)
        with pytest.raises(jpgx.JpgxError):
            P.C.pad_host(buf, 0, **a)
    with pytest.raises(ValueError):
        P.C.pad_host(buf.reshape(8, 8), 0, 3, 5, 9, 45, 1, 8, 8)


@pytest.mark.skipif(not P.san_build.HAVE_CC, reason="needs gcc and g++")
def test_the_twin_under_the_sanitizers():
    rc, out, err = P.run_san()
    assert rc == 0 and "pad_rule_san: clean" in out, (out[-2000:], err[-4000:])
    print(out)
    assert "cases %d " % (len(P.sweep()) * len(P.SAMPLINGS)) in out
