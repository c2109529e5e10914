"""Time the device JFIF coder (jpgx_jfif_gpu) on the hot path's own output and write
profiles/jfif_gpu.json: 8 x 4K frames, q90, 4:4:4, one MCU row per restart interval, coefficients
from the transform kernel, for two inputs -- the flagship's splitmix noise (every coefficient
nonzero: the coder's worst case) and a photo-like frame (flat 8 x 8 tiles plus +-6 of noise).
Per input:
  coder_us        jpgx_jfif_gpu per batch, HIP events around 10 calls, 5 rounds after 0.5 s of
                  settling (all rounds listed, sorted)
  bytes           what the algorithm needs (coefficients once + files once) and what this design
                  moves (coefficients twice, offsets written and read, the unstuffed stream written
                  and read twice, files once), each over the minimum time
  host_route_s    the route to the same bytes without the device coder: the coefficients copied to
                  the host (into pinned memory: the best case) + jpgx_write_jfif_ex, restart_rows 1,
                  16 threads, frame after frame; best of 2
  speedup         host_route_s / coder time
  xform_us, xform_plus_coder_us   the transform alone and transform + coder per batch (events)
  bytes_equal     every frame's device bytes == the host writer's
With --optimize the run compares the coder with per-image Huffman tables (JPGX_JFIF_OPTIMIZE,
jpgx_jfif_gpu_ex) against the standard one, in the same session and on the same coefficients, and
writes profiles/jfif_gpu_opt.json; per input:
  coder_us, coder_opt_us, opt_over_std      the two coders' times per batch (as above) and the medians' ratio
  file_bytes_per_frame, file_bytes_per_frame_opt, opt_bytes_over_std
  xform_plus_coder_us, xform_plus_coder_opt_us
  bytes_equal     every frame's optimised device bytes == jpgx_write_jfif_opt on 16 host threads
  host_route_s    D2H copy + jpgx_write_jfif_opt, frame after frame; best of 2
With --decode the run times the way back (jpgx_jfif_decode_gpu) on the files the
coder writes from the same coefficients and writes profiles/jfif_gpu_dec.json; per input:
  decode_us       jpgx_jfif_decode_gpu per batch (events, as above; all rounds, sorted)
  host_route_s    the route without it: the files copied to pinned host memory + jpgx_read_jfif on 16
                  threads, frame after frame; best of 2 (host_route_d2h_s: the copy alone)
  device_over_host   decode time (median) / host_route_s: above 1, the host route is the faster one
  intervals       restart intervals of the batch = the lanes that work
  coefficients_equal   every frame's status 0 and its coefficients == the ones that were coded
With --decode --subinterval the run times the decoder that works inside a restart interval
(JPGX_JFIF_DECODE_SUBINTERVAL, jpgx_jfif_decode_gpu_ex) against flags 0 in the same
process on the same files and writes profiles/jfif_gpu_dec_sub.json; per input:
  decode_us, decode_sub_us    flags 0 and the flag per batch (events, as above; all rounds, sorted)
  sub_slowest_over_plain_fastest   below 1: the flag's slowest round beats the fastest of flags 0
  coder_us, sub_over_coder    the coder's time for the same files and the flag's median over it
  host_route_s, plain_over_host, sub_over_host   the host route as above
  coefficients_equal          statuses 0 and coefficients == the coded ones, both ways, before and after
and once, for the photo-like input: "no_dri", its first frame recoded without restart intervals by
the host writer, decoded both ways (1 call per round, 3 rounds: flags 0 is one lane's work).
With --pixels the run times the pixel half of the way back (jpgx_pixels_gpu) on the
transform's own coefficients with jpgx_jfif_qt's tables and writes profiles/jfif_gpu_px.json; per
input and sample mode (4:4:4, and true 4:2:2 / 4:2:0 from JPGX_FLAG_SUBSAMPLE):
  pixels_us       jpgx_pixels_gpu per batch (events, as above; all rounds, sorted); for 4:2:x both launches
  bytes_per_px, fraction_of_8TBps   9 / 7 / 6 B per pixel (int16 coefficients in, RGB out) over the
                  minimum time, as a fraction of 8 TB/s
  xform_us, xform_fraction_of_8TBps   the forward transform kernel (k_mxs for 4:4:4) on the same box,
                  same protocol, same bytes per pixel in the other direction
  host_route_s    the route without it: the coefficients copied to pinned host memory +
                  jpgx_pixels_host on 16 threads, frame after frame; best of 2 (host_route_d2h_s: the copy)
  pixels_equal    every frame == jpgx_pixels_host, before and after the timed calls
With --pixels --any-size the run times the entry points for files of any size (jpgx_pixels_gpu_any,
jpgx_jfif_decode_gpu_any) beside the plain ones and writes profiles/jfif_gpu_px_any.json; per input and
sample mode, the calls taken in turn, several passes, in one process:
  plain_us        (a) jpgx_pixels_gpu at 3840 x 2160, this library; parent_plain_us: the same call on the
                  library named by --parent-lib=PATH (a build of the parent commit), when given
  any_full_us     (b) jpgx_pixels_gpu_any at 3840 x 2160; any_full_over_plain: the medians' ratio
  any_odd_us      (c) jpgx_pixels_gpu_any at 3839 x 2159 on the same coefficients (the coded frame is the
                  same); any_odd_over_plain
  pixels_equal    (b) == (a) on every frame; (c) == jpgx_pixels_host_any on two frames, and no byte outside
                  [0, 3 * 3839) x [0, 2159) written
and once, for the photo-like input, "decoder_3839x2159": its frames cropped, written by Pillow with one MCU
row per restart interval (4:4:4 and 4:2:0) and decoded by jpgx_jfif_decode_gpu_any with both scan kernels
(decode_us, decode_sub_us; statuses 0, both equal, frame 0 == jpgx_read_jfif_any).
With --gray the run times the one-component (grayscale) entry points (jpgx_jfif_decode_gpu_gray,
jpgx_pixels_gpu_gray) on 8 grayscale files of 3840 x 2160 at q 90 and writes
profiles/jfif_gpu_gray.json.  The inputs are made on the host (noise, and flat 8 x 8 tiles plus +-6 of noise) and
the files written by Pillow -- or read from --gray-files=DIR, which a run with Pillow fills when it is given and
empty.  Per input, "with_dri" (one block row per restart interval) and "no_dri":
  decode_us, decode_sub_us    jpgx_jfif_decode_gpu_gray with flags 0 and JPGX_JFIF_DECODE_SUBINTERVAL per batch
                  (events, as above; without DRI 1 call per round, 3 rounds: flags 0 is one lane's work per file)
  coefficients_equal          statuses 0, both ways equal, frame 0 == jpgx_read_jfif_gray
and per input:
  px1_us, px3_us  k_px_gray with 1 and 3 channels per batch; px1_fraction_of_8TBps at 3 B per pixel (2 read,
                  1 written), px3_fraction_of_8TBps at 5
  px444_us, px444_fraction_of_8TBps   k_px444 (jpgx_pixels_gpu, 4:4:4) at 9 B per pixel in the same session, on
                  the forward transform's coefficients of the same image as R = G = B
  host_route_s    the files copied to pinned host memory + jpgx_read_jfif_gray + jpgx_pixels_host_gray (1 channel)
                  on 16 threads, frame after frame; best of 2
  pixels_equal    both channel counts == jpgx_pixels_host_gray on two frames, before and after the timed calls
With --encode-any the run times the encode side's entry points for images of any size (jpgx_blocks_gpu_any with
k_pad_edge, jpgx_jfif_gpu_any) on 8 frames of 3839 x 2159 -- the inputs' top left, rows 11517 bytes
apart -- beside the plain ones on 3840 x 2160 and writes profiles/jfif_gpu_enc_any.json; per input, the four calls
taken in turn, several passes, in one process:
  plain_xform_us, any_xform_us    jpgx_blocks_gpu at 3840 x 2160 and jpgx_blocks_gpu_any at 3839 x 2159 per batch
                  (events around 10 calls; all passes, sorted); any_xform_over_plain: the medians' ratio
  plain_coder_us, any_coder_us, any_coder_over_plain   jpgx_jfif_gpu_ex and jpgx_jfif_gpu_any the same way
  any_route_over_plain            (any_xform + any_coder) / (plain_xform + plain_coder), medians
  pad_us_by_difference, pad_fraction_of_8TBps_by_difference   any_xform - plain_xform (medians): k_pad_edge and the
                  gap between the two launches, and 6 B per pixel of the coded frames (3 read, 3 written) over it
  pad_kernel_us, pad_fraction_of_8TBps   k_pad_edge's own time, the average of a kernel trace taken in a run of its
                  own and named by --kernel-stats=FILE.csv (rocprofv3 --kernel-trace --stats); absent without one
  bytes_equal     every frame's coefficients == jpgx_blocks_gpu's for the image padded by torch's replicate rule,
                  and frame 0's file == jpgx_write_jfif_any's on the host; repeat_equal: the same after the timed calls
With --encode-gray the run times the encode side of the one-component family (jpgx_blocks_gpu_gray = k_gray,
jpgx_jfif_gpu_gray) on 8 one-channel frames of 3840 x 2160 and of 3839 x 2159 (the inputs' top left,
rows 3839 bytes apart) at q 90 and writes profiles/jfif_gpu_enc_gray.json.  The inputs are --gray's (noise, and flat
8 x 8 tiles plus +-6 of noise).  Per input:
  gray_xform_us, rgb_xform_us     jpgx_blocks_gpu_gray on the 3840 x 2160 frames and jpgx_blocks_gpu on the same frames
                  as R = G = B, taken in turn, several passes, in one process (events around 10 calls; all passes,
                  sorted); gray_over_rgb: the medians' ratio, which must be below 1 (the gate; exit status 1 otherwise)
  gray_fraction_of_8TBps          3 B per pixel (1 read, 2 written) over gray_xform_us's minimum
  flagged_share   {quality: flagged coefficients / coefficients} at q 50, 90, 97: k_gray's fp32 sequence and band on
                  the host (jx_selftest_gray_blocks) over the first 20,000 blocks of frame 0; blocks_with_a_flag likewise
and per size ("3840x2160", "3839x2159"):
  xform_us        jpgx_blocks_gpu_gray per batch (events, as above; all rounds, sorted); fraction_of_8TBps
  coder_us, coder_opt_us          jpgx_jfif_gpu_gray per batch, standard and JPGX_JFIF_OPTIMIZE, one block row per interval
  host_route_s    the coefficients copied to pinned host memory + jpgx_write_jfif_gray, restart_rows 1, 16 threads,
                  frame after frame; best of 2
  bytes_equal     frame 0's coefficients == k_gray's restatement on the host (jx_gray_host_blocks), and frame 0's
                  files, standard and optimised, == jpgx_write_jfif_gray's; repeat_equal: the same after the timed calls
With --pixels --scale the run times the decode at 1/2, 1/4 and 1/8 of the size (jpgx_pixels_gpu_scaled,
jpgx_pixels_gpu_gray_scaled) beside the full-size call on the same coefficient batches: the
three sample modes and one-component frames with 1 and 3 channels, the calls taken in turn, the
full-size call timed before and after the scaled ones.  Per scale: the rounds, the fraction of 8 TB/s
at the algorithmic bytes (the coefficient array read + the pixels written), the ratio to the full-size
call's median and whether the scaled median is no longer than the full-size call's slowest round (the
bar; reported, the exit status is the pixel checks').  Frames 0 and 7 of every scaled call are compared
with the host twin.  Written to profiles/jfif_gpu_px_scaled.json.

Usage (GPU box): python tools/jfif_gpu_bench.py [--optimize | --decode [--subinterval] | --pixels [--scale | --any-size
[--parent-lib=PATH]] | --gray [--gray-files=DIR] | --encode-any [--kernel-stats=FILE.csv] | --encode-gray] [OUT.json]"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "jpeg-encoder-and-decoder_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import jpgx  # noqa: E402
import jpgx.compat as C  # noqa: E402

W, H, F, Q = 3840, 2160, 8, 90
HOST_THREADS = 16


def timed(fn, calls=10, rounds=5, settle=0.5):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < settle:
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / calls)
    return sorted(ts)


def measure(name, d_rgb, dev):
    nb = (W // 8) * (H // 8)
    per = 3 * nb * 64
    coef = torch.empty((F, per), dtype=torch.int16, device=dev)
    fr = jpgx.frames(W, H, nframes=F, out_frame_stride=per)
    p = jpgx.default_params(W, H, Q, 0)
    xws = torch.empty(max(jpgx.workspace_size(fr), 1), dtype=torch.uint8, device=dev)

    def xform():
        jpgx.blocks_gpu(fr, p, d_rgb, coef, xws)

    xform()
    torch.cuda.synchronize()
    # the capacity: ask with a small one, take what the library reports
    _, lens = jpgx.jfif_gpu(coef, W, H, Q, 0, 1, cap=1 << 20)
    cap = (int(lens.max()) + 4095) // 4096 * 4096
    out = torch.empty((F, cap), dtype=torch.uint8, device=dev)
    lens = torch.empty(F, dtype=torch.int64, device=dev)
    wsb = int(jpgx.lib.jpgx_jfif_gpu_workspace_size(W, H, 0, 1, F, cap))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def coder():
        rc = jpgx.lib.jpgx_jfif_gpu(coef.data_ptr(), per, F, W, H, Q, 0, 1, out.data_ptr(), cap, cap,
                                    lens.data_ptr(), ws.data_ptr(), wsb, stream)
        assert rc == 0, rc

    def both():
        xform()
        coder()

    coder()
    torch.cuda.synchronize()
    n = lens.cpu().numpy()
    assert (n > 0).all(), n
    first = [out[f, :n[f]].cpu().numpy().tobytes() for f in range(F)]
    t_coder = timed(coder)
    t_xform = timed(xform)
    t_both = timed(both)
    repeat_equal = all(out[f, :n[f]].cpu().numpy().tobytes() == first[f] for f in range(F))

    # the host route
    pinned = torch.empty((F, per), dtype=torch.int16).pin_memory()
    host_s, d2h_s, files = [], [], None
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(coef)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        hc = pinned.numpy()
        files = [C.write_jfif_ex(hc[f].reshape(-1, 64), W, H, Q, 0, restart_rows=1, nthreads=HOST_THREADS,
                                 cap=cap) for f in range(F)]
        t2 = time.perf_counter()
        d2h_s.append(t1 - t0)
        host_s.append(t2 - t0)
    equal = all(files[f] == first[f] for f in range(F))

    file_bytes = int(n.sum())
    unstuffed = file_bytes                       # within a per cent: stuffing and markers
    alg = F * per * 2 + file_bytes
    moved = 2 * F * per * 2 + 2 * 4 * F * 3 * nb + 3 * unstuffed + file_bytes
    tmin = t_coder[0]
    return {
        "input": name, "file_bytes_per_frame": [int(x) for x in n],
        "coder_us": t_coder, "xform_us": t_xform, "xform_plus_coder_us": t_both,
        "coder_over_xform": t_coder[2] / t_xform[2],
        "bytes": {"algorithmic": alg, "moved_by_design": moved,
                  "algorithmic_GBps": alg / tmin / 1e3, "moved_GBps": moved / tmin / 1e3},
        "gpx_per_s": F * W * H / tmin / 1e3,
        "host_route_s": min(host_s), "host_route_d2h_s": min(d2h_s), "host_threads": HOST_THREADS,
        "speedup": min(host_s) / (t_coder[2] * 1e-6),
        "bytes_equal": bool(equal), "repeat_equal": bool(repeat_equal),
    }


def measure_opt(name, d_rgb, dev):
    nb = (W // 8) * (H // 8)
    per = 3 * nb * 64
    coef = torch.empty((F, per), dtype=torch.int16, device=dev)
    fr = jpgx.frames(W, H, nframes=F, out_frame_stride=per)
    p = jpgx.default_params(W, H, Q, 0)
    xws = torch.empty(max(jpgx.workspace_size(fr), 1), dtype=torch.uint8, device=dev)

    def xform():
        jpgx.blocks_gpu(fr, p, d_rgb, coef, xws)

    xform()
    torch.cuda.synchronize()
    _, lens = jpgx.jfif_gpu(coef, W, H, Q, 0, 1, cap=1 << 20)      # the standard file is the longer one
    cap = (int(lens.max()) + 4095) // 4096 * 4096
    out = torch.empty((F, cap), dtype=torch.uint8, device=dev)
    lens = torch.empty(F, dtype=torch.int64, device=dev)
    wsb = int(jpgx.lib.jpgx_jfif_gpu_workspace_size_ex(W, H, 0, 1, F, cap, jpgx.JFIF_OPTIMIZE))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def coder(flags):
        def run():
            rc = jpgx.lib.jpgx_jfif_gpu_ex(coef.data_ptr(), per, F, W, H, Q, 0, 1, flags, out.data_ptr(), cap, cap,
                                           lens.data_ptr(), ws.data_ptr(), wsb, stream)
            assert rc == 0, rc
        return run

    def both(flags):
        run = coder(flags)

        def go():
            xform()
            run()
        return go

    res = {"input": name}
    files = {}
    for key, flags in (("", 0), ("_opt", jpgx.JFIF_OPTIMIZE)):
        coder(flags)()
        torch.cuda.synchronize()
        n = lens.cpu().numpy()
        assert (n > 0).all(), n
        files[key] = [out[f, :n[f]].cpu().numpy().tobytes() for f in range(F)]
        res["file_bytes_per_frame" + key] = [int(x) for x in n]
        res["coder%s_us" % key] = timed(coder(flags))
        res["xform_plus_coder%s_us" % key] = timed(both(flags))
        res["repeat_equal" + key] = all(out[f, :n[f]].cpu().numpy().tobytes() == files[key][f] for f in range(F))
    res["xform_us"] = timed(xform)
    res["opt_over_std"] = res["coder_opt_us"][2] / res["coder_us"][2]
    res["opt_bytes_over_std"] = sum(res["file_bytes_per_frame_opt"]) / sum(res["file_bytes_per_frame"])

    pinned = torch.empty((F, per), dtype=torch.int16).pin_memory()
    host_s, host = [], None
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(coef)
        torch.cuda.synchronize()
        hc = pinned.numpy()
        host = [C.write_jfif_ex(hc[f].reshape(-1, 64), W, H, Q, 0, restart_rows=1, nthreads=HOST_THREADS,
                                cap=cap, optimize=True) for f in range(F)]
        host_s.append(time.perf_counter() - t0)
    res["host_route_s"] = min(host_s)
    res["host_threads"] = HOST_THREADS
    res["speedup"] = min(host_s) / (res["coder_opt_us"][2] * 1e-6)
    res["bytes_equal"] = all(host[f] == files["_opt"][f] for f in range(F))
    res["repeat_equal"] = bool(res.pop("repeat_equal") and res.pop("repeat_equal_opt"))
    return res


def measure_dec(name, d_rgb, dev):
    nb = (W // 8) * (H // 8)
    per = 3 * nb * 64
    coef = torch.empty((F, per), dtype=torch.int16, device=dev)
    fr = jpgx.frames(W, H, nframes=F, out_frame_stride=per)
    p = jpgx.default_params(W, H, Q, 0)
    xws = torch.empty(max(jpgx.workspace_size(fr), 1), dtype=torch.uint8, device=dev)
    jpgx.blocks_gpu(fr, p, d_rgb, coef, xws)
    torch.cuda.synchronize()
    _, lens = jpgx.jfif_gpu(coef, W, H, Q, 0, 1, cap=1 << 20)
    cap = (int(lens.max()) + 4095) // 4096 * 4096
    files, lens = jpgx.jfif_gpu(coef, W, H, Q, 0, 1, cap=cap)
    n = lens.cpu().numpy()
    assert (n > 0).all(), n
    back = torch.empty((F, per), dtype=torch.int16, device=dev)
    qt = torch.empty((F, 2, 64), dtype=torch.uint16, device=dev)
    status = torch.empty(F, dtype=torch.int32, device=dev)
    wsb = int(jpgx.lib.jpgx_jfif_decode_gpu_workspace_size(W, H, 0, F, cap))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def dec():
        rc = jpgx.lib.jpgx_jfif_decode_gpu(files.data_ptr(), cap, lens.data_ptr(), F, W, H, 0, back.data_ptr(), per,
                                           qt.data_ptr(), status.data_ptr(), ws.data_ptr(), wsb, stream)
        assert rc == 0, rc

    back.fill_(0x5A5A)
    dec()
    torch.cuda.synchronize()
    equal = bool((status == 0).all()) and bool(torch.equal(back, coef))
    t_dec = timed(dec)
    equal = equal and bool((status == 0).all()) and bool(torch.equal(back, coef))

    pinned = torch.empty((F, cap), dtype=torch.uint8).pin_memory()
    host_s, d2h_s, host_equal = [], [], True
    hc = coef.cpu().numpy()
    got = [np.empty(per, np.int16) for _ in range(F)]
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(files)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for f in range(F):                           # the library itself on the pinned bytes: no copy in between
            rc = jpgx.lib.jpgx_read_jfif(pinned.data_ptr() + f * cap, int(n[f]), HOST_THREADS, got[f].ctypes.data,
                                         per, None, None)
            assert rc == 0, rc
        t2 = time.perf_counter()
        d2h_s.append(t1 - t0)
        host_s.append(t2 - t0)
        host_equal = host_equal and all(np.array_equal(got[f], hc[f]) for f in range(F))
    return {
        "input": name, "file_bytes_per_frame": [int(x) for x in n], "intervals": F * (H // 8),
        "decode_us": t_dec, "gpx_per_s": F * W * H / t_dec[0] / 1e3,
        "host_route_s": min(host_s), "host_route_d2h_s": min(d2h_s), "host_threads": HOST_THREADS,
        "device_over_host": t_dec[2] * 1e-6 / min(host_s),
        "coefficients_equal": bool(equal), "host_coefficients_equal": bool(host_equal),
        "bytes_equal": bool(equal and host_equal), "repeat_equal": bool(equal),
    }


def measure_dec_sub(name, d_rgb, dev):
    nb = (W // 8) * (H // 8)
    per = 3 * nb * 64
    SUB = jpgx.JFIF_DECODE_SUBINTERVAL
    coef = torch.empty((F, per), dtype=torch.int16, device=dev)
    fr = jpgx.frames(W, H, nframes=F, out_frame_stride=per)
    p = jpgx.default_params(W, H, Q, 0)
    xws = torch.empty(max(jpgx.workspace_size(fr), 1), dtype=torch.uint8, device=dev)
    jpgx.blocks_gpu(fr, p, d_rgb, coef, xws)
    torch.cuda.synchronize()
    _, lens = jpgx.jfif_gpu(coef, W, H, Q, 0, 1, cap=1 << 20)
    cap = (int(lens.max()) + 4095) // 4096 * 4096
    files = torch.empty((F, cap), dtype=torch.uint8, device=dev)
    lens = torch.empty(F, dtype=torch.int64, device=dev)
    cwsb = int(jpgx.lib.jpgx_jfif_gpu_workspace_size(W, H, 0, 1, F, cap))
    cws = torch.empty(cwsb, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def coder():
        rc = jpgx.lib.jpgx_jfif_gpu(coef.data_ptr(), per, F, W, H, Q, 0, 1, files.data_ptr(), cap, cap,
                                    lens.data_ptr(), cws.data_ptr(), cwsb, stream)
        assert rc == 0, rc

    coder()
    torch.cuda.synchronize()
    n = lens.cpu().numpy()
    assert (n > 0).all(), n
    t_coder = timed(coder)

    def decoder(d_files, stride, d_lens, nf, flags):
        back = torch.empty((nf, per), dtype=torch.int16, device=dev)
        qt = torch.empty((nf, 2, 64), dtype=torch.uint16, device=dev)
        status = torch.empty(nf, dtype=torch.int32, device=dev)
        wsb = int(jpgx.lib.jpgx_jfif_decode_gpu_workspace_size_ex(W, H, 0, nf, stride, flags))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

        def dec():
            rc = jpgx.lib.jpgx_jfif_decode_gpu_ex(d_files.data_ptr(), stride, d_lens.data_ptr(), nf, W, H, 0, flags,
                                                  back.data_ptr(), per, qt.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                                  wsb, stream)
            assert rc == 0, rc

        def equal():
            return bool((status == 0).all()) and bool(torch.equal(back, coef[:nf]))
        return dec, equal, back

    res = {"input": name, "file_bytes_per_frame": [int(x) for x in n], "intervals": F * (H // 8),
           "sub_shape": list(jpgx.jfif_decode_sub_shape()), "coder_us": t_coder}
    ok = True
    for key, flags in (("decode_us", 0), ("decode_sub_us", SUB)):
        dec, equal, back = decoder(files, cap, lens, F, flags)
        back.fill_(0x5A5A)
        dec()
        torch.cuda.synchronize()
        ok = ok and equal()
        res[key] = timed(dec)
        ok = ok and equal()
        del back
    res["sub_slowest_over_plain_fastest"] = res["decode_sub_us"][-1] / res["decode_us"][0]
    res["sub_over_plain"] = res["decode_sub_us"][2] / res["decode_us"][2]
    res["sub_over_coder"] = res["decode_sub_us"][2] / t_coder[2]
    res["gpx_per_s_sub"] = F * W * H / res["decode_sub_us"][0] / 1e3

    pinned = torch.empty((F, cap), dtype=torch.uint8).pin_memory()
    host_s, host_equal = [], True
    hc = coef.cpu().numpy()
    got = [np.empty(per, np.int16) for _ in range(F)]
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(files)
        torch.cuda.synchronize()
        for f in range(F):
            rc = jpgx.lib.jpgx_read_jfif(pinned.data_ptr() + f * cap, int(n[f]), HOST_THREADS, got[f].ctypes.data,
                                         per, None, None)
            assert rc == 0, rc
        host_s.append(time.perf_counter() - t0)
        host_equal = host_equal and all(np.array_equal(got[f], hc[f]) for f in range(F))
    res.update(host_route_s=min(host_s), host_threads=HOST_THREADS,
               plain_over_host=res["decode_us"][2] * 1e-6 / min(host_s),
               sub_over_host=res["decode_sub_us"][2] * 1e-6 / min(host_s))

    if name.startswith("flat"):
        one = C.write_jfif(hc[0].reshape(3, nb, 64), W, H, Q)
        assert C.jfif_info(one)["restart_interval"] == 0
        d_one = torch.from_numpy(np.frombuffer(one, np.uint8).copy()).to(dev).reshape(1, -1)
        d_len = torch.tensor([len(one)], dtype=torch.int64, device=dev)
        no_dri = {"file_bytes": len(one)}
        for key, flags in (("decode_us", 0), ("decode_sub_us", SUB)):
            dec, equal, back = decoder(d_one, len(one), d_len, 1, flags)
            back.fill_(0x5A5A)
            dec()
            torch.cuda.synchronize()
            ok = ok and equal()
            no_dri[key] = timed(dec, calls=1, rounds=3, settle=0.0)
            ok = ok and equal()
            del back
        no_dri["sub_over_plain"] = no_dri["decode_sub_us"][1] / no_dri["decode_us"][1]
        res["no_dri"] = no_dri
    res.update(coefficients_equal=bool(ok), host_coefficients_equal=bool(host_equal),
               bytes_equal=bool(ok and host_equal), repeat_equal=bool(ok))
    return res


def measure_px(name, d_rgb, dev):
    nb = (W // 8) * (H // 8)
    qt_host = jpgx.jfif_qt(Q)
    d_qt = torch.from_numpy(qt_host.view(np.int16)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    res = {"input": name, "modes": []}
    for sr in (0, 1, 2):
        flags = jpgx.FLAG_SUBSAMPLE if sr else 0
        nbc = jpgx.chroma_blocks(W, 0, H // 8, sr, flags)
        per = (nb + 2 * nbc) * 64
        coef = torch.empty((F, per), dtype=torch.int16, device=dev)
        fr = jpgx.frames(W, H, nframes=F, out_frame_stride=per)
        p = jpgx.default_params(W, H, Q, sr, flags=flags)
        xws = torch.empty(max(jpgx.workspace_size(fr), 1), dtype=torch.uint8, device=dev)

        def xform():
            jpgx.blocks_gpu(fr, p, d_rgb, coef, xws)

        xform()
        torch.cuda.synchronize()
        rgb = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
        wsb = int(jpgx.lib.jpgx_pixels_gpu_workspace_size(W, H, sr, F))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)

        def pixels():
            rc = jpgx.lib.jpgx_pixels_gpu(coef.data_ptr(), per, F, W, H, sr, d_qt.data_ptr(), 0, None, rgb.data_ptr(),
                                          3 * W, 3 * W * H, ws.data_ptr() if wsb else None, wsb, stream)
            assert rc == 0, rc

        # the host route, which is also the check
        pinned = torch.empty((F, per), dtype=torch.int16).pin_memory()
        want = np.empty((F, H, W, 3), np.uint8)
        host_s, d2h_s = [], []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pinned.copy_(coef)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for f in range(F):                           # the library itself on the pinned coefficients
                rc = jpgx.lib.jpgx_pixels_host(pinned.data_ptr() + f * per * 2, W, H, sr, qt_host.ctypes.data,
                                               want[f].ctypes.data, 3 * W, HOST_THREADS)
                assert rc == 0, rc
            t2 = time.perf_counter()
            d2h_s.append(t1 - t0)
            host_s.append(t2 - t0)
        d_want = torch.from_numpy(want).to(dev)
        rgb.fill_(0)
        pixels()
        torch.cuda.synchronize()
        equal = bool(torch.equal(rgb, d_want))
        t_px = timed(pixels)
        repeat = bool(torch.equal(rgb, d_want))
        t_xform = timed(xform)
        bpp = (9, 7, 6)[sr]
        nbytes = F * W * H * bpp
        res["modes"].append({
            "sample_ratio": sr, "bytes_per_px": bpp, "pixels_us": t_px, "xform_us": t_xform,
            "fraction_of_8TBps": nbytes / (t_px[0] * 1e-6) / 8e12,
            "xform_fraction_of_8TBps": nbytes / (t_xform[0] * 1e-6) / 8e12,
            "gpx_per_s": F * W * H / t_px[0] / 1e3,
            "host_route_s": min(host_s), "host_route_d2h_s": min(d2h_s), "host_threads": HOST_THREADS,
            "speedup": min(host_s) / (t_px[2] * 1e-6),
            "pixels_equal": equal, "repeat_equal": repeat,
        })
        del coef, rgb, ws, d_want, pinned
    res["bytes_equal"] = all(m["pixels_equal"] for m in res["modes"])
    res["repeat_equal"] = all(m["repeat_equal"] for m in res["modes"])
    return res


def measure_px_scaled(name, d_rgb, dev):
    """--pixels --scale: jpgx_pixels_gpu_scaled / jpgx_pixels_gpu_gray_scaled at 1/2, 1/4 and 1/8 beside the
    full-size call (jpgx_pixels_gpu, jpgx_pixels_gpu_gray: kernels this commit does not touch) on the same
    coefficients, in the same process, the calls taken in turn and the full-size one timed before and after
    the scaled ones.  Frames 0 and F - 1 of every scaled call are checked against the host twin."""
    nb = (W // 8) * (H // 8)
    qt_host = jpgx.jfif_qt(Q)
    d_qt = torch.from_numpy(qt_host.view(np.int16)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    L = jpgx.lib
    res = {"input": name, "modes": []}
    for mode in (0, 1, 2, "gray1", "gray3"):
        gray = isinstance(mode, str)
        sr = 0 if gray else mode
        channels = int(mode[-1]) if gray else 3
        flags = jpgx.FLAG_SUBSAMPLE if sr else 0
        nbc = jpgx.chroma_blocks(W, 0, H // 8, sr, flags)
        per = (nb + 2 * nbc) * 64
        coef = torch.empty((F, per), dtype=torch.int16, device=dev)
        fr = jpgx.frames(W, H, nframes=F, out_frame_stride=per)
        p = jpgx.default_params(W, H, Q, sr, flags=flags)
        xws = torch.empty(max(jpgx.workspace_size(fr), 1), dtype=torch.uint8, device=dev)
        jpgx.blocks_gpu(fr, p, d_rgb, coef, xws)         # a one-component frame: the Y blocks and Y's table
        torch.cuda.synchronize()
        del xws
        coef_bytes = F * (nb if gray else nb + 2 * nbc) * 128

        def call(d):
            ow, oh = jpgx.scaled_size(W, H, d)
            pitch = (channels * ow + 7) // 8 * 8
            out = torch.empty((F, oh, pitch), dtype=torch.uint8, device=dev)
            if gray:
                def run():
                    rc = (L.jpgx_pixels_gpu_gray(coef.data_ptr(), per, F, W, H, d_qt.data_ptr(), 0, None, out.data_ptr(),
                                                 pitch, oh * pitch, channels, stream) if d == 1 else
                          L.jpgx_pixels_gpu_gray_scaled(coef.data_ptr(), per, F, W, H, d, d_qt.data_ptr(), 0, None,
                                                        out.data_ptr(), pitch, oh * pitch, channels, stream))
                    assert rc == 0, rc
                return run, out, ow, oh, 0
            wsb = int(L.jpgx_pixels_gpu_workspace_size(W, H, sr, F) if d == 1 else
                      L.jpgx_pixels_gpu_scaled_workspace_size(W, H, sr, d, F))
            ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)

            def run():
                rc = (L.jpgx_pixels_gpu(coef.data_ptr(), per, F, W, H, sr, d_qt.data_ptr(), 0, None, out.data_ptr(), pitch,
                                        oh * pitch, ws.data_ptr() if wsb else None, wsb, stream) if d == 1 else
                      L.jpgx_pixels_gpu_scaled(coef.data_ptr(), per, F, W, H, sr, d, d_qt.data_ptr(), 0, None,
                                               out.data_ptr(), pitch, oh * pitch, ws.data_ptr() if wsb else None, wsb,
                                               stream))
                assert rc == 0, rc
            return run, out, ow, oh, wsb

        full, _, _, _, _ = call(1)
        t_full = [timed(full)]
        entry = {"mode": mode, "sample_ratio": sr, "channels": channels, "coef_bytes": coef_bytes, "scales": []}
        for d in (2, 4, 8):
            run, out, ow, oh, wsb = call(d)
            out.fill_(0)
            run()
            torch.cuda.synchronize()
            equal = True
            for f in (0, F - 1):
                c = coef[f].cpu().numpy()
                want = (C.pixels_host_gray(c, W, H, qt_host[0], channels, HOST_THREADS, scale=d) if gray else
                        C.pixels_host(c, W, H, sr, qt_host, HOST_THREADS, scale=d))
                got = out[f, :, :channels * ow].cpu().numpy().reshape(want.shape)
                equal = equal and bool(np.array_equal(got, want))
            t = timed(run)
            nbytes = coef_bytes + F * ow * oh * channels
            entry["scales"].append({"scale_denom": d, "out": [ow, oh], "us": t, "workspace_bytes": wsb,
                                    "algorithmic_bytes": nbytes,
                                    "fraction_of_8TBps": nbytes / (median(t) * 1e-6) / 8e12, "pixels_equal": equal})
            del out
        t_full.append(timed(full))
        both = sorted(t_full[0] + t_full[1])
        full_bytes = coef_bytes + F * W * H * channels
        entry.update({"full_us_before": t_full[0], "full_us_after": t_full[1], "full_median_us": median(both),
                      "full_spread_us": [both[0], both[-1]], "full_algorithmic_bytes": full_bytes,
                      "full_fraction_of_8TBps": full_bytes / (median(both) * 1e-6) / 8e12})
        for s in entry["scales"]:
            s["ratio_to_full"] = median(s["us"]) / median(both)
            # the bar: no longer than the full-size call, with no margin beyond that call's own spread
            s["within_bar"] = bool(median(s["us"]) <= both[-1])
        res["modes"].append(entry)
        del coef
    res["bytes_equal"] = all(s["pixels_equal"] for m in res["modes"] for s in m["scales"])
    res["repeat_equal"] = res["bytes_equal"]
    res["within_bar"] = all(s["within_bar"] for m in res["modes"] for s in m["scales"])
    return res


PARENT = None                           # --parent-lib: the parent commit's library, loaded beside this one
FILL = 0x7A


def median(ts):
    return sorted(ts)[len(ts) // 2]


def decoder_any(d_rgb, dev):
    """the photo-like frames at 3839 x 2159, Pillow's files with one MCU row per interval, both scan kernels"""
    import io

    from PIL import Image
    Wo, Ho = W - 1, H - 1
    host = d_rgb[:, :Ho, :Wo].cpu().numpy()
    stream = torch.cuda.current_stream().cuda_stream
    out = []
    for sr in (0, 2):
        files = []
        for f in range(F):
            b = io.BytesIO()
            Image.fromarray(host[f]).save(b, "JPEG", quality=Q, subsampling=sr, restart_marker_rows=1)
            files.append(b.getvalue())
        cap = (max(len(x) for x in files) + 15) // 16 * 16
        packed = np.zeros((F, cap), np.uint8)
        for f, x in enumerate(files):
            packed[f, :len(x)] = np.frombuffer(x, np.uint8)
        d_files = torch.from_numpy(packed).to(dev)
        d_lens = torch.tensor([len(x) for x in files], dtype=torch.int64, device=dev)
        cw, ch = jpgx.coded_size(Wo, Ho, sr)
        nb = (cw // 8) * (ch // 8)
        per = (nb + 2 * (nb // (1, 2, 4)[sr])) * 64
        qt = torch.empty((F, 2, 64), dtype=torch.int16, device=dev)
        status = torch.empty(F, dtype=torch.int32, device=dev)
        got, ts = {}, {}
        for flags in (0, jpgx.JFIF_DECODE_SUBINTERVAL):
            coef = torch.empty((F, per), dtype=torch.int16, device=dev)
            need = int(jpgx.lib.jpgx_jfif_decode_gpu_any_workspace_size(Wo, Ho, sr, F, cap, flags))
            ws = torch.empty(need, dtype=torch.uint8, device=dev)

            def dec():
                rc = jpgx.lib.jpgx_jfif_decode_gpu_any(d_files.data_ptr(), cap, d_lens.data_ptr(), F, Wo, Ho, sr, flags,
                                                       coef.data_ptr(), per, qt.data_ptr(), status.data_ptr(),
                                                       ws.data_ptr(), need, stream)
                assert rc == 0, rc

            dec()
            torch.cuda.synchronize()
            ok = status.cpu().tolist() == [0] * F
            ts[flags] = timed(dec, calls=5)
            got[flags] = (coef, ok)
        ref = C.read_jfif(files[0], HOST_THREADS, any_size=True)["coef"].reshape(-1)
        equal = bool(got[0][1] and got[1][1] and torch.equal(got[0][0], got[1][0])
                     and np.array_equal(got[0][0][0].cpu().numpy(), ref))
        out.append({"sample_ratio": sr, "width": Wo, "height": Ho, "file_bytes": [len(x) for x in files],
                    "decode_us": ts[0], "decode_sub_us": ts[1], "coefficients_equal": equal})
    return out


def measure_px_any(name, d_rgb, dev):
    nb = (W // 8) * (H // 8)
    Wo, Ho = W - 1, H - 1               # the same coded frame in all three sample modes
    qt_host = jpgx.jfif_qt(Q)
    d_qt = torch.from_numpy(qt_host.view(np.int16)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    res = {"input": name, "modes": []}
    for sr in (0, 1, 2):
        assert jpgx.coded_size(Wo, Ho, sr) == (W, H)
        flags = jpgx.FLAG_SUBSAMPLE if sr else 0
        nbc = jpgx.chroma_blocks(W, 0, H // 8, sr, flags)
        per = (nb + 2 * nbc) * 64
        coef = torch.empty((F, per), dtype=torch.int16, device=dev)
        fr = jpgx.frames(W, H, nframes=F, out_frame_stride=per)
        p = jpgx.default_params(W, H, Q, sr, flags=flags)
        xws = torch.empty(max(jpgx.workspace_size(fr), 1), dtype=torch.uint8, device=dev)
        jpgx.blocks_gpu(fr, p, d_rgb, coef, xws)
        torch.cuda.synchronize()
        rgb = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
        wsb = int(jpgx.lib.jpgx_pixels_gpu_workspace_size(W, H, sr, F))
        assert wsb == int(jpgx.lib.jpgx_pixels_gpu_any_workspace_size(Wo, Ho, sr, F))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)

        def call(fn, w, h):
            def run():
                rc = fn(coef.data_ptr(), per, F, w, h, sr, d_qt.data_ptr(), 0, None, rgb.data_ptr(), 3 * W, 3 * W * H,
                        ws.data_ptr() if wsb else None, wsb, stream)
                assert rc == 0, rc
            return run

        fns = {"plain_us": call(jpgx.lib.jpgx_pixels_gpu, W, H),
               "any_full_us": call(jpgx.lib.jpgx_pixels_gpu_any, W, H),
               "any_odd_us": call(jpgx.lib.jpgx_pixels_gpu_any, Wo, Ho)}
        if PARENT is not None:
            fns["parent_plain_us"] = call(PARENT.jpgx_pixels_gpu, W, H)
        # the checks: (b) == (a); (c) == the host on two frames, nothing written outside the visible frame
        fns["plain_us"]()
        want = rgb.clone()
        rgb.fill_(FILL)
        fns["any_full_us"]()
        equal = bool(torch.equal(rgb, want))
        rgb.fill_(FILL)
        fns["any_odd_us"]()
        torch.cuda.synchronize()
        equal = equal and bool((rgb[:, :, Wo:] == FILL).all()) and bool((rgb[:, Ho:] == FILL).all())
        host_coef = coef[:2].cpu().numpy()
        for f in range(2):
            ref = C.pixels_host(host_coef[f], Wo, Ho, sr, qt_host, HOST_THREADS, any_size=True)
            equal = equal and bool(np.array_equal(rgb[f, :Ho, :Wo].cpu().numpy(), ref))
        ts = {k: [] for k in fns}
        for _ in range(3):                               # the calls taken in turn, pass after pass
            for k in sorted(fns):
                ts[k] += timed(fns[k], calls=10, rounds=3, settle=0.3)
        m = {"sample_ratio": sr, "pixels_equal": equal, "repeat_equal": equal}
        for k in fns:
            m[k] = sorted(ts[k])
        base = median(ts["plain_us"])
        m["plain_median_us"] = base
        m["any_full_over_plain"] = median(ts["any_full_us"]) / base
        m["any_odd_over_plain"] = median(ts["any_odd_us"]) / base
        if PARENT is not None:
            m["parent_plain_median_us"] = median(ts["parent_plain_us"])
            m["parent_spread_us"] = max(ts["parent_plain_us"]) - min(ts["parent_plain_us"])
            m["plain_minus_parent_us"] = base - m["parent_plain_median_us"]
        res["modes"].append(m)
        del coef, rgb, ws, want
    if name.startswith("flat"):
        res["decoder_3839x2159"] = decoder_any(d_rgb, dev)
    res["bytes_equal"] = all(m["pixels_equal"] for m in res["modes"]) and all(
        d["coefficients_equal"] for d in res.get("decoder_3839x2159", []))
    res["repeat_equal"] = res["bytes_equal"]
    return res


KERNEL_STATS = None                     # --kernel-stats=FILE.csv


def pad_kernel_us():
    """k_pad_edge's average time in a rocprofv3 --kernel-trace --stats table, in microseconds; None without one"""
    if not KERNEL_STATS:
        return None
    import csv
    with open(KERNEL_STATS, newline="") as fh:
        for row in csv.DictReader(fh):
            if "k_pad_edge" in row.get("Name", ""):
                return float(row["AverageNs"]) / 1e3
    raise SystemExit("no k_pad_edge in " + KERNEL_STATS)


def measure_enc_any(name, d_rgb, dev):
    import ctypes
    VW, VH = W - 1, H - 1
    nb = (W // 8) * (H // 8)
    per = 3 * nb * 64
    d_any = d_rgb[:, :VH, :VW].contiguous()              # rows of 11517 bytes, frames an odd number apart
    coef = torch.empty((F, per), dtype=torch.int16, device=dev)
    coef_any = torch.empty((F, per), dtype=torch.int16, device=dev)
    fr = jpgx.frames(W, H, nframes=F, out_frame_stride=per)
    p = jpgx.default_params(W, H, Q, 0)
    fra = jpgx.frames(VW, VH, nframes=F, rows=(0, H // 8), in_pitch=3 * VW, in_frame_stride=3 * VW * VH,
                      out_frame_stride=per)
    xws = torch.empty(max(jpgx.workspace_size(fr), 16), dtype=torch.uint8, device=dev)
    need = int(jpgx.lib.jpgx_workspace_size_any(ctypes.byref(fra), ctypes.byref(p)))
    aws = torch.empty(need, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def plain_xform():
        jpgx.blocks_gpu(fr, p, d_rgb, coef, xws)

    def any_xform():
        rc = jpgx.lib.jpgx_blocks_gpu_any(ctypes.byref(fra), ctypes.byref(p), d_any.data_ptr(), coef_any.data_ptr(),
                                          aws.data_ptr(), need, stream)
        assert rc == 0, rc

    # what the any-size call must equal: the plain one on the image padded by the edge rule
    padded = torch.cat([d_any, d_any[:, :, -1:]], 2)
    padded = torch.cat([padded, padded[:, -1:]], 1).contiguous()
    want = torch.empty((F, per), dtype=torch.int16, device=dev)
    jpgx.blocks_gpu(fr, p, padded, want, xws)
    plain_xform()
    any_xform()
    torch.cuda.synchronize()
    equal = bool(torch.equal(coef_any, want))
    del padded

    _, lens0 = jpgx.jfif_gpu(coef, W, H, Q, 0, 1, cap=1 << 20)
    _, lens1 = jpgx.jfif_gpu(coef_any, VW, VH, Q, 0, 1, cap=1 << 20, any_size=True)
    cap = (int(max(lens0.max(), lens1.max())) + 4095) // 4096 * 4096
    out = torch.empty((F, cap), dtype=torch.uint8, device=dev)
    out_any = torch.empty((F, cap), dtype=torch.uint8, device=dev)
    lens, lens_any = (torch.empty(F, dtype=torch.int64, device=dev) for _ in range(2))
    wsb = int(jpgx.lib.jpgx_jfif_gpu_workspace_size_ex(W, H, 0, 1, F, cap, 0))
    assert wsb == int(jpgx.lib.jpgx_jfif_gpu_any_workspace_size(VW, VH, 0, 1, F, cap, 0))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def plain_coder():
        rc = jpgx.lib.jpgx_jfif_gpu_ex(coef.data_ptr(), per, F, W, H, Q, 0, 1, 0, out.data_ptr(), cap, cap,
                                       lens.data_ptr(), ws.data_ptr(), wsb, stream)
        assert rc == 0, rc

    def any_coder():
        rc = jpgx.lib.jpgx_jfif_gpu_any(coef_any.data_ptr(), per, F, VW, VH, Q, 0, 1, 0, out_any.data_ptr(), cap, cap,
                                        lens_any.data_ptr(), ws.data_ptr(), wsb, stream)
        assert rc == 0, rc

    def file0():
        n = int(lens_any[0])
        return out_any[0, :n].cpu().numpy().tobytes()

    any_coder()
    torch.cuda.synchronize()
    host = C.write_jfif_ex(coef_any[0].cpu().numpy().reshape(-1, 64), VW, VH, Q, 0, restart_rows=1,
                           nthreads=HOST_THREADS, cap=cap, any_size=True)
    equal = equal and file0() == host
    calls = (("plain_xform_us", plain_xform), ("any_xform_us", any_xform), ("plain_coder_us", plain_coder),
             ("any_coder_us", any_coder))
    ts = {k: [] for k, _ in calls}
    for _ in range(7):                                   # the four in turn, pass after pass
        for k, fn in calls:
            ts[k] += timed(fn, rounds=1, settle=0.2)
    ts = {k: sorted(v) for k, v in ts.items()}
    torch.cuda.synchronize()
    repeat_equal = bool(torch.equal(coef_any, want)) and file0() == host
    m = {k: median(v) for k, v in ts.items()}
    pad = m["any_xform_us"] - m["plain_xform_us"]
    moved = 6 * F * W * H                                # the coded frames: 3 B read and 3 B written per pixel
    res = {"input": name, **ts,
           "any_xform_over_plain": m["any_xform_us"] / m["plain_xform_us"],
           "any_coder_over_plain": m["any_coder_us"] / m["plain_coder_us"],
           "any_route_over_plain": (m["any_xform_us"] + m["any_coder_us"]) / (m["plain_xform_us"] + m["plain_coder_us"]),
           "pad_us_by_difference": pad, "pad_bytes": moved,
           "pad_fraction_of_8TBps_by_difference": moved / (pad * 1e-6) / 8e12 if pad > 0 else None,
           "workspace_bytes": need, "file_bytes_per_frame": [int(x) for x in lens_any.cpu()],
           "bytes_equal": equal, "repeat_equal": repeat_equal}
    k_us = pad_kernel_us()
    if k_us is not None:
        res["pad_kernel_us"] = k_us
        res["pad_fraction_of_8TBps"] = moved / (k_us * 1e-6) / 8e12
    return res


GRAY_FILES = None                       # --gray-files=DIR


def gray_inputs():
    """[(name, slug, uint8 [F][H][W])], made on the host: the files must be the same wherever they are written"""
    g = np.random.default_rng(7)
    noise = g.integers(0, 256, (F, H, W), dtype=np.uint8)
    tiles = g.integers(0, 256, (F, H // 8, W // 8), dtype=np.int16).repeat(8, 1).repeat(8, 2)
    flat = np.clip(tiles + g.integers(-6, 7, tiles.shape, dtype=np.int16), 0, 255).astype(np.uint8)
    return [("noise", "noise", noise), ("flat 8x8 tiles + noise of +-6", "flat", flat)]


def gray_files(slug, images, dri):
    """the F files of an input: from --gray-files=DIR when they are there, else from Pillow (and into DIR)"""
    names = ["%s_%s_%d.jpg" % (slug, "dri" if dri else "nodri", f) for f in range(F)]
    if GRAY_FILES and all(os.path.exists(os.path.join(GRAY_FILES, n)) for n in names):
        return [open(os.path.join(GRAY_FILES, n), "rb").read() for n in names]
    import io

    from PIL import Image
    files = []
    for f in range(F):
        b = io.BytesIO()
        Image.fromarray(images[f], "L").save(b, "JPEG", quality=Q, **(dict(restart_marker_rows=1) if dri else {}))
        files.append(b.getvalue())
    if GRAY_FILES:
        os.makedirs(GRAY_FILES, exist_ok=True)
        for n, data in zip(names, files):
            with open(os.path.join(GRAY_FILES, n), "wb") as fh:
                fh.write(data)
    return files


def measure_gray(name, slug, images, dev):
    nb = (W // 8) * (H // 8)
    per = nb * 64
    SUB = jpgx.JFIF_DECODE_SUBINTERVAL
    stream = torch.cuda.current_stream().cuda_stream
    res = {"input": name}
    ok = True
    coef = torch.empty((F, per), dtype=torch.int16, device=dev)
    qt = torch.empty((F, 64), dtype=torch.int16, device=dev)
    status = torch.empty(F, dtype=torch.int32, device=dev)
    for key, dri in (("with_dri", True), ("no_dri", False)):
        files = gray_files(slug, images, dri)
        cap = (max(len(x) for x in files) + 15) // 16 * 16
        packed = np.zeros((F, cap), np.uint8)
        for f, x in enumerate(files):
            packed[f, :len(x)] = np.frombuffer(x, np.uint8)
        d_files = torch.from_numpy(packed).to(dev)
        d_lens = torch.tensor([len(x) for x in files], dtype=torch.int64, device=dev)
        info = C.jfif_info_gray(files[0])
        assert (info["width"], info["height"], info["restart_interval"]) == (W, H, W // 8 if dri else 0), info
        ref = C.read_jfif_gray(files[0], HOST_THREADS)["coef"].reshape(-1)
        part = {"file_bytes": [len(x) for x in files], "intervals": F * (H // 8 if dri else 1)}
        got = {}
        for tkey, flags in (("decode_us", 0), ("decode_sub_us", SUB)):
            need = int(jpgx.lib.jpgx_jfif_decode_gpu_gray_workspace_size(W, H, F, cap, flags))
            ws = torch.empty(need, dtype=torch.uint8, device=dev)

            def dec():
                rc = jpgx.lib.jpgx_jfif_decode_gpu_gray(d_files.data_ptr(), cap, d_lens.data_ptr(), F, W, H, flags,
                                                        coef.data_ptr(), per, qt.data_ptr(), status.data_ptr(),
                                                        ws.data_ptr(), need, stream)
                assert rc == 0, rc

            coef.fill_(0x5A5A)
            dec()
            torch.cuda.synchronize()
            ok = ok and status.cpu().tolist() == [0] * F
            part[tkey] = timed(dec) if dri else timed(dec, calls=1, rounds=3, settle=0.0)
            ok = ok and status.cpu().tolist() == [0] * F and bool(np.array_equal(coef[0].cpu().numpy(), ref))
            got[flags] = coef.clone()
        ok = ok and bool(torch.equal(got[0], got[SUB]))
        part["sub_over_plain"] = median(part["decode_sub_us"]) / median(part["decode_us"])
        part["gpx_per_s_sub"] = F * W * H / part["decode_sub_us"][0] / 1e3
        res[key] = part
        del got
        if not dri:
            continue
        # the host route on the files with restart intervals, which is also the pixels' check
        pinned = torch.empty((F, cap), dtype=torch.uint8).pin_memory()
        hcoef, hqt = np.empty((F, per), np.int16), np.empty((F, 64), np.uint16)
        want = np.empty((F, H, W), np.uint8)
        host_s = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pinned.copy_(d_files)
            torch.cuda.synchronize()
            for f in range(F):
                rc = jpgx.lib.jpgx_read_jfif_gray(pinned.data_ptr() + f * cap, len(files[f]), HOST_THREADS,
                                                  hcoef[f].ctypes.data, per, hqt[f].ctypes.data, None)
                assert rc == 0, rc
                rc = jpgx.lib.jpgx_pixels_host_gray(hcoef[f].ctypes.data, W, H, hqt[f].ctypes.data, want[f].ctypes.data,
                                                    W, 1, HOST_THREADS)
                assert rc == 0, rc
            host_s.append(time.perf_counter() - t0)
        res["host_route_s"], res["host_threads"] = min(host_s), HOST_THREADS
        # the pixel kernel on what the decoder left
        equal = True
        for ch in (1, 3):
            out = torch.empty((F, H, W * ch), dtype=torch.uint8, device=dev)

            def pixels():
                rc = jpgx.lib.jpgx_pixels_gpu_gray(coef.data_ptr(), per, F, W, H, qt.data_ptr(), 64, status.data_ptr(),
                                                   out.data_ptr(), ch * W, ch * W * H, ch, stream)
                assert rc == 0, rc

            def check():
                px = out[:2].cpu().numpy().reshape(2, H, W, ch)
                return all(np.array_equal(px[f, :, :, c], want[f]) for f in range(2) for c in range(ch))

            out.fill_(FILL)
            pixels()
            torch.cuda.synchronize()
            equal = equal and check()
            t = timed(pixels)
            equal = equal and check()
            bpp = 2 + ch
            res["px%d_us" % ch] = t
            res["px%d_bytes_per_px" % ch] = bpp
            res["px%d_fraction_of_8TBps" % ch] = F * W * H * bpp / (t[0] * 1e-6) / 8e12
            del out
        res["speedup"] = min(host_s) / ((median(res["with_dri"]["decode_sub_us"]) + median(res["px1_us"])) * 1e-6)
        res["pixels_equal"] = bool(equal)
    # k_px444 in the same session: the same image as R = G = B through the forward transform
    per3 = 3 * per
    d_rgb = torch.from_numpy(images).to(dev).unsqueeze(3).expand(F, H, W, 3).contiguous()
    coef3 = torch.empty((F, per3), dtype=torch.int16, device=dev)
    fr = jpgx.frames(W, H, nframes=F, out_frame_stride=per3)
    p = jpgx.default_params(W, H, Q, 0)
    xws = torch.empty(max(jpgx.workspace_size(fr), 1), dtype=torch.uint8, device=dev)
    jpgx.blocks_gpu(fr, p, d_rgb, coef3, xws)
    torch.cuda.synchronize()
    d_qt2 = torch.from_numpy(jpgx.jfif_qt(Q).view(np.int16)).to(dev)
    rgb = d_rgb                                              # the input is no longer needed: the output takes its place

    def px444():
        rc = jpgx.lib.jpgx_pixels_gpu(coef3.data_ptr(), per3, F, W, H, 0, d_qt2.data_ptr(), 0, None, rgb.data_ptr(),
                                      3 * W, 3 * W * H, None, 0, stream)
        assert rc == 0, rc

    t = timed(px444)
    res["px444_us"] = t
    res["px444_fraction_of_8TBps"] = F * W * H * 9 / (t[0] * 1e-6) / 8e12
    res["px1_fraction_over_px444"] = res["px1_fraction_of_8TBps"] / res["px444_fraction_of_8TBps"]
    res["coefficients_equal"] = bool(ok)
    res["bytes_equal"] = bool(ok and res["pixels_equal"])
    res["repeat_equal"] = res["bytes_equal"]
    return res


def main_gray(dst):
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    res = {"what": "tools/jfif_gpu_bench.py --gray", "width": W, "height": H, "frames": F, "quality": Q,
           "device": torch.cuda.get_device_name(0), "version": jpgx.version(), "runs": []}
    for name, slug, images in gray_inputs():
        res["runs"].append(measure_gray(name, slug, images, dev))
        print(json.dumps(res["runs"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    ok = all(r["bytes_equal"] and r["repeat_equal"] for r in res["runs"])
    print("bytes equal:", ok)
    sys.exit(0 if ok else 1)


def measure_enc_gray(name, images, dev):
    import ctypes
    stream = torch.cuda.current_stream().cuda_stream
    L = jpgx.lib
    L.jx_gray_host_blocks.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_void_p]
    L.jx_selftest_gray_blocks.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_longlong), ctypes.c_void_p]
    L.jx_selftest_gray_blocks.restype = ctypes.c_longlong
    res = {"input": name}
    ok = again = True
    full = {}
    for VW, VH in ((W, H), (W - 1, H - 1)):
        bw, bh = (VW + 7) // 8, (VH + 7) // 8
        nb = bw * bh
        per = nb * 64
        host_img = np.ascontiguousarray(images[:, :VH, :VW])
        d = torch.from_numpy(host_img).to(dev)
        coef = torch.empty((F, per), dtype=torch.int16, device=dev)

        def fwd(d=d, coef=coef, VW=VW, VH=VH, per=per):        # bound now: the gate below calls the first size's
            rc = L.jpgx_blocks_gpu_gray(d.data_ptr(), VW, VW * VH, F, VW, VH, Q, 0, coef.data_ptr(), per, stream)
            assert rc == 0, rc

        want0 = np.empty((nb, 64), np.int16)
        rc = L.jx_gray_host_blocks(host_img[0].ctypes.data, VW, VH, VW, Q, 0, want0.ctypes.data)
        assert rc == 0, rc
        coef.fill_(0x5A5A)
        fwd()
        torch.cuda.synchronize()
        ok = ok and bool(np.array_equal(coef[0].cpu().numpy().reshape(nb, 64), want0))
        part = {"blocks_per_frame": nb, "xform_us": timed(fwd)}
        part["fraction_of_8TBps"] = 3 * F * VW * VH / (part["xform_us"][0] * 1e-6) / 8e12

        _, lens0 = jpgx.jfif_gpu_gray(coef, VW, VH, Q, 1, cap=1 << 20)
        cap = (int(lens0.max()) + 4095) // 4096 * 4096
        out = torch.empty((F, cap), dtype=torch.uint8, device=dev)
        lens = torch.empty(F, dtype=torch.int64, device=dev)
        files0 = {}
        for key, flags in (("coder_us", 0), ("coder_opt_us", jpgx.JFIF_OPTIMIZE)):
            wsb = int(L.jpgx_jfif_gpu_gray_workspace_size(VW, VH, 1, F, cap, flags))
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

            def coder():
                rc = L.jpgx_jfif_gpu_gray(coef.data_ptr(), per, F, VW, VH, Q, 1, flags, out.data_ptr(), cap, cap,
                                          lens.data_ptr(), ws.data_ptr(), wsb, stream)
                assert rc == 0, rc

            def file0():
                return out[0, :int(lens[0])].cpu().numpy().tobytes()

            host = C.write_jfif_gray(want0, VW, VH, Q, restart_rows=1, nthreads=HOST_THREADS, optimize=bool(flags), cap=cap)
            coder()
            torch.cuda.synchronize()
            ok = ok and file0() == host
            part[key] = timed(coder)
            again = again and file0() == host
            files0[key] = len(host)
        part["file_bytes_frame0"], part["file_bytes_frame0_opt"] = files0["coder_us"], files0["coder_opt_us"]
        part["opt_over_std"] = median(part["coder_opt_us"]) / median(part["coder_us"])
        # the host route: D2H of the coefficients into pinned memory + the host writer, frame after frame
        pinned = torch.empty((F, per), dtype=torch.int16).pin_memory()
        buf = np.empty(cap, np.uint8)
        n = ctypes.c_size_t()
        host_s = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pinned.copy_(coef)
            torch.cuda.synchronize()
            for f in range(F):
                rc = L.jpgx_write_jfif_gray(pinned.data_ptr() + f * per * 2, VW, VH, Q, 1, HOST_THREADS, 0,
                                            buf.ctypes.data, cap, ctypes.byref(n))
                assert rc == 0, rc
            host_s.append(time.perf_counter() - t0)
        part["host_route_s"], part["host_threads"] = min(host_s), HOST_THREADS
        part["speedup"] = min(host_s) / (median(part["coder_us"]) * 1e-6)
        fwd()
        torch.cuda.synchronize()
        again = again and bool(np.array_equal(coef[0].cpu().numpy().reshape(nb, 64), want0))
        res["%dx%d" % (VW, VH)] = part
        if (VW, VH) == (W, H):
            full = {"d": d, "coef": coef, "fwd": fwd}
        del out, pinned

    # the gate: the same frames as R = G = B through jpgx_blocks_gpu, the two taken in turn
    per3 = 3 * (W // 8) * (H // 8) * 64
    d_rgb = full["d"].unsqueeze(3).expand(F, H, W, 3).contiguous()
    coef3 = torch.empty((F, per3), dtype=torch.int16, device=dev)
    fr = jpgx.frames(W, H, nframes=F, out_frame_stride=per3)
    p = jpgx.default_params(W, H, Q, 0)
    xws = torch.empty(max(jpgx.workspace_size(fr), 16), dtype=torch.uint8, device=dev)

    def rgb_xform():
        jpgx.blocks_gpu(fr, p, d_rgb, coef3, xws)

    calls = (("gray_xform_us", full["fwd"]), ("rgb_xform_us", rgb_xform))
    ts = {k: [] for k, _ in calls}
    for _ in range(7):
        for k, fn in calls:
            ts[k] += timed(fn, rounds=1, settle=0.2)
    ts = {k: sorted(v) for k, v in ts.items()}
    res.update(ts)
    res["gray_over_rgb"] = median(ts["gray_xform_us"]) / median(ts["rgb_xform_us"])
    res["gray_fraction_of_8TBps"] = 3 * F * W * H / (ts["gray_xform_us"][0] * 1e-6) / 8e12
    res["rgb_fraction_of_8TBps"] = 9 * F * W * H / (ts["rgb_xform_us"][0] * 1e-6) / 8e12
    res["gate_gray_below_rgb"] = bool(res["gray_over_rgb"] < 1.0)

    # the flagged share: the kernel's fp32 sequence and band on the host, over frame 0's first blocks
    nsample = 20000
    blocks = np.ascontiguousarray(images[0, :H // 8 * 8, :W].reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)
                                  .reshape(-1, 64)[:nsample])
    res["flagged_share"], res["blocks_with_a_flag"] = {}, {}
    for q in (50, 90, 97):
        flagged = ctypes.c_longlong()
        mask = np.zeros(len(blocks), np.uint64)
        bad = L.jx_selftest_gray_blocks(blocks.ctypes.data, len(blocks), q, ctypes.byref(flagged), mask.ctypes.data)
        ok = ok and bad == 0
        res["flagged_share"][str(q)] = flagged.value / (64.0 * len(blocks))
        res["blocks_with_a_flag"][str(q)] = float((mask != 0).mean())
    res["bytes_equal"], res["repeat_equal"] = bool(ok), bool(again)
    return res


def main_enc_gray(dst):
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    res = {"what": "tools/jfif_gpu_bench.py --encode-gray", "width": W, "height": H, "frames": F, "quality": Q,
           "restart_rows": 1, "device": torch.cuda.get_device_name(0), "version": jpgx.version(), "runs": []}
    for name, _, images in gray_inputs():
        res["runs"].append(measure_enc_gray(name, images, dev))
        print(json.dumps(res["runs"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    ok = all(r["bytes_equal"] and r["repeat_equal"] for r in res["runs"])
    gate = all(r["gate_gray_below_rgb"] for r in res["runs"])
    print("bytes equal:", ok, " gate (gray below rgb):", gate)
    sys.exit(0 if ok and gate else 1)


def main():
    global PARENT, GRAY_FILES, KERNEL_STATS
    modes = ("--optimize", "--decode", "--pixels", "--subinterval", "--any-size", "--gray", "--encode-any", "--encode-gray")
    scaled = "--scale" in sys.argv[1:]
    if scaled:
        sys.argv.remove("--scale")
        assert "--pixels" in sys.argv[1:] and "--any-size" not in sys.argv[1:], "--scale goes with --pixels alone"
    for a in sys.argv[1:]:
        if a.startswith("--parent-lib="):
            # an older build has only the plain entry points: bind the one call that is timed
            import ctypes
            PARENT = ctypes.CDLL(os.path.abspath(a.split("=", 1)[1]))
            PARENT.jpgx_pixels_gpu.argtypes = jpgx.lib.jpgx_pixels_gpu.argtypes
        if a.startswith("--gray-files="):
            GRAY_FILES = os.path.abspath(a.split("=", 1)[1])
        if a.startswith("--kernel-stats="):
            KERNEL_STATS = os.path.abspath(a.split("=", 1)[1])
    args = [a for a in sys.argv[1:] if a not in modes and not a.startswith(("--parent-lib=", "--gray-files=", "--kernel-stats="))]
    optimize, decoding, pixels, sub, any_size, gray, enc_any, enc_gray = (m in sys.argv[1:] for m in modes)
    if enc_gray:
        assert not (optimize or decoding or pixels or gray or enc_any), "--encode-gray stands alone"
        return main_enc_gray(args[0] if args else os.path.join(REPO, "profiles", "jfif_gpu_enc_gray.json"))
    assert not enc_any or not (optimize or decoding or pixels or gray), "--encode-any stands alone"
    if gray:
        assert not (optimize or decoding or pixels), "--gray stands alone"
        return main_gray(args[0] if args else os.path.join(REPO, "profiles", "jfif_gpu_gray.json"))
    assert decoding or not sub, "--subinterval goes with --decode"
    assert pixels or not any_size, "--any-size goes with --pixels"
    run = measure_px_scaled if scaled else measure_enc_any if enc_any else measure_px_any if any_size else measure_px if pixels else measure_dec_sub if sub else measure_dec if decoding else \
        measure_opt if optimize else measure
    dst = args[0] if args else os.path.join(
        REPO, "profiles", "jfif_gpu_px_scaled.json" if scaled else "jfif_gpu_enc_any.json" if enc_any else "jfif_gpu_px_any.json" if any_size else "jfif_gpu_px.json" if pixels else "jfif_gpu_dec_sub.json" if sub else
        "jfif_gpu_dec.json" if decoding else "jfif_gpu_opt.json" if optimize else "jfif_gpu.json")
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    res = {"what": "tools/jfif_gpu_bench.py" + (" --encode-any" if enc_any else " --pixels --scale" if scaled else " --pixels --any-size" if any_size else " --pixels" if pixels else " --decode --subinterval" if sub else " --decode" if decoding else " --optimize" if optimize else ""), "width": W, "height": H, "frames": F, "quality": Q,
           "sample_ratio": 0, "restart_rows": 1, "device": torch.cuda.get_device_name(0),
           "version": jpgx.version(), "runs": []}
    d = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    for f in range(F):
        jpgx.gen_splitmix_gpu(d[f], 1000 + f)
    res["runs"].append(run("splitmix noise (the flagship's input)", d, dev))
    print(json.dumps(res["runs"][-1]), flush=True)
    g = torch.Generator(device=dev).manual_seed(7)
    tiles = torch.randint(0, 256, (F, H // 8, W // 8, 3), generator=g, dtype=torch.uint8, device=dev)
    big = tiles.repeat_interleave(8, 1).repeat_interleave(8, 2).to(torch.int16)
    big += torch.randint(-6, 7, big.shape, generator=g, dtype=torch.int16, device=dev)
    d.copy_(big.clamp_(0, 255))
    del big, tiles
    res["runs"].append(run("flat 8x8 tiles + noise of +-6", d, dev))
    print(json.dumps(res["runs"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    ok = all(r["bytes_equal"] and r["repeat_equal"] for r in res["runs"])
    print("bytes equal:", ok)
    if scaled:
        print("every scaled call within the full-size call's time:", all(r["within_bar"] for r in res["runs"]))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
