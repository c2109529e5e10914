"""jpgx -- Python view of libjpgx.so, the MI355X-native JPEG block-transform hot path.

Everything here calls through the C ABI declared in include/jpgx.h; there is no Python or
CPU implementation of the transform in this package.  If the shared library is missing the
import fails loudly (ImportError) instead of falling back.

Reference mapping (matthewT53/JPEG-Encoder-and-Decoder):
    blocks_gpu / blocks   <- preprocess_jpeg + chroma_subsample + dct + quantise + zig_zag
                             (src/jpg_encode.c:32-44), output = JpgData.zig_zag_{Y,Cb,Cr}
    default_params        <- encode_bmp_to_jpeg(quality, sample_ratio) (src/jpg_encode.c:19)
    scale_table           <- scale_table (src/quantise.c:74-86)
No counterpart in the reference (its decoder is an empty header): jfif_decode_gpu,
decode_jpeg_coefficients -- baseline JFIF files back to the coefficients;
pixels_gpu, decode_jpeg -- the coefficients to RGB, libjpeg's default decoder's pixels (4.9).
These four take any_size=True for files whose width and height are no multiple of the MCU (the
library's _any entry points); coded_size is the size such a file's coefficients are of.
The way there takes images of any size too: encode_blocks, jfif_gpu and encode_jpeg with any_size=True
(jpgx_blocks_gpu_any, jpgx_jfif_gpu_any) transform and code the image's coded frame, the image with its
last column and row repeated up to the MCU (pad_edge), and the file states the image's own size.
One-component (grayscale) files go through jfif_decode_gpu_gray and pixels_gpu_gray (the library's
_gray entry points), or through decode_jpeg / decode_jpeg_coefficients with gray=True.  The way there:
encode_blocks_gray (jpgx_blocks_gpu_gray: a one-channel image of any size and any row pitch to Y
[nb][64]), jfif_gpu_gray (jpgx_jfif_gpu_gray: those coefficients to one-component files), or
encode_jpeg with gray=True; the contract is the project's own (include/jpgx.h).
pixels_gpu, pixels_gpu_gray and decode_jpeg take scale=2, 4 or 8 for libjpeg's decode at that fraction of
the size (the library's _scaled entry points); scaled_size is the output's size.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("JPGX_LIB") or os.path.join(PKG_ROOT, "lib", "libjpgx.so")

NO_CHROMA_SUBSAMPLING = 0
HORIZONTAL_SUBSAMPLING = 1
HORIZONTAL_VERTICAL_SUBSAMPLING = 2
FLAG_FORCE_EXACT = 1
FLAG_SUBSAMPLE = 2      # true 4:2:2 / 4:2:0 chroma (extension; see include/jpgx.h)
JFIF_OPTIMIZE = 1       # a flag of the JFIF writers: per-image Huffman tables (JPGX_JFIF_OPTIMIZE)
JFIF_DECODE_SUBINTERVAL = 1     # a flag of the device decoder: decode inside the restart intervals

OK, EGEOMETRY, EQUALITY, ESAMPLE, EARG, EHIP, EWORKSPACE, ENODEV, ENOMEM = 0, -1, -2, -3, -4, -5, -6, -7, -8
EJFIF_HEADER, EJFIF_SCAN = -9, -10      # the JFIF decoder's two refusals (include/jpgx.h)
_ERRNAMES = {-1: "EGEOMETRY", -2: "EQUALITY", -3: "ESAMPLE", -4: "EARG", -5: "EHIP",
             -6: "EWORKSPACE", -7: "ENODEV", -8: "ENOMEM", -9: "EJFIF_HEADER", -10: "EJFIF_SCAN"}

# every function include/jpgx.h and include/jpgx_compat.h declare (tests check the library
# exports them all)
EXPORTS = [
    "jpgx_validate", "jpgx_default_params", "jpgx_glibc_underflow", "jpgx_scale_table",
    "jpgx_guard_band", "jpgx_workspace_size", "jpgx_blocks_gpu", "jpgx_blocks_gpu_ev",
    "jpgx_blocks_gpu_timed",
    "jpgx_gen_splitmix_gpu",
    "jpgx_gen_tie_gpu", "jpgx_blocks", "jpgx_blocks_multi", "jpgx_stripe",
    "jpgx_device_count", "jpgx_version", "jpgx_chroma_blocks", "jpgx_entropy_workspace_size",
    "jpgx_entropy_stats_gpu", "jpgx_entropy_workspace_size_batch", "jpgx_entropy_stats_gpu_batch",
    "jpgx_host_create", "jpgx_host_destroy", "jpgx_host_blocks",
    "jpgx_host_register", "jpgx_host_unregister", "jpgx_host_release",
    "jpgx_jfif_gpu_workspace_size", "jpgx_jfif_gpu",
    "jpgx_jfif_gpu_workspace_size_ex", "jpgx_jfif_gpu_ex",
    "jpgx_jfif_decode_gpu_workspace_size", "jpgx_jfif_decode_gpu",
    "jpgx_jfif_decode_gpu_workspace_size_ex", "jpgx_jfif_decode_gpu_ex", "jpgx_jfif_decode_sub_shape",
    "jpgx_pixels_gpu_workspace_size", "jpgx_pixels_gpu", "jpgx_jfif_qt",
    "jpgx_coded_size", "jpgx_jfif_decode_gpu_any_workspace_size", "jpgx_jfif_decode_gpu_any",
    "jpgx_pixels_gpu_any_workspace_size", "jpgx_pixels_gpu_any",
    "jpgx_jfif_decode_gpu_gray_workspace_size", "jpgx_jfif_decode_gpu_gray", "jpgx_pixels_gpu_gray",
    "jpgx_workspace_size_any", "jpgx_blocks_gpu_any", "jpgx_jfif_gpu_any_workspace_size", "jpgx_jfif_gpu_any",
    "jpgx_blocks_gpu_gray", "jpgx_jfif_gpu_gray_workspace_size", "jpgx_jfif_gpu_gray", "jpgx_guard_band_gray",
    "jpgx_scaled_size", "jpgx_pixels_gpu_scaled_workspace_size", "jpgx_pixels_gpu_scaled",
    "jpgx_pixels_gpu_gray_scaled",
]
COMPAT_EXPORTS = [
    "jpgx_new_block", "jpgx_get_value_block", "jpgx_set_value_block", "jpgx_copy_block",
    "jpgx_show_block", "jpgx_destroy_block", "jpgx_dct_block", "jpgx_quantise_block",
    "jpgx_quantise_lum", "jpgx_quantise_chr", "jpgx_scale_table_inplace", "jpgx_zig_zag_block",
    "jpgx_fill_jpgdata", "jpgx_free_jpgdata", "jpgx_dpcm", "jpgx_dpcm_dc", "jpgx_bmp_read",
    "jpgx_free", "jpgx_encode_bmp", "jpgx_jfif_bound", "jpgx_write_jfif",
    "jpgx_encode_bmp_to_jpeg", "jpgx_write_jfif_sub", "jpgx_encode_bmp_to_jpeg_ex",
    "jpgx_encode_rgb_to_jpeg", "jpgx_write_jfif_ex", "jpgx_write_jfif_opt",
    "jpgx_jfif_info_of", "jpgx_read_jfif", "jpgx_read_jfif_sub", "jpgx_pixels_host",
    "jpgx_jfif_info_of_any", "jpgx_read_jfif_any", "jpgx_read_jfif_sub_any", "jpgx_pixels_host_any",
    "jpgx_jfif_info_of_gray", "jpgx_read_jfif_gray", "jpgx_read_jfif_sub_gray", "jpgx_pixels_host_gray",
    "jpgx_write_jfif_any", "jpgx_pad_edge", "jpgx_encode_rgb_to_jpeg_any", "jpgx_write_jfif_gray",
    "jpgx_pixels_host_scaled", "jpgx_pixels_host_gray_scaled",
]


class JpgxError(RuntimeError):
    def __init__(self, rc: int, what: str):
        super().__init__(f"{what} failed: {_ERRNAMES.get(rc, rc)}")
        self.rc = rc


class Params(ctypes.Structure):
    _fields_ = [("quality", ctypes.c_int), ("sample_ratio", ctypes.c_int),
                ("flags", ctypes.c_uint), ("underflow", (ctypes.c_uint8 * 8) * 3)]


class Frames(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int),
                ("row_begin", ctypes.c_int), ("row_end", ctypes.c_int),
                ("nframes", ctypes.c_int), ("in_pitch", ctypes.c_size_t),
                ("in_frame_stride", ctypes.c_size_t), ("out_frame_stride", ctypes.c_size_t)]


ALT_LIB_PATH = os.path.join(PKG_ROOT, "lib", "libjpgx_alt.so")


def _load(path: str = LIB_PATH) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise ImportError(f"{os.path.basename(path)} not built ({path}); run __graft_entry__.build()")
    # libjpgx.so and torch both need libamdhip64.so.7 (same soname): load torch first so the
    # process has ONE HIP runtime and device pointers/streams are shared.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(path)
    vp, sz, i, u8p = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
    P, Fp = ctypes.POINTER(Params), ctypes.POINTER(Frames)
    L.jpgx_validate.argtypes = [i, i, P]
    L.jpgx_default_params.argtypes = [P, i, i, i, i]
    L.jpgx_default_params.restype = None
    L.jpgx_glibc_underflow.argtypes = [ctypes.c_longlong, ctypes.c_longlong, u8p]
    L.jpgx_glibc_underflow.restype = None
    L.jpgx_scale_table.argtypes = [i, i, vp]
    L.jpgx_guard_band.argtypes = [i, vp, vp]
    L.jpgx_workspace_size.argtypes = [Fp]
    L.jpgx_workspace_size.restype = sz
    L.jpgx_blocks_gpu.argtypes = [Fp, P, vp, vp, vp, sz, vp]
    L.jpgx_blocks_gpu_ev.argtypes = [Fp, P, vp, vp, vp, sz, vp, vp]
    L.jpgx_blocks_gpu_timed.argtypes = [Fp, P, vp, vp, vp, sz, vp, vp, vp]
    L.jpgx_gen_splitmix_gpu.argtypes = [vp, sz, ctypes.c_uint64, vp]
    L.jpgx_gen_tie_gpu.argtypes = [vp, i, i, vp]
    L.jpgx_blocks.argtypes = [vp, i, i, sz, P, vp, i]
    L.jpgx_blocks_multi.argtypes = [vp, i, i, sz, P, vp, i]
    L.jpgx_stripe.argtypes = [i, i, i, ctypes.POINTER(i), ctypes.POINTER(i)]
    L.jpgx_stripe.restype = None
    L.jpgx_device_count.argtypes = []
    L.jpgx_chroma_blocks.argtypes = [i, i, i, i, ctypes.c_uint]
    L.jpgx_chroma_blocks.restype = sz
    L.jpgx_entropy_workspace_size.argtypes = [sz, sz]
    L.jpgx_entropy_workspace_size.restype = sz
    L.jpgx_entropy_stats_gpu.argtypes = [vp, sz, sz, vp, vp, vp, vp, sz, vp]
    L.jpgx_entropy_workspace_size_batch.argtypes = [sz, sz, sz]
    L.jpgx_entropy_workspace_size_batch.restype = sz
    L.jpgx_entropy_stats_gpu_batch.argtypes = [vp, sz, sz, sz, sz, vp, vp, vp, vp, sz, vp]
    L.jpgx_jfif_gpu_workspace_size.argtypes = [i, i, i, i, sz, sz]
    L.jpgx_jfif_gpu_workspace_size.restype = sz
    L.jpgx_jfif_gpu.argtypes = [vp, sz, sz, i, i, i, i, i, vp, sz, sz, vp, vp, sz, vp]
    L.jpgx_jfif_gpu_workspace_size_ex.argtypes = [i, i, i, i, sz, sz, ctypes.c_uint]
    L.jpgx_jfif_gpu_workspace_size_ex.restype = sz
    L.jpgx_jfif_gpu_ex.argtypes = [vp, sz, sz, i, i, i, i, i, ctypes.c_uint, vp, sz, sz, vp, vp, sz, vp]
    L.jpgx_jfif_decode_gpu_workspace_size.argtypes = [i, i, i, sz, sz]
    L.jpgx_jfif_decode_gpu_workspace_size.restype = sz
    L.jpgx_jfif_decode_gpu.argtypes = [vp, sz, vp, sz, i, i, i, vp, sz, vp, vp, vp, sz, vp]
    L.jpgx_jfif_decode_gpu_workspace_size_ex.argtypes = [i, i, i, sz, sz, ctypes.c_uint]
    L.jpgx_jfif_decode_gpu_workspace_size_ex.restype = sz
    L.jpgx_jfif_decode_gpu_ex.argtypes = [vp, sz, vp, sz, i, i, i, ctypes.c_uint, vp, sz, vp, vp, vp, sz, vp]
    L.jpgx_jfif_decode_sub_shape.argtypes = [vp, vp]
    L.jpgx_jfif_decode_sub_shape.restype = None
    L.jpgx_pixels_gpu_workspace_size.argtypes = [i, i, i, sz]
    L.jpgx_pixels_gpu_workspace_size.restype = sz
    L.jpgx_pixels_gpu.argtypes = [vp, sz, sz, i, i, i, vp, sz, vp, vp, sz, sz, vp, sz, vp]
    L.jpgx_jfif_qt.argtypes = [i, vp]
    L.jpgx_coded_size.argtypes = [i, i, i, ctypes.POINTER(i), ctypes.POINTER(i)]
    L.jpgx_jfif_decode_gpu_any_workspace_size.argtypes = L.jpgx_jfif_decode_gpu_workspace_size_ex.argtypes
    L.jpgx_jfif_decode_gpu_any_workspace_size.restype = sz
    L.jpgx_jfif_decode_gpu_any.argtypes = L.jpgx_jfif_decode_gpu_ex.argtypes
    L.jpgx_pixels_gpu_any_workspace_size.argtypes = L.jpgx_pixels_gpu_workspace_size.argtypes
    L.jpgx_pixels_gpu_any_workspace_size.restype = sz
    L.jpgx_pixels_gpu_any.argtypes = L.jpgx_pixels_gpu.argtypes
    L.jpgx_jfif_decode_gpu_gray_workspace_size.argtypes = [i, i, sz, sz, ctypes.c_uint]
    L.jpgx_jfif_decode_gpu_gray_workspace_size.restype = sz
    L.jpgx_jfif_decode_gpu_gray.argtypes = [vp, sz, vp, sz, i, i, ctypes.c_uint, vp, sz, vp, vp, vp, sz, vp]
    L.jpgx_pixels_gpu_gray.argtypes = [vp, sz, sz, i, i, vp, sz, vp, vp, sz, sz, i, vp]
    L.jpgx_workspace_size_any.argtypes = [Fp, P]
    L.jpgx_workspace_size_any.restype = sz
    L.jpgx_blocks_gpu_any.argtypes = L.jpgx_blocks_gpu.argtypes
    L.jpgx_jfif_gpu_any_workspace_size.argtypes = L.jpgx_jfif_gpu_workspace_size_ex.argtypes
    L.jpgx_jfif_gpu_any_workspace_size.restype = sz
    L.jpgx_jfif_gpu_any.argtypes = L.jpgx_jfif_gpu_ex.argtypes
    L.jpgx_pad_edge.argtypes = [vp, i, i, sz, i, i, vp]
    L.jpgx_blocks_gpu_gray.argtypes = [vp, sz, sz, sz, i, i, i, ctypes.c_uint, vp, sz, vp]
    L.jpgx_jfif_gpu_gray_workspace_size.argtypes = [i, i, i, sz, sz, ctypes.c_uint]
    L.jpgx_jfif_gpu_gray_workspace_size.restype = sz
    L.jpgx_jfif_gpu_gray.argtypes = [vp, sz, sz, i, i, i, i, ctypes.c_uint, vp, sz, sz, vp, vp, sz, vp]
    L.jpgx_guard_band_gray.argtypes = [i, vp, vp]
    L.jpgx_scaled_size.argtypes = [i, i, i, ctypes.POINTER(i), ctypes.POINTER(i)]
    L.jpgx_pixels_gpu_scaled_workspace_size.argtypes = [i, i, i, i, sz]
    L.jpgx_pixels_gpu_scaled_workspace_size.restype = sz
    L.jpgx_pixels_gpu_scaled.argtypes = [vp, sz, sz, i, i, i, i, vp, sz, vp, vp, sz, sz, vp, sz, vp]
    L.jpgx_pixels_gpu_gray_scaled.argtypes = [vp, sz, sz, i, i, i, vp, sz, vp, vp, sz, sz, i, vp]
    L.jpgx_version.restype = ctypes.c_char_p
    L.jpgx_host_create.argtypes = [ctypes.POINTER(vp), i, vp, i]
    L.jpgx_host_destroy.argtypes = [vp]
    L.jpgx_host_destroy.restype = None
    L.jpgx_host_blocks.argtypes = [vp, vp, i, i, sz, P, vp]
    L.jpgx_host_register.argtypes = [vp, sz]
    L.jpgx_host_unregister.argtypes = [vp]
    L.jpgx_host_release.argtypes = []
    L.jpgx_host_release.restype = None
    return L


lib = _load()
_alt = None


def alt_library() -> ctypes.CDLL:
    """The TEST-ONLY cross-check library (lib/libjpgx_alt.so), loaded on first use: the same C
    ABI, with csrc/jpgx_device.hip calling the second implementation (csrc/jpgx_kernels.hip,
    linked into this library only: k_xform for 4:4:4, k_xform + k_chroma for true 4:2:x) where
    the product calls the MFMA kernels.  Tests swap it in for `lib` to run every parity check on
    the second implementation; the product never loads it."""
    global _alt
    if _alt is None:
        _alt = _load(ALT_LIB_PATH)
    return _alt


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise JpgxError(rc, what)


def version() -> str:
    return lib.jpgx_version().decode()


def device_count() -> int:
    return lib.jpgx_device_count()


def glibc_underflow(n_pixels: int, bmp_file_size: int | None = None) -> bytes:
    if bmp_file_size is None:
        bmp_file_size = 54 + 3 * n_pixels
    out = (ctypes.c_uint8 * 8)()
    lib.jpgx_glibc_underflow(n_pixels, bmp_file_size, ctypes.cast(out, ctypes.c_void_p))
    return bytes(out)


def default_params(width: int, height: int, quality: int, sample_ratio: int = 0,
                   underflow=None, flags: int = 0) -> Params:
    """underflow: None (glibc default), 8 bytes (same for all planes) or [3][8] per plane."""
    p = Params()
    lib.jpgx_default_params(ctypes.byref(p), width, height, quality, sample_ratio)
    if underflow is not None:
        u = np.asarray(list(underflow) if isinstance(underflow, (bytes, bytearray))
                       else underflow, np.uint8)
        u = np.tile(u, (3, 1)) if u.shape == (8,) else u.reshape(3, 8)
        for k in range(3):
            for x in range(8):
                p.underflow[k][x] = int(u[k, x])
    p.flags = flags
    return p


def validate(width: int, height: int, params: Params) -> int:
    return lib.jpgx_validate(width, height, ctypes.byref(params))


def scale_table(which: int, quality: int) -> np.ndarray:
    out = np.zeros((8, 8), np.int32)
    _check(lib.jpgx_scale_table(which, quality, out.ctypes.data), "jpgx_scale_table")
    return out


def guard_band(quality: int) -> tuple[np.ndarray, np.ndarray]:
    w = np.zeros((3, 64), np.float32)
    lim = np.zeros((3, 64), np.float32)
    _check(lib.jpgx_guard_band(quality, w.ctypes.data, lim.ctypes.data), "jpgx_guard_band")
    return w, lim


def guard_band_gray(quality: int) -> tuple[np.ndarray, np.ndarray]:
    """jpgx_guard_band_gray: (scale, lim) float32 [64] of the one-channel forward path, [v * 8 + u]."""
    w = np.zeros(64, np.float32)
    lim = np.zeros(64, np.float32)
    _check(lib.jpgx_guard_band_gray(quality, w.ctypes.data, lim.ctypes.data), "jpgx_guard_band_gray")
    return w, lim


def stripe(block_rows: int, nshards: int, k: int) -> tuple[int, int]:
    a, b = ctypes.c_int(), ctypes.c_int()
    lib.jpgx_stripe(block_rows, nshards, k, ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def frames(width: int, height: int, nframes: int = 1, rows: tuple[int, int] | None = None,
           in_pitch: int | None = None, in_frame_stride: int | None = None,
           out_frame_stride: int | None = None) -> Frames:
    r0, r1 = rows if rows is not None else (0, height // 8)
    fr = Frames()
    fr.width, fr.height, fr.row_begin, fr.row_end, fr.nframes = width, height, r0, r1, nframes
    fr.in_pitch = in_pitch if in_pitch is not None else width * 3
    fr.in_frame_stride = in_frame_stride if in_frame_stride is not None else fr.in_pitch * height
    nb = (r1 - r0) * (width // 8)
    fr.out_frame_stride = out_frame_stride if out_frame_stride is not None else 3 * nb * 64
    return fr


def workspace_size(fr: Frames) -> int:
    return lib.jpgx_workspace_size(ctypes.byref(fr))


# ---- torch (device-memory) helpers -------------------------------------------------------
def _stream_ptr(stream) -> int:
    import torch
    if stream is None:
        stream = torch.cuda.current_stream()
    return stream.cuda_stream


def blocks_gpu(fr: Frames, params: Params, d_rgb, d_out, d_ws, stream=None,
               event_between=None, kernel_events=None) -> None:
    """Launch the hot path on device tensors (uint8 input, int16 output, uint8 workspace).
    d_rgb must point at pixel (0, 8*row_begin) of frame 0 (pass a tensor view or an int).
    event_between: a torch.cuda.Event recorded right after the transform kernel (it must have
    been recorded once already so that its handle exists).
    kernel_events: (start, stop) torch.cuda.Events (timing-enabled, recorded once already) that
    jpgx_blocks_gpu_timed sets to the transform kernel's own begin / end."""
    def ptr(t):
        return t if isinstance(t, int) else t.data_ptr()
    ws_bytes = d_ws.numel() if hasattr(d_ws, "numel") else workspace_size(fr)
    if kernel_events is not None:                 # (start, stop): the kernel's own interval
        e0, e1 = (e.cuda_event for e in kernel_events)
        _check(lib.jpgx_blocks_gpu_timed(ctypes.byref(fr), ctypes.byref(params), ptr(d_rgb), ptr(d_out),
                                         ptr(d_ws), ws_bytes, _stream_ptr(stream), e0, e1),
               "jpgx_blocks_gpu_timed")
        return
    ev = event_between.cuda_event if event_between is not None else None
    _check(lib.jpgx_blocks_gpu_ev(ctypes.byref(fr), ctypes.byref(params), ptr(d_rgb),
                                  ptr(d_out), ptr(d_ws), ws_bytes, _stream_ptr(stream), ev),
           "jpgx_blocks_gpu")


def gen_splitmix_gpu(d_dst, seed: int, nbytes: int | None = None, stream=None) -> None:
    n = d_dst.numel() if nbytes is None else nbytes
    _check(lib.jpgx_gen_splitmix_gpu(d_dst.data_ptr(), n, seed, _stream_ptr(stream)),
           "jpgx_gen_splitmix_gpu")


def gen_tie_gpu(d_dst, width: int, height: int, stream=None) -> None:
    _check(lib.jpgx_gen_tie_gpu(d_dst.data_ptr(), width, height, _stream_ptr(stream)),
           "jpgx_gen_tie_gpu")


def chroma_blocks(width: int, row_begin: int, row_end: int, sample_ratio: int = 0,
                  flags: int = 0) -> int:
    """Chroma blocks per channel of a stripe (== luma blocks unless FLAG_SUBSAMPLE)."""
    return int(lib.jpgx_chroma_blocks(width, row_begin, row_end, sample_ratio, flags))


def coded_size(width: int, height: int, sample_ratio: int = 0) -> tuple[int, int]:
    """jpgx_coded_size: (width, height) rounded up to the MCU of sample_ratio -- the frame a file of
    that size codes, and the one its coefficients are of (nb = (cw // 8) * (ch // 8))."""
    cw, ch = ctypes.c_int(), ctypes.c_int()
    _check(lib.jpgx_coded_size(width, height, sample_ratio, ctypes.byref(cw), ctypes.byref(ch)), "jpgx_coded_size")
    return cw.value, ch.value


SCALES = (1, 2, 4, 8)


def _scale_arg(fn: str, scale) -> int:
    """scale as an int, one of SCALES"""
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or int(scale) not in SCALES:
        raise ValueError(f"{fn}: scale must be 1, 2, 4 or 8")
    return int(scale)


def scaled_size(width: int, height: int, scale: int) -> tuple[int, int]:
    """jpgx_scaled_size: (ceil(width / scale), ceil(height / scale)), the size of a decode at 1 / scale
    (scale 1, 2, 4 or 8; width and height 1 .. 65535)."""
    scale = _scale_arg("scaled_size", scale)
    ow, oh = ctypes.c_int(), ctypes.c_int()
    if lib.jpgx_scaled_size(width, height, scale, ctypes.byref(ow), ctypes.byref(oh)):
        raise ValueError("scaled_size: width and height must be 1 .. 65535")
    return ow.value, oh.value


def _frame(fn: str, width: int, height: int, sample_ratio: int, flags: int | None = None, d_coef=None,
           whole_blocks: bool = False, any_size: bool = False):
    """(nb, nbc, int16 elements per frame, elements between frames) of a frame's coefficients,
    Y [nb][64] | Cb [nbc][64] | Cr [nbc][64].  flags None: a coded frame (csrc/jx_frame.h), its
    geometry checked and its chroma subsampled as sample_ratio says; else the forward path's output
    under `flags`.  d_coef ([nframes][...]): every frame must be contiguous and hold that much
    (whole_blocks: and be laid out as the JFIF coder needs it); without it the fourth value is None.
    any_size: width and height are a file's, any 1 .. 65535; the counts are its coded frame's."""
    if any_size:
        if sample_ratio not in (0, 1, 2) or not (0 < width < 65536 and 0 < height < 65536):
            raise ValueError(f"{fn}: bad geometry or sample_ratio")
        width, height = coded_size(width, height, sample_ratio)
    if flags is None:
        if sample_ratio not in (0, 1, 2) or width <= 0 or height <= 0 or width % 8 or height % 8:
            raise ValueError(f"{fn}: bad geometry or sample_ratio")
        flags = FLAG_SUBSAMPLE if sample_ratio else 0
    nb = (width // 8) * (height // 8)
    nbc = chroma_blocks(width, 0, height // 8, sample_ratio, flags)
    per_frame = (nb + 2 * nbc) * 64
    if d_coef is None:
        return nb, nbc, per_frame, None
    return nb, nbc, per_frame, _coef_stride(fn, d_coef, per_frame, "nb + 2 nbc", whole_blocks)


def _coef_stride(fn: str, d_coef, per_frame: int, blocks: str, whole_blocks: bool = False) -> int:
    """int16 elements between the frames of d_coef ([nframes][...]), each of which must be contiguous and
    hold per_frame elements (`blocks` in the refusal), and with whole_blocks be laid out as the JFIF coder
    needs it"""
    if not d_coef[0].is_contiguous() or d_coef[0].numel() < per_frame:
        raise ValueError(f"{fn}: each frame must be contiguous and hold {blocks} blocks")
    stride = int(d_coef.stride(0)) if d_coef.shape[0] > 1 else int(d_coef[0].numel())
    if whole_blocks and (d_coef.data_ptr() % 16 or stride % 64):
        raise ValueError(f"{fn}: 16-byte aligned frames, a stride of whole blocks")
    return stride


# ---- the argument rules of the device entry points, each written once; fn: the public function's name
def _device_tensor(t, dtype=None, contiguous: bool = False) -> bool:
    """t is a torch tensor on a GPU (of dtype; contiguous)"""
    import torch
    return (isinstance(t, torch.Tensor) and t.is_cuda and (dtype is None or t.dtype == dtype)
            and (not contiguous or t.is_contiguous()))


def _files_batch(fn: str, d_files, lens):
    """(nf, cap, fstride) of a batch of files in device memory, d_files uint8 [nf][cap] and lens int64 [nf]:
    bytes per file and bytes between files.  Files that overlap, a stride below cap, are the caller's to
    refuse: a bad geometry is reported before them."""
    import torch
    for name, t, dt in (("d_files", d_files, torch.uint8), ("lens", lens, torch.int64)):
        if not _device_tensor(t):
            raise ValueError(f"{fn}: {name} must be a device tensor")
        if t.dtype != dt:
            raise ValueError(f"{fn}: {name} must be {dt}")
    if d_files.dim() != 2 or lens.dim() != 1 or lens.shape[0] != d_files.shape[0] or d_files.shape[0] == 0:
        raise ValueError(f"{fn}: d_files [nframes][cap] and lens [nframes]")
    if d_files.stride(1) != 1 or not lens.is_contiguous() or d_files.shape[1] == 0:
        raise ValueError(f"{fn}: each file must be contiguous")
    nf, cap = int(d_files.shape[0]), int(d_files.shape[1])
    return nf, cap, int(d_files.stride(0)) if nf > 1 else cap


def _qt_stride(fn: str, d_qt, nf: int, size: int) -> int:
    """uint16 elements between the frames' tables of `size` (128: [2][64], 64: [64]); 0: one for the batch"""
    if d_qt.numel() not in (size, size * nf):
        one = "[2][64]" if size == 128 else "[64]"
        raise ValueError(f"{fn}: d_qt must be {one} or [nframes]{one}")
    return 0 if d_qt.numel() == size else size


def _status_arg(fn: str, status, nf: int):
    """the pointer a pixel entry point takes for `status`, int32 [nf] or None"""
    import torch
    if status is None:
        return None
    if (not isinstance(status, torch.Tensor) or status.dtype != torch.int32 or status.numel() != nf
            or not status.is_contiguous()):
        raise ValueError(f"{fn}: status must be a contiguous int32 [nframes] tensor")
    return status.data_ptr()


def _pitch_out(fn: str, pitch, out, nf: int, width: int, height: int, bpp: int, bpp_name: str, packed: bool, dev):
    """(pitch, out) of a pixel entry point: bytes between pixel rows, a multiple of 8 and at least
    bpp * width (bpp_name in the refusal), by default that many (packed) or that rounded up to 8; out, the
    caller's buffer of nf * height * pitch bytes or a fresh one on dev"""
    import torch
    if pitch is None:
        pitch = bpp * width if packed else (bpp * width + 7) // 8 * 8
    pitch = int(pitch)
    if pitch < bpp * width or pitch % 8:
        raise ValueError(f"{fn}: pitch must be a multiple of 8 and at least {bpp_name} * width")
    if out is None:
        out = torch.empty(nf * height * pitch, dtype=torch.uint8, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or not out.is_contiguous()
          or out.numel() != nf * height * pitch):
        raise ValueError(f"{fn}: out must be a contiguous uint8 buffer of nframes * H * pitch bytes")
    return pitch, out


def _workspace(need: int, dev, stream=None):
    """an entry point's own workspace of `need` bytes, kept until `stream` is past it"""
    import torch
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    if stream is not None:
        ws.record_stream(stream)
    return ws


def _upload_files(files, dev):
    """host files -> (d_files uint8 [n][cap], lens int64 [n]) on dev; cap: the longest file's length"""
    import torch
    cap = max(len(f) for f in files)
    host = np.zeros((len(files), cap), np.uint8)
    for k, f in enumerate(files):
        host[k, :len(f)] = np.frombuffer(f, np.uint8)
    return torch.from_numpy(host).to(dev), torch.tensor([len(f) for f in files], dtype=torch.int64, device=dev)


def entropy_stats_gpu(d_coef, nb_y: int, nb_c: int, carry=None, stream=None):
    """(dc int32 [nb_y + 2 nb_c], hist uint32 [4][257]) device tensors: the reference's dpcm and
    huffman_encode frequency pass over d_coef (torch int16 tensor, Y|Cb|Cr blocks)."""
    import torch
    dev = d_coef.device
    dc = torch.empty(nb_y + 2 * nb_c, dtype=torch.int32, device=dev)
    hist = torch.empty((4, 257), dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.jpgx_entropy_workspace_size(nb_y, nb_c)), 8), dtype=torch.uint8,
                     device=dev)
    cy = None
    if carry is not None:
        cy = (ctypes.c_int32 * 3)(*[int(x) for x in carry])
    _check(lib.jpgx_entropy_stats_gpu(d_coef.data_ptr(), nb_y, nb_c,
                                      ctypes.cast(cy, ctypes.c_void_p) if cy is not None else None,
                                      dc.data_ptr(), hist.data_ptr(), ws.data_ptr(), ws.numel(),
                                      _stream_ptr(stream)), "jpgx_entropy_stats_gpu")
    return dc, hist


def entropy_stats_gpu_batch(d_coef, nb_y: int, nb_c: int, stream=None):
    """The same over a frame batch d_coef [nframes][>= nb_y + 2 nb_c][64] (int16; each frame
    contiguous, frames d_coef.stride(0) elements apart, e.g. a slice of a padded batch):
    (dc int32 [nframes][nb_y + 2 nb_c], hist uint32 [nframes][4][257]), every frame from the image
    start."""
    import torch
    if d_coef.dtype != torch.int16 or d_coef.dim() < 2:
        raise ValueError("entropy_stats_gpu_batch: d_coef must be an int16 [nframes][...] tensor")
    if not d_coef[0].is_contiguous() or d_coef[0].numel() < (nb_y + 2 * nb_c) * 64:
        raise ValueError("entropy_stats_gpu_batch: each frame must be contiguous and hold nb_y + 2 nb_c blocks")
    if d_coef.data_ptr() % 16 or d_coef.stride(0) % 64:
        raise ValueError("entropy_stats_gpu_batch: 16-byte aligned frames, a stride of whole blocks")
    dev = d_coef.device
    nf = d_coef.shape[0]
    dc = torch.empty((nf, nb_y + 2 * nb_c), dtype=torch.int32, device=dev)
    hist = torch.empty((nf, 4, 257), dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.jpgx_entropy_workspace_size_batch(nb_y, nb_c, nf)), 8),
                     dtype=torch.uint8, device=dev)
    _check(lib.jpgx_entropy_stats_gpu_batch(d_coef.data_ptr(), d_coef.stride(0), nf, nb_y, nb_c, None,
                                            dc.data_ptr(), hist.data_ptr(), ws.data_ptr(), ws.numel(),
                                            _stream_ptr(stream)), "jpgx_entropy_stats_gpu_batch")
    return dc, hist


def jfif_gpu(d_coef, width: int, height: int, quality: int, sample_ratio: int = 0,
             restart_rows: int = -1, cap: int | None = None, stream=None, optimize: bool = False,
             any_size: bool = False):
    """The JFIF files of a frame batch, coded on the device (jpgx_jfif_gpu): d_coef int16
    [nframes][...] as encode_blocks / blocks_gpu write each frame ([3][nb][64], or Y | Cb | Cr with
    FLAG_SUBSAMPLE for sample_ratio 1, 2; each frame contiguous, frames d_coef.stride(0) elements
    apart) -> (out uint8 [nframes][cap], lens int64 [nframes]): frame f's file is
    out[f, :lens[f]], byte for byte compat.write_jfif_ex(coef, ..., restart_rows, nthreads=1)
    (restart_rows -1: one MCU row per interval).  cap: bytes per frame (default as
    compat.write_jfif_ex); when a frame needs more, one retry with the capacity the library
    reports (that reads lens back, a synchronisation).  optimize: JFIF_OPTIMIZE, every frame coded
    with Huffman tables built from its own symbols (jpgx_jfif_gpu_ex), byte for byte
    compat.write_jfif_ex(..., optimize=True).  any_size: jpgx_jfif_gpu_any -- width and height are the
    file's own, any 1 .. 65535, d_coef holds the coded frames (encode_blocks(any_size=True)); byte for
    byte compat.write_jfif_ex(..., any_size=True)."""
    return _jfif_gpu("jfif_gpu", d_coef, width, height, quality, restart_rows, cap, stream, optimize,
                     sample_ratio=sample_ratio, any_size=any_size)


def jfif_gpu_gray(d_coef, width: int, height: int, quality: int, restart_rows: int = -1, cap: int | None = None,
                  stream=None, optimize: bool = False):
    """jfif_gpu for one-component (grayscale) files (jpgx_jfif_gpu_gray): d_coef int16 [nframes][>= nb][64]
    as encode_blocks_gray writes it, nb = ceil(W / 8) * ceil(H / 8), width and height any 1 .. 65535 ->
    (out uint8 [nframes][cap], lens int64 [nframes]); frame f's file is byte for byte
    compat.write_jfif_gray(coef, ..., restart_rows, nthreads=1) (restart_rows counts block rows; -1: one).
    cap, the retry on capacity, stream and optimize as jfif_gpu's."""
    return _jfif_gpu("jfif_gpu_gray", d_coef, width, height, quality, restart_rows, cap, stream, optimize, gray=True)


def _jfif_gpu(fn: str, d_coef, width, height, quality, restart_rows, cap, stream, optimize, sample_ratio: int = 0,
              any_size: bool = False, gray: bool = False):
    """jfif_gpu and, with gray, jfif_gpu_gray: the library's call takes the frame's geometry as (width, height,
    quality, sample_ratio), a one-component frame's as (width, height, quality); a frame holds _frame's blocks
    or _gray_blocks'"""
    import torch
    if not _device_tensor(d_coef):
        raise ValueError(f"{fn}: d_coef must be a device tensor")
    if d_coef.dtype != torch.int16 or d_coef.dim() < 2:
        raise ValueError(f"{fn}: d_coef must be an int16 [nframes][...] tensor")
    if gray:
        per_frame = _gray_blocks(fn, width, height) * 64
        fstride = _coef_stride(fn, d_coef, per_frame, "nb", whole_blocks=True)
        size_fn, code_fn = lib.jpgx_jfif_gpu_gray_workspace_size, lib.jpgx_jfif_gpu_gray
        size_geometry, geometry = (width, height), (width, height, quality)
    else:
        _, _, per_frame, fstride = _frame(fn, width, height, sample_ratio, d_coef=d_coef, whole_blocks=True,
                                          any_size=any_size)
        size_fn = lib.jpgx_jfif_gpu_any_workspace_size if any_size else lib.jpgx_jfif_gpu_workspace_size_ex
        code_fn = lib.jpgx_jfif_gpu_any if any_size else lib.jpgx_jfif_gpu_ex
        size_geometry, geometry = (width, height, sample_ratio), (width, height, quality, sample_ratio)
    nf = d_coef.shape[0]
    dev = d_coef.device
    cap = int(cap) if cap else max(1 << 20, per_frame // 2)
    jflags = JFIF_OPTIMIZE if optimize else 0
    for attempt in range(2):
        out = torch.empty((nf, cap), dtype=torch.uint8, device=dev)
        lens = torch.empty(nf, dtype=torch.int64, device=dev)
        need = int(size_fn(*size_geometry, restart_rows, nf, cap, jflags))
        ws = _workspace(need, dev)          # synchronised below: nothing to keep it for
        _check(code_fn(d_coef.data_ptr(), fstride, nf, *geometry, restart_rows, jflags, out.data_ptr(), cap, cap,
                       lens.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(stream)), "jpgx_" + fn)
        if stream is not None:
            stream.synchronize()
        host = lens.cpu()
        if attempt or not bool((host < 0).any()):
            break
        cap = int((host[host < 0] & ((1 << 62) - 1)).max())   # bit 63: the capacity that suffices
    return out, lens


def encode_jpeg(rgb, quality: int, sample_ratio: int = 0, flags: int = 0, restart_rows: int = -1,
                optimize: bool = False, any_size: bool = False, gray: bool = False) -> bytes:
    """One device image (H, W, 3 uint8 torch tensor on a GPU) -> its JFIF file: encode_blocks, then
    jfif_gpu, then a device-to-host copy of the file's bytes.  With FLAG_SUBSAMPLE and sample_ratio
    1 / 2 the file is 4:2:2 / 4:2:0, otherwise 4:4:4.  optimize: per-image Huffman tables (jfif_gpu).  any_size: an image of
    any width and height, 1 .. 65535 each: the file states H x W and codes the coded frame of its own
    sampling (pad_edge; the forward path gets the file's ratio, 0 without FLAG_SUBSAMPLE, so that both
    agree on the MCU); decode_jpeg(..., any_size=True) reads it back.  gray: the image is one channel,
    (H, W) uint8 of any size, and the file a one-component one (encode_blocks_gray, jfif_gpu_gray; flags:
    0 or FLAG_FORCE_EXACT, sample_ratio unused); decode_jpeg(..., gray=True) reads it back.  The default
    refuses a 2-D tensor."""
    import torch
    if not _device_tensor(rgb):
        raise ValueError("encode_jpeg: rgb must be a device tensor")
    if gray:
        if rgb.dim() != 2:
            raise ValueError("encode_jpeg: gray=True takes an (H, W) uint8 tensor")
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
        coef = encode_blocks_gray(rgb, quality, flags=flags)
        out, lens = jfif_gpu_gray(coef.reshape(1, -1), W, H, quality, restart_rows, optimize=optimize)
    else:
        if rgb.dim() != 3:
            raise ValueError("encode_jpeg: rgb must be (H, W, 3) uint8; a one-channel image takes gray=True")
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
        sub = sample_ratio if flags & FLAG_SUBSAMPLE else 0
        coef = encode_blocks(rgb, quality, sub if any_size else sample_ratio,
                             flags=flags if sub else flags & ~FLAG_SUBSAMPLE, any_size=any_size)
        out, lens = jfif_gpu(coef.reshape(1, -1), W, H, quality, sub, restart_rows, optimize=optimize, any_size=any_size)
    n = int(lens[0])
    if n < 0:
        raise JpgxError(EARG, "jpgx_jfif_gpu (capacity)")
    return out[0, :n].cpu().numpy().tobytes()


def jfif_decode_sub_shape() -> tuple[int, int]:
    """(bytes per subsequence, subsequences per tile) of the decoder that works inside a restart
    interval (jpgx_jfif_decode_sub_shape)."""
    s, t = ctypes.c_uint32(), ctypes.c_uint32()
    lib.jpgx_jfif_decode_sub_shape(ctypes.addressof(s), ctypes.addressof(t))
    return s.value, t.value


def jfif_decode_gpu(d_files, lens, width: int, height: int, sample_ratio: int = 0, stream=None,
                    subinterval: bool = False, any_size: bool = False):
    """The coefficients of a batch of baseline JFIF files in device memory (jpgx_jfif_decode_gpu;
    entropy decoding only): d_files uint8 [nframes][cap] and lens int64 [nframes] as jfif_gpu returns
    them, every file of the stated width, height and sample_ratio ->
    (coef int16 [nframes][nb + 2 nbc][64], qt uint16 [nframes][2][64], status int32 [nframes]), all
    on the device.  Frame f's layout is encode_blocks' ([3][nb][64] viewed as [3 nb][64] for
    sample_ratio 0, Y | Cb | Cr for 1, 2); status[f] is 0, EJFIF_HEADER or EJFIF_SCAN, what
    compat.read_jfif reports for the same bytes; a frame with a nonzero status has unspecified
    coefficients.  Nothing is copied to the host and nothing waits.  subinterval:
    JFIF_DECODE_SUBINTERVAL, a workgroup per restart interval instead of a lane (jpgx_jfif_decode_gpu_ex;
    DESIGN.md 4.8a): the same outputs, faster where intervals are long or few.  any_size:
    jpgx_jfif_decode_gpu_any -- width and height are the files' own, any 1 .. 65535, and nb, nbc are
    the coded frame's (coded_size); statuses and coefficients are compat.read_jfif(any_size=True)'s."""
    return _jfif_decode("jfif_decode_gpu", d_files, lens, width, height, stream, subinterval,
                        sample_ratio=sample_ratio, any_size=any_size)


def _gray_blocks(fn: str, width: int, height: int) -> int:
    """the blocks a one-component file of width x height codes: ceil(W / 8) * ceil(H / 8)"""
    if not (0 < width < 65536 and 0 < height < 65536):
        raise ValueError(f"{fn}: bad geometry")
    return ((width + 7) // 8) * ((height + 7) // 8)


def jfif_decode_gpu_gray(d_files, lens, width: int, height: int, stream=None, subinterval: bool = False):
    """jfif_decode_gpu for one-component (grayscale) baseline files (jpgx_jfif_decode_gpu_gray): d_files
    uint8 [nframes][cap], lens int64 [nframes], every file of the stated width and height, any
    1 .. 65535 -> (coef int16 [nframes][nb][64] with nb = ceil(W / 8) * ceil(H / 8), qt uint16
    [nframes][64], status int32 [nframes]), all on the device; status[f], the coefficients and the table
    are compat.read_jfif_gray's for the same bytes, and a three-component file has EJFIF_HEADER.
    Nothing is copied to the host and nothing waits.  subinterval: as jfif_decode_gpu's."""
    return _jfif_decode("jfif_decode_gpu_gray", d_files, lens, width, height, stream, subinterval, gray=True)


def _jfif_decode(fn: str, d_files, lens, width, height, stream, subinterval, sample_ratio: int = 0,
                 any_size: bool = False, gray: bool = False):
    """jfif_decode_gpu and, with gray, jfif_decode_gpu_gray: the library's call takes the frame's geometry as
    (width, height, sample_ratio), a one-component frame's as (width, height)"""
    import torch
    nf, cap, fstride = _files_batch(fn, d_files, lens)
    if gray:
        nblk, geometry = _gray_blocks(fn, width, height), (width, height)
        size_fn, decode_fn = lib.jpgx_jfif_decode_gpu_gray_workspace_size, lib.jpgx_jfif_decode_gpu_gray
    else:
        nb, nbc, _, _ = _frame(fn, width, height, sample_ratio, any_size=any_size)
        nblk, geometry = nb + 2 * nbc, (width, height, sample_ratio)
        size_fn = lib.jpgx_jfif_decode_gpu_any_workspace_size if any_size else lib.jpgx_jfif_decode_gpu_workspace_size_ex
        decode_fn = lib.jpgx_jfif_decode_gpu_any if any_size else lib.jpgx_jfif_decode_gpu_ex
    if fstride < cap:
        raise ValueError(f"{fn}: overlapping files")
    dev = d_files.device
    coef = torch.empty((nf, nblk, 64), dtype=torch.int16, device=dev)
    qt = torch.empty((nf, 64) if gray else (nf, 2, 64), dtype=torch.uint16, device=dev)
    status = torch.empty(nf, dtype=torch.int32, device=dev)
    dflags = JFIF_DECODE_SUBINTERVAL if subinterval else 0
    ws = _workspace(int(size_fn(*geometry, nf, fstride, dflags)), dev, stream)
    _check(decode_fn(d_files.data_ptr(), fstride, lens.data_ptr(), nf, *geometry, dflags, coef.data_ptr(), nblk * 64,
                     qt.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(stream)), "jpgx_" + fn)
    return coef, qt, status


def decode_jpeg_coefficients(data: bytes, device, subinterval: bool = False, any_size: bool = False,
                             gray: bool = False):
    """One baseline JFIF file in host memory -> its coefficients on `device`: the header walk on the
    host for the geometry (compat.jfif_info), one host-to-device copy of the bytes, jfif_decode_gpu.
    Returns compat.read_jfif's dict with device tensors: coef int16 ([3][nb][64] for 4:4:4,
    [nb + 2 nbc][64] otherwise), qt uint16 [2][64], width, height, sample_ratio, restart_interval.
    Raises JpgxError on a nonzero status (that reads the status back, a synchronisation).
    subinterval, any_size: as jfif_decode_gpu's (any_size: the coefficients are the coded frame's,
    width and height the file's).  gray: the file is a one-component one of any size
    (jfif_decode_gpu_gray): coef [nb][64], qt [64], sample_ratio 0, restart_interval in blocks."""
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("decode_jpeg_coefficients: device must be a GPU")
    info, geometry, decode, _, what = _decode_path(data, subinterval, any_size, gray)
    d_files, lens = _upload_files([bytes(data)], dev)
    coef, qt, status = decode(d_files, lens, *geometry)
    _check(int(status[0]), what)
    out = coef[0].reshape(3, -1, 64) if info["sample_ratio"] == 0 and not gray else coef[0]
    return dict(coef=out, qt=qt[0], width=info["width"], height=info["height"],
                sample_ratio=info["sample_ratio"], restart_interval=info["restart_interval"])


def _decode_path(data, subinterval: bool, any_size: bool, gray: bool):
    """decode_jpeg's and decode_jpeg_coefficients' way for their kind of file: (data's header as a dict; the
    geometry the next two take after their tensors; the decoder; the pixel call; a nonzero status' name)"""
    from functools import partial
    from . import compat
    info = compat.jfif_info_gray(data) if gray else compat.jfif_info(data, any_size=any_size)
    if gray:
        return (info, (info["width"], info["height"]), partial(jfif_decode_gpu_gray, subinterval=subinterval),
                pixels_gpu_gray, "jpgx_jfif_decode_gpu_gray")
    return (info, (info["width"], info["height"], info["sample_ratio"]),
            partial(jfif_decode_gpu, subinterval=subinterval, any_size=any_size), partial(pixels_gpu, any_size=any_size),
            "jpgx_jfif_decode_gpu")


def jfif_qt(quality: int) -> np.ndarray:
    """jpgx_jfif_qt: uint16 [2][64], the two tables the JFIF writers put into DQT for `quality`
    (the divisors the forward path applied; zig-zag order)."""
    qt = np.zeros((2, 64), np.uint16)
    _check(lib.jpgx_jfif_qt(quality, qt.ctypes.data), "jpgx_jfif_qt")
    return qt


def pixels_gpu(d_coef, width: int, height: int, sample_ratio: int = 0, d_qt=None, status=None, out=None,
               pitch: int | None = None, stream=None, any_size: bool = False, scale: int = 1):
    """The pixels of a batch of coefficient frames (jpgx_pixels_gpu): d_coef int16
    [nframes][...] as jfif_decode_gpu returns it (each frame contiguous, frames d_coef.stride(0)
    elements apart), d_qt uint16 [nframes][2][64] (one pair per frame) or [2][64] (one for the batch),
    status int32 [nframes] or None: a frame with a nonzero status is skipped, its output untouched.
    Returns uint8 [nframes][H][W][3] on the device: a fresh tensor, or, with a pitch (bytes between
    pixel rows, a multiple of 8, at least 3 W), a view of the padded buffer; out: a contiguous uint8
    buffer of nframes * H * pitch bytes to use instead of a fresh one.  Nothing is copied to the host
    and nothing waits.  any_size: jpgx_pixels_gpu_any -- d_coef holds the coded frame's coefficients
    (jfif_decode_gpu(any_size=True)), width and height are the visible frame's, any 1 .. 65535; the
    default pitch is 3 W rounded up to 8, and only bytes [0, 3 W) of the H rows are written.  scale 2, 4
    or 8: jpgx_pixels_gpu_scaled -- libjpeg's decode at 1 / scale of the size, uint8
    [nframes][oh][ow][3] with (ow, oh) = scaled_size(W, H, scale); d_coef, width and height as with
    any_size, whether or not it is set; pitch at least 3 ow, by default that rounded up to 8."""
    return _pixels("pixels_gpu", d_coef, width, height, d_qt, status, out, pitch, stream, sample_ratio=sample_ratio,
                   any_size=any_size, scale=scale)


def pixels_gpu_gray(d_coef, width: int, height: int, d_qt, status=None, channels: int = 1, out=None,
                    pitch: int | None = None, stream=None, scale: int = 1):
    """The pixels of a batch of one-component frames (jpgx_pixels_gpu_gray): d_coef int16
    [nframes][>= nb][64] as jfif_decode_gpu_gray returns it, d_qt uint16 [nframes][64] (a table per
    frame) or [64] (one for the batch), status as pixels_gpu's.  Returns uint8 [nframes][H][W]
    (channels 1) or [nframes][H][W][3] (channels 3, R = G = B) on the device: libjpeg's default
    decoder's pixels.  pitch (bytes between pixel rows, a multiple of 8, at least channels * W; default:
    channels * W rounded up to 8) and out as pixels_gpu's.  Nothing is copied to the host and nothing waits.
    scale 2, 4 or 8: jpgx_pixels_gpu_gray_scaled -- the decode at 1 / scale of the size, [nframes][oh][ow]
    (or [...][3]) with (ow, oh) = scaled_size(W, H, scale), the pitch measured against ow."""
    return _pixels("pixels_gpu_gray", d_coef, width, height, d_qt, status, out, pitch, stream, channels=channels,
                   scale=scale)


def _pixels(fn: str, d_coef, width, height, d_qt, status, out, pitch, stream, sample_ratio: int = 0,
            any_size: bool = False, channels: int | None = None, scale: int = 1):
    """pixels_gpu and, with channels, pixels_gpu_gray: a pixel is 3 bytes or `channels`, a frame holds
    _frame's blocks or _gray_blocks', its tables are 128 elements or 64, and only pixels_gpu on whole MCUs
    packs its rows by default.  scale 2, 4, 8: the _scaled entry points, a frame of any size, the output
    scaled_size's"""
    import torch
    gray = channels is not None
    scale = _scale_arg(fn, scale)
    any_size = any_size or scale > 1
    if not _device_tensor(d_coef, torch.int16) or d_coef.dim() < 2:
        raise ValueError(f"{fn}: d_coef must be an int16 [nframes][...] device tensor")
    if not _device_tensor(d_qt, torch.uint16, contiguous=True):
        raise ValueError(f"{fn}: d_qt must be a contiguous uint16 device tensor")
    if gray and channels not in (1, 3):
        raise ValueError(f"{fn}: channels must be 1 or 3")
    nf = int(d_coef.shape[0])
    if gray:
        cstride = _coef_stride(fn, d_coef, _gray_blocks(fn, width, height) * 64, "nb")
    else:
        _, _, _, cstride = _frame(fn, width, height, sample_ratio, d_coef=d_coef, any_size=any_size)
    qstride = _qt_stride(fn, d_qt, nf, 64 if gray else 128)
    d_status = _status_arg(fn, status, nf)
    bpp = channels if gray else 3
    if scale > 1:
        ow, oh = scaled_size(width, height, scale)
        pitch, out = _pitch_out(fn, pitch, out, nf, ow, oh, bpp, "channels" if gray else "3", packed=False,
                                dev=d_coef.device)
        if gray:
            rc = lib.jpgx_pixels_gpu_gray_scaled(d_coef.data_ptr(), cstride, nf, width, height, scale, d_qt.data_ptr(),
                                                 qstride, d_status, out.data_ptr(), pitch, oh * pitch, channels,
                                                 _stream_ptr(stream))
        else:
            need = int(lib.jpgx_pixels_gpu_scaled_workspace_size(width, height, sample_ratio, scale, nf))
            ws = _workspace(need, d_coef.device, stream)
            rc = lib.jpgx_pixels_gpu_scaled(d_coef.data_ptr(), cstride, nf, width, height, sample_ratio, scale,
                                            d_qt.data_ptr(), qstride, d_status, out.data_ptr(), pitch, oh * pitch,
                                            ws.data_ptr() if need else None, need, _stream_ptr(stream))
        _check(rc, "jpgx_" + fn + "_scaled")
        px = out.view(nf, oh, pitch)[:, :, :bpp * ow]
        return px if bpp == 1 else px.unflatten(2, (ow, 3))
    pitch, out = _pitch_out(fn, pitch, out, nf, width, height, bpp, "channels" if gray else "3",
                            packed=not (gray or any_size), dev=d_coef.device)
    if gray:
        rc = lib.jpgx_pixels_gpu_gray(d_coef.data_ptr(), cstride, nf, width, height, d_qt.data_ptr(), qstride, d_status,
                                      out.data_ptr(), pitch, height * pitch, channels, _stream_ptr(stream))
    else:
        size_fn = lib.jpgx_pixels_gpu_any_workspace_size if any_size else lib.jpgx_pixels_gpu_workspace_size
        pixels_fn = lib.jpgx_pixels_gpu_any if any_size else lib.jpgx_pixels_gpu
        need = int(size_fn(width, height, sample_ratio, nf))
        ws = _workspace(need, d_coef.device, stream)
        rc = pixels_fn(d_coef.data_ptr(), cstride, nf, width, height, sample_ratio, d_qt.data_ptr(), qstride, d_status,
                       out.data_ptr(), pitch, height * pitch, ws.data_ptr() if need else None, need, _stream_ptr(stream))
    _check(rc, "jpgx_" + fn)
    px = out.view(nf, height, pitch)[:, :, :bpp * width]
    return px if bpp == 1 else px.unflatten(2, (width, 3))


def decode_jpeg(data, device, subinterval: bool = False, any_size: bool = False, gray: bool = False,
                scale: int = 1):
    """Baseline JFIF file(s) in host memory -> RGB on `device`: decode_jpeg_coefficients' header step
    on the host for the geometry, one host-to-device copy of the bytes, then jfif_decode_gpu and
    pixels_gpu on one stream; the coefficients never leave the device.  data: bytes -> uint8 [H][W][3];
    a list of files of one geometry -> [n][H][W][3].  The pixels are libjpeg's default decoder's.
    Raises JpgxError for a frame whose status is nonzero (that reads the statuses back, a
    synchronisation).  subinterval: as jfif_decode_gpu's; the choice for files without restart
    intervals, which one lane decodes otherwise.  any_size: files of any width and height (a list is
    still files of one geometry); the default refuses a size that is no multiple of the MCU.  gray:
    one-component files of any size (jfif_decode_gpu_gray, pixels_gpu_gray): uint8 [H][W], or
    [n][H][W] for a list; the default refuses such files.  scale 2, 4 or 8: the pixels of libjpeg's
    decode at 1 / scale of the size (scaled_size(W, H, scale)), from the same coefficients; files of any
    width and height, whether or not any_size is set."""
    import torch
    scale = _scale_arg("decode_jpeg", scale)
    any_size = any_size or scale > 1
    single = isinstance(data, (bytes, bytearray, memoryview))
    files = [bytes(data)] if single else [bytes(d) for d in data]
    if not files:
        raise ValueError("decode_jpeg: no files")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("decode_jpeg: device must be a GPU")
    _, geometry, decode, pixels, what = _decode_path(files[0], subinterval, any_size, gray)
    d_files, lens = _upload_files(files, dev)
    coef, qt, status = decode(d_files, lens, *geometry)
    px = pixels(coef, *geometry, d_qt=qt, status=status, scale=scale)
    for rc in status.cpu().tolist():
        _check(int(rc), what)
    return px[0] if single else px


def split_sub(out, nb: int, nbc: int):
    """(Y [nb][64], CbCr [2][nbc][64]) views of one frame's FLAG_SUBSAMPLE output."""
    return out[:nb], out[nb:nb + 2 * nbc].reshape(2, nbc, 64)


def pad_edge(rgb: np.ndarray, sample_ratio: int = 0) -> np.ndarray:
    """jpgx_pad_edge: a host image (H, W, 3 uint8) -> its coded frame (ch, cw, 3), coded_size(W, H,
    sample_ratio), by the edge rule of the encode side's any-size entry points: the last column repeated
    to the right, the last row downwards -- np.pad(rgb, ((0, ch - H), (0, cw - W), (0, 0)), mode="edge")."""
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.strides[1:] != (3, 1) or rgb.strides[0] < 3 * rgb.shape[1]:
        raise ValueError("pad_edge: rgb must be (H, W, 3) uint8 with packed pixels and top-down rows")
    H, W = rgb.shape[:2]
    cw, ch = coded_size(W, H, sample_ratio)
    out = np.empty((ch, cw, 3), np.uint8)
    _check(lib.jpgx_pad_edge(rgb.ctypes.data, W, H, rgb.strides[0], cw, ch, out.ctypes.data), "jpgx_pad_edge")
    return out


def encode_blocks(rgb, quality: int, sample_ratio: int = 0, underflow: bytes | None = None,
                  flags: int = 0, device=None, any_size: bool = False, stream=None):
    """Convenience: one image (H,W,3 uint8 torch tensor on a GPU, or numpy on the host) ->
    int16 [3][nb][64] (with FLAG_SUBSAMPLE: [nb + 2 nbc][64], see split_sub).  Device tensors
    stay on the device; numpy goes through jpgx_blocks.  any_size: W and H are any 1 .. 65535; the
    result is the plain call's for the image's coded frame (pad_edge; coded_size(W, H, sample_ratio)),
    the underflow bytes, unless given, those of the coded size.  A device tensor goes through
    jpgx_blocks_gpu_any, rows of any pitch as they are (only the pixels must be packed); numpy is padded
    on the host and takes the plain route.  stream (any_size, device tensors): the stream to launch on."""
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    if any_size:
        return _encode_blocks_any(rgb, W, H, quality, sample_ratio, underflow, flags, device, stream)
    nb, nbc, per_frame, _ = _frame("encode_blocks", W, H, sample_ratio, flags)
    shape = (nb + 2 * nbc, 64) if flags & FLAG_SUBSAMPLE else (3, nb, 64)
    if isinstance(rgb, np.ndarray):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        p = default_params(W, H, quality, sample_ratio, underflow, flags)
        out = np.empty(shape, np.int16)
        dev = 0 if device is None else int(device)
        _check(lib.jpgx_blocks(rgb.ctypes.data, W, H, W * 3, ctypes.byref(p), out.ctypes.data,
                               dev), "jpgx_blocks")
        return out
    import torch
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    p = default_params(W, H, quality, sample_ratio, underflow, flags)
    _check(validate(W, H, p), "jpgx_validate")
    fr = frames(W, H)
    fr.out_frame_stride = per_frame
    out = torch.empty(shape, dtype=torch.int16, device=rgb.device)
    ws = torch.empty(workspace_size(fr), dtype=torch.uint8, device=rgb.device)
    blocks_gpu(fr, p, rgb.contiguous(), out, ws)
    return out


def _encode_blocks_any(rgb, W, H, quality, sample_ratio, underflow, flags, device, stream):
    """encode_blocks(any_size=True)"""
    nb, nbc, per_frame, _ = _frame("encode_blocks", W, H, sample_ratio, flags, any_size=True)
    if isinstance(rgb, np.ndarray):
        return encode_blocks(pad_edge(np.ascontiguousarray(rgb, np.uint8), sample_ratio), quality, sample_ratio,
                             underflow, flags, device)
    import torch
    if not _device_tensor(rgb):
        raise ValueError("encode_blocks: rgb must be a numpy array or a device tensor")
    if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3:
        raise ValueError("encode_blocks: rgb must be (H, W, 3) uint8")
    if (W > 1 and tuple(rgb.stride()[1:]) != (3, 1)) or (H > 1 and rgb.stride(0) < 3 * W):
        rgb = rgb.contiguous()
    pitch = int(rgb.stride(0)) if H > 1 else 3 * W
    cw, ch = coded_size(W, H, sample_ratio)
    p = default_params(cw, ch, quality, sample_ratio, underflow, flags)
    fr = frames(W, H, rows=(0, ch // 8), in_pitch=pitch, in_frame_stride=pitch * H, out_frame_stride=per_frame)
    out = torch.empty((nb + 2 * nbc, 64) if flags & FLAG_SUBSAMPLE else (3, nb, 64), dtype=torch.int16,
                      device=rgb.device)
    need = int(lib.jpgx_workspace_size_any(ctypes.byref(fr), ctypes.byref(p)))
    if not need:                                    # the refusal, by its code
        _check(lib.jpgx_blocks_gpu_any(ctypes.byref(fr), ctypes.byref(p), None, None, None, 0, None), "jpgx_blocks_gpu_any")
    ws = _workspace(need, rgb.device, stream)
    _check(lib.jpgx_blocks_gpu_any(ctypes.byref(fr), ctypes.byref(p), rgb.data_ptr(), out.data_ptr(),
                                   ws.data_ptr(), need, _stream_ptr(stream)), "jpgx_blocks_gpu_any")
    return out


def encode_blocks_gray(gray, quality: int, flags: int = 0, stream=None):
    """One-channel images on a GPU -> their coefficients (jpgx_blocks_gpu_gray, one launch of k_gray):
    gray uint8 [H][W] or [n][H][W], W and H any 1 .. 65535, of any strides as long as the pixels of a row
    are adjacent and the rows top-down (a slice of a wider tensor is read where it is, whatever its pitch and
    alignment; frames may overlap or be one frame expanded, the input is only read) ->
    int16 [nb][64] or [n][nb][64], nb = ceil(W / 8) * ceil(H / 8) blocks in raster order: the frame of
    jfif_decode_gpu_gray and pixels_gpu_gray, the pixels beyond the image by the edge rule.  flags: 0 or
    FLAG_FORCE_EXACT.  Nothing is copied to the host and nothing waits."""
    import torch
    if not _device_tensor(gray):
        raise ValueError("encode_blocks_gray: gray must be a device tensor")
    if gray.dtype != torch.uint8 or gray.dim() not in (2, 3):
        raise ValueError("encode_blocks_gray: gray must be (H, W) or (n, H, W) uint8")
    batch = gray if gray.dim() == 3 else gray.unsqueeze(0)
    nf, H, W = (int(x) for x in batch.shape)
    nb = _gray_blocks("encode_blocks_gray", W, H)
    if nf == 0:
        raise ValueError("encode_blocks_gray: no frames")
    if W > 1 and batch.stride(2) != 1:
        raise ValueError("encode_blocks_gray: the pixels of a row must be adjacent")
    pitch = int(batch.stride(1)) if H > 1 else W
    fstride = int(batch.stride(0)) if nf > 1 else pitch * H
    if pitch < W:
        raise ValueError("encode_blocks_gray: rows top-down with a pitch >= W")
    out = torch.empty((nf, nb, 64), dtype=torch.int16, device=gray.device)
    _check(lib.jpgx_blocks_gpu_gray(batch.data_ptr(), pitch, fstride, nf, W, H, quality, flags, out.data_ptr(),
                                    nb * 64, _stream_ptr(stream)), "jpgx_blocks_gpu_gray")
    if stream is not None:
        gray.record_stream(stream)
        out.record_stream(stream)
    return out if gray.dim() == 3 else out[0]


def encode_blocks_multi(rgb: np.ndarray, quality: int, ngpus: int, sample_ratio: int = 0,
                        underflow: bytes | None = None, flags: int = 0) -> np.ndarray:
    """Host image -> host coefficients, block-row stripes over GPUs 0..ngpus-1."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    p = default_params(W, H, quality, sample_ratio, underflow, flags)
    nb, nbc, _, _ = _frame("encode_blocks_multi", W, H, sample_ratio, flags)
    out = np.empty((nb + 2 * nbc, 64) if flags & FLAG_SUBSAMPLE else (3, nb, 64), np.int16)
    _check(lib.jpgx_blocks_multi(rgb.ctypes.data, W, H, W * 3, ctypes.byref(p), out.ctypes.data,
                                 ngpus), "jpgx_blocks_multi")
    return out


class HostContext:
    """jpgx_host_ctx: `nshards` block-row shards of every image, shard k on GPU devices[k]
    (None: k modulo the device count), chunks of `chunk_rows` block rows (0: auto); device
    buffers, streams and pinned staging persist across calls until close()."""

    def __init__(self, nshards: int = 1, devices=None, chunk_rows: int = 0):
        self._h = ctypes.c_void_p()
        arr = None
        if devices is not None:
            devices = list(devices)
            if len(devices) != nshards:
                raise ValueError("one device per shard")
            arr = (ctypes.c_int * nshards)(*devices)
        self._lib = lib                           # the library that owns the handle
        _check(self._lib.jpgx_host_create(ctypes.byref(self._h), nshards,
                                    ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None,
                                    chunk_rows), "jpgx_host_create")
        self.nshards = nshards

    def blocks(self, rgb: np.ndarray, quality: int, sample_ratio: int = 0, underflow=None,
               flags: int = 0, out: np.ndarray | None = None) -> np.ndarray:
        """Host (H, W, 3) uint8 -> host int16 coefficients (layout as encode_blocks)."""
        if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.strides[1:] != (3, 1):
            raise ValueError("rgb must be (H, W, 3) uint8 with packed pixels")
        H, W = rgb.shape[:2]
        if rgb.strides[0] < 3 * W:                # flipped or overlapping rows: not a pitch
            raise ValueError("rgb rows must be laid out top-down with a pitch >= 3 * width")
        p = default_params(W, H, quality, sample_ratio, underflow, flags)
        nb, nbc, _, _ = _frame("HostContext.blocks", W, H, sample_ratio, flags)
        shape = (nb + 2 * nbc, 64) if flags & FLAG_SUBSAMPLE else (3, nb, 64)
        if out is None:
            out = np.empty(shape, np.int16)
        elif out.shape != shape or out.dtype != np.int16 or not out.flags.c_contiguous:
            raise ValueError(f"out must be a contiguous int16 array of shape {shape}")
        _check(self._lib.jpgx_host_blocks(self._h, rgb.ctypes.data, W, H, rgb.strides[0],
                                    ctypes.byref(p), out.ctypes.data), "jpgx_host_blocks")
        return out

    def close(self) -> None:
        if self._h:
            self._lib.jpgx_host_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_register(a: np.ndarray) -> None:
    """Page-lock a numpy buffer (jpgx_host_register) so jpgx_host_blocks DMAs it directly."""
    _check(lib.jpgx_host_register(a.ctypes.data, a.nbytes), "jpgx_host_register")


def host_unregister(a: np.ndarray) -> None:
    _check(lib.jpgx_host_unregister(a.ctypes.data), "jpgx_host_unregister")
