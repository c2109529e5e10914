"""ctypes view of include/jpgx_compat.h: the reference-compatible Block API, the JpgData
adapter, the DC recurrence, the BMP reader and the encode stage sequence (all in libjpgx.so).

Reference mapping (matthewT53/JPEG-Encoder-and-Decoder):
    Block, new_block ... destroy_block  <- src/block.c:15-67
    dct_block                           <- src/dct.c:36-59
    quantise_block / quantise_lum/chr   <- src/quantise.c:52-72 (transposed table use)
    scale_table_inplace                 <- src/quantise.c:74-86
    zig_zag_block                       <- src/zig_zag.c:48-58
    JpegData, fill_jpgdata, dpcm        <- src/headers/jpg_encode.h:21-70, src/zig_zag.c:24-32,
                                           src/dpcm.c:6-21
    bmp_read                            <- src/bitmap.c:41-152
    encode_bmp                          <- encode_bmp_to_jpeg, src/jpg_encode.c:19-47
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import EARG, JpgxError, _scale_arg, coded_size, lib

c_int_p = ctypes.POINTER(ctypes.c_int)


class BlockStruct(ctypes.Structure):
    _fields_ = [("values", ctypes.c_double * 64)]


BlockPtr = ctypes.POINTER(BlockStruct)


class HuffmanData(ctypes.Structure):
    _fields_ = [("freq", ctypes.c_int * 257), ("code_len", ctypes.c_int * 257),
                ("others", ctypes.c_int * 257), ("bits", ctypes.c_int * 32),
                ("huffval", ctypes.c_int * 256)]


class JpegData(ctypes.Structure):
    _fields_ = [("output_filename", ctypes.c_char_p), ("input_filename", ctypes.c_char_p),
                ("width", ctypes.c_int), ("height", ctypes.c_int),
                ("sample_ratio", ctypes.c_int), ("quality", ctypes.c_int),
                ("num_blocks_Y", ctypes.c_int), ("num_blocks_Cb", ctypes.c_int),
                ("num_blocks_Cr", ctypes.c_int),
                ("Y", ctypes.POINTER(BlockPtr)), ("Cb", ctypes.POINTER(BlockPtr)),
                ("Cr", ctypes.POINTER(BlockPtr)),
                ("zig_zag_Y", ctypes.POINTER(c_int_p)), ("zig_zag_Cb", ctypes.POINTER(c_int_p)),
                ("zig_zag_Cr", ctypes.POINTER(c_int_p)),
                ("lum_DC", HuffmanData), ("lum_AC", HuffmanData),
                ("chrom_DC", HuffmanData), ("chrom_AC", HuffmanData)]


class JfifInfo(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("sample_ratio", ctypes.c_int),
                ("restart_interval", ctypes.c_uint), ("scan_offset", ctypes.c_size_t),
                ("nb_y", ctypes.c_size_t), ("nb_c", ctypes.c_size_t)]


def _setup(L):
    d, i, vp = ctypes.c_double, ctypes.c_int, ctypes.c_void_p
    L.jpgx_new_block.restype = BlockPtr
    L.jpgx_new_block.argtypes = []
    L.jpgx_get_value_block.restype = d
    L.jpgx_get_value_block.argtypes = [BlockPtr, i, i]
    L.jpgx_set_value_block.restype = None
    L.jpgx_set_value_block.argtypes = [BlockPtr, i, i, d]
    L.jpgx_copy_block.restype = BlockPtr
    L.jpgx_copy_block.argtypes = [BlockPtr]
    for f in ("jpgx_show_block", "jpgx_destroy_block", "jpgx_dct_block", "jpgx_quantise_lum",
              "jpgx_quantise_chr"):
        getattr(L, f).restype = None
        getattr(L, f).argtypes = [BlockPtr]
    L.jpgx_quantise_block.restype = None
    L.jpgx_quantise_block.argtypes = [BlockPtr, vp]
    L.jpgx_scale_table_inplace.restype = None
    L.jpgx_scale_table_inplace.argtypes = [vp, i]
    L.jpgx_zig_zag_block.restype = None
    L.jpgx_zig_zag_block.argtypes = [BlockPtr, vp]
    J = ctypes.POINTER(JpegData)
    L.jpgx_fill_jpgdata.argtypes = [J, vp]
    L.jpgx_free_jpgdata.restype = None
    L.jpgx_free_jpgdata.argtypes = [J]
    L.jpgx_dpcm.restype = None
    L.jpgx_dpcm.argtypes = [J]
    L.jpgx_dpcm_dc.argtypes = [vp, ctypes.c_size_t, vp, vp]
    L.jpgx_bmp_read.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp), c_int_p, c_int_p,
                                ctypes.POINTER(ctypes.c_size_t)]
    L.jpgx_free.restype = None
    L.jpgx_free.argtypes = [vp]
    L.jpgx_encode_bmp.argtypes = [ctypes.c_char_p, i, i, i, i, J]
    L.jpgx_jfif_bound.restype = ctypes.c_size_t
    L.jpgx_jfif_bound.argtypes = [i, i]
    L.jpgx_write_jfif.argtypes = [vp, i, i, i, vp, ctypes.c_size_t,
                                  ctypes.POINTER(ctypes.c_size_t)]
    L.jpgx_encode_bmp_to_jpeg.argtypes = [ctypes.c_char_p, ctypes.c_char_p, i, i]
    L.jpgx_write_jfif_ex.argtypes = [vp, i, i, i, i, i, i, vp, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_size_t)]
    L.jpgx_write_jfif_opt.argtypes = [vp, i, i, i, i, i, i, ctypes.c_uint, vp, ctypes.c_size_t,
                                      ctypes.POINTER(ctypes.c_size_t)]
    L.jpgx_encode_rgb_to_jpeg.argtypes = [vp, i, i, ctypes.c_size_t, ctypes.c_char_p, i, i,
                                          ctypes.c_uint, i]
    L.jpgx_encode_rgb_to_jpeg_any.argtypes = L.jpgx_encode_rgb_to_jpeg.argtypes
    L.jpgx_write_jfif_any.argtypes = L.jpgx_write_jfif_opt.argtypes
    L.jpgx_write_jfif_gray.argtypes = [vp, i, i, i, i, i, ctypes.c_uint, vp, ctypes.c_size_t,
                                       ctypes.POINTER(ctypes.c_size_t)]


    L.jpgx_jfif_info_of.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(JfifInfo)]
    L.jpgx_read_jfif.argtypes = [vp, ctypes.c_size_t, i, vp, ctypes.c_size_t, vp, ctypes.POINTER(JfifInfo)]
    L.jpgx_read_jfif_sub.argtypes = [vp, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_size_t, vp,
                                     ctypes.POINTER(JfifInfo), vp]
    L.jpgx_pixels_host.argtypes = [vp, i, i, i, vp, vp, ctypes.c_size_t, i]
    for name in ("jpgx_jfif_info_of", "jpgx_read_jfif", "jpgx_read_jfif_sub", "jpgx_pixels_host"):
        getattr(L, name + "_any").argtypes = getattr(L, name).argtypes
    for name in ("jpgx_jfif_info_of", "jpgx_read_jfif", "jpgx_read_jfif_sub"):
        getattr(L, name + "_gray").argtypes = getattr(L, name).argtypes
    L.jpgx_pixels_host_gray.argtypes = [vp, i, i, vp, vp, ctypes.c_size_t, i, i]
    L.jpgx_pixels_host_scaled.argtypes = [vp, i, i, i, i, vp, vp, ctypes.c_size_t, i]
    L.jpgx_pixels_host_gray_scaled.argtypes = [vp, i, i, i, vp, vp, ctypes.c_size_t, i, i]


_setup(lib)


def _check(rc, what):
    if rc != 0:
        raise JpgxError(rc, what)


class Block:
    """One reference Block (64 doubles, values[y*8+x]) owned by libjpgx."""

    def __init__(self, values=None):
        self.ptr = lib.jpgx_new_block()
        if values is not None:
            v = np.asarray(values, np.float64).reshape(64)
            for k in range(64):
                self.ptr.contents.values[k] = float(v[k])

    def __del__(self):
        if getattr(self, "ptr", None):
            lib.jpgx_destroy_block(self.ptr)
            self.ptr = None

    @classmethod
    def _wrap(cls, ptr):
        b = cls.__new__(cls)
        b.ptr = ptr
        return b

    def get(self, x, y):
        return lib.jpgx_get_value_block(self.ptr, x, y)

    def set(self, x, y, v):
        lib.jpgx_set_value_block(self.ptr, x, y, v)

    def copy(self):
        return Block._wrap(lib.jpgx_copy_block(self.ptr))

    def show(self):
        lib.jpgx_show_block(self.ptr)

    def values(self) -> np.ndarray:
        return np.ctypeslib.as_array(self.ptr.contents.values).copy()

    def dct(self):
        lib.jpgx_dct_block(self.ptr)

    def quantise(self, table):
        t = np.ascontiguousarray(table, np.int32)
        lib.jpgx_quantise_block(self.ptr, t.ctypes.data)

    def quantise_lum(self):
        lib.jpgx_quantise_lum(self.ptr)

    def quantise_chr(self):
        lib.jpgx_quantise_chr(self.ptr)

    def zig_zag(self) -> np.ndarray:
        zz = np.zeros(64, np.int32)
        lib.jpgx_zig_zag_block(self.ptr, zz.ctypes.data)
        return zz


def legacy_table(which: int) -> np.ndarray:
    """A live numpy view of jpgx_q_table_lum (0) / jpgx_q_table_chr (1)."""
    name = "jpgx_q_table_lum" if which == 0 else "jpgx_q_table_chr"
    arr = (ctypes.c_int * 64).in_dll(lib, name)
    return np.ctypeslib.as_array(arr).reshape(8, 8)


def scale_table_inplace(table: np.ndarray, quality: int) -> None:
    assert table.dtype == np.int32 and table.flags.c_contiguous and table.shape == (8, 8)
    lib.jpgx_scale_table_inplace(table.ctypes.data, quality)


def dpcm_dc(coef: np.ndarray, carry=(0, 0, 0)) -> np.ndarray:
    coef = np.ascontiguousarray(coef, np.int16)
    nb = coef.shape[1]
    dc = np.empty((3, nb), np.int32)
    c = np.asarray(carry, np.int32)
    _check(lib.jpgx_dpcm_dc(coef.ctypes.data, nb, c.ctypes.data, dc.ctypes.data), "jpgx_dpcm_dc")
    return dc


def jpgdata_from_coef(width: int, height: int, coef: np.ndarray) -> JpegData:
    j = JpegData()
    j.width, j.height = width, height
    coef = np.ascontiguousarray(coef, np.int16)
    _check(lib.jpgx_fill_jpgdata(ctypes.byref(j), coef.ctypes.data), "jpgx_fill_jpgdata")
    return j


def jpgdata_zigzag(j: JpegData) -> np.ndarray:
    """zig_zag_{Y,Cb,Cr} -> int32 [3][nb][64]"""
    nb = j.num_blocks_Y
    out = np.empty((3, nb, 64), np.int32)
    for c, rows in enumerate((j.zig_zag_Y, j.zig_zag_Cb, j.zig_zag_Cr)):
        for i in range(nb):
            out[c, i] = np.ctypeslib.as_array(rows[i], shape=(64,))
    return out


def dpcm(j: JpegData) -> None:
    lib.jpgx_dpcm(ctypes.byref(j))


def free_jpgdata(j: JpegData) -> None:
    lib.jpgx_free_jpgdata(ctypes.byref(j))


def bmp_read(path: str):
    """-> (rgb [H][W][3] uint8, file_size)"""
    p = ctypes.c_void_p()
    w, h, fs = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    _check(lib.jpgx_bmp_read(path.encode(), ctypes.byref(p), ctypes.byref(w), ctypes.byref(h),
                             ctypes.byref(fs)), "jpgx_bmp_read")
    n = w.value * h.value * 3
    out = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(n,)).copy()
    lib.jpgx_free(p)
    return out.reshape(h.value, w.value, 3), fs.value


def encode_bmp(path: str, quality: int, sample_ratio: int = 0, device: int = 0,
               do_dpcm: bool = False) -> JpegData:
    j = JpegData()
    j._path = path.encode()             # j.input_filename points at it (jpg_encode.c:29)
    _check(lib.jpgx_encode_bmp(j._path, quality, sample_ratio, device, int(do_dpcm),
                               ctypes.byref(j)), "jpgx_encode_bmp")
    return j


def write_jfif(coef: np.ndarray, width: int, height: int, quality: int) -> bytes:
    """int16 [3][nb][64] -> baseline JFIF bytes (jpgx_write_jfif)."""
    coef = np.ascontiguousarray(coef, np.int16)
    cap = lib.jpgx_jfif_bound(width, height)
    buf = (ctypes.c_uint8 * cap)()
    n = ctypes.c_size_t()
    _check(lib.jpgx_write_jfif(coef.ctypes.data, width, height, quality,
                               ctypes.cast(buf, ctypes.c_void_p), cap, ctypes.byref(n)),
           "jpgx_write_jfif")
    return bytes(buf[:n.value])


def write_jfif_ex(coef: np.ndarray, width: int, height: int, quality: int, sample_ratio: int = 0,
                  restart_rows: int = -1, nthreads: int = 0, cap: int | None = None,
                  optimize: bool = False, any_size: bool = False) -> bytes:
    """jpgx_write_jfif_ex: restart intervals of `restart_rows` MCU rows (-1 auto, 0 none) coded on
    `nthreads` host threads (0: one per CPU).  `cap`: output buffer size (default: grown on
    demand from the size the library reports).  optimize: jpgx_write_jfif_opt with
    JPGX_JFIF_OPTIMIZE, Huffman tables built from the image's own symbols.  any_size:
    jpgx_write_jfif_any -- width and height are the file's own, any 1 .. 65535, and coef holds the
    blocks of its coded frame (coded_size), all of which are coded."""
    coef = np.ascontiguousarray(coef, np.int16)
    n = ctypes.c_size_t()
    cap = cap or max(1 << 20, coef.size // 2)
    write = lib.jpgx_write_jfif_any if any_size else lib.jpgx_write_jfif_opt
    if any_size and sample_ratio in (0, 1, 2) and 0 < width < 65536 and 0 < height < 65536:
        cw, ch = coded_size(width, height, sample_ratio)
        if coef.size < (cw // 8) * (ch // 8) * (3, 2, 1.5)[sample_ratio] * 64:
            raise ValueError("write_jfif_ex: coef must hold the coded frame's nb + 2 nbc blocks")
    for _ in range(2):
        buf = np.empty(cap, np.uint8)
        rc = write(coef.ctypes.data, width, height, quality, sample_ratio,
                                     restart_rows, nthreads, 1 if optimize else 0, buf.ctypes.data, cap,
                                     ctypes.byref(n))
        if rc == 0:
            return buf[:n.value].tobytes()
        if rc != -4 or n.value <= cap:                      # JPGX_EARG with the size needed
            break
        cap = n.value
    _check(rc, "jpgx_write_jfif_ex")
    raise JpgxError(rc, "jpgx_write_jfif_ex")


def write_jfif_gray(coef: np.ndarray, width: int, height: int, quality: int, restart_rows: int = 0,
                    nthreads: int = 1, optimize: bool = False, cap: int | None = None) -> bytes:
    """jpgx_write_jfif_gray: int16 Y [nb][64], nb = ceil(width / 8) * ceil(height / 8), -> the bytes of a
    one-component baseline file of width x height, any 1 .. 65535 (read_jfif_gray reads it back).
    restart_rows counts block rows (-1 auto, 0 none); nthreads, optimize and cap as write_jfif_ex's."""
    coef = np.ascontiguousarray(coef, np.int16)
    if 0 < width < 65536 and 0 < height < 65536 and coef.size < ((width + 7) // 8) * ((height + 7) // 8) * 64:
        raise ValueError("write_jfif_gray: coef must hold ceil(width / 8) * ceil(height / 8) blocks")
    n = ctypes.c_size_t()
    cap = cap or max(1 << 20, coef.size // 2)
    for _ in range(2):
        buf = np.empty(cap, np.uint8)
        rc = lib.jpgx_write_jfif_gray(coef.ctypes.data, width, height, quality, restart_rows, nthreads,
                                      1 if optimize else 0, buf.ctypes.data, cap, ctypes.byref(n))
        if rc == 0:
            return buf[:n.value].tobytes()
        if rc != -4 or n.value <= cap:                      # JPGX_EARG with the size needed
            break
        cap = n.value
    _check(rc, "jpgx_write_jfif_gray")
    raise JpgxError(rc, "jpgx_write_jfif_gray")


def write_jfif_sub(coef: np.ndarray, width: int, height: int, quality: int,
                   sample_ratio: int) -> bytes:
    """Y|Cb|Cr blocks of the JPGX_FLAG_SUBSAMPLE layout -> 4:2:2 / 4:2:0 JFIF bytes."""
    coef = np.ascontiguousarray(coef, np.int16)
    cap = lib.jpgx_jfif_bound(width, height)
    buf = (ctypes.c_uint8 * cap)()
    n = ctypes.c_size_t()
    _check(lib.jpgx_write_jfif_sub(ctypes.c_void_p(coef.ctypes.data), width, height, quality,
                                   sample_ratio, ctypes.cast(buf, ctypes.c_void_p),
                                   ctypes.c_size_t(cap), ctypes.byref(n)),
           "jpgx_write_jfif_sub")
    return bytes(buf[:n.value])


def _info_dict(info: JfifInfo) -> dict:
    return dict(width=info.width, height=info.height, sample_ratio=info.sample_ratio,
                restart_interval=info.restart_interval, scan_offset=info.scan_offset,
                nb_y=info.nb_y, nb_c=info.nb_c)


def jfif_info(data, any_size: bool = False) -> dict:
    """jpgx_jfif_info_of: the header walk of a baseline JFIF file (bytes) -> width, height,
    sample_ratio, restart_interval, scan_offset, nb_y, nb_c.  JpgxError(EJFIF_HEADER) when refused.
    any_size: jpgx_jfif_info_of_any -- any width and height; nb_y and nb_c are the coded frame's."""
    return _jfif_info(lib.jpgx_jfif_info_of_any if any_size else lib.jpgx_jfif_info_of, data)


def _what(lib_fn) -> str:
    """the name a call's failure is reported under: an _any entry point's is its plain sibling's"""
    return lib_fn.__name__.replace("_any", "")


def _jfif_info(lib_fn, data) -> dict:
    """jfif_info and jfif_info_gray: one of the library's header walks over data"""
    buf = np.frombuffer(bytes(data) or b"\0", np.uint8)
    info = JfifInfo()
    _check(lib_fn(buf.ctypes.data, len(data), ctypes.byref(info)), _what(lib_fn))
    return _info_dict(info)


def _read_jfif(lib_fn, data, info: dict, qt_shape, nthreads: int = 1, sub_args=None) -> dict:
    """The four readers: one of the library's readers over data, a file of `info`, into fresh buffers.
    sub_args: (sub_bytes, tile_subs) of a twin of the device decoder, which takes them where a reader
    takes nthreads and counts into `stats`."""
    buf = np.frombuffer(bytes(data), np.uint8)
    coef = np.empty((info["nb_y"] + 2 * info["nb_c"], 64), np.int16)
    qt = np.zeros(qt_shape, np.uint16)
    got, stats = JfifInfo(), JfifSubStats()
    how, tail = ((nthreads,), ()) if sub_args is None else (sub_args, (ctypes.byref(stats),))
    _check(lib_fn(buf.ctypes.data, len(buf), *how, coef.ctypes.data, coef.size, qt.ctypes.data, ctypes.byref(got),
                  *tail), _what(lib_fn))
    if info["sample_ratio"] == 0 and info["nb_c"]:          # 4:4:4: three planes of nb blocks
        coef = coef.reshape(3, info["nb_y"], 64)
    out = dict(coef=coef, qt=qt, width=info["width"], height=info["height"],
               sample_ratio=info["sample_ratio"], restart_interval=info["restart_interval"])
    if sub_args is not None:
        out["stats"] = {n: int(getattr(stats, n)) for n, _ in JfifSubStats._fields_}
    return out


def read_jfif(data, nthreads: int = 1, any_size: bool = False) -> dict:
    """jpgx_read_jfif: a baseline JFIF file (bytes) -> dict(coef, qt, width, height, sample_ratio,
    restart_interval): coef int16 [3][nb][64] for 4:4:4, [nb + 2 nbc][64] (Y | Cb | Cr) for 4:2:2 /
    4:2:0 -- what the writers above take; qt uint16 [2][64] (Y's table, the chroma table; zig-zag
    order).  The restart intervals are decoded on `nthreads` threads (0: one per CPU).
    JpgxError(EJFIF_HEADER / EJFIF_SCAN) when the file is refused.  any_size: jpgx_read_jfif_any --
    a file of any width and height; width and height are the file's, coef the coded frame's."""
    return _read_jfif(lib.jpgx_read_jfif_any if any_size else lib.jpgx_read_jfif, data, jfif_info(data, any_size),
                      (2, 64), nthreads)


class JfifSubStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in (
        "subsequences", "tiles", "rounds_max", "redecodes", "wrong_first_guesses", "starts_on_stuffing",
        "units_across_sub", "units_across_tile")]


def read_jfif_sub(data, sub_bytes: int = 0, tile_subs: int = 0, any_size: bool = False) -> dict:
    """jpgx_read_jfif_sub: read_jfif by the routines of the device decoder that works inside a restart
    interval, subsequences of sub_bytes bytes and tiles of tile_subs subsequences
    (0, 0: the kernel's shape).  read_jfif's dict and `stats`, a dict of the twin's counters.
    any_size: jpgx_read_jfif_sub_any, as read_jfif's."""
    return _read_jfif(lib.jpgx_read_jfif_sub_any if any_size else lib.jpgx_read_jfif_sub, data, jfif_info(data, any_size),
                      (2, 64), sub_args=(sub_bytes, tile_subs))


def pixels_host(coef: np.ndarray, width: int, height: int, sample_ratio: int, qt: np.ndarray,
                nthreads: int = 0, pitch: int | None = None, any_size: bool = False, scale: int = 1) -> np.ndarray:
    """jpgx_pixels_host: one frame's coefficients (read_jfif's layout) and its uint16 [2][64] zig-zag
    tables -> uint8 [H][W][3], libjpeg's default decoder's pixels, on `nthreads`
    threads (0: one per CPU).  pitch: bytes between pixel rows of the buffer the result is a view of.
    any_size: jpgx_pixels_host_any -- coef is the coded frame's, width and height the visible frame's.
    scale 2, 4 or 8: jpgx_pixels_host_scaled -- libjpeg's decode at 1 / scale of the size, uint8
    [ceil(H / scale)][ceil(W / scale)][3]; coef, width and height as with any_size, set or not."""
    scale = _scale_arg("pixels_host", scale)
    any_size = any_size or scale > 1
    coef = np.ascontiguousarray(coef, np.int16)
    qt = np.ascontiguousarray(qt, np.uint16)
    cw, ch = width, height
    if any_size and sample_ratio in (0, 1, 2) and 0 < width < 65536 and 0 < height < 65536:
        cw, ch = coded_size(width, height, sample_ratio)
    nb = (cw // 8) * (ch // 8)
    nbc = (nb, nb // 2, nb // 4)[sample_ratio] if sample_ratio in (0, 1, 2) else nb
    if qt.shape != (2, 64) or width <= 0 or height <= 0 or coef.size < (nb + 2 * nbc) * 64:
        raise ValueError("pixels_host: qt [2][64], and coef must hold nb + 2 nbc blocks")
    if scale > 1:
        ow, oh = -(-width // scale), -(-height // scale)
        pitch = 3 * ow if pitch is None else int(pitch)
        buf = np.empty((oh, max(pitch, 1)), np.uint8)
        _check(lib.jpgx_pixels_host_scaled(coef.ctypes.data, width, height, sample_ratio, scale, qt.ctypes.data,
                                           buf.ctypes.data, pitch, nthreads), "jpgx_pixels_host_scaled")
        return buf[:, :3 * ow].reshape(oh, ow, 3)
    pitch = 3 * width if pitch is None else int(pitch)
    buf = np.empty((height, max(pitch, 1)), np.uint8)
    _check((lib.jpgx_pixels_host_any if any_size else lib.jpgx_pixels_host)(coef.ctypes.data, width, height, sample_ratio, qt.ctypes.data, buf.ctypes.data,
                                pitch, nthreads), "jpgx_pixels_host")
    return buf[:, :3 * width].reshape(height, width, 3)


def jfif_info_gray(data) -> dict:
    """jpgx_jfif_info_of_gray: jfif_info for a one-component (grayscale) file of any width and height:
    sample_ratio 0, nb_y = ceil(W / 8) * ceil(H / 8), nb_c 0, restart_interval in blocks."""
    return _jfif_info(lib.jpgx_jfif_info_of_gray, data)


def read_jfif_gray(data, nthreads: int = 1) -> dict:
    """jpgx_read_jfif_gray: a one-component baseline file -> dict(coef int16 [nb][64], qt uint16 [64],
    width, height, sample_ratio 0, restart_interval).  JpgxError(EJFIF_HEADER / EJFIF_SCAN) when refused."""
    return _read_jfif(lib.jpgx_read_jfif_gray, data, jfif_info_gray(data), 64, nthreads)


def read_jfif_sub_gray(data, sub_bytes: int = 0, tile_subs: int = 0) -> dict:
    """jpgx_read_jfif_sub_gray: read_jfif_gray by the routines of the device decoder that works inside a
    restart interval (read_jfif_sub's shapes and `stats`)."""
    return _read_jfif(lib.jpgx_read_jfif_sub_gray, data, jfif_info_gray(data), 64, sub_args=(sub_bytes, tile_subs))


def pixels_host_gray(coef: np.ndarray, width: int, height: int, qt: np.ndarray, channels: int = 1,
                     nthreads: int = 0, pitch: int | None = None, scale: int = 1) -> np.ndarray:
    """jpgx_pixels_host_gray: a one-component frame's coefficients [nb][64] and its uint16 [64] zig-zag
    table -> uint8 [H][W] (channels 1) or [H][W][3] (channels 3, R = G = B): libjpeg's default decoder's
    pixels.  pitch: bytes between pixel rows of the buffer the result is a view of.  scale 2, 4 or 8:
    jpgx_pixels_host_gray_scaled -- the decode at 1 / scale of the size, [ceil(H / scale)][ceil(W / scale)]."""
    scale = _scale_arg("pixels_host_gray", scale)
    coef = np.ascontiguousarray(coef, np.int16)
    qt = np.ascontiguousarray(qt, np.uint16)
    if qt.size != 64 or (0 < width < 65536 and 0 < height < 65536
                         and coef.size < ((width + 7) // 8) * ((height + 7) // 8) * 64):
        raise ValueError("pixels_host_gray: qt [64], and coef must hold ceil(W / 8) * ceil(H / 8) blocks")
    if scale > 1:
        ow, oh = max(-(-width // scale), 0), max(-(-height // scale), 0)
        pitch = channels * ow if pitch is None else int(pitch)
        buf = np.empty((max(oh, 1), max(pitch, 1)), np.uint8)
        _check(lib.jpgx_pixels_host_gray_scaled(coef.ctypes.data, width, height, scale, qt.ctypes.data, buf.ctypes.data,
                                                pitch, channels, nthreads), "jpgx_pixels_host_gray_scaled")
        px = buf[:oh, :channels * ow]
        return px if channels == 1 else px.reshape(oh, ow, 3)
    pitch = channels * width if pitch is None else int(pitch)
    buf = np.empty((max(height, 1), max(pitch, 1)), np.uint8)
    _check(lib.jpgx_pixels_host_gray(coef.ctypes.data, width, height, qt.ctypes.data, buf.ctypes.data, pitch,
                                     channels, nthreads), "jpgx_pixels_host_gray")
    px = buf[:height, :channels * width]
    return px if channels == 1 else px.reshape(height, width, 3)


PAD_STATS = 17      # JX_PAD_NSTAT (csrc/jx_pad.h)


def pad_host(buf: np.ndarray, base_off: int, width: int, height: int, in_pitch: int, in_frame_stride: int,
             nframes: int, coded_width: int, coded_height: int, trace: bool = True, library=None):
    """jx_pad_host (csrc/jpgx_pad_host.cpp, test-only): k_pad_edge's chunk rule (csrc/jx_pad.h) on the host
    over the frames of `buf`, uint8 [len]; pixel (0, 0) of frame f is buf[base_off + f * in_frame_stride].
    -> (bad, coded uint8 [nframes][coded_height][coded_width][3], touched uint8 [len] or None, stats uint64
    [PAD_STATS]).  trace: every load is checked against buf and recorded in `touched` (1: byte loads, 2:
    dword loads); bad counts the refused ones.  stats: fast chunks by the row start's residue [0:4], slow
    chunks by reason [4:8] (a row's first chunk off a dword, repeated columns or a row's short end, the
    fifth dword past the row, the straddling chunk), chunks with an index >= 256 [8], and by residue the
    chunks that met the fifth dword's bound exactly [9:13] and missed it by one byte [13:17]."""
    L = library or lib
    fn = L.jx_pad_host
    vp, i, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    fn.argtypes = [vp, z, z, i, i, z, z, i, i, i, vp, vp, vp]
    fn.restype = ctypes.c_longlong
    if buf.dtype != np.uint8 or buf.ndim != 1 or not buf.flags.c_contiguous:
        raise ValueError("pad_host: buf must be a contiguous uint8 vector")
    out = np.zeros((nframes, coded_height, coded_width, 3), np.uint8)
    touched = np.zeros(len(buf), np.uint8) if trace else None
    stats = np.zeros(PAD_STATS, np.uint64)
    bad = fn(buf.ctypes.data, len(buf), base_off, width, height, in_pitch, in_frame_stride, nframes, coded_width,
             coded_height, out.ctypes.data, touched.ctypes.data if trace else None, stats.ctypes.data)
    if bad < 0:
        raise JpgxError(EARG, "jx_pad_host")
    return int(bad), out, touched, stats


def encode_bmp_to_jpeg_ex(src: str, dst: str, quality: int, sample_ratio: int, flags: int,
                          device: int = 0) -> None:
    _check(lib.jpgx_encode_bmp_to_jpeg_ex(src.encode(), dst.encode(), quality, sample_ratio,
                                          ctypes.c_uint(flags), device),
           "jpgx_encode_bmp_to_jpeg_ex")


def encode_bmp_to_jpeg(src: str, dst: str, quality: int, sample_ratio: int = 0) -> None:
    _check(lib.jpgx_encode_bmp_to_jpeg(src.encode(), dst.encode(), quality, sample_ratio),
           "jpgx_encode_bmp_to_jpeg")


def encode_rgb_to_jpeg(rgb: np.ndarray, dst: str, quality: int, sample_ratio: int = 0,
                       flags: int = 0, device: int = 0, any_size: bool = False) -> None:
    """In-memory (H, W, 3) uint8 image -> JFIF file (jpgx_encode_rgb_to_jpeg).  any_size:
    jpgx_encode_rgb_to_jpeg_any, an image of any width and height."""
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.strides[1:] != (3, 1):
        raise ValueError("rgb must be (H, W, 3) uint8 with packed pixels")
    H, W = rgb.shape[:2]
    fn = lib.jpgx_encode_rgb_to_jpeg_any if any_size else lib.jpgx_encode_rgb_to_jpeg
    _check(fn(rgb.ctypes.data, W, H, rgb.strides[0], dst.encode(), quality, sample_ratio, ctypes.c_uint(flags),
              device), "jpgx_encode_rgb_to_jpeg")
