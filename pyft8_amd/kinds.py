"""Input sample kinds: the Python counterpart of csrc/sample_fmt.hpp.  The ABI's eight kinds (include/ft8rx.h
FT8RX_DDC_* 0 .. 3, FT8RX_WIDE_* 16 .. 19) name six sample formats; kinds 0 / 16 and 2 / 17 are the same bytes.  Here: the numbers, and
per kind its name, dtype, components per sample, bytes per sample, the one routine that packs a stream, the sample values the float64
twins and the integer blanker twin work on, and the blanker's default threshold.  ddc, ddc_wide, ddc_rat and blank_in show the kinds
they take as views of this table (view) and keep what is their own: which kinds, kind_of's policy and the texts of their refusals."""
import numpy as np

from . import _lib

REAL_I16, REAL_F32, IQ_I16, IQ_F32 = range(4)                           # FT8RX_DDC_*
WIDE_REAL_I16, WIDE_IQ_I16, WIDE_IQ_U8, WIDE_IQ_I8 = range(16, 20)      # FT8RX_WIDE_*
NAMES = {REAL_I16: "real int16", REAL_F32: "real float32", IQ_I16: "IQ int16", IQ_F32: "IQ float32",
         WIDE_REAL_I16: "real int16", WIDE_IQ_I16: "IQ int16", WIDE_IQ_U8: "IQ uint8", WIDE_IQ_I8: "IQ int8"}
DTYPE = {REAL_I16: np.int16, REAL_F32: np.float32, IQ_I16: np.int16, IQ_F32: np.float32,
         WIDE_REAL_I16: np.int16, WIDE_IQ_I16: np.int16, WIDE_IQ_U8: np.uint8, WIDE_IQ_I8: np.int8}
COMPONENTS = {REAL_I16: 1, REAL_F32: 1, IQ_I16: 2, IQ_F32: 2, WIDE_REAL_I16: 1, WIDE_IQ_I16: 2, WIDE_IQ_U8: 2, WIDE_IQ_I8: 2}
BLANK_IN_THRESHOLD_REAL, BLANK_IN_THRESHOLD_IQ = 8.0, 5.5               # FT8RX_BLANK_IN_THRESHOLD_Q8_DEFAULT_REAL / _IQ over 256


def view(taken):
    """(KINDS, KIND_NAMES, _DTYPE) of the kinds a module takes"""
    return tuple(taken), {k: NAMES[k] for k in taken}, {k: DTYPE[k] for k in taken}


def is_iq(kind):
    return COMPONENTS[kind] == 2


def is_integer(kind):
    return np.dtype(DTYPE[kind]).kind != "f"


def sample_bytes(kind):
    return np.dtype(DTYPE[kind]).itemsize * COMPONENTS[kind]


def shape(kind, n):
    """the shape of n packed samples of one stream"""
    return (n, 2) if is_iq(kind) else (n,)


def blank_in_threshold(kind):
    """the input blanker's default threshold k of a kind (threshold_q8 = 256 k)"""
    return BLANK_IN_THRESHOLD_IQ if is_iq(kind) else BLANK_IN_THRESHOLD_REAL


def as_dtype(a, kind, range_text):
    """a as a C-contiguous array of the kind's dtype.  An integer kind takes integers in its dtype's range; anything else is refused
    with range_text, formatted with name, kind, dtype and got (the dtype that came)."""
    dt = np.dtype(DTYPE[kind])
    if a.dtype != dt and is_integer(kind):
        info = np.iinfo(dt)
        if not np.issubdtype(a.dtype, np.integer) or (a.size and (a.min() < info.min or a.max() > info.max)):
            raise _lib.Ft8rxError(range_text.format(name=NAMES[kind], kind=kind, dtype=dt.name, got=a.dtype))
    return np.ascontiguousarray(a, dt)


def pack_stream(samples, kind, shape_text, range_text):
    """ONE stream's samples as the C-contiguous array the entries take for `kind` -> (array, n): a real kind [n], an IQ kind (I, Q)
    pairs [n, 2], IQ float32 also complex [n].  Another shape is refused with shape_text (formatted with name, form, shape and got),
    values the dtype does not hold with range_text (as_dtype)."""
    a = np.asarray(samples)
    iq = is_iq(kind)
    if kind == IQ_F32 and a.dtype.kind == "c" and a.ndim == 1:
        a = np.ascontiguousarray(a, np.complex64)
        return a.view(np.float32).reshape(-1, 2), a.shape[0]
    if a.dtype.kind == "c" or a.ndim != (2 if iq else 1) or (iq and a.shape[1] != 2):
        raise _lib.Ft8rxError(shape_text.format(name=NAMES[kind], form="(I, Q) pairs [n, 2]" if iq else "[n]", shape=a.shape, got=a.dtype))
    a = as_dtype(a, kind, range_text)
    return a, a.shape[0]


def values(a, kind):
    """packed samples of one stream -> float64 [n] (real) or complex128 [n] (IQ) on the int16 scale, as the float64 twins take them:
    uint8 u -> 256 (u - 127.5), int8 s -> 256 s, the 16-bit and float kinds as they are"""
    a = a.astype(np.float64)
    if kind == WIDE_IQ_U8:
        a = 256.0 * (a - 127.5)
    elif kind == WIDE_IQ_I8:
        a = 256.0 * a
    return a[:, 0] + 1j * a[:, 1] if is_iq(kind) else a


def components(a, kind):
    """packed samples -> the int64 component values c the input blanker works on, [n] or [n, 2]: uint8 u -> 2 u - 255"""
    c = a.astype(np.int64)
    return 2 * c - 255 if kind == WIDE_IQ_U8 else c


def store(c, kind):
    """component values -> the kind's bytes"""
    return ((c + 255) >> 1).astype(np.uint8) if kind == WIDE_IQ_U8 else c.astype(DTYPE[kind])
