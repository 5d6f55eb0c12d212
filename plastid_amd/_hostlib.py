"""ctypes binding of the host library (``csrc/bam_stager.cpp`` and ``csrc/host_shims.h``, built as
``libplastid_bam.so``): the BAM / SAM stager and the CPU models of what the GPU reads and writes.

The one place that knows the ``pb_*`` entry points: :data:`SIGNATURES` is pinned to the C definitions by
``tests/test_hostlib_abi.py``, :func:`load` binds all of them at once, and :func:`call` / :func:`opened` turn the
library's failures into exceptions.
"""
import contextlib
import ctypes
import os

from . import build
from .exceptions import EngineError

_vp, _i64, _int, _str, _dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_char_p, ctypes.c_double
_names = ctypes.POINTER(ctypes.c_char_p)
_image = [_vp, _i64, _str]      # (image, size, name): a file's bytes and what to call it in messages

#: every ``pb_*`` function the library exports: name -> (restype, argtypes), as the C definitions have them
SIGNATURES = {
    "pb_last_error": (_str, []),
    "pb_open": (_vp, [_str]),
    "pb_open_indexed": (_vp, [_str, _str]),
    "pb_open_sam": (_vp, [_str]),
    "pb_close": (None, [_vp]),
    "pb_load": (_int, [_vp, _int]),
    "pb_load_regions": (_int, [_vp, _int, _int, _names, _vp, _vp]),
    "pb_resolve_regions": (_int, [_vp, _int, _names] + [_vp] * 9),
    "pb_resolve_chunks": (_int, [_vp, _int, _names, _vp, _vp, _i64] + [_vp] * 8),
    "pb_nref": (_int, [_vp]),
    "pb_ref_name": (_str, [_vp, _int]),
    "pb_ref_length": (ctypes.c_int32, [_vp, _int]),
    "pb_counts": (_int, [_vp, _vp]),
    "pb_wide_count": (_i64, [_vp]),
    "pb_fill_wide": (_int, [_vp] * 4),
    "pb_fill": (_int, [_vp] * 8),
    "pb_fill_nh": (_int, [_vp] * 2),
    "pb_fill_sam": (_int, [_vp] * 4),
    "pb_load_sorted": (_int, [_vp, _int]),
    "pb_sort_stats": (_int, [_vp, _vp]),
    "pb_file_order": (_int, [_vp, _vp]),
    # count tracks as text (track_host.h)
    "pb_track_read": (_vp, _image),
    "pb_track_close": (None, [_vp]),
    "pb_track_rows": (_i64, [_vp]),
    "pb_track_nchrom": (_int, [_vp]),
    "pb_track_chrom": (_str, [_vp, _int]),
    "pb_track_fill": (_int, [_vp] * 7),
    "pb_track_stats": (_int, [_vp, _vp]),
    "pb_track_writer_open": (_vp, []),
    "pb_track_writer_close": (None, [_vp]),
    "pb_track_writer_add": (_int, [_vp, _int, _str, _vp, _i64]),
    "pb_track_writer_add_counts": (_int, [_vp, _int, _int, _str, _vp, _i64, _i64]),
    "pb_track_writer_size": (_i64, [_vp]),
    "pb_track_writer_text": (_vp, [_vp]),       # (text of pb_track_writer_size bytes: read with string_at)
    "pb_track_writer_stats": (_int, [_vp, _vp]),
    "pb_float_repr": (_int, [_vp, _i64, _vp, _vp]),
    # bigWig read (bigwig_host.h)
    "pb_bigwig_read": (_vp, _image),
    "pb_bigwig_close": (None, [_vp]),
    "pb_bigwig_rows": (_i64, [_vp]),
    "pb_bigwig_nchrom": (_int, [_vp]),
    "pb_bigwig_chrom": (_str, [_vp, _int]),
    "pb_bigwig_chrom_size": (_i64, [_vp, _int]),
    "pb_bigwig_nblocks": (_i64, [_vp]),
    "pb_bigwig_fill": (_int, [_vp] * 8),
    "pb_bigwig_stats": (_int, [_vp, _vp]),
    # zlib encoder and bigWig writer (deflate_host.h, bigwig_write_host.h)
    "pb_deflate_zlib_mode": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _int]),
    "pb_deflate_zlib": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp]),
    "pb_huffman_lengths": (_int, [_vp, _i64, _int, _vp]),
    "pb_bigwig_write_open_zoom": (_vp, [_i64, _i64, _int, _i64]),
    "pb_bigwig_write_open": (_vp, [_i64, _i64, _int]),
    "pb_bigwig_write_close": (None, [_vp]),
    "pb_bigwig_write_add": (_int, [_vp, _str, _i64, _vp, _i64]),
    "pb_bigwig_write_finish": (_int, [_vp]),
    "pb_bigwig_write_size": (_i64, [_vp]),
    "pb_bigwig_write_image": (_vp, [_vp]),
    "pb_bigwig_write_stats": (_int, [_vp, _vp]),
    "pb_bigwig_write_block_types": (_int, [_vp, _vp]),
    "pb_bigwig_write_zoom_stats": (_int, [_vp, _vp, _int, _vp]),
    # zoom levels and binned summaries (bigwig_write_host.h, bigwig_summary_host.h)
    "pb_bigwig_zoom_info": (_int, _image + [_vp, _int, _vp]),
    "pb_bigwig_zoom_read": (_vp, _image + [_i64]),
    "pb_bigwig_zoom_close": (None, [_vp]),
    "pb_bigwig_zoom_rows": (_i64, [_vp]),
    "pb_bigwig_zoom_fill": (_int, [_vp] * 9),
    "pb_bigwig_summary_open": (_vp, _image),
    "pb_bigwig_summary_close": (None, [_vp]),
    "pb_bigwig_summary_nchrom": (_int, [_vp]),
    "pb_bigwig_summary_chrom": (_str, [_vp, _int]),
    "pb_bigwig_summary_query": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    "pb_bigwig_summary_values": (_int, [_i64, _vp, _vp, _i64, _vp, _dbl, _int, _vp]),
    "pb_bigwig_summary_stats": (_int, [_vp, _vp, _int, _vp]),
}

_lib = None


def load():
    """Load the library at ``plastid_amd.build.BAM_LIB`` (built first when the file is missing) and bind every entry of
    :data:`SIGNATURES`, once per process."""
    global _lib
    if _lib is None:
        if not os.path.exists(build.BAM_LIB):
            build.build_bam_library()
        lib = ctypes.CDLL(build.BAM_LIB)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:   # a stale library must fail HERE, not at some later call
                raise EngineError("%s lacks %s: rebuild it with `python -m plastid_amd.build --force`" % (build.BAM_LIB, name))
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def last_error():
    msg = load().pb_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def call(fn, *args, exc=ValueError):
    """``fn(*args)`` of a ``pb_*`` function that can fail: a NULL handle (of a function that returns one) or a non-zero
    status raises `exc` with the library's message; the handle is returned."""
    out = fn(*args)
    if (not out) if fn.restype is _vp else out != 0:
        raise exc(last_error())
    return out


@contextlib.contextmanager
def opened(open_fn, close_fn, *args):
    """The handle ``open_fn(*args)`` gives (``ValueError`` for NULL), closed with `close_fn` on exit."""
    h = call(open_fn, *args)
    try:
        yield h
    finally:
        close_fn(h)


def buffer_of(source, image=False):
    """``(pointer or None, size, name, keep-alive)`` of a file's content for the entry points that take it in memory.
    `source`: a path or an open file (text or binary); with `image` also the bytes themselves, named ``<memory>``.  The
    pointer holds while the keep-alive object does."""
    if image and isinstance(source, (bytes, bytearray, memoryview)):
        data, name = bytes(source), "<memory>"
    elif isinstance(source, (str, bytes, os.PathLike)):
        path = os.fspath(source)
        if not os.path.isfile(path):
            raise IOError("No such file: %r" % (path,))
        with open(path, "rb") as fh:
            data, name = fh.read(), os.fsdecode(path)
    else:
        data, name = source.read(), getattr(source, "name", None)
        data = data.encode("utf-8") if isinstance(data, str) else bytes(data)
        name = name if isinstance(name, str) else "<memory>"
    buf = ctypes.create_string_buffer(data, len(data)) if data else None
    return (ctypes.cast(buf, _vp) if buf is not None else None), len(data), os.fsencode(name), buf


def stats_dict(keys, values, kind=int):
    """A filled stats or timing array as a dict under `keys`."""
    return dict(zip(keys, (kind(x) for x in values)))
