"""What the Python faces of the located checks share (``canary.py``, ``pace.py``, ``ldspath.py``,
``hostlink.py``): the packed site of ``ops/site.h``, the ctypes loader and the record
arrays of the host-only reductions.
"""
from __future__ import annotations

import ctypes
import os

XCCS = 16              # HW_REG_XCC_ID is 4 bits wide
SITE_SLOTS = 1 << 14   # packed sites: simd 1:0 | cu 5:2 | sh 6 | se 9:7 | xcc 13:10
UNWRITTEN = 0xFFFFFFFF  # a wave-site entry, or a record's site_first, that no wave wrote


def decode_site(packed: int) -> dict:
    """Fields of a packed site: simd bits 1:0, cu 5:2, sh 6, se 9:7, xcc 13:10 (the layout
    ``site_id()`` in ``ops/canary_common.h`` builds from HW_REG_HW_ID and HW_REG_XCC_ID)."""
    p = int(packed)
    return {"xcc": (p >> 10) & 0xF, "se": (p >> 7) & 0x7, "sh": (p >> 6) & 0x1, "cu": (p >> 2) & 0xF, "simd": p & 0x3}


def format_site(packed: int, simd: bool = True) -> str:
    """``xcc3/se1/sh0/cu7/simd2``: XCD, shader engine, shader array, CU within it, SIMD
    (``xcc3/se1/sh0/cu7`` without ``simd``)."""
    return ("xcc%(xcc)d/se%(se)d/sh%(sh)d/cu%(cu)d/simd%(simd)d" if simd else
            "xcc%(xcc)d/se%(se)d/sh%(sh)d/cu%(cu)d") % decode_site(packed)


def pack_site(xcc: int, se: int = 0, sh: int = 0, cu: int = 0, simd: int = 0) -> int:
    """The packed form of a site, as ``site_id()`` in ``ops/canary_common.h`` builds it."""
    return (int(xcc) & 0xF) << 10 | (int(se) & 0x7) << 7 | (int(sh) & 0x1) << 6 | (int(cu) & 0xF) << 2 | (int(simd) & 0x3)


def xcc_names(mask: int) -> list:
    return ["xcc%d" % x for x in range(XCCS) if mask >> x & 1]


_libs = {}


def load_library(path: str, build: str, declare):
    """The library at ``path``, loaded once: built with ``_build.<build>()`` if the file is
    missing, then ``declare(lib)`` sets the prototypes."""
    lib = _libs.get(path)
    if lib is None:
        if not os.path.exists(path):
            from .. import _build
            getattr(_build, build)(verbose=False)
        lib = ctypes.CDLL(path)
        declare(lib)
        _libs[path] = lib
    return lib


def as_records(a, dtype, from_rows):
    """``a`` as a contiguous record array of ``dtype``: ``None`` is empty, a structured array is
    taken as it is, anything else is rows for ``from_rows``."""
    import numpy as np

    if a is None:
        return np.zeros(0, dtype=dtype)
    a = a if isinstance(a, np.ndarray) and a.dtype.names else from_rows(a)
    return np.ascontiguousarray(a, dtype=dtype)
