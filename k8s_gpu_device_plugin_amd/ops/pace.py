"""Python face of the canary's pace check (``ops/pace/pace.hip``; the C ABI mirrored here is
declared in ``ops/pace/pace.h`` and ``ops/pace/pace_host.h``).

``pace_check(device)`` loads ``ops/pace/libamdgpu_pace.so`` with ctypes and measures, inside
kernels, the shader clock every XCD ran, the cycles every SIMD needed per MFMA and the time
every XCD's workgroups needed to stream the same bytes from memory.  ``reduce`` is the host's
reduction of the waves' records on its own and needs no GPU.  Missing library => it is built,
or a loud ``RuntimeError`` (never a silent pass).
"""
from __future__ import annotations

import ctypes
import os

from ._sites import SITE_SLOTS, UNWRITTEN, XCCS, as_records, format_site, load_library, pack_site  # noqa: F401
from ._sites import xcc_names as _xcc_names

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pace", "libamdgpu_pace.so")

WAVES = 4  # per workgroup: records[block * 4 + wave]
INJECT = ("slow_xcc", "slow_waves", "result")
# numpy mirror of amdgpu_pace_record: 32 bytes
RECORD_DTYPE = [("site_first", "<u4"), ("site_last", "<u4"), ("cycles", "<u8"), ("ticks", "<u8"), ("work", "<u4"),
                ("bad", "<u4")]


class Record(ctypes.Structure):
    _fields_ = [("site_first", ctypes.c_uint), ("site_last", ctypes.c_uint), ("cycles", ctypes.c_ulonglong),
                ("ticks", ctypes.c_ulonglong), ("work", ctypes.c_uint), ("bad", ctypes.c_uint)]


class SiteSlot(ctypes.Structure):
    _fields_ = [("cycles_per_mfma", ctypes.c_double), ("clock_mhz", ctypes.c_double), ("waves", ctypes.c_uint),
                ("bad", ctypes.c_uint)]


class XccSlot(ctypes.Structure):
    _fields_ = [("clock_mhz", ctypes.c_double), ("cycles_per_mfma", ctypes.c_double), ("us_per_mib", ctypes.c_double),
                ("waves", ctypes.c_uint), ("blocks", ctypes.c_uint), ("bad_mfma", ctypes.c_ulonglong),
                ("bad_mem", ctypes.c_ulonglong)]


_COUNTS = ("mfma_errors", "mem_errors", "unlocated_errors", "pace_errors", "waves", "moved", "mem_waves", "mem_moved")
_FIGURES = ("tick_mhz", "clock_max_mhz", "slow_ratio", "clock_mhz_min", "clock_mhz_max", "clock_mhz_median",
            "clock_fraction", "xcd_pace_ratio", "xcd_mem_ratio", "cycles_per_mfma_min", "cycles_per_mfma_median",
            "cycles_per_mfma_max", "us_per_mib_median", "us_per_mib_max", "mfma_ms", "fill_ms", "mem_ms")
_INTS = ("launches", "cus_reached", "simds_reached", "cus_expected", "mem_cus_reached", "xccs_reached",
         "mem_xccs_reached", "pace_xcc", "mem_xcc", "n_bad")
_TAIL = ("slow_xccs_clock", "slow_xccs_cycles", "slow_xccs_mem", "iters", "slice_kb", "blocks", "mem_blocks")


class PaceResult(ctypes.Structure):
    _fields_ = [(f, ctypes.c_ulonglong) for f in _COUNTS] + [(f, ctypes.c_double) for f in _FIGURES] + \
        [(f, ctypes.c_int) for f in _INTS] + [("bad_sites", ctypes.c_uint * 16), ("n_slow", ctypes.c_int),
                                              ("slow_sites", ctypes.c_uint * 16)] + \
        [(f, ctypes.c_uint) for f in _TAIL[:3]] + [(f, ctypes.c_int) for f in _TAIL[3:]]


def _declare(lib) -> None:
    lib.amdgpu_pace_run.argtypes = [ctypes.c_int] * 4 + [ctypes.c_double] + [ctypes.c_int] * 4 + \
        [ctypes.POINTER(SiteSlot), ctypes.POINTER(XccSlot), ctypes.POINTER(ctypes.c_uint), ctypes.c_int,
         ctypes.POINTER(PaceResult), ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_pace_run.restype = ctypes.c_int
    lib.amdgpu_pace_reduce.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + \
        [ctypes.c_double] * 3 + [ctypes.POINTER(SiteSlot), ctypes.POINTER(XccSlot), ctypes.POINTER(PaceResult)]
    lib.amdgpu_pace_reduce.restype = ctypes.c_int
    lib.amdgpu_pace_describe.argtypes = [ctypes.POINTER(PaceResult), ctypes.POINTER(XccSlot), ctypes.c_char_p,
                                         ctypes.c_int]
    lib.amdgpu_pace_describe.restype = ctypes.c_int
    lib.amdgpu_pace_note.argtypes = [ctypes.POINTER(PaceResult), ctypes.POINTER(XccSlot), ctypes.POINTER(SiteSlot),
                                     ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_pace_note.restype = ctypes.c_int
    lib.amdgpu_pace_sizeof.argtypes = [ctypes.c_int]
    lib.amdgpu_pace_sizeof.restype = ctypes.c_int
    lib.amdgpu_pace_default_iters.argtypes = []
    lib.amdgpu_pace_default_iters.restype = ctypes.c_int


def load():
    return load_library(LIB_PATH, "build_pace", _declare)


def default_iters() -> int:
    return int(load().amdgpu_pace_default_iters())


def _as_dict(lib, r, sites, xccs) -> dict:
    out = {f: int(getattr(r, f)) for f in _COUNTS + _INTS + _TAIL[3:] + ("n_slow",)}
    out.update({f: float(getattr(r, f)) for f in _FIGURES})
    out["xccs"] = {"xcc%d" % x: {"clock_mhz": s.clock_mhz, "cycles_per_mfma": s.cycles_per_mfma,
                                 "us_per_mib": s.us_per_mib, "waves": int(s.waves), "blocks": int(s.blocks),
                                 "bad_mfma": int(s.bad_mfma), "bad_mem": int(s.bad_mem),
                                 "bad": int(s.bad_mfma) + int(s.bad_mem)}
                   for x, s in enumerate(xccs) if s.waves or s.blocks or s.bad_mem}
    out["sites"] = {format_site(p): {"cycles_per_mfma": s.cycles_per_mfma, "clock_mhz": s.clock_mhz,
                                     "waves": int(s.waves), "bad": int(s.bad)}
                    for p, s in enumerate(sites) if s.waves}
    out["bad_sites"] = [format_site(p) for p in r.bad_sites[:min(r.n_bad, 16)]]
    out["slow_sites"] = [format_site(p) for p in r.slow_sites[:min(r.n_slow, 16)]]
    out["slow_xccs_by"] = {"clock": _xcc_names(r.slow_xccs_clock), "cycles": _xcc_names(r.slow_xccs_cycles),
                           "mem": _xcc_names(r.slow_xccs_mem)}
    out["slow_xccs"] = _xcc_names(r.slow_xccs_clock | r.slow_xccs_cycles | r.slow_xccs_mem)
    out["pace_xcc"] = None if r.pace_xcc < 0 else "xcc%d" % r.pace_xcc
    out["mem_xcc"] = None if r.mem_xcc < 0 else "xcc%d" % r.mem_xcc
    text = ctypes.create_string_buffer(256)
    lib.amdgpu_pace_note(ctypes.byref(r), xccs, sites, text, 256)
    out["note"] = text.value.decode(errors="replace")
    lib.amdgpu_pace_describe(ctypes.byref(r), xccs, text, 256)
    out["error"] = text.value.decode(errors="replace") if out["pace_errors"] else ""
    out["ms"] = out["mfma_ms"] + out["fill_ms"] + out["mem_ms"]
    out["ok"] = out["pace_errors"] == 0  # slowness is reported, never a failure here
    return out


def pace_check(device: int = 0, blocks: int = 0, iters: int = 0, slice_kb: int = 1024, slow_ratio: float = 1.5,
               inject=None, inject_xcc: int = 0, inject_factor: int = 4, inject_waves: int = 0) -> dict:
    """Where on the partition time goes, in two stages of 4-wave workgroups (one wave per SIMD,
    one workgroup resident per CU) whose waves record their site and bracket their work with
    the shader-clock counter and the constant-rate counter.  ``pace_mfma``: ``iters``
    iterations (0: the default) of four MFMA accumulator chains, verified against their closed
    form; ``blocks=0``: 2 workgroups per CU plus up to 3 top-up launches while a CU or SIMD has
    no located record, ``blocks>0``: one launch.  ``pace_mem``: workgroup ``b`` streams slice
    ``b`` (``slice_kb`` KiB) of a buffer an earlier launch filled and compares every word;
    ``blocks=0``: one workgroup per CU.  ``inject``: ``slow_xcc`` (every wave on ``inject_xcc``
    does ``inject_factor`` times the work it records), ``slow_waves`` (the first
    ``inject_waves`` MFMA waves do), ``result`` (lane 3 of the first ``inject_waves`` waves
    perturbs one operand of the last MFMA).

    Returns the counts (``pace_errors`` = ``mfma_errors`` + ``mem_errors`` +
    ``unlocated_errors``; ``waves``, ``moved``, ``launches``, ``cus_reached`` /
    ``cus_expected``, ``simds_reached``), ``xccs`` (``"xcc5"`` -> ``clock_mhz``,
    ``cycles_per_mfma``, ``us_per_mib``, ``waves``, ``blocks``, ``bad``), ``sites`` (site ->
    ``cycles_per_mfma``, ``clock_mhz``, ``waves``, ``bad``), ``wave_sites`` /
    ``mem_wave_sites`` (the site of each wave of the first launch of either kernel),
    ``clock_mhz_min`` / ``clock_mhz_max`` over XCDs, ``clock_max_mhz`` (the part's maximum) and
    ``clock_fraction``, ``xcd_pace_ratio`` and ``xcd_mem_ratio`` (1.0 when balanced, below 1
    when one XCD lags: ``pace_xcc`` / ``mem_xcc``), ``slow_sites`` (the first 16 of ``n_slow``),
    ``slow_xccs`` (and ``slow_xccs_by``: clock, cycles, mem), ``mfma_ms``, ``mem_ms``, ``ms``,
    ``note`` (what was slow, in words), ``error`` (the text of the first failing stage) and
    ``ok``.  Only wrong results clear ``ok``: slowness is reported."""
    kind = -1 if inject is None else INJECT.index(inject)
    lib = load()
    r = PaceResult()
    sites = (SiteSlot * SITE_SLOTS)()
    xccs = (XccSlot * XCCS)()
    n_waves = WAVES * (int(blocks) if blocks > 0 else 2 * 1024)  # automatic: room for 1024 CUs
    wave_sites = (ctypes.c_uint * (2 * n_waves))()  # pace_mfma's, then pace_mem's
    err = ctypes.create_string_buffer(512)
    rc = lib.amdgpu_pace_run(int(device), int(blocks), int(iters) if iters else default_iters(), int(slice_kb),
                             float(slow_ratio), kind, int(inject_xcc), int(inject_factor), int(inject_waves), sites,
                             xccs, wave_sites, n_waves, ctypes.byref(r), err, 512)
    if rc != 0:
        raise RuntimeError("pace_check failed: " + err.value.decode(errors="replace"))
    out = _as_dict(lib, r, sites, xccs)
    out["wave_sites"] = [format_site(p) for p in wave_sites[:n_waves] if p != UNWRITTEN]  # unwritten: all-ones
    out["mem_wave_sites"] = [format_site(p) for p in wave_sites[n_waves:] if p != UNWRITTEN]
    return out


def records(rows) -> "numpy.ndarray":  # noqa: F821
    """A record array from ``(site_first, site_last, cycles, ticks, work, bad)`` rows."""
    import numpy as np

    return np.array([tuple(int(v) for v in row) for row in rows], dtype=RECORD_DTYPE)


def reduce(mfma_records, tick_mhz: float, clock_max_mhz: float, slow_ratio: float = 1.5, mem_records=None) -> dict:
    """The check's host reduction on caller-supplied records (numpy arrays of ``RECORD_DTYPE``,
    or rows for ``records()``), no GPU: ``mfma_records`` in launch order, ``mem_records`` (four
    per workgroup, wave 0 first) optional.  Returns what ``pace_check`` returns except the
    coverage target, the device times and ``wave_sites``."""
    a, m = (as_records(x, RECORD_DTYPE, records) for x in (mfma_records, mem_records))
    lib = load()
    r = PaceResult()
    sites = (SiteSlot * SITE_SLOTS)()
    xccs = (XccSlot * XCCS)()
    rc = lib.amdgpu_pace_reduce(a.ctypes.data if a.size else None, int(a.size), m.ctypes.data if m.size else None,
                                int(m.size), float(tick_mhz), float(clock_max_mhz), float(slow_ratio), sites, xccs,
                                ctypes.byref(r))
    if rc != 0:
        raise ValueError("pace.reduce: bad arguments (tick_mhz > 0, clock_max_mhz >= 0, slow_ratio >= 1, sites below "
                         "%d, four memory records per workgroup)" % SITE_SLOTS)
    return _as_dict(lib, r, sites, xccs)
