"""Python face of the canary's LDS-path check (``ops/ldspath/ldspath.hip``; the C ABI mirrored
here is declared in ``ops/ldspath/ldspath.h`` and ``ops/ldspath/ldspath_host.h``).

``ldspath_check(device)`` loads ``ops/ldspath/libamdgpu_ldspath.so`` with ctypes and checks,
on every CU, the LDS at every access width, its atomics, the LDS-DMA fill and the transposed
read, and on every SIMD each lane-crossing instruction against its lane map.  ``reduce``,
``lane_map``, ``tr_map`` and ``atomic_expected`` are the host's side on its own and need no
GPU; ``lane_sources`` is the hardware's own account of every lane map.  Missing library => it is
built, or a loud ``RuntimeError`` (never a silent pass).
"""
from __future__ import annotations

import ctypes
import os

from ._sites import SITE_SLOTS, UNWRITTEN, as_records, format_site, load_library, pack_site  # noqa: F401

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ldspath", "libamdgpu_ldspath.so")

WAVES = 4  # per workgroup: records[block * 4 + wave]
STAGES = ("widths", "atomic", "lane", "tr")
SUBS = 48
INJECT = ("lds", "subword", "dma", "atomic", "lane", "tr")
SRC_ZERO = 128  # lane_map code of a lane that reads 0 (64 + l: the second value of lane l)
ATOMIC_WORDS = 512
TR_IMAGE_BYTES = 128 * 1024
TR_FIXED_ROUNDS = 6
# numpy mirror of amdgpu_ldspath_record: 208 bytes
RECORD_DTYPE = [("site_first", "<u4"), ("site_last", "<u4"), ("first_sub", "<u4"), ("first_at", "<u4"),
                ("bad", "<u4", (SUBS,))]


class Record(ctypes.Structure):
    _fields_ = [("site_first", ctypes.c_uint), ("site_last", ctypes.c_uint), ("first_sub", ctypes.c_uint),
                ("first_at", ctypes.c_uint), ("bad", ctypes.c_uint * SUBS)]


_COUNTS = ("lds_errors", "plain_errors", "subword_errors", "conflict_errors", "dma_errors", "lds_atomic_errors",
           "lane_errors", "tr_errors", "unlocated_errors", "ldspath_errors", "waves", "moved")
_INTS = ("launches", "cus_reached", "simds_reached", "cus_expected", "n_bad")
_TAIL = ("blocks", "reps", "steps", "rounds")


class LdsPathResult(ctypes.Structure):
    _fields_ = [(f, ctypes.c_ulonglong) for f in _COUNTS] + \
        [("stage_waves", ctypes.c_ulonglong * 4), ("stage_moved", ctypes.c_ulonglong * 4),
         ("lds_bytes", ctypes.c_ulonglong), ("sub_bad", (ctypes.c_ulonglong * SUBS) * 4),
         ("stage_ms", ctypes.c_double * 4)] + [(f, ctypes.c_int) for f in _INTS] + \
        [("bad_sites", ctypes.c_uint * 16), ("stage_n_bad", ctypes.c_int * 4), ("stage_first_site", ctypes.c_uint * 4),
         ("stage_first_sub", ctypes.c_uint * 4), ("stage_first_at", ctypes.c_uint * 4)] + \
        [(f, ctypes.c_int) for f in _TAIL]


def _declare(lib) -> None:
    uint_p, int_p = ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_int)
    lib.amdgpu_ldspath_run.argtypes = [ctypes.c_int] * 8 + [uint_p, ctypes.c_int, ctypes.POINTER(LdsPathResult),
                                                            ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_ldspath_reduce.argtypes = [ctypes.c_void_p, ctypes.c_int] * 4 + [ctypes.POINTER(LdsPathResult)]
    lib.amdgpu_ldspath_lane_sources.argtypes = [ctypes.c_int, uint_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_ldspath_lane_map.argtypes = [ctypes.c_int, int_p]
    lib.amdgpu_ldspath_tr_map.argtypes = [ctypes.c_int, int_p, int_p]
    lib.amdgpu_ldspath_atomic_expected.argtypes = [ctypes.c_int, ctypes.c_int, uint_p, ctypes.c_int]
    lib.amdgpu_ldspath_describe.argtypes = [ctypes.POINTER(LdsPathResult), ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_ldspath_sizeof.argtypes = [ctypes.c_int]
    lib.amdgpu_ldspath_ops.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    for name in ("run", "reduce", "lane_sources", "lane_map", "tr_map", "atomic_expected", "describe", "sizeof", "ops"):
        getattr(lib, "amdgpu_ldspath_" + name).restype = ctypes.c_int


def load():
    return load_library(LIB_PATH, "build_ldspath", _declare)


def _names(table: int) -> tuple:
    lib = load()
    buf = ctypes.create_string_buffer(128)
    out = []
    for i in range(lib.amdgpu_ldspath_ops(table, -1, None, 0)):
        lib.amdgpu_ldspath_ops(table, i, buf, 128)
        out.append(buf.value.decode())
    return tuple(out)


_TABLES = {"LANE_OPS": 0, "ATOMIC_FORMS": 1, "WIDTH_PASSES": 2, "WIDTH_PASS_KINDS": 3}


def _table(name: str) -> tuple:
    if name not in globals():
        globals()[name] = _names(_TABLES[name])
    return globals()[name]


def __getattr__(name):  # the tables are the library's: read on first use, so importing this module builds nothing
    if name in _TABLES:
        return _table(name)
    raise AttributeError(name)


def _as_dict(lib, r) -> dict:
    out = {f: int(getattr(r, f)) for f in _COUNTS + _INTS + _TAIL}
    out["lds_bytes"] = int(r.lds_bytes)
    out["stage_waves"] = dict(zip(STAGES, (int(v) for v in r.stage_waves)))
    out["stage_moved"] = dict(zip(STAGES, (int(v) for v in r.stage_moved)))
    tables = (_table("WIDTH_PASSES"), _table("ATOMIC_FORMS"), _table("LANE_OPS"), ("tr",))
    # which pass, form or op: only the ones with a wrong word
    out["bad_by"] = {stage: {name: int(r.sub_bad[s][k]) for k, name in enumerate(tables[s]) if r.sub_bad[s][k]}
                     for s, stage in enumerate(STAGES)}
    out["bad_sites"] = [format_site(p) for p in r.bad_sites[:min(r.n_bad, 16)]]
    text = ctypes.create_string_buffer(256)
    out["texts"] = {}
    for s, stage in enumerate(STAGES):
        lib.amdgpu_ldspath_describe(ctypes.byref(r), s, text, 256)
        out["texts"][stage] = text.value.decode(errors="replace")
    lib.amdgpu_ldspath_describe(ctypes.byref(r), -1, text, 256)
    out["error"] = text.value.decode(errors="replace") if out["ldspath_errors"] else ""
    out["widths_ms"], out["atomic_ms"], out["lane_ms"], out["tr_ms"] = (float(v) for v in r.stage_ms)
    out["ms"] = sum(float(v) for v in r.stage_ms)
    out["ok"] = out["ldspath_errors"] == 0
    return out


def ldspath_check(device: int = 0, blocks: int = 0, reps: int = 1, steps: int = 4, rounds: int = 4, inject=None,
                  inject_waves: int = 0, inject_op: int = 0) -> dict:
    """The data path beside the ALUs, in four stages of 4-wave workgroups (one wave per SIMD, one
    workgroup resident per CU) whose waves record their site first and last.  ``lds_widths``:
    ``reps`` repetitions of the width passes (``WIDTH_PASSES``) over the whole LDS allocation;
    ``lds_atomic``: ``steps`` operations per thread and form (``ATOMIC_FORMS``) against the table
    the host predicts; ``lane_xchg``: ``rounds`` rounds of every op of ``LANE_OPS`` against its
    lane map; ``lds_tr``: the transposed read, 6 fixed rounds and ``rounds`` hashed ones.
    ``blocks=0``: 2 workgroups per CU plus up to 3 top-up launches while a CU or SIMD has no
    located record, ``blocks>0``: one launch.  ``inject``: ``lds``, ``subword``, ``dma``, ``lane``
    (op ``inject_op``), ``tr``: the first ``inject_waves`` waves perturb one compared value;
    ``atomic``: the first ``inject_waves`` workgroups perturb one operand of form ``inject_op``.

    Returns the counts (``ldspath_errors`` = ``lds_errors`` (plain + subword + conflict) +
    ``lds_atomic_errors`` + ``lane_errors`` + ``tr_errors`` + ``unlocated_errors``, and
    ``dma_errors`` while ``lds_errors`` is 0), ``waves``, ``moved``, ``launches``,
    ``cus_reached`` / ``cus_expected``, ``simds_reached``, ``lds_bytes``, ``bad_by`` (stage ->
    pass, form or op -> wrong words), ``bad_sites`` (the first 16), ``wave_sites`` (stage -> the
    site of each wave of the first launch), ``texts`` (stage -> its error text), ``error`` (the
    first failing stage's), the device ms per stage and ``ok``."""
    kind = -1 if inject is None else INJECT.index(inject)
    lib = load()
    r = LdsPathResult()
    n_waves = WAVES * (int(blocks) if blocks > 0 else 2 * 1024)  # automatic: room for 1024 CUs
    wave_sites = (ctypes.c_uint * (len(STAGES) * n_waves))()
    err = ctypes.create_string_buffer(512)
    rc = lib.amdgpu_ldspath_run(int(device), int(blocks), int(reps), int(steps), int(rounds), kind, int(inject_waves),
                                int(inject_op), wave_sites, n_waves, ctypes.byref(r), err, 512)
    if rc != 0:
        raise RuntimeError("ldspath_check failed: " + err.value.decode(errors="replace"))
    out = _as_dict(lib, r)
    out["wave_sites"] = {stage: [format_site(p) for p in wave_sites[s * n_waves:(s + 1) * n_waves] if p != UNWRITTEN]
                         for s, stage in enumerate(STAGES)}
    return out


def records(rows) -> "numpy.ndarray":  # noqa: F821
    """A record array from ``(site_first, site_last, first_sub, first_at, {sub: wrong words})`` rows."""
    import numpy as np

    a = np.zeros(len(rows), dtype=RECORD_DTYPE)
    for i, (site_first, site_last, first_sub, first_at, bad) in enumerate(rows):
        a[i]["site_first"], a[i]["site_last"], a[i]["first_sub"], a[i]["first_at"] = site_first, site_last, first_sub, first_at
        for k, v in dict(bad).items():
            a[i]["bad"][k] = v
    return a


def reduce(widths=None, atomic=None, lane=None, tr=None) -> dict:
    """The check's host reduction on caller-supplied records of the four stages (numpy arrays of
    ``RECORD_DTYPE``, or rows for ``records()``), no GPU.  Returns what ``ldspath_check`` returns
    except the coverage target, the device times and ``wave_sites``."""
    arrays = [as_records(a, RECORD_DTYPE, records) for a in (widths, atomic, lane, tr)]
    lib = load()
    r = LdsPathResult()
    args = []
    for a in arrays:
        args += [a.ctypes.data if a.size else None, int(a.size)]
    if lib.amdgpu_ldspath_reduce(*args, ctypes.byref(r)) != 0:
        raise ValueError("ldspath.reduce: bad arguments (sites below %d)" % SITE_SLOTS)
    return _as_dict(lib, r)


def lane_map(op: int) -> list:
    """The table's lane map of op ``op`` (index into ``LANE_OPS``): one list of 64 source codes per
    output (two for the swaps): 0..63 the ``x`` of that lane, ``64 + l`` the second value of lane
    ``l`` (what DPP and writelane keep, the swaps' other operand), ``SRC_ZERO`` a zero."""
    out = (ctypes.c_int * 128)()
    n = load().amdgpu_ldspath_lane_map(int(op), out)
    if n < 1:
        raise ValueError("ldspath.lane_map: no op %r" % (op,))
    return [list(out[o * 64:(o + 1) * 64]) for o in range(n)]


def tr_map(round_: int):
    """Round ``round_`` of the transposed read: ``(addresses, sources)``, the byte address each
    of the 64 lanes supplies and, per lane, the four 16-bit element indices it receives."""
    addr, src = (ctypes.c_int * 64)(), (ctypes.c_int * 256)()
    if load().amdgpu_ldspath_tr_map(int(round_), addr, src) != 0:
        raise ValueError("ldspath.tr_map: no round %r" % (round_,))
    return list(addr), [list(src[4 * l:4 * l + 4]) for l in range(64)]


def atomic_expected(form: int, steps: int) -> list:
    """The 512 words form ``form`` (index into ``ATOMIC_FORMS``) holds after ``steps`` steps of 256 threads."""
    out = (ctypes.c_uint * ATOMIC_WORDS)()
    if load().amdgpu_ldspath_atomic_expected(int(form), int(steps), out, ATOMIC_WORDS) != 0:
        raise ValueError("ldspath.atomic_expected: bad arguments (form %r, steps %r)" % (form, steps))
    return list(out)


def lane_sources(device: int = 0) -> list:
    """What the hardware does: one wave with ``x = lane`` and the second value ``64 + lane`` runs
    every op of ``LANE_OPS`` once; returns per op one list of the 64 values received per output,
    comparable with ``lane_map`` (a lane that reads 0 shows 0, not ``SRC_ZERO``)."""
    lib = load()
    n = lib.amdgpu_ldspath_ops(0, -1, None, 0)
    out = (ctypes.c_uint * (n * 128))()
    err = ctypes.create_string_buffer(512)
    if lib.amdgpu_ldspath_lane_sources(int(device), out, n * 128, err, 512) != 0:
        raise RuntimeError("lane_sources failed: " + err.value.decode(errors="replace"))
    res = []
    for k in range(n):
        both = [list(out[(2 * k + o) * 64:(2 * k + o + 1) * 64]) for o in range(2)]
        res.append(both if both[1][0] != UNWRITTEN else both[:1])
    return res
