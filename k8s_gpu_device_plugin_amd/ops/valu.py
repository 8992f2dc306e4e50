"""Python face of the stand-alone vector-ALU check (``ops/valu/valu.hip``; the C ABI mirrored here
is declared in ``ops/valu/valu.h`` and ``ops/valu/valu_host.h``, the ops in ``ops/valu/valu_ops.h``).

``valu_check(device)`` loads ``ops/valu/libamdgpu_valu.so`` with ctypes and runs, on every CU and
SIMD, every op of ``OPS``: the vector-ALU instructions no other kernel of the canary issues.  An
*exact* op is compared bit for bit with a host reference; a *consensus* op (the transcendentals,
``prng``, stochastic rounding) with what most waves computed.  ``expected``, ``operands`` and
``reduce`` are the host's side on its own and need no GPU; ``raw`` runs one op on caller-supplied
operand words.  ``canary.run()`` and the plugin do not call this check yet.  Missing library =>
it is built, or a loud ``RuntimeError`` (never a silent pass).

``python -m k8s_gpu_device_plugin_amd.ops.valu [--device N] [--ops a,b,...] [--rounds R]`` prints
one JSON line.
"""
from __future__ import annotations

import ctypes
import functools
import os

from ._sites import SITE_SLOTS, UNWRITTEN, as_records, format_site, load_library, pack_site  # noqa: F401

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "valu", "libamdgpu_valu.so")

WAVES = 4         # per workgroup: records[block * 4 + wave]
MAX_OPS = 128     # room in a result
GROUP_OPS = 32    # room for a group's ops in a record
MAX_GROUPS = 8
MAX_ROUNDS = 16
MAX_RESULTS = 32  # a lane's raw result words
WIDE = 32         # elements of a wide conversion's operand (``expand``)
ROUNDS = 8        # the default: the largest power of two whose ms stays below site_probe's (docs/CANARY.md, "The vector ALU")
SEED = 0x56414C55
INJECT_LANE = 3
# (tests/test_valu_abi.py compares each of the constants above with the library's own)
# numpy mirror of amdgpu_valu_record: 272 bytes
RECORD_DTYPE = [("site_first", "<u4"), ("site_last", "<u4"), ("first_op", "<u4"), ("first_lane", "<u4"),
                ("bad", "<u4", (GROUP_OPS,)), ("digest", "<u4", (GROUP_OPS,))]
_INFO = ("group", "cls", "kind_a", "kind_b", "kind_c", "results", "rkind")
CLASSES = ("exact", "consensus")


class Record(ctypes.Structure):
    _fields_ = [("site_first", ctypes.c_uint), ("site_last", ctypes.c_uint), ("first_op", ctypes.c_uint),
                ("first_lane", ctypes.c_uint), ("bad", ctypes.c_uint * GROUP_OPS), ("digest", ctypes.c_uint * GROUP_OPS)]


_COUNTS = ("unlocated_errors", "valu_errors", "waves", "moved")
_INTS = ("launches", "cus_reached", "simds_reached", "cus_expected", "n_bad")
_TAIL = ("blocks", "rounds")


class ValuResult(ctypes.Structure):
    _fields_ = [("errors", ctypes.c_ulonglong * MAX_OPS), ("group_errors", ctypes.c_ulonglong * MAX_GROUPS)] + \
        [(f, ctypes.c_ulonglong) for f in _COUNTS] + [("group_ms", ctypes.c_double * MAX_GROUPS), ("ms", ctypes.c_double)] + \
        [(f, ctypes.c_int) for f in _INTS] + \
        [("bad_sites", ctypes.c_uint * 16), ("op_n_bad", ctypes.c_int * MAX_OPS), ("op_first_site", ctypes.c_uint * MAX_OPS),
         ("op_first_lane", ctypes.c_uint * MAX_OPS), ("selected", ctypes.c_ubyte * MAX_OPS),
         ("unjudged", ctypes.c_ubyte * MAX_OPS)] + [(f, ctypes.c_int) for f in _TAIL]


EXPORTS = ("run", "reduce", "raw", "operands", "expected", "expand", "ops", "op_ints", "kind", "describe", "sizeof")


def _declare(lib) -> None:
    uint_p, res_p = ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ValuResult)
    lib.amdgpu_valu_run.argtypes = [ctypes.c_int] * 3 + [ctypes.c_uint, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, uint_p,
                                                         ctypes.c_int, res_p, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_valu_reduce.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, res_p]
    lib.amdgpu_valu_raw.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_valu_operands.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_int] + [ctypes.c_void_p] * 3
    lib.amdgpu_valu_expected.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_void_p]
    lib.amdgpu_valu_ops.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_valu_op_ints.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.amdgpu_valu_describe.argtypes = [res_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_valu_sizeof.argtypes = [ctypes.c_int]
    lib.amdgpu_valu_expand.argtypes = [ctypes.c_int, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_void_p]
    lib.amdgpu_valu_kind.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    for name in EXPORTS:
        getattr(lib, "amdgpu_valu_" + name).restype = ctypes.c_int


def load():
    return load_library(LIB_PATH, "build_valu", _declare)


@functools.lru_cache(None)
def _names(what: int) -> tuple:
    lib = load()
    buf = ctypes.create_string_buffer(128)
    out = []
    for i in range(lib.amdgpu_valu_ops(-1, 0, None, 0)):
        lib.amdgpu_valu_ops(i, what, buf, 128)
        out.append(buf.value.decode())
    return tuple(out)


_TABLES = {"OPS": 0, "MNEMONICS": 1, "OP_GROUPS": 2, "GROUPS": None}


def _table(name: str) -> tuple:
    return tuple(dict.fromkeys(_names(2))) if name == "GROUPS" else _names(_TABLES[name])


@functools.lru_cache(None)
def kind_name(kind: int) -> str:
    """The name of an operand kind of ``ops/valu/valu_ops.h`` (``f32_pos``, ``enc_fp8``, ...)."""
    buf = ctypes.create_string_buffer(32)
    if load().amdgpu_valu_kind(int(kind), buf, 32) < 0:
        raise ValueError("valu: no operand kind %r" % (kind,))
    return buf.value.decode()


def __getattr__(name):  # the table is the library's (kOps): read on first use, so importing this module builds nothing
    if name in _TABLES:
        return _table(name)
    raise AttributeError(name)


def op_index(op) -> int:
    """The index into ``OPS`` of a name or an index."""
    names = _table("OPS")
    if isinstance(op, str):
        if op not in names:
            raise ValueError("valu: no op %r (have %s)" % (op, ", ".join(names)))
        return names.index(op)
    if not 0 <= int(op) < len(names):
        raise ValueError("valu: no op %r" % (op,))
    return int(op)


def op_info(op) -> dict:
    """The table's row: ``name``, ``mnemonic``, ``group`` (a name of ``GROUPS``), ``cls`` (``exact``
    or ``consensus``), ``kinds`` (the names of the operand kinds of a, b, c; ``none``: unused), ``wide`` (its operand
    word a stands for 32 elements: ``expand``), ``results`` (32-bit
    result words), ``rkind`` (0 bits, 1 f32, 2 f64 as word pairs, 3 two f16) and ``slot`` (its place
    in its group's records)."""
    i = op_index(op)
    out = (ctypes.c_int * 7)()
    load().amdgpu_valu_op_ints(i, out)
    d = dict(zip(_INFO, (int(v) for v in out)))
    groups = _table("OP_GROUPS")
    return {"index": i, "name": _table("OPS")[i], "mnemonic": _table("MNEMONICS")[i], "group": groups[i],
            "cls": CLASSES[d["cls"]], "kinds": tuple(kind_name(d[k]) for k in ("kind_a", "kind_b", "kind_c")),
            "wide": kind_name(d["kind_a"]) in ("fp6_codes", "enc_seed"), "results": d["results"],
            "rkind": d["rkind"], "slot": i - groups.index(groups[i])}


def _selected(ops):
    names = _table("OPS")
    sel = (ctypes.c_ubyte * MAX_OPS)()
    for i in (range(len(names)) if ops is None else [op_index(o) for o in ops]):
        sel[i] = 1
    return sel


def _as_dict(lib, r) -> dict:
    names, groups, of = _table("OPS"), _table("GROUPS"), _table("OP_GROUPS")
    selected = [i for i in range(len(names)) if r.selected[i]]
    used = [g for g in groups if any(of[i] == g for i in selected)]
    out = {f: int(getattr(r, f)) for f in _COUNTS + _INTS + _TAIL}
    out["ops"] = [names[i] for i in selected]
    out["errors"] = {names[i]: int(r.errors[i]) for i in selected}
    out["group_errors"] = {g: int(r.group_errors[groups.index(g)]) for g in used}
    out["bad_sites"] = [format_site(p) for p in r.bad_sites[:min(r.n_bad, 16)]]
    out["bad_by"] = {names[i]: {"sites": int(r.op_n_bad[i]), "first_site": format_site(r.op_first_site[i]),
                                "first_lane": None if r.op_first_lane[i] == UNWRITTEN else int(r.op_first_lane[i])}
                     for i in selected if r.errors[i]}
    out["unjudged"] = [names[i] for i in selected if r.unjudged[i]]
    text = ctypes.create_string_buffer(256)
    lib.amdgpu_valu_describe(ctypes.byref(r), -1, text, 256)
    out["error"] = text.value.decode(errors="replace") if out["valu_errors"] else ""
    out["group_ms"] = {g: float(r.group_ms[groups.index(g)]) for g in used}
    out["ms"] = float(r.ms)
    out["ok"] = out["valu_errors"] == 0
    return out


def valu_check(device: int = 0, blocks: int = 0, rounds=None, ops=None, seed: int = SEED, inject_op=None,
               inject_waves: int = 0) -> dict:
    """One ``valu_sweep`` kernel per group that holds one of ``ops`` (names or indices, default: all
    of ``OPS``): 4-wave workgroups (one wave per SIMD, one workgroup resident per CU) whose waves
    record their site first and last, run ``rounds`` rounds (1..16, default ``ROUNDS``) of every
    selected op on operands that depend on (seed, op, round, lane) only, fold the result words into
    one digest per lane and op and compare it with the host's (exact ops), or leave the wave's
    digest for the host's majority vote (consensus ops).  ``blocks=0``: 2 workgroups per CU plus up
    to 3 top-up launches while a CU or SIMD has no located record of some selected group,
    ``blocks>0``: one launch.  ``inject_op``: lane 3 of the first ``inject_waves`` waves adds 1 to
    the first result word of that op in round 0.

    Returns ``errors`` (op -> located wrong results), ``group_errors``, ``unlocated_errors``,
    ``valu_errors`` (their sum), ``waves`` and ``moved`` (records over all groups), ``launches``,
    ``cus_reached`` / ``cus_expected``, ``simds_reached``, ``bad_sites`` (the first 16), ``bad_by``
    (op -> sites, first site, first lane), ``unjudged`` (consensus ops without a majority),
    ``wave_sites`` (group -> the site of each wave of the first launch), ``error``, ``group_ms``,
    ``ms`` and ``ok``."""
    lib = load()
    groups = _table("GROUPS")
    sel = _selected(ops)
    inject = -1 if inject_op is None else op_index(inject_op)
    r = ValuResult()
    n_waves = WAVES * (int(blocks) if blocks > 0 else 2 * 1024)  # automatic: room for 1024 CUs
    wave_sites = (ctypes.c_uint * (len(groups) * n_waves))()
    err = ctypes.create_string_buffer(512)
    rc = lib.amdgpu_valu_run(int(device), int(blocks), int(ROUNDS if rounds is None else rounds), int(seed) & 0xFFFFFFFF, sel,
                             inject, int(inject_waves), wave_sites, n_waves, ctypes.byref(r), err, 512)
    if rc != 0:
        raise RuntimeError("valu_check failed: " + err.value.decode(errors="replace"))
    out = _as_dict(lib, r)
    out["wave_sites"] = {g: [format_site(p) for p in wave_sites[k * n_waves:(k + 1) * n_waves] if p != UNWRITTEN]
                         for k, g in enumerate(groups) if g in out["group_ms"]}
    return out


def records(rows) -> "numpy.ndarray":  # noqa: F821
    """A record array from ``(site_first, site_last, {slot: wrong lanes}, {slot: digest})`` rows."""
    import numpy as np

    a = np.zeros(len(rows), dtype=RECORD_DTYPE)
    for i, (site_first, site_last, bad, digest) in enumerate(rows):
        a[i]["site_first"], a[i]["site_last"], a[i]["first_op"], a[i]["first_lane"] = site_first, site_last, UNWRITTEN, UNWRITTEN
        for k, v in dict(bad).items():
            a[i]["bad"][k] = v
        for k, v in dict(digest).items():
            a[i]["digest"][k] = v
    return a


def reduce(recs, group_of, ops=None) -> dict:
    """The check's host reduction on caller-supplied records (a numpy array of ``RECORD_DTYPE`` or
    rows for ``records()``); ``group_of[i]`` is the group (a name of ``GROUPS``) record ``i``
    belongs to.  No GPU.  Returns what ``valu_check`` returns except the coverage target, the
    device times and ``wave_sites``."""
    import numpy as np

    a = as_records(recs, RECORD_DTYPE, records)
    groups = _table("GROUPS")
    of = np.ascontiguousarray([groups.index(g) for g in group_of], dtype=np.int32)
    if of.size != a.size:
        raise ValueError("valu.reduce: one group per record")
    lib = load()
    r = ValuResult()
    if lib.amdgpu_valu_reduce(a.ctypes.data if a.size else None, of.ctypes.data if of.size else None, int(a.size),
                              _selected(ops), ctypes.byref(r)) != 0:
        raise ValueError("valu.reduce: bad arguments (sites below %d, groups among those of the selected ops)" % SITE_SLOTS)
    return _as_dict(lib, r)


def operands(op, seed: int = SEED, rounds: int = 1):
    """The operand words ``(a, b, c)`` of the op, host only: uint64 arrays of shape (rounds, 64)."""
    import numpy as np

    a, b, c = (np.zeros((rounds, 64), dtype=np.uint64) for _ in range(3))
    if not 1 <= rounds <= MAX_ROUNDS or load().amdgpu_valu_operands(op_index(op), int(seed) & 0xFFFFFFFF, int(rounds),
                                                                    a.ctypes.data, b.ctypes.data, c.ctypes.data) != 0:
        raise ValueError("valu.operands: bad arguments (rounds %r)" % (rounds,))
    return a, b, c


def expand(op, a: int, c: int):
    """The 32 elements a wide conversion makes of its operand words, host only (uint32): the
    six-bit codes of a pk32 decoder, the f32 encoder inputs of a 2xpk16 encoder."""
    import numpy as np

    out = np.zeros(WIDE, dtype=np.uint32)
    if load().amdgpu_valu_expand(op_index(op), int(a), int(c), out.ctypes.data) != 0:
        raise ValueError("valu.expand: not a wide op")
    return out


def expected(op, seed: int = SEED, rounds: int = 1):
    """The 64 lane digests of an exact op over ``rounds`` rounds (uint32), host only."""
    import numpy as np

    out = np.zeros(64, dtype=np.uint32)
    rc = load().amdgpu_valu_expected(op_index(op), int(seed) & 0xFFFFFFFF, int(rounds), out.ctypes.data)
    if rc == -2:
        raise RuntimeError("vector ALU check: a generated case of %s is not a normal number or a zero" % op_info(op)["name"])
    if rc != 0:
        raise ValueError("valu.expected: bad arguments (an exact op, rounds %r in 1..%d)" % (rounds, MAX_ROUNDS))
    return out


def fold(words):
    """The lane digests of result words (..., 64, n): ``rotl(digest, 5) ^ word * 0x9E3779B1`` over
    the leading axes in order, then over the words."""
    import numpy as np

    w = np.asarray(words, dtype=np.uint64).reshape(-1, 64, np.shape(words)[-1])
    d = np.zeros(64, dtype=np.uint64)
    for r in range(w.shape[0]):
        for i in range(w.shape[2]):
            d = (((d << np.uint64(5)) | (d >> np.uint64(27))) ^ (w[r, :, i] * np.uint64(0x9E3779B1))) & np.uint64(0xFFFFFFFF)
    return d.astype(np.uint32)


def raw(op, a, b=None, c=None, device: int = 0):
    """One op on caller-supplied operand words: ``a``, ``b``, ``c`` uint64 of shape (n, 64) (default
    zeros).  Returns every lane's result words, uint32 (n, 64, results)."""
    import numpy as np

    a = np.ascontiguousarray(a, dtype=np.uint64)
    b, c = (np.zeros_like(a) if x is None else np.ascontiguousarray(x, dtype=np.uint64) for x in (b, c))
    n = a.shape[0]
    if a.shape != (n, 64) or b.shape != a.shape or c.shape != a.shape:
        raise ValueError("valu.raw: operands of shape (n, 64)")
    out = np.zeros((n, 64, MAX_RESULTS), dtype=np.uint32)
    err = ctypes.create_string_buffer(512)
    if load().amdgpu_valu_raw(int(device), op_index(op), a.ctypes.data, b.ctypes.data, c.ctypes.data, out.ctypes.data, n,
                              err, 512) != 0:
        raise RuntimeError("valu.raw failed: " + err.value.decode(errors="replace"))
    return out[:, :, :op_info(op)["results"]]


def main(argv=None) -> int:
    import argparse
    import json

    ap = argparse.ArgumentParser(description="The vector-ALU check on one device; prints one JSON line.")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--ops", default=None, help="comma-separated names (default: every op of the table)")
    ap.add_argument("--rounds", type=int, default=None)
    args = ap.parse_args(argv)
    r = valu_check(args.device, ops=args.ops.split(",") if args.ops else None, rounds=args.rounds)
    del r["wave_sites"]
    print(json.dumps(r))
    return 0 if r["ok"] else 1


if __name__ == "__main__":
    import sys

    sys.exit(main())
