"""Python face of the stand-alone matrix-forms check (``ops/matforms/matforms.hip``; the C ABI
mirrored here is declared in ``ops/matforms/matforms.h`` and ``ops/matforms/matforms_host.h``,
the forms in ``ops/matforms/matforms_forms.h``).

``matrix_forms_check(device)`` loads ``ops/matforms/libamdgpu_matforms.so`` with ctypes and runs,
on every CU and SIMD, an exact and located MFMA check of every form of ``FORMS``: f16, i8, f32,
f64, fp6, the mixed MX formats and the 16x16 shapes.  ``reduce``, ``operands``, ``expected``,
``inject_expected``, ``table_map`` and ``encode`` are the host's side on its own and need no GPU;
``raw`` runs single-wave MFMAs on caller-supplied registers and ``operand_map`` drives it with
one-hot operands: the hardware's own account of every operand map.  ``canary.run()`` and the
plugin do not call this check yet.  Missing library => it is built, or a loud ``RuntimeError``
(never a silent pass).

``python -m k8s_gpu_device_plugin_amd.ops.matforms [--device N] [--rates] [--forms a,b,...]``
prints one JSON line.
"""
from __future__ import annotations

import ctypes
import os

from ._sites import SITE_SLOTS, UNWRITTEN, as_records, format_site, load_library, pack_site  # noqa: F401

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "matforms", "libamdgpu_matforms.so")

WAVES = 4        # per workgroup: records[block * 4 + wave]
MAX_FORMS = 16   # room in a record and a result
MAX_KSTEPS = 8
OPERAND_WORDS = 8  # a lane's raw operand
ACC_WORDS = 16     # a lane's raw accumulators
RATE_ITERS = 2048
# numpy mirror of amdgpu_matforms_record: 80 bytes
RECORD_DTYPE = [("site_first", "<u4"), ("site_last", "<u4"), ("first_form", "<u4"), ("first_reg", "<u4"),
                ("bad", "<u4", (MAX_FORMS,))]
_INFO = ("m", "k", "elems", "r", "acc_kind", "acc", "scaled", "bits_a", "bits_b", "map_a", "map_b", "key_offset")


class Record(ctypes.Structure):
    _fields_ = [("site_first", ctypes.c_uint), ("site_last", ctypes.c_uint), ("first_form", ctypes.c_uint),
                ("first_reg", ctypes.c_uint), ("bad", ctypes.c_uint * MAX_FORMS)]


_COUNTS = ("unlocated_errors", "matforms_errors", "waves", "moved")
_INTS = ("launches", "cus_reached", "simds_reached", "cus_expected", "n_bad")
_TAIL = ("blocks", "ksteps", "vary_scale")


class MatFormsResult(ctypes.Structure):
    _fields_ = [("errors", ctypes.c_ulonglong * MAX_FORMS)] + [(f, ctypes.c_ulonglong) for f in _COUNTS] + \
        [("form_waves", ctypes.c_ulonglong * MAX_FORMS), ("tflops", ctypes.c_double * MAX_FORMS),
         ("form_ms", ctypes.c_double * MAX_FORMS), ("ms", ctypes.c_double)] + [(f, ctypes.c_int) for f in _INTS] + \
        [("bad_sites", ctypes.c_uint * 16), ("form_n_bad", ctypes.c_int * MAX_FORMS),
         ("form_first_site", ctypes.c_uint * MAX_FORMS), ("form_first_reg", ctypes.c_uint * MAX_FORMS),
         ("forms", ctypes.c_uint)] + [(f, ctypes.c_int) for f in _TAIL]


EXPORTS = ("run", "reduce", "raw", "operands", "expected", "inject_expected", "map", "forms", "form_ints", "encode",
           "describe", "sizeof")


def _declare(lib) -> None:
    uint_p, int_p = ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_int)
    res_p = ctypes.POINTER(MatFormsResult)
    lib.amdgpu_matforms_run.argtypes = [ctypes.c_int] * 4 + [ctypes.c_uint] + [ctypes.c_int] * 3 + \
        [uint_p, ctypes.c_int, res_p, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_matforms_reduce.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, res_p]
    lib.amdgpu_matforms_raw.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5 + \
        [ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_matforms_operands.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_int] + \
        [ctypes.c_void_p] * 4
    lib.amdgpu_matforms_expected.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.amdgpu_matforms_inject_expected.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.amdgpu_matforms_map.argtypes = [ctypes.c_int, int_p, int_p, int_p, int_p]
    lib.amdgpu_matforms_forms.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_matforms_form_ints.argtypes = [ctypes.c_int, uint_p]
    lib.amdgpu_matforms_encode.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong)]
    lib.amdgpu_matforms_describe.argtypes = [res_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_matforms_sizeof.argtypes = [ctypes.c_int]
    for name in EXPORTS:
        getattr(lib, "amdgpu_matforms_" + name).restype = ctypes.c_int


def load():
    return load_library(LIB_PATH, "build_matforms", _declare)


def _names(what: int) -> tuple:
    lib = load()
    buf = ctypes.create_string_buffer(128)
    out = []
    for i in range(lib.amdgpu_matforms_forms(-1, 0, None, 0)):
        lib.amdgpu_matforms_forms(i, what, buf, 128)
        out.append(buf.value.decode())
    return tuple(out)


_TABLES = {"FORMS": 0, "FORM_TEXTS": 1, "INSTRUCTIONS": 2}


def _table(name: str) -> tuple:
    if name not in globals():
        globals()[name] = _names(_TABLES[name])
    return globals()[name]


def __getattr__(name):  # the table is the library's (kForms): read on first use, so importing this module builds nothing
    if name in _TABLES:
        return _table(name)
    raise AttributeError(name)


def form_index(form) -> int:
    """The index into ``FORMS`` of a name or an index."""
    names = _table("FORMS")
    if isinstance(form, str):
        if form not in names:
            raise ValueError("matforms: no form %r (have %s)" % (form, ", ".join(names)))
        return names.index(form)
    if not 0 <= int(form) < len(names):
        raise ValueError("matforms: no form %r" % (form,))
    return int(form)


def form_info(form) -> dict:
    """The table's row: ``m``, ``k`` (of one MFMA), ``elems`` (per lane and operand), ``r``
    (values in [-r, r]), ``acc_kind`` (0 f32, 1 i32, 2 f64), ``acc`` (accumulators per lane),
    ``scaled``, ``bits_a`` / ``bits_b``, ``map_a`` / ``map_b`` (0 linear, 1 halves), ``key_offset``,
    and ``name``, ``text``, ``instruction``."""
    f = form_index(form)
    out = (ctypes.c_uint * 12)()
    load().amdgpu_matforms_form_ints(f, out)
    d = dict(zip(_INFO, (int(v) for v in out)))
    d.update(index=f, name=_table("FORMS")[f], text=_table("FORM_TEXTS")[f], instruction=_table("INSTRUCTIONS")[f])
    return d


def _mask(forms) -> int:
    if forms is None:
        return (1 << len(_table("FORMS"))) - 1
    mask = 0
    for f in forms:
        mask |= 1 << form_index(f)
    return mask


def _as_dict(lib, r) -> dict:
    names = _table("FORMS")
    selected = [f for f in range(len(names)) if r.forms >> f & 1]
    out = {f: int(getattr(r, f)) for f in _COUNTS + _INTS + _TAIL}
    out["forms"] = [names[f] for f in selected]
    out["errors"] = {names[f]: int(r.errors[f]) for f in selected}
    out["form_waves"] = {names[f]: int(r.form_waves[f]) for f in selected}
    out["bad_sites"] = [format_site(p) for p in r.bad_sites[:min(r.n_bad, 16)]]
    out["bad_by"] = {names[f]: {"sites": int(r.form_n_bad[f]), "first_site": format_site(r.form_first_site[f]),
                                "first_reg": int(r.form_first_reg[f])} for f in selected if r.errors[f]}
    text = ctypes.create_string_buffer(256)
    lib.amdgpu_matforms_describe(ctypes.byref(r), -1, text, 256)
    out["error"] = text.value.decode(errors="replace") if out["matforms_errors"] else ""
    out["form_ms"] = {names[f]: float(r.form_ms[f]) for f in selected}
    out["ms"] = float(r.ms)
    out["tflops"] = {names[f]: float(r.tflops[f]) for f in selected if r.tflops[f] != 0.0}
    out["ok"] = out["matforms_errors"] == 0
    return out


def matrix_forms_check(device: int = 0, blocks: int = 0, ksteps: int = 4, vary_scale: bool = True, forms=None,
                       inject_form=None, inject_waves: int = 0, rates: bool = False, rate_iters: int = RATE_ITERS) -> dict:
    """One ``form_sweep`` kernel per form of ``forms`` (names or indices, default: all of ``FORMS``):
    4-wave workgroups (one wave per SIMD, one workgroup resident per CU) whose waves record their
    site first and last and compare every accumulator of C = A B over ``ksteps`` MFMAs (1..8) on
    integer operands with an integer reference; the E8M0 scales of the scaled forms vary unless
    ``vary_scale`` is false.  ``blocks=0``: 2 workgroups per CU plus up to 3 top-up launches while
    a CU or SIMD has no located record of some form, ``blocks>0``: one launch.  ``inject_form``:
    lane 0 of the first ``inject_waves`` waves perturbs element 0 of A in step 0 of that form.
    ``rates``: the rate chain of every selected form runs too (``rate_iters`` MFMAs per chain).

    Returns ``errors`` (form -> located wrong accumulators), ``unlocated_errors``,
    ``matforms_errors`` (their sum), ``waves`` and ``moved`` (records over all forms),
    ``form_waves``, ``launches``, ``cus_reached`` / ``cus_expected``, ``simds_reached``,
    ``bad_sites`` (the first 16), ``bad_by`` (form -> sites, first site, first register),
    ``wave_sites`` (form -> the site of each wave of the first launch), ``error``, ``form_ms``,
    ``ms``, ``tflops`` (form -> dense TFLOP/s, TOP/s for i8; empty without ``rates``) and ``ok``."""
    lib = load()
    names = _table("FORMS")
    mask = _mask(forms)
    inject = -1 if inject_form is None else form_index(inject_form)
    r = MatFormsResult()
    n_waves = WAVES * (int(blocks) if blocks > 0 else 2 * 1024)  # automatic: room for 1024 CUs
    wave_sites = (ctypes.c_uint * (len(names) * n_waves))()
    err = ctypes.create_string_buffer(512)
    rc = lib.amdgpu_matforms_run(int(device), int(blocks), int(ksteps), int(bool(vary_scale)), mask, inject,
                                 int(inject_waves), int(rate_iters) if rates else 0, wave_sites, n_waves,
                                 ctypes.byref(r), err, 512)
    if rc != 0:
        raise RuntimeError("matrix_forms_check failed: " + err.value.decode(errors="replace"))
    out = _as_dict(lib, r)
    out["wave_sites"] = {names[f]: [format_site(p) for p in wave_sites[f * n_waves:(f + 1) * n_waves] if p != UNWRITTEN]
                         for f in range(len(names)) if mask >> f & 1}
    return out


def records(rows) -> "numpy.ndarray":  # noqa: F821
    """A record array from ``(site_first, site_last, first_form, first_reg, {form index: wrong})`` rows."""
    import numpy as np

    a = np.zeros(len(rows), dtype=RECORD_DTYPE)
    for i, (site_first, site_last, first_form, first_reg, bad) in enumerate(rows):
        a[i]["site_first"], a[i]["site_last"], a[i]["first_form"], a[i]["first_reg"] = site_first, site_last, first_form, first_reg
        for k, v in dict(bad).items():
            a[i]["bad"][k] = v
    return a


def reduce(recs, form_of, forms=None) -> dict:
    """The check's host reduction on caller-supplied records (a numpy array of ``RECORD_DTYPE``
    or rows for ``records()``); ``form_of[i]`` is the form (name or index) record ``i`` belongs
    to.  No GPU.  Returns what ``matrix_forms_check`` returns except the coverage target, the
    device times, the rates and ``wave_sites``."""
    import numpy as np

    a = as_records(recs, RECORD_DTYPE, records)
    of = np.ascontiguousarray([form_index(f) for f in form_of], dtype=np.int32)
    if of.size != a.size:
        raise ValueError("matforms.reduce: one form per record")
    lib = load()
    r = MatFormsResult()
    if lib.amdgpu_matforms_reduce(a.ctypes.data if a.size else None, of.ctypes.data if of.size else None, int(a.size),
                                  _mask(forms), ctypes.byref(r)) != 0:
        raise ValueError("matforms.reduce: bad arguments (sites below %d, forms among the selected)" % SITE_SLOTS)
    return _as_dict(lib, r)


def operands(form, key: int, ksteps: int = 1, vary_scale: bool = True, inject: bool = False):
    """What a wave with key ``key`` feeds its MFMAs, host only: ``(a_words, b_words, scale_a,
    scale_b)``, uint32 arrays of shape (ksteps, 64, 8), (ksteps, 64, 8), (ksteps, 64), (ksteps, 64)."""
    import numpy as np

    a, b = (np.zeros((ksteps, 64, OPERAND_WORDS), dtype=np.uint32) for _ in range(2))
    sa, sb = (np.zeros((ksteps, 64), dtype=np.uint32) for _ in range(2))
    if not 1 <= ksteps <= MAX_KSTEPS or load().amdgpu_matforms_operands(
            form_index(form), int(key), int(ksteps), int(bool(vary_scale)), int(bool(inject)), a.ctypes.data, b.ctypes.data,
            sa.ctypes.data, sb.ctypes.data) != 0:
        raise ValueError("matforms.operands: bad arguments (ksteps %r)" % (ksteps,))
    return a, b, sa, sb


def expected(form, key: int, ksteps: int = 1, vary_scale: bool = True):
    """The integer reference C (int64, M x M) of that wave, host only."""
    import numpy as np

    m = form_info(form)["m"]
    out = np.zeros((m, m), dtype=np.int64)
    if not 1 <= ksteps <= MAX_KSTEPS or load().amdgpu_matforms_expected(form_index(form), int(key), int(ksteps),
                                                                        int(bool(vary_scale)), out.ctypes.data) != 0:
        raise ValueError("matforms.expected: bad arguments (ksteps %r)" % (ksteps,))
    return out


def inject_expected(form, wave: int) -> int:
    """Accumulators wave ``wave`` of the first launch must report wrong under the injection: the
    columns whose B element at the perturbed k is not zero."""
    n = load().amdgpu_matforms_inject_expected(form_index(form), int(wave))
    if n < 0:
        raise ValueError("matforms.inject_expected: bad arguments")
    return n


def encode(form, which: int, value: int) -> int:
    """The code of integer ``value`` in the format of operand ``which`` (0 A, 1 B) of the form."""
    code = ctypes.c_ulonglong()
    if load().amdgpu_matforms_encode(form_index(form), int(which), int(value), ctypes.byref(code)) < 0:
        raise ValueError("matforms.encode: %r is outside the form's range" % (value,))
    return int(code.value)


def table_map(form) -> dict:
    """The table's map of the form, host only: ``a_k`` / ``b_k`` (64 x elems: the k of element j
    of a lane, whose row / column is ``lane % m``), ``cd_row`` (64 x acc) and ``scale_block``
    (64; -1 for an unscaled form)."""
    import numpy as np

    info = form_info(form)
    a_k, b_k = (np.zeros((64, info["elems"]), dtype=np.int32) for _ in range(2))
    cd = np.zeros((64, info["acc"]), dtype=np.int32)
    sb = np.zeros(64, dtype=np.int32)
    as_p = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_int))  # noqa: E731
    if load().amdgpu_matforms_map(info["index"], as_p(a_k), as_p(b_k), as_p(cd), as_p(sb)) != 0:
        raise ValueError("matforms.table_map: no such form")
    return {"a_k": a_k, "b_k": b_k, "cd_row": cd, "scale_block": sb}


def pack(codes, bits: int):
    """Element codes (..., elems) as a lane's operand words (..., 8), element j at bit j * bits."""
    import numpy as np

    codes = np.asarray(codes, dtype=np.uint64)
    words = np.zeros(codes.shape[:-1] + (OPERAND_WORDS,), dtype=np.uint64)
    low = np.uint64(0xFFFFFFFF)
    for j in range(codes.shape[-1]):
        i, sh = (j * bits) >> 5, (j * bits) & 31
        words[..., i] |= (codes[..., j] << np.uint64(sh)) & low
        if sh + bits > 32:
            words[..., i + 1] |= (codes[..., j] >> np.uint64(32 - sh)) & low
    return words.astype(np.uint32)


def raw(form, a_words, b_words, scale_a=None, scale_b=None, device: int = 0):
    """Single-wave MFMAs of the form on raw operand registers, zero accumulators in: ``a_words`` /
    ``b_words`` (n, 64, 8) uint32, ``scale_a`` / ``scale_b`` (n, 64) E8M0 bytes (default 127).
    Returns every lane's raw accumulators, (n, 64, 16) uint32."""
    import numpy as np

    a = np.ascontiguousarray(a_words, dtype=np.uint32)
    b = np.ascontiguousarray(b_words, dtype=np.uint32)
    n = a.shape[0]
    if a.shape != (n, 64, OPERAND_WORDS) or b.shape != a.shape:
        raise ValueError("matforms.raw: operands of shape (n, 64, %d)" % OPERAND_WORDS)
    sa, sb = (np.full((n, 64), 127, dtype=np.uint32) if s is None else np.ascontiguousarray(s, dtype=np.uint32)
              for s in (scale_a, scale_b))
    if sa.shape != (n, 64) or sb.shape != (n, 64):
        raise ValueError("matforms.raw: scales of shape (n, 64)")
    out = np.zeros((n, 64, ACC_WORDS), dtype=np.uint32)
    err = ctypes.create_string_buffer(512)
    if load().amdgpu_matforms_raw(int(device), form_index(form), a.ctypes.data, b.ctypes.data, sa.ctypes.data,
                                  sb.ctypes.data, out.ctypes.data, n, err, 512) != 0:
        raise RuntimeError("matforms.raw failed: " + err.value.decode(errors="replace"))
    return out


def accumulators(form, out):
    """Raw accumulators (n, 64, 16) as matrices C (n, m, m) by the table's C/D map: float64 for
    the f32 and f64 forms (exact), int64 for i8."""
    import numpy as np

    info = form_info(form)
    cd = table_map(form)["cd_row"]
    out = np.ascontiguousarray(out, dtype=np.uint32)
    if info["acc_kind"] == 0:
        vals = out[..., :info["acc"]].copy().view(np.float32).astype(np.float64)
    elif info["acc_kind"] == 1:
        vals = out[..., :info["acc"]].copy().view(np.int32).astype(np.int64)
    else:
        vals = out[..., :2 * info["acc"]].copy().view(np.float64)
    c = np.zeros((out.shape[0], info["m"], info["m"]), dtype=vals.dtype)
    c[:, cd, (np.arange(64) % info["m"])[:, None]] = vals
    return c


def operand_map(form, device: int = 0) -> dict:
    """The hardware's own account of the form's operand map, from one-hot operands through ``raw``.
    An A element against an all-ones B fills its row; a B element against an all-ones A its
    column.  The B elements of column 0 are numbered 0..K-1, which labels the k classes (the
    labels are arbitrary, the partition is not): a one-hot A against column 0 holding 1 or 2 by a
    bit of that number reads its class bit by bit, and the B elements are classed the same way
    against row 0 of A.  For a scaled form, doubling one lane's scale byte shows which (row or
    column, class) pairs it scales.

    Returns ``a_row``, ``a_class``, ``b_col``, ``b_class`` (64 x elems lists) and, for scaled
    forms, ``scale_a`` / ``scale_b``: per lane ``{row or column: [classes]}``."""
    import numpy as np

    info = form_info(form)
    f, m, K, elems = info["index"], info["m"], info["k"], info["elems"]
    one = [np.uint64(encode(f, w, 1)) for w in (0, 1)]
    two = [np.uint64(encode(f, w, 2)) for w in (0, 1)]
    bits = [info["bits_a"], info["bits_b"]]
    n = 64 * elems
    lanes, js = np.divmod(np.arange(n), elems)

    def run(codes_a, codes_b, sa=None, sb=None):
        return accumulators(f, raw(f, pack(codes_a, bits[0]), pack(codes_b, bits[1]), sa, sb, device))

    def one_hot(which):
        codes = np.zeros((n, 64, elems), dtype=np.uint64)
        codes[np.arange(n), lanes, js] = one[which]
        return codes

    def ones(which, count):
        return np.full((count, 64, elems), one[which], dtype=np.uint64)

    def sole(line_of, what):  # the one row (or column) each wave filled with ones
        hit = (line_of == 1).all(axis=2)
        if not ((hit.sum(axis=1) == 1).all() and (np.abs(line_of).sum(axis=(1, 2)) == m).all()):
            raise RuntimeError("matforms.operand_map(%s): a one-hot %s element does not fill one line with ones" % (info["name"], what))
        return hit.argmax(axis=1)

    a_row = sole(run(one_hot(0), ones(1, n)), "A")
    b_col = sole(run(ones(0, n), one_hot(1)).transpose(0, 2, 1), "B")

    def classes(which, line, ref_elems, ref_class):
        # elements of operand `which` (their line: a_row or b_col) against the other operand's
        # reference line 0, whose element i (lane, j) holds 2 where bit b of ref_class[i] is set, else 1
        got = np.zeros(n, dtype=np.int64)
        for b in range(max(1, (K - 1).bit_length())):
            ref = np.zeros((64, elems), dtype=np.uint64)
            for (lane, j), c in zip(ref_elems, ref_class):
                ref[lane, j] = two[1 - which] if c >> b & 1 else one[1 - which]
            ref = np.broadcast_to(ref, (n, 64, elems))
            c = run(one_hot(0), ref) if which == 0 else run(ref, one_hot(1))
            v = c[np.arange(n), line, 0] if which == 0 else c[np.arange(n), 0, line]
            if not (np.isin(v, (1, 2)).all() and (np.abs(c).sum(axis=(1, 2)) == v).all()):
                raise RuntimeError("matforms.operand_map(%s): an element pairs with none or several of line 0" % info["name"])
            got |= (v == 2).astype(np.int64) << b
        return got

    b0 = [(int(l), int(j)) for l, j in zip(lanes, js) if b_col[l * elems + j] == 0]
    if len(b0) != K:
        raise RuntimeError("matforms.operand_map(%s): column 0 of B has %d elements, K is %d" % (info["name"], len(b0), K))
    a_class = classes(0, a_row, b0, list(range(K)))
    a0 = [(int(l), int(j)) for l, j in zip(lanes, js) if a_row[l * elems + j] == 0]
    b_class = classes(1, b_col, a0, [int(a_class[l * elems + j]) for l, j in a0])
    out = {"form": info["name"], "instruction": info["instruction"], "m": m, "k": K, "elems": elems,
           "a_row": a_row.reshape(64, elems).tolist(), "a_class": a_class.reshape(64, elems).tolist(),
           "b_col": b_col.reshape(64, elems).tolist(), "b_class": b_class.reshape(64, elems).tolist()}
    if not info["scaled"]:
        return out
    rounds = K // m
    for which, name in ((0, "scale_a"), (1, "scale_b")):
        # the other operand's line c holds the one element of class t * m + c: C[r][c] is the scale of (r, that class)
        line, cls = (b_col, b_class) if which == 0 else (a_row, a_class)
        sparse = np.zeros((rounds, 64, elems), dtype=np.uint64)
        for t in range(rounds):
            keep = (cls == t * m + line).reshape(64, elems)
            sparse[t][keep] = one[1 - which]
        sparse = np.tile(sparse, (64, 1, 1))                    # wave = lane * rounds + t
        scale = np.full((64 * rounds, 64), 127, dtype=np.uint32)
        scale[np.arange(64 * rounds), np.repeat(np.arange(64), rounds)] = 128
        full = ones(which, 64 * rounds)
        c = run(full, sparse, scale, None) if which == 0 else run(sparse, full, None, scale)
        if not np.isin(c, (1, 2)).all():
            raise RuntimeError("matforms.operand_map(%s): a doubled scale byte gives something else than 1 or 2" % info["name"])
        per_lane = []
        for lane in range(64):
            found = {}
            for t in range(rounds):
                mat = c[lane * rounds + t] if which == 0 else c[lane * rounds + t].T  # [scaled line][other line]
                for rc, other in zip(*np.nonzero(mat == 2)):
                    found.setdefault(int(rc), []).append(t * m + int(other))
            per_lane.append({rc: sorted(v) for rc, v in sorted(found.items())})
        out[name] = per_lane
    return out


def map_mismatches(form, hw: dict) -> list:
    """Where ``hw`` (an ``operand_map``, or its JSON dump) and the table's map of the form differ,
    as texts; empty when they describe the same partition: every element's row or column, which
    A and B elements share a k (one bijection between the hardware's classes and the table's
    k), and which (row or column, k-block) each lane's scale byte scales."""
    import numpy as np

    info, table = form_info(form), table_map(form)
    m, K = info["m"], info["k"]
    wrong = []
    line = (np.arange(64) % m)[:, None]
    if not (np.asarray(hw["a_row"]) == line).all():
        wrong.append("rows of A")
    if not (np.asarray(hw["b_col"]) == line).all():
        wrong.append("columns of B")
    to_k, to_class = {}, {}
    for name, k in (("a_class", table["a_k"]), ("b_class", table["b_k"])):
        for c, kk in zip(np.asarray(hw[name]).ravel().tolist(), k.ravel().tolist()):
            if to_k.setdefault(c, kk) != kk or to_class.setdefault(kk, c) != c:
                wrong.append("k classes (%s: class %d against k %d)" % (name, c, kk))
                break
    if sorted(to_class) != list(range(K)):
        wrong.append("k classes do not cover 0..%d" % (K - 1))
    if info["scaled"] and not wrong:
        for name in ("scale_a", "scale_b"):
            for lane, got in enumerate(hw[name]):
                block = int(table["scale_block"][lane])
                want = {lane % m: sorted(to_class[k] for k in range(32 * block, 32 * block + 32))}
                if {int(rc): sorted(v) for rc, v in got.items()} != want:
                    wrong.append("%s of lane %d" % (name, lane))
                    break
    return wrong


def main(argv=None) -> int:
    import argparse
    import json

    ap = argparse.ArgumentParser(description="The matrix-forms check on one device; prints one JSON line.")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--rates", action="store_true", help="also run the rate chain of every selected form")
    ap.add_argument("--forms", default=None, help="comma-separated names (default: every form of the table)")
    args = ap.parse_args(argv)
    r = matrix_forms_check(args.device, forms=args.forms.split(",") if args.forms else None, rates=args.rates)
    del r["wave_sites"]
    print(json.dumps(r))
    return 0 if r["ok"] else 1


if __name__ == "__main__":
    import sys

    sys.exit(main())
