"""Python face of the canary's host-link check (``ops/hostlink/hostlink.hip``; the C ABI
mirrored here is declared in ``ops/hostlink/hostlink.h``).

``host_link_check(device)`` loads ``ops/hostlink/libamdgpu_hostlink.so`` with ctypes and moves a
payload over the GPU's link to the host in both directions and by both paths: kernels that
read and write pinned host memory, the copy engine (``hipMemcpyAsync``), and system-scope
atomics on a pinned table that the host updates at the same time.  ``pattern_words``,
``host_verify``, ``atomic_expected`` and ``atomic_wrong`` are the host-side model and need no
GPU.  Missing library => it is built, or a loud ``RuntimeError`` (never a silent pass).
"""
from __future__ import annotations

import ctypes
import os

from ._sites import XCCS, load_library

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostlink", "libamdgpu_hostlink.so")

# the system-scope atomic forms, in the order of ops/hostlink/hostlink_host.h
ATOMIC_OPS = ("u32_add", "u64_add", "ticket", "cas_inc", "swap")
INJECT = ("read", "write", "h2d", "d2h", "atomic")
STAGES = ("read", "write", "h2d", "d2h")
ATOMIC_MAX_BLOCKS = 64
MAX_WAVES = 4 * ATOMIC_MAX_BLOCKS
SWAP_SLOTS = 64
# element type of each table: ticket is the ticket word followed by seen[256], swap the 64
# slots followed by what each of up to 256 waves got back
_ATOMIC_DTYPES = {"u32_add": "uint32", "u64_add": "uint64", "ticket": "uint32", "cas_inc": "uint64", "swap": "uint64"}
# seed of each bulk stage's pattern (repetition r adds r)
SEEDS = {"read": 0x48520000, "write": 0x48570000, "h2d": 0x48320000, "d2h": 0x44320000}


class XccSlot(ctypes.Structure):
    _fields_ = [("read_blocks", ctypes.c_ulonglong), ("read_bytes", ctypes.c_ulonglong),
                ("read_bad", ctypes.c_ulonglong), ("write_blocks", ctypes.c_ulonglong),
                ("write_bad", ctypes.c_ulonglong)]


class HostLinkResult(ctypes.Structure):
    _fields_ = [("read_errors", ctypes.c_ulonglong), ("write_errors", ctypes.c_ulonglong),
                ("h2d_errors", ctypes.c_ulonglong), ("d2h_errors", ctypes.c_ulonglong),
                ("atomic_errors", ctypes.c_ulonglong), ("atomic_bad", ctypes.c_ulonglong * len(ATOMIC_OPS)),
                ("unlocated_errors", ctypes.c_ulonglong), ("moved", ctypes.c_ulonglong),
                ("first_bad_offset", ctypes.c_longlong * len(STAGES)), ("bytes", ctypes.c_ulonglong),
                ("first_bad_op", ctypes.c_int), ("first_bad_elem", ctypes.c_int), ("first_bad_xcc", ctypes.c_int * 2),
                ("xccs_reached", ctypes.c_int), ("blocks", ctypes.c_int), ("atomic_blocks", ctypes.c_int),
                ("reps", ctypes.c_int), ("atomic_overlap", ctypes.c_int), ("host_adds", ctypes.c_int),
                ("stage_ms", ctypes.c_double * len(STAGES)), ("atomic_ms", ctypes.c_double),
                ("host_cpu_ms", ctypes.c_double)]


def _declare(lib) -> None:
    lib.amdgpu_hostlink_run.argtypes = [ctypes.c_int, ctypes.c_ulonglong] + [ctypes.c_int] * 8 + \
        [ctypes.POINTER(XccSlot), ctypes.POINTER(ctypes.c_uint), ctypes.c_int, ctypes.POINTER(HostLinkResult),
         ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_hostlink_run.restype = ctypes.c_int
    lib.amdgpu_hostlink_describe.argtypes = [ctypes.POINTER(HostLinkResult), ctypes.POINTER(XccSlot),
                                             ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_hostlink_describe.restype = ctypes.c_int
    lib.amdgpu_hostlink_sizeof.argtypes = [ctypes.c_int]
    lib.amdgpu_hostlink_sizeof.restype = ctypes.c_int
    lib.amdgpu_hostlink_tile_words.argtypes = [ctypes.c_int]
    lib.amdgpu_hostlink_tile_words.restype = ctypes.c_int
    lib.amdgpu_hostlink_pattern.argtypes = [ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_void_p]
    lib.amdgpu_hostlink_pattern.restype = ctypes.c_int
    lib.amdgpu_hostlink_verify.argtypes = [ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_uint,
                                           ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_longlong)]
    lib.amdgpu_hostlink_verify.restype = ctypes.c_int
    lib.amdgpu_hostlink_atomic_expected.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                    ctypes.c_int]
    lib.amdgpu_hostlink_atomic_expected.restype = ctypes.c_int
    lib.amdgpu_hostlink_atomic_compare.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                   ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.amdgpu_hostlink_atomic_compare.restype = ctypes.c_longlong
    lib.amdgpu_hostlink_atomic_op_name.argtypes = [ctypes.c_int]
    lib.amdgpu_hostlink_atomic_op_name.restype = ctypes.c_char_p


def load():
    return load_library(LIB_PATH, "build_hostlink", _declare)


def tile_words(unroll: int = 0) -> int:
    """16-byte words of one tile of the bulk kernels (``unroll=0``: the default): the writer
    (and reader) of word ``i`` is workgroup ``(i // tile_words) % blocks``."""
    n = load().amdgpu_hostlink_tile_words(int(unroll))
    if n < 0:
        raise ValueError("no kernel with unroll %r (2, 4 or 8)" % (unroll,))
    return n


def host_link_check(device: int = 0, nbytes: int = 64 << 20, blocks: int = 0, reps: int = 1, host_adds: int = 1024,
                    inject=None, inject_op=None, inject_n: int = 0, *, unroll: int = 0, atomic_blocks: int = 0) -> dict:
    """The GPU's link to the host, in five stages over ``nbytes`` (a positive multiple of 16)
    of pinned, coherent host memory, the first four repeated ``reps`` times: ``host_read``
    (workgroups read the buffer the host filled, and compare), ``host_write`` (workgroups
    write it, the host verifies), ``copy_h2d`` and ``copy_d2h`` (``hipMemcpyAsync``, verified
    on the far side) and ``host_atomic`` (system-scope add, exchange and CAS on a small pinned
    table while the calling thread makes ``host_adds`` adds to the same words).  ``blocks``:
    the grid of the two bulk kernels (0: one workgroup per CU).  ``inject`` (``read``,
    ``write``, ``h2d``, ``d2h``: ``inject_n`` words or workgroups; ``atomic``: one operand of
    form ``inject_op``) plants a fault in values that are then compared.

    Returns the counts (``read_errors``, ``write_errors``, ``h2d_errors``, ``d2h_errors``,
    ``atomic_errors``, ``unlocated_errors``, ``moved``), ``atomic`` (form -> wrong elements),
    ``first_bad`` (stage -> byte offset, and the xcc for ``read`` / ``write``; ``atomic``: op,
    element), ``xccs`` (``"xcc5"`` -> blocks, bytes and wrong words read, blocks that wrote
    and wrong words the host found in what they wrote), ``read_block_xcc`` /
    ``write_block_xcc`` (the xcc of each workgroup, -1 if it had no work), the four rates
    (``kernel_read_gbps``, ``kernel_write_gbps``, ``copy_h2d_gbps``, ``copy_d2h_gbps``:
    ``nbytes * reps`` over the stage's device time), the per-stage ms, ``host_cpu_ms``,
    ``atomic_overlap``, ``error`` (the text for the first failing stage) and ``ok``."""
    kind = -1 if inject is None else INJECT.index(inject)
    op = 0 if inject_op is None else ATOMIC_OPS.index(inject_op)
    lib = load()
    r = HostLinkResult()
    xt = (XccSlot * XCCS)()
    n_blocks = int(blocks) if blocks > 0 else 4096
    bx = (ctypes.c_uint * (2 * n_blocks))()
    err = ctypes.create_string_buffer(512)
    rc = lib.amdgpu_hostlink_run(int(device), int(nbytes), int(blocks), int(reps), kind, op, int(inject_n),
                                 int(host_adds), int(unroll), int(atomic_blocks), xt, bx, n_blocks, ctypes.byref(r),
                                 err, 512)
    if rc != 0:
        raise RuntimeError("host_link_check failed: " + err.value.decode(errors="replace"))
    out = {f: int(getattr(r, f)) for f in ("read_errors", "write_errors", "h2d_errors", "d2h_errors", "atomic_errors",
                                           "unlocated_errors", "moved", "xccs_reached", "blocks", "atomic_blocks",
                                           "reps", "bytes", "host_adds", "atomic_overlap")}
    out["atomic"] = {name: int(r.atomic_bad[i]) for i, name in enumerate(ATOMIC_OPS)}
    first = {s: None if r.first_bad_offset[i] < 0 else {"offset": int(r.first_bad_offset[i])}
             for i, s in enumerate(STAGES)}
    for i, s in enumerate(("read", "write")):
        if first[s] is not None:
            first[s]["xcc"] = int(r.first_bad_xcc[i])
    first["atomic"] = None if r.first_bad_op < 0 else {"op": ATOMIC_OPS[r.first_bad_op], "element": r.first_bad_elem}
    out["first_bad"] = first
    out["xccs"] = {"xcc%d" % x: {"read_blocks": int(s.read_blocks), "read_bytes": int(s.read_bytes),
                                 "read_bad": int(s.read_bad), "write_blocks": int(s.write_blocks),
                                 "write_bad": int(s.write_bad)}
                   for x, s in enumerate(xt) if s.read_blocks or s.write_blocks}
    as_xcc = [-1 if x == 0xFFFFFFFF else int(x) for x in bx]
    out["read_block_xcc"] = as_xcc[:r.blocks]
    out["write_block_xcc"] = as_xcc[n_blocks:n_blocks + r.blocks]
    for i, (stage, rate) in enumerate((("read_ms", "kernel_read_gbps"), ("write_ms", "kernel_write_gbps"),
                                       ("h2d_ms", "copy_h2d_gbps"), ("d2h_ms", "copy_d2h_gbps"))):
        ms = float(r.stage_ms[i])
        out[stage] = ms
        out[rate] = int(nbytes) * int(reps) / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    out["atomic_ms"], out["host_cpu_ms"] = r.atomic_ms, r.host_cpu_ms
    out["ms"] = sum(r.stage_ms) + r.atomic_ms
    errors = out["read_errors"] + out["write_errors"] + out["h2d_errors"] + out["d2h_errors"] + out["atomic_errors"]
    lib.amdgpu_hostlink_describe(ctypes.byref(r), xt, err, 512)
    out["error"] = err.value.decode(errors="replace") if errors else ""
    out["ok"] = errors == 0
    return out


def pattern_words(idx0: int, n: int, seed: int):
    """The pattern of 16-byte words ``idx0 .. idx0 + n``: a uint32 array [n, 4]."""
    import numpy as np

    out = np.empty((int(n), 4), dtype=np.uint32)
    if load().amdgpu_hostlink_pattern(int(idx0), int(n), int(seed) & 0xFFFFFFFF, out.ctypes.data) != 0:
        raise ValueError("pattern_words(%r, %r, %r)" % (idx0, n, seed))
    return out


def host_verify(buf, seed: int) -> tuple:
    """The host's verifier on a caller-supplied buffer (a whole number of 16-byte words that
    should hold the pattern of words 0 ..): ``(wrong 32-bit words, byte offset of the first or -1)``."""
    import numpy as np

    a = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    if a.size % 16:
        raise ValueError("host_verify: %d bytes is not a whole number of 16-byte words" % a.size)
    a = np.require(a.view(np.uint32), requirements=["A", "C"])
    wrong, first = ctypes.c_ulonglong(), ctypes.c_longlong()
    if load().amdgpu_hostlink_verify(a.ctypes.data, a.size // 4, int(seed) & 0xFFFFFFFF, ctypes.byref(wrong),
                                     ctypes.byref(first)) != 0:
        raise ValueError("host_verify: bad buffer")
    return int(wrong.value), int(first.value)


def _atomic_args(op: str, blocks: int, host_adds: int):
    if not (1 <= int(blocks) <= ATOMIC_MAX_BLOCKS and int(host_adds) >= 0):
        raise ValueError("atomic tables: blocks must be in 1..%d and host_adds >= 0, got %r, %r"
                         % (ATOMIC_MAX_BLOCKS, blocks, host_adds))
    return ATOMIC_OPS.index(op), int(blocks), int(host_adds)


def atomic_expected(op: str, blocks: int, host_adds: int = 0):
    """The table form ``op`` (one of ``ATOMIC_OPS``) holds after ``blocks`` workgroups (1..64)
    of ``host_atomic`` and ``host_adds`` adds by the host, computed on the host: 1024 elements
    (``u32_add``, ``u64_add``), the ticket word followed by ``seen[256]``, the 64 words of
    ``cas_inc``, or the 64 slots of ``swap`` followed by what each wave got back when the waves
    run in index order (one of the orders ``atomic_wrong`` accepts)."""
    import numpy as np

    buf = np.zeros(1024, dtype=np.uint64)
    n = load().amdgpu_hostlink_atomic_expected(*_atomic_args(op, blocks, host_adds), buf.ctypes.data, buf.nbytes)
    if n < 0:
        raise ValueError("atomic_expected(%s, %r, %r)" % (op, blocks, host_adds))
    return buf.view(np.uint8)[:n].view(_ATOMIC_DTYPES[op]).copy()


def atomic_wrong(op: str, blocks: int, table, host_adds: int = 0) -> tuple:
    """The check's acceptance rule on a caller-supplied table of form ``op``, laid out as
    ``atomic_expected`` returns it: ``(wrong elements, the first of them or -1)``.  ``swap``
    accepts every order: what the waves got back and what the slots hold must together be the
    tokens and the slots' initial values, each exactly once."""
    import numpy as np

    t = np.ascontiguousarray(table, dtype=_ATOMIC_DTYPES[op])
    first = ctypes.c_int(-1)
    n = load().amdgpu_hostlink_atomic_compare(*_atomic_args(op, blocks, host_adds), t.ctypes.data, t.nbytes,
                                              ctypes.byref(first))
    if n < 0:
        raise ValueError("atomic_wrong(%s, %r): a table of %d bytes is too short" % (op, blocks, t.nbytes))
    return int(n), int(first.value)
