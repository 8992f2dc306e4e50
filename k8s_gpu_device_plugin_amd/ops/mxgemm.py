"""Python face of the stand-alone block-scaled matrix-path check (``ops/mxgemm/mxgemm.hip``; the C
ABI mirrored here is declared in ``ops/mxgemm/mxgemm.h`` and ``ops/mxgemm/mxgemm_host.h``).

``mx_gemm_check(device)`` loads ``ops/mxgemm/libamdgpu_mxgemm.so`` with ctypes and runs an LDS-staged
GEMM on MX-fp8, bf8 and fp4 operands with E8M0 block scales (``v_mfma_scale_f32_32x32x64_f8f6f4``):
packed rows HBM -> LDS DMA -> ``ds_read_b128`` -> scaled MFMA -> store of C, on exact integer data,
verified by row and column checksums.  ``mx_gemm`` runs the same kernels on caller-supplied codes
and scales; ``pack`` and ``operands`` are the host's side on its own and need no GPU.
``canary.run()`` and the plugin do not call this check yet.  Missing library => it is built, or a
loud ``RuntimeError`` (never a silent pass).

``python -m k8s_gpu_device_plugin_amd.ops.mxgemm [--device N] [--fmt fp8|bf8|fp4] [--size S] [--k K]
[--iters I] [--kernel ID] [--inject]`` prints one JSON line.
"""
from __future__ import annotations

import ctypes
import functools
import os

from ._sites import load_library

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mxgemm", "libamdgpu_mxgemm.so")

FORMATS = {"fp8": 0, "bf8": 1, "fp4": 4}  # the project's format ids (ops/mfma_forms.h)
INJECT, SKIP_VERIFIED_LAUNCH = 1, 2       # flags of amdgpu_mxgemm_check, as in mxgemm.h
SCALE_BLOCK = 32                          # k per E8M0 byte


class MxGemmResult(ctypes.Structure):
    _fields_ = [("row_errors", ctypes.c_ulonglong), ("col_errors", ctypes.c_ulonglong), ("ms", ctypes.c_double),
                ("tflops", ctypes.c_double)] + [(f, ctypes.c_int) for f in ("fmt", "kernel", "m", "n", "k", "iters")]


EXPORTS = ("run", "check", "describe", "kernels", "pick", "operand", "sizeof")


def _declare(lib) -> None:
    res_p, ptr = ctypes.POINTER(MxGemmResult), ctypes.c_void_p
    lib.amdgpu_mxgemm_run.argtypes = [ctypes.c_int] * 3 + [ptr] * 5 + [ctypes.c_int] * 3 + [ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_mxgemm_check.argtypes = [ctypes.c_int] * 9 + [res_p, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_mxgemm_describe.argtypes = [res_p, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_mxgemm_kernels.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.amdgpu_mxgemm_pick.argtypes = [ctypes.c_int] * 5
    lib.amdgpu_mxgemm_operand.argtypes = [ctypes.c_int] * 5 + [ptr] * 3
    lib.amdgpu_mxgemm_sizeof.argtypes = [ctypes.c_int]
    for name in EXPORTS:
        getattr(lib, "amdgpu_mxgemm_" + name).restype = ctypes.c_int


def load():
    return load_library(LIB_PATH, "build_mxgemm", _declare)


@functools.lru_cache(None)
def _kernels() -> dict:
    lib = load()
    out, table = (ctypes.c_int * 3)(), {}
    for i in range(1, lib.amdgpu_mxgemm_kernels(-1, None)):
        lib.amdgpu_mxgemm_kernels(i, out)
        table[i] = {"tile": int(out[0]), "threads": int(out[1]), "lds_bytes": int(out[2])}
    return table


def __getattr__(name):  # the table is the library's (kMxVariants): read on first use, so importing this module builds nothing
    if name == "KERNELS":
        return _kernels()
    raise AttributeError(name)


def tile_k(fmt: str) -> int:
    """BK: the k of one K-tile, 128 B of an operand row (128 for fp8 and bf8, 256 for fp4)."""
    return 256 if FORMATS[fmt] == 4 else 128


def pick(m: int, n: int, k: int, fmt: str = "fp8", kernel: int = 0) -> int:
    """The kernel id that runs for ``kernel`` at this shape (0: the library's choice), 0 if it is refused.  No GPU."""
    return int(load().amdgpu_mxgemm_pick(FORMATS[fmt], int(kernel), int(m), int(n), int(k)))


def pack(codes, fmt: str):
    """Rows of one code per byte as the kernels read them: unchanged for fp8 and bf8; for fp4 two
    codes per byte, element ``k`` in the low nibble when ``k`` is even."""
    import numpy as np

    c = np.ascontiguousarray(codes, dtype=np.uint8)
    if FORMATS[fmt] != 4:
        return c
    if c.shape[-1] % 2:
        raise ValueError("mxgemm.pack: an even number of fp4 codes per row")
    return np.ascontiguousarray((c[..., 0::2] & 0xF) | ((c[..., 1::2] & 0xF) << 4))


def operands(m: int, n: int, k: int, fmt: str = "fp8", vary_scale: bool = True) -> dict:
    """The check's own integer data, host only: ``a_codes`` [m, k] and ``bt_codes`` [n, k] (one OCP
    code per byte), ``a_scales`` [m, k/32] and ``b_scales`` [n, k/32] (E8M0 bytes, 127 or 128), and
    ``a_values`` / ``bt_values``, the integers in [-4, 4] the codes stand for (int64)."""
    import numpy as np

    out = {}
    for which, (name, rows) in enumerate((("a", m), ("bt", n))):
        codes, values = np.zeros((rows, k), dtype=np.uint8), np.zeros((rows, k), dtype=np.int64)
        scales = np.zeros((rows, k // SCALE_BLOCK), dtype=np.uint8)
        if load().amdgpu_mxgemm_operand(FORMATS[fmt], which, int(rows), int(k), int(bool(vary_scale)), codes.ctypes.data,
                                        scales.ctypes.data, values.ctypes.data) != 0:
            raise ValueError("mxgemm.operands: positive rows and k %% %d == 0, not (%d, %d)" % (SCALE_BLOCK, rows, k))
        out[name + "_codes"], out[name + "_values"], out[name[0] + "_scales"] = codes, values, scales
    return out


def mx_gemm(a_codes, bt_codes, a_scales, b_scales, fmt: str = "fp8", device: int = 0, kernel: int = 0):
    """C = dequant(A) @ dequant(Bt).T through the LDS-staged block-scaled GEMM.  The arguments of
    ``canary.lowp_gemm``: ``a_codes`` uint8 [M, K] and ``bt_codes`` uint8 [N, K] hold one OCP code
    per element (fp4 in the low nibble; packed here), ``a_scales`` [M, K/32] and ``b_scales``
    [N, K/32] are E8M0 bytes (127 = 1.0).  M, N multiples of the kernel's tile edge (``KERNELS``),
    K a multiple of ``tile_k(fmt)`` and at most 65536.  Returns float32 [M, N]."""
    import numpy as np

    a, bt = (np.ascontiguousarray(x, dtype=np.uint8) for x in (a_codes, bt_codes))
    sa, sb = (np.ascontiguousarray(x, dtype=np.uint8) for x in (a_scales, b_scales))
    if a.ndim != 2 or bt.ndim != 2 or a.shape[1] != bt.shape[1] or \
            sa.shape != (a.shape[0], a.shape[1] // SCALE_BLOCK) or sb.shape != (bt.shape[0], a.shape[1] // SCALE_BLOCK):
        raise ValueError("shapes do not match: A %s, Bt %s, scales %s / %s" % (a.shape, bt.shape, sa.shape, sb.shape))
    (m, k), n = a.shape, bt.shape[0]
    lib = load()
    if lib.amdgpu_mxgemm_pick(FORMATS[fmt], int(kernel), m, n, k) != 0:  # pack only what the library will take
        a, bt = pack(a, fmt), pack(bt, fmt)
    c = np.empty((m, n), dtype=np.float32)
    err = ctypes.create_string_buffer(256)
    if lib.amdgpu_mxgemm_run(int(device), FORMATS[fmt], int(kernel), a.ctypes.data, bt.ctypes.data, sa.ctypes.data,
                             sb.ctypes.data, c.ctypes.data, m, n, k, err, 256) != 0:
        raise RuntimeError("mx_gemm failed: " + err.value.decode(errors="replace"))
    return c


def mx_gemm_check(device: int = 0, m: int = 4096, n: int = 4096, k: int = 4096, fmt=None, iters: int = 10, kernel: int = 0,
                  vary_scale: bool = True, inject: bool = False, skip_verified_launch: bool = False) -> dict:
    """The block-scaled matrix path on ``fmt`` (``None``: each of ``FORMATS``): device-generated
    integer codes in [-4, 4] with scales of 2^0 or 2^1, one warm-up GEMM, ``iters`` timed ones, then
    one more written into a poisoned (all 0xFF) C, and the row / column checksums of that one.
    ``inject`` corrupts one element of the verified product (2 errors expected);
    ``skip_verified_launch`` leaves the poison in place (``m + n`` expected).

    Returns ``ok``, ``error`` (the first failing format's text), ``ms`` (device time of the timed
    launches over all formats), ``mxgemm_errors`` (wrong rows + wrong columns over all formats),
    ``kernel`` (the id that ran), ``shape`` and, per format, ``row_errors``, ``col_errors``, ``ms``
    and ``tflops`` (dense, reported and never judged)."""
    lib = load()
    flags = (INJECT if inject else 0) | (SKIP_VERIFIED_LAUNCH if skip_verified_launch else 0)
    out = {"ok": True, "error": "", "ms": 0.0, "mxgemm_errors": 0, "kernel": int(kernel), "shape": (m, n, k)}
    for f in (tuple(FORMATS) if fmt is None else (fmt,)):
        r = MxGemmResult()
        err = ctypes.create_string_buffer(256)
        if lib.amdgpu_mxgemm_check(int(device), FORMATS[f], int(kernel), int(m), int(n), int(k), int(iters),
                                   int(bool(vary_scale)), flags, ctypes.byref(r), err, 256) != 0:
            raise RuntimeError("mx_gemm_check failed: " + err.value.decode(errors="replace"))
        out[f] = {"row_errors": int(r.row_errors), "col_errors": int(r.col_errors), "ms": float(r.ms), "tflops": float(r.tflops)}
        out["kernel"] = int(r.kernel)
        out["ms"] += float(r.ms)
        out["mxgemm_errors"] += int(r.row_errors + r.col_errors)
        if not out["error"]:
            lib.amdgpu_mxgemm_describe(ctypes.byref(r), err, 256)
            out["error"] = err.value.decode(errors="replace")
    out["ok"] = out["mxgemm_errors"] == 0
    return out


def main(argv=None) -> int:
    import argparse
    import json

    ap = argparse.ArgumentParser(description="The block-scaled matrix-path check on one device; prints one JSON line.")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--fmt", choices=tuple(FORMATS), default=None, help="default: every format")
    ap.add_argument("--size", type=int, default=4096, help="M and N")
    ap.add_argument("--k", type=int, default=None, help="default: --size")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--kernel", type=int, default=0, help="an id of KERNELS (default 0: the library's choice)")
    ap.add_argument("--inject", action="store_true", help="corrupt one element of the verified product")
    args = ap.parse_args(argv)
    r = mx_gemm_check(args.device, args.size, args.size, args.k or args.size, args.fmt, args.iters, args.kernel,
                      inject=args.inject)
    print(json.dumps(r))
    return 0 if r["ok"] else 1


if __name__ == "__main__":
    import sys

    sys.exit(main())
