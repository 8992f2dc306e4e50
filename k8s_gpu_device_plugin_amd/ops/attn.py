"""Python face of the stand-alone attention-path check (``ops/attn/attn.hip``; the C ABI mirrored
here is declared in ``ops/attn/attn.h`` and ``ops/attn/attn_host.h``).

``attention_check(device)`` loads ``ops/attn/libamdgpu_attn.so`` with ctypes and runs a fused bf16
flash-attention forward (head dimension 128): K and V tiles HBM -> LDS DMA, ``K Q^T`` on
``v_mfma_f32_32x32x16_bf16``, an online base-2 softmax (``v_exp_f32``, a cross-lane row maximum and
sum, a running rescale), the probabilities packed to bf16 and fed back into ``V^T P^T`` with V read
by ``ds_read_b64_tr_b16``.  Two data sets have outputs that are exact by construction and are
compared bit for bit on the device; a third is held to a derived bound against float64 on the host.
``attention`` runs the same kernel on caller-supplied bf16 bit patterns; ``operands`` and
``expected`` are the host's side on its own and need no GPU.  ``canary.run()`` and the plugin do not
call this check yet.  Missing library => it is built, or a loud ``RuntimeError`` (never a silent pass).

``python -m k8s_gpu_device_plugin_amd.ops.attn [--device N] [--heads H] [--seq S] [--seq-k SK]
[--causal] [--iters I] [--inject]`` prints one JSON line.
"""
from __future__ import annotations

import ctypes
import os

from ._sites import load_library

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn", "libamdgpu_attn.so")

HEAD_DIM = 128
SETS = ("uniform", "routed", "hashed")   # ids 0, 1, 2 of attn_host.h; the first two are exact
INJECT, SKIP_VERIFIED_LAUNCH = 1, 2      # flags of amdgpu_attn_check, as in attn.h


class AttnResult(ctypes.Structure):
    _fields_ = [(f, ctypes.c_ulonglong * 3) for f in ("o_errors", "lse_errors", "first_bad", "first_bad_lse")] + \
               [("ms", ctypes.c_double * 3), ("tflops", ctypes.c_double), ("max_err", ctypes.c_double),
                ("max_lse_err", ctypes.c_double)] + \
               [(f, ctypes.c_int) for f in ("heads", "seq_q", "seq_k", "causal", "iters", "rows")]


EXPORTS = ("run", "check", "describe", "operands", "expected", "sizeof")


def _declare(lib) -> None:
    res_p, ptr = ctypes.POINTER(AttnResult), ctypes.c_void_p
    lib.amdgpu_attn_run.argtypes = [ctypes.c_int] + [ptr] * 5 + [ctypes.c_int] * 4 + [ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_attn_check.argtypes = [ctypes.c_int] * 8 + [res_p, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_attn_describe.argtypes = [res_p, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_attn_operands.argtypes = [ctypes.c_int] * 4 + [ptr] * 3
    lib.amdgpu_attn_expected.argtypes = [ctypes.c_int] * 5 + [ptr] * 2
    lib.amdgpu_attn_sizeof.argtypes = [ctypes.c_int]
    for name in EXPORTS:
        getattr(lib, "amdgpu_attn_" + name).restype = ctypes.c_int


def load():
    return load_library(LIB_PATH, "build_attn", _declare)


def operands(set, heads: int, seq_q: int, seq_k: int):
    """The check's own data of ``set`` (a name of ``SETS``), host only: ``q`` [heads, seq_q, 128],
    ``k`` and ``v`` [heads, seq_k, 128] as bf16 bit patterns (uint16)."""
    import numpy as np

    q = np.zeros((heads, seq_q, HEAD_DIM), dtype=np.uint16)
    k, v = (np.zeros((heads, seq_k, HEAD_DIM), dtype=np.uint16) for _ in range(2))
    if load().amdgpu_attn_operands(SETS.index(set), int(heads), int(seq_q), int(seq_k), q.ctypes.data, k.ctypes.data,
                                   v.ctypes.data) != 0:
        raise ValueError("attn.operands: positive sizes, not (%d, %d, %d)" % (heads, seq_q, seq_k))
    return q, k, v


def expected(set, heads: int, seq_q: int, seq_k: int, causal: bool = False):
    """What a healthy kernel gives for an exact set, host only: ``o`` float32 [heads, seq_q, 128], bit
    for bit (the integer sum of V over the visible keys of highest score, one IEEE division by
    their number), and ``lse`` float64 [heads, seq_q] (the log of that number plus the highest score)."""
    import numpy as np

    o, lse = np.zeros((heads, seq_q, HEAD_DIM), dtype=np.float32), np.zeros((heads, seq_q), dtype=np.float64)
    if load().amdgpu_attn_expected(SETS.index(set), int(heads), int(seq_q), int(seq_k), int(bool(causal)), o.ctypes.data,
                                   lse.ctypes.data) != 0:
        raise ValueError("attn.expected: an exact set (uniform, routed) and seq_k >= seq_q when causal, not %s (%d, %d, %d)"
                         % (set, heads, seq_q, seq_k))
    return o, lse


def attention(q, k, v, causal: bool = False, device: int = 0):
    """``softmax(q k^T / sqrt(128)) v`` through the fused kernel.  ``q`` [H, Sq, 128], ``k`` and ``v``
    [H, Sk, 128]: bf16 bit patterns (uint16, the convention of ``canary.abft``'s ``a_bits``).  Sq a
    positive multiple of 128, Sk of 64, Sk >= Sq when causal (key ``j`` is visible to query ``i``
    when ``j <= i + (Sk - Sq)``).  Returns ``o`` float32 [H, Sq, 128] and ``lse`` float32 [H, Sq],
    the natural-log sum of exponentials of the scaled scores."""
    import numpy as np

    q, k, v = (np.ascontiguousarray(x, dtype=np.uint16) for x in (q, k, v))
    if q.ndim != 3 or k.shape != v.shape or k.ndim != 3 or q.shape[0] != k.shape[0] or \
            q.shape[2] != HEAD_DIM or k.shape[2] != HEAD_DIM:
        raise ValueError("shapes do not match: q %s, k %s, v %s (head dimension %d)" % (q.shape, k.shape, v.shape, HEAD_DIM))
    (h, sq, _), sk = q.shape, k.shape[1]
    o, lse = np.empty((h, sq, HEAD_DIM), dtype=np.float32), np.empty((h, sq), dtype=np.float32)
    err = ctypes.create_string_buffer(256)
    if load().amdgpu_attn_run(int(device), q.ctypes.data, k.ctypes.data, v.ctypes.data, o.ctypes.data, lse.ctypes.data,
                              h, sq, sk, int(bool(causal)), err, 256) != 0:
        raise RuntimeError("attention failed: " + err.value.decode(errors="replace"))
    return o, lse


def attention_check(device: int = 0, heads: int = 0, seq_q: int = 0, seq_k: int = 0, causal: bool = False, iters: int = 20,
                    rows: int = 8, inject: bool = False, skip_verified_launch: bool = False) -> dict:
    """The attention path on each of ``SETS``: device-generated operands, one warm-up launch,
    ``iters`` timed ones, then one more written into poisoned (all 0xFF) O and lse, and the verdict
    on that output.  ``uniform`` and ``routed`` are compared bit for bit with the closed form on the
    device; ``hashed`` is held to ``|o - ref| <= 2^-6`` and ``|lse - ref| <= 2^-8 + 2^-20 |ref|``
    against float64 on the host for ``rows`` rows per head.  Sizes of 0 mean the default workload
    (32 heads of 4096 x 4096).  ``inject`` corrupts one element of each verified output (1 error per
    set); ``skip_verified_launch`` leaves the poison in place.

    Returns ``ok``, ``error`` (the first failing set's text), ``ms`` (device time of all timed
    launches), ``tflops`` (reported, never judged), ``o_errors``, ``lse_errors``, ``attn_errors``
    (their sum), ``max_err`` and ``max_lse_err`` (the hashed set's largest deviations), ``heads``,
    ``seq_q``, ``seq_k``, ``causal``, and ``sets``: per set ``o_errors``, ``lse_errors`` and ``ms``."""
    lib = load()
    flags = (INJECT if inject else 0) | (SKIP_VERIFIED_LAUNCH if skip_verified_launch else 0)
    r, err = AttnResult(), ctypes.create_string_buffer(256)
    if lib.amdgpu_attn_check(int(device), int(heads), int(seq_q), int(seq_k), int(bool(causal)), int(iters), int(rows), flags,
                             ctypes.byref(r), err, 256) != 0:
        raise RuntimeError("attention_check failed: " + err.value.decode(errors="replace"))
    lib.amdgpu_attn_describe(ctypes.byref(r), err, 256)
    sets = {name: {"o_errors": int(r.o_errors[i]), "lse_errors": int(r.lse_errors[i]), "ms": float(r.ms[i])}
            for i, name in enumerate(SETS)}
    o_errors, lse_errors = sum(r.o_errors), sum(r.lse_errors)
    return {"ok": o_errors + lse_errors == 0, "error": err.value.decode(errors="replace"), "ms": sum(r.ms),
            "tflops": float(r.tflops), "o_errors": int(o_errors), "lse_errors": int(lse_errors),
            "attn_errors": int(o_errors + lse_errors), "max_err": float(r.max_err), "max_lse_err": float(r.max_lse_err),
            "sets": sets, "heads": int(r.heads), "seq_q": int(r.seq_q), "seq_k": int(r.seq_k), "causal": bool(r.causal),
            "iters": int(r.iters), "rows": int(r.rows)}


def main(argv=None) -> int:
    import argparse
    import json

    ap = argparse.ArgumentParser(description="The attention-path check on one device; prints one JSON line.")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--heads", type=int, default=0, help="default 0: the library's workload (32)")
    ap.add_argument("--seq", type=int, default=0, help="queries and keys; default 0: the library's workload (4096)")
    ap.add_argument("--seq-k", type=int, default=0, help="keys, when they differ from --seq")
    ap.add_argument("--causal", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--inject", action="store_true", help="corrupt one element of each verified output")
    args = ap.parse_args(argv)
    r = attention_check(args.device, args.heads, args.seq, args.seq_k, args.causal, args.iters, inject=args.inject)
    print(json.dumps(r))
    return 0 if r["ok"] else 1


if __name__ == "__main__":
    import sys

    sys.exit(main())
