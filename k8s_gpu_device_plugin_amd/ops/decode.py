"""Python face of the stand-alone decode-attention check (``ops/decode/decode.hip``; the C ABI mirrored
here is declared in ``ops/decode/decode.h`` and ``ops/decode/decode_host.h``).

``decode_check(device)`` loads ``ops/decode/libamdgpu_decode.so`` with ctypes and runs decode
attention as an inference container does: one query token per sequence, ``G`` query heads sharing a
KV head, a bf16 KV cache in pages of 16 keys behind a block table, the key range split over
workgroups.  ``decode_split`` streams each wave's own pages HBM -> LDS by DMA from addresses it
derives from the table, computes ``K Q^T`` and ``V^T P^T`` on ``v_mfma_f32_32x32x16_bf16`` around a
base-2 online softmax, masks the ragged tail, and merges the four waves' ``(m, l, o)`` through LDS;
``decode_combine`` merges the partitions through HBM and normalises.  Two data sets have outputs that
are exact by construction and are compared bit for bit on the device; a third is held to a derived
bound against float64 on the host.  ``decode_attention`` runs the same kernels on caller-supplied
arrays; ``operands`` and ``expected`` are the host's side on its own and need no GPU.
``canary.run()`` and the plugin do not call this check yet.  Missing library => it is built, or a
loud ``RuntimeError`` (never a silent pass).

``python -m k8s_gpu_device_plugin_amd.ops.decode [--device N] [--batch B] [--q-heads H] [--kv-heads K]
[--seq S] [--splits P] [--iters I] [--inject]`` prints one JSON line.
"""
from __future__ import annotations

import ctypes
import os

from ._sites import load_library

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decode", "libamdgpu_decode.so")

HEAD_DIM, PAGE = 128, 16
SETS = ("uniform", "routed", "hashed")   # ids 0, 1, 2 of decode_host.h; the first two are exact
INJECT, SKIP_VERIFIED_LAUNCH = 1, 2      # flags of amdgpu_decode_check, as in decode.h


class DecodeResult(ctypes.Structure):
    _fields_ = [(f, ctypes.c_ulonglong * 3) for f in ("o_errors", "lse_errors", "first_bad", "first_bad_lse")] + \
               [("ms", ctypes.c_double * 3), ("kv_gbps", ctypes.c_double), ("max_err", ctypes.c_double),
                ("max_lse_err", ctypes.c_double)] + \
               [(f, ctypes.c_int) for f in ("batch", "q_heads", "kv_heads", "seq", "splits", "iters")]


EXPORTS = ("run", "check", "describe", "operands", "expected", "sizeof")


def _declare(lib) -> None:
    res_p, ptr = ctypes.POINTER(DecodeResult), ctypes.c_void_p
    lib.amdgpu_decode_run.argtypes = [ctypes.c_int] + [ptr] * 7 + [ctypes.c_int] * 6 + [ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_decode_check.argtypes = [ctypes.c_int] * 8 + [res_p, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_decode_describe.argtypes = [res_p, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_decode_operands.argtypes = [ctypes.c_int] * 5 + [ptr] * 5
    lib.amdgpu_decode_expected.argtypes = [ctypes.c_int] * 5 + [ptr] * 2
    lib.amdgpu_decode_sizeof.argtypes = [ctypes.c_int]
    for name in EXPORTS:
        getattr(lib, "amdgpu_decode_" + name).restype = ctypes.c_int


def load():
    return load_library(LIB_PATH, "build_decode", _declare)


def operands(set, batch: int, q_heads: int, kv_heads: int, seq: int):
    """The check's own data of ``set`` (a name of ``SETS``) as the check lays it out, host only:
    ``q`` [batch, q_heads, 128], ``k_cache`` and ``v_cache`` [batch * ceil(seq / 16), kv_heads, 16, 128]
    as bf16 bit patterns (uint16; 0xFFFF, a NaN, wherever no visible key lies), ``block_table``
    [batch, ceil(seq / 16)] (int32, a permutation of the pages, -1 past a sequence's last page) and
    ``seq_lens`` [batch] (int32, hashed in [seq / 2, seq]; the first is ``seq``, the second odd)."""
    import numpy as np

    pages = max(0, -(-int(seq) // PAGE))
    q = np.zeros((batch, q_heads, HEAD_DIM), dtype=np.uint16)
    k, v = (np.zeros((batch * pages, kv_heads, PAGE, HEAD_DIM), dtype=np.uint16) for _ in range(2))
    table, lens = np.zeros((batch, pages), dtype=np.int32), np.zeros(batch, dtype=np.int32)
    if load().amdgpu_decode_operands(SETS.index(set), int(batch), int(q_heads), int(kv_heads), int(seq), q.ctypes.data,
                                     k.ctypes.data, v.ctypes.data, table.ctypes.data, lens.ctypes.data) != 0:
        raise ValueError("decode.operands: positive sizes, q_heads = G kv_heads with G in 1, 2, 4, 8, 16, not (%d, %d/%d, %d)"
                         % (batch, q_heads, kv_heads, seq))
    return q, k, v, table, lens


def expected(set, batch: int, q_heads: int, kv_heads: int, seq: int):
    """What healthy kernels give for an exact set on ``operands(set, ...)``, host only: ``o`` float32
    [batch, q_heads, 128], bit for bit (the integer sum of V over the visible keys of highest score,
    one IEEE division by their number), and ``lse`` float64 [batch, q_heads] (the log of that number
    plus the highest scaled score)."""
    import numpy as np

    o, lse = np.zeros((batch, q_heads, HEAD_DIM), dtype=np.float32), np.zeros((batch, q_heads), dtype=np.float64)
    if load().amdgpu_decode_expected(SETS.index(set), int(batch), int(q_heads), int(kv_heads), int(seq), o.ctypes.data,
                                     lse.ctypes.data) != 0:
        raise ValueError("decode.expected: an exact set (uniform, routed) and a shape operands() takes, not %s (%d, %d/%d, %d)"
                         % (set, batch, q_heads, kv_heads, seq))
    return o, lse


def decode_attention(q, k_cache, v_cache, block_table, seq_lens, splits: int = 0, device: int = 0):
    """``softmax(q k^T / sqrt(128)) v`` of one query token per sequence over a paged KV cache.  ``q``
    [B, Hq, 128], ``k_cache`` and ``v_cache`` [P, Hkv, 16, 128]: bf16 bit patterns (uint16).
    ``block_table`` [B, max_pages] int32: entry ``t`` is the physical page of keys ``16 t .. 16 t + 15``
    (entries past a sequence's last page are not read).  ``seq_lens`` [B] int32, each in 1 .. 65536.
    ``Hq = G Hkv`` with G in 1, 2, 4, 8, 16; query head ``hq`` reads KV head ``hq // G``.  ``splits``
    partitions of each sequence's key range, at most 64; 0: the library chooses.  A call that does
    not fit is refused with a text before anything is launched.  Returns ``o`` float32 [B, Hq, 128]
    and ``lse`` float32 [B, Hq], the natural-log sum of exponentials of the scaled scores."""
    import numpy as np

    q, k_cache, v_cache = (np.ascontiguousarray(x, dtype=np.uint16) for x in (q, k_cache, v_cache))
    block_table, seq_lens = (np.ascontiguousarray(x, dtype=np.int32) for x in (block_table, seq_lens))
    if q.ndim != 3 or k_cache.ndim != 4 or k_cache.shape != v_cache.shape or block_table.ndim != 2 or \
            seq_lens.shape != (q.shape[0],) or block_table.shape[0] != q.shape[0] or q.shape[2] != HEAD_DIM or \
            k_cache.shape[2:] != (PAGE, HEAD_DIM):
        raise ValueError("shapes do not match: q %s, k_cache %s, v_cache %s, block_table %s, seq_lens %s"
                         % (q.shape, k_cache.shape, v_cache.shape, block_table.shape, seq_lens.shape))
    (b, hq, _), (p, hkv) = q.shape, k_cache.shape[:2]
    o, lse = np.empty((b, hq, HEAD_DIM), dtype=np.float32), np.empty((b, hq), dtype=np.float32)
    err = ctypes.create_string_buffer(256)
    if load().amdgpu_decode_run(int(device), q.ctypes.data, k_cache.ctypes.data, v_cache.ctypes.data, block_table.ctypes.data,
                                seq_lens.ctypes.data, o.ctypes.data, lse.ctypes.data, b, hq, hkv, p, block_table.shape[1],
                                int(splits), err, 256) != 0:
        raise RuntimeError("decode_attention failed: " + err.value.decode(errors="replace"))
    return o, lse


def decode_check(device: int = 0, batch: int = 0, q_heads: int = 0, kv_heads: int = 0, seq: int = 0, splits: int = 0,
                 iters: int = 20, inject: bool = False, skip_verified_launch: bool = False) -> dict:
    """The decode-attention path on each of ``SETS``: the caches filled on the device through the
    check's permuted block table (NaN wherever no visible key lies), one warm-up launch pair,
    ``iters`` timed pairs, then one more written into poisoned (all 0xFF) o and lse, and the verdict
    on that output.  ``uniform`` and ``routed`` are compared bit for bit with the closed form on the
    device; ``hashed`` is held to ``|o - ref| <= (2^-8 + 2^-20) 4`` and ``|lse - ref| <= 2^-8 + 2^-20 |ref|``
    against float64 on the host for every sequence and head.  Sizes of 0 mean the default workload
    (64 sequences of up to 8192 keys, 32 query heads on 8 KV heads); ``splits`` 0 lets the library
    choose.  ``inject`` corrupts one element of each verified output (1 error per set);
    ``skip_verified_launch`` leaves the poison in place.

    Returns ``ok``, ``error`` (the first failing set's text), ``ms`` (device time of all timed
    pairs), ``kv_gbps`` (bytes of K and V of all visible pages over that time; reported, never
    judged), ``o_errors``, ``lse_errors``, ``decode_errors`` (their sum), ``max_err`` and
    ``max_lse_err`` (the hashed set's largest deviations), ``batch``, ``q_heads``, ``kv_heads``,
    ``seq``, ``splits`` (as run), ``iters``, and ``sets``: per set ``o_errors``, ``lse_errors`` and ``ms``."""
    lib = load()
    flags = (INJECT if inject else 0) | (SKIP_VERIFIED_LAUNCH if skip_verified_launch else 0)
    r, err = DecodeResult(), ctypes.create_string_buffer(256)
    if lib.amdgpu_decode_check(int(device), int(batch), int(q_heads), int(kv_heads), int(seq), int(splits), int(iters), flags,
                               ctypes.byref(r), err, 256) != 0:
        raise RuntimeError("decode_check failed: " + err.value.decode(errors="replace"))
    lib.amdgpu_decode_describe(ctypes.byref(r), err, 256)
    sets = {name: {"o_errors": int(r.o_errors[i]), "lse_errors": int(r.lse_errors[i]), "ms": float(r.ms[i])}
            for i, name in enumerate(SETS)}
    o_errors, lse_errors = sum(r.o_errors), sum(r.lse_errors)
    return {"ok": o_errors + lse_errors == 0, "error": err.value.decode(errors="replace"), "ms": sum(r.ms),
            "kv_gbps": float(r.kv_gbps), "o_errors": int(o_errors), "lse_errors": int(lse_errors),
            "decode_errors": int(o_errors + lse_errors), "max_err": float(r.max_err), "max_lse_err": float(r.max_lse_err),
            "sets": sets, "batch": int(r.batch), "q_heads": int(r.q_heads), "kv_heads": int(r.kv_heads), "seq": int(r.seq),
            "splits": int(r.splits), "iters": int(r.iters)}


def main(argv=None) -> int:
    import argparse
    import json

    ap = argparse.ArgumentParser(description="The decode-attention check on one device; prints one JSON line.")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--batch", type=int, default=0, help="sequences; default 0: the library's workload (64)")
    ap.add_argument("--q-heads", type=int, default=0, help="default 0: the library's workload (32)")
    ap.add_argument("--kv-heads", type=int, default=0, help="default 0: the library's workload (8)")
    ap.add_argument("--seq", type=int, default=0, help="keys of the longest sequence; default 0: the library's workload (8192)")
    ap.add_argument("--splits", type=int, default=0, help="partitions of a sequence's keys; default 0: the library chooses")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--inject", action="store_true", help="corrupt one element of each verified output")
    args = ap.parse_args(argv)
    r = decode_check(args.device, args.batch, args.q_heads, args.kv_heads, args.seq, args.splits, args.iters, inject=args.inject)
    print(json.dumps(r))
    return 0 if r["ok"] else 1


if __name__ == "__main__":
    import sys

    sys.exit(main())
