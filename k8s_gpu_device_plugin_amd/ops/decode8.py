"""Python face of the stand-alone fp8 decode-attention check (``ops/decode8/decode8.hip``; the C ABI mirrored
here is declared in ``ops/decode8/decode8.h`` and ``ops/decode8/decode8_host.h``).

``decode_check(device)`` loads ``ops/decode8/libamdgpu_decode8.so`` with ctypes and runs decode
attention as ``ops/decode`` does, on the cache inference containers actually keep: K and V as OCP
e4m3 codes in pages of 16 keys (2 KiB per page and KV head) behind a block table, with one
dequantisation scale per KV head for K and one for V.  ``kv8_split`` streams each wave's own pages
HBM -> LDS by DMA as 128 B rows, decodes fp8 to bf16 in registers between the LDS read and
``v_mfma_f32_32x32x16_bf16`` for both products, reads V through the 8-bit transposed LDS read
(``ds_read_b64_tr_b8``), folds ``k_scale`` into the score factor and merges the four waves' states
through LDS; ``kv8_combine`` merges the partitions through HBM, normalises and applies ``v_scale``.
Two data sets have outputs that are exact by construction and are compared bit for bit on the
device; a third is held to a derived bound against float64 on the host.  ``decode_attention`` runs
the same kernels on caller-supplied arrays; ``operands`` and ``expected`` are the host's side on its
own and need no GPU.  ``canary.run()`` and the plugin do not call this check yet.  Missing library
=> it is built, or a loud ``RuntimeError`` (never a silent pass).

``python -m k8s_gpu_device_plugin_amd.ops.decode8 [--device N] [--batch B] [--q-heads H] [--kv-heads K]
[--seq S] [--splits P] [--iters I] [--inject]`` prints one JSON line.
"""
from __future__ import annotations

import ctypes
import os

from ._sites import load_library

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decode8", "libamdgpu_decode8.so")

HEAD_DIM, PAGE = 128, 16
SETS = ("uniform", "routed", "hashed")   # ids 0, 1, 2 of decode_host.h; the first two are exact
INJECT, SKIP_VERIFIED_LAUNCH = 1, 2      # flags of amdgpu_decode8_check, as in decode8.h


class Decode8Result(ctypes.Structure):
    _fields_ = [(f, ctypes.c_ulonglong * 3) for f in ("o_errors", "lse_errors", "first_bad", "first_bad_lse")] + \
               [("ms", ctypes.c_double * 3), ("kv_gbps", ctypes.c_double), ("max_err", ctypes.c_double),
                ("max_lse_err", ctypes.c_double)] + \
               [(f, ctypes.c_int) for f in ("batch", "q_heads", "kv_heads", "seq", "splits", "iters")]


EXPORTS = ("run", "check", "describe", "operands", "expected", "sizeof")


def _declare(lib) -> None:
    res_p, ptr = ctypes.POINTER(Decode8Result), ctypes.c_void_p
    lib.amdgpu_decode8_run.argtypes = [ctypes.c_int] + [ptr] * 9 + [ctypes.c_int] * 6 + [ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_decode8_check.argtypes = [ctypes.c_int] * 8 + [res_p, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_decode8_describe.argtypes = [res_p, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_decode8_operands.argtypes = [ctypes.c_int] * 5 + [ptr] * 7
    lib.amdgpu_decode8_expected.argtypes = [ctypes.c_int] * 5 + [ptr] * 2
    lib.amdgpu_decode8_sizeof.argtypes = [ctypes.c_int]
    for name in EXPORTS:
        getattr(lib, "amdgpu_decode8_" + name).restype = ctypes.c_int


def load():
    return load_library(LIB_PATH, "build_decode8", _declare)


def operands(set, batch: int, q_heads: int, kv_heads: int, seq: int):
    """The check's own data of ``set`` (a name of ``SETS``) as the check lays it out, host only:
    ``q`` [batch, q_heads, 128] as bf16 bit patterns (uint16), ``k_cache`` and ``v_cache``
    [batch * ceil(seq / 16), kv_heads, 16, 128] as e4m3 codes (uint8; 0xFF, a NaN, wherever no visible
    key lies), ``k_scale`` and ``v_scale`` [kv_heads] (float32), ``block_table`` [batch, ceil(seq / 16)]
    (int32, a permutation of the pages, -1 past a sequence's last page) and ``seq_lens`` [batch]."""
    import numpy as np

    pages = max(0, -(-int(seq) // PAGE))
    q = np.zeros((batch, q_heads, HEAD_DIM), dtype=np.uint16)
    k, v = (np.zeros((batch * pages, kv_heads, PAGE, HEAD_DIM), dtype=np.uint8) for _ in range(2))
    ks, vs = (np.zeros(max(kv_heads, 0), dtype=np.float32) for _ in range(2))
    table, lens = np.zeros((batch, pages), dtype=np.int32), np.zeros(batch, dtype=np.int32)
    if load().amdgpu_decode8_operands(SETS.index(set), int(batch), int(q_heads), int(kv_heads), int(seq), q.ctypes.data,
                                      k.ctypes.data, v.ctypes.data, ks.ctypes.data, vs.ctypes.data, table.ctypes.data,
                                      lens.ctypes.data) != 0:
        raise ValueError("decode8.operands: positive sizes, q_heads = G kv_heads with G in 1, 2, 4, 8, 16, not (%d, %d/%d, %d)"
                         % (batch, q_heads, kv_heads, seq))
    return q, k, v, ks, vs, table, lens


def expected(set, batch: int, q_heads: int, kv_heads: int, seq: int):
    """What healthy kernels give for an exact set on ``operands(set, ...)``, host only: ``o`` float32
    [batch, q_heads, 128], bit for bit (the integer sum of the V codes' values over the visible keys of
    highest score, one IEEE division by their number, one exact multiply by the head's power-of-two
    ``v_scale``), and ``lse`` float64 [batch, q_heads] (the log of that number plus the highest
    scaled score, ``k_scale`` included)."""
    import numpy as np

    o, lse = np.zeros((batch, q_heads, HEAD_DIM), dtype=np.float32), np.zeros((batch, q_heads), dtype=np.float64)
    if load().amdgpu_decode8_expected(SETS.index(set), int(batch), int(q_heads), int(kv_heads), int(seq), o.ctypes.data,
                                      lse.ctypes.data) != 0:
        raise ValueError("decode8.expected: an exact set (uniform, routed) and a shape operands() takes, not %s (%d, %d/%d, %d)"
                         % (set, batch, q_heads, kv_heads, seq))
    return o, lse


def decode_attention(q, k_cache, v_cache, k_scale, v_scale, block_table, seq_lens, splits: int = 0, device: int = 0):
    """``softmax(q k^T / sqrt(128)) v`` of one query token per sequence over a paged fp8 KV cache.  ``q``
    [B, Hq, 128]: bf16 bit patterns (uint16).  ``k_cache`` and ``v_cache`` [P, Hkv, 16, 128]: OCP e4m3
    codes (uint8; bias 7, largest value 448, 0x7F / 0xFF are NaN).  ``k_scale`` and ``v_scale`` [Hkv]
    float32, finite and positive: key ``j`` of KV head ``h`` is ``k_scale[h] * fp8(k_cache[...])``,
    likewise V.  ``block_table``, ``seq_lens``, ``Hq = G Hkv`` and ``splits`` are ``decode.decode_attention``'s.
    A call that does not fit is refused with a text before anything is launched.  Returns ``o``
    float32 [B, Hq, 128] and ``lse`` float32 [B, Hq], the natural-log sum of exponentials of the scaled scores."""
    import numpy as np

    q = np.ascontiguousarray(q, dtype=np.uint16)
    k_cache, v_cache = (np.ascontiguousarray(x, dtype=np.uint8) for x in (k_cache, v_cache))
    k_scale, v_scale = (np.ascontiguousarray(x, dtype=np.float32) for x in (k_scale, v_scale))
    block_table, seq_lens = (np.ascontiguousarray(x, dtype=np.int32) for x in (block_table, seq_lens))
    if q.ndim != 3 or k_cache.ndim != 4 or k_cache.shape != v_cache.shape or block_table.ndim != 2 or \
            seq_lens.shape != (q.shape[0],) or block_table.shape[0] != q.shape[0] or q.shape[2] != HEAD_DIM or \
            k_cache.shape[2:] != (PAGE, HEAD_DIM) or k_scale.shape != (k_cache.shape[1],) or v_scale.shape != k_scale.shape:
        raise ValueError("shapes do not match: q %s, k_cache %s, v_cache %s, k_scale %s, v_scale %s, block_table %s, seq_lens %s"
                         % (q.shape, k_cache.shape, v_cache.shape, k_scale.shape, v_scale.shape, block_table.shape, seq_lens.shape))
    (b, hq, _), (p, hkv) = q.shape, k_cache.shape[:2]
    o, lse = np.empty((b, hq, HEAD_DIM), dtype=np.float32), np.empty((b, hq), dtype=np.float32)
    err = ctypes.create_string_buffer(256)
    if load().amdgpu_decode8_run(int(device), q.ctypes.data, k_cache.ctypes.data, v_cache.ctypes.data, k_scale.ctypes.data,
                                 v_scale.ctypes.data, block_table.ctypes.data, seq_lens.ctypes.data, o.ctypes.data,
                                 lse.ctypes.data, b, hq, hkv, p, block_table.shape[1], int(splits), err, 256) != 0:
        raise RuntimeError("decode_attention failed: " + err.value.decode(errors="replace"))
    return o, lse


def decode_check(device: int = 0, batch: int = 0, q_heads: int = 0, kv_heads: int = 0, seq: int = 0, splits: int = 0,
                 iters: int = 20, inject: bool = False, skip_verified_launch: bool = False) -> dict:
    """The fp8 decode-attention path on each of ``SETS``: both caches set to 0xFF (an e4m3 NaN) and
    filled on the device through the check's permuted block table, one warm-up launch pair, ``iters``
    timed pairs, then one more written into poisoned (all 0xFF) o and lse, and the verdict on that
    output.  ``uniform`` and ``routed`` (power-of-two scales that differ per KV head) are compared bit
    for bit with the closed form on the device; ``hashed`` (scales in [1/2, 2), no powers of two) is
    held to ``|o - ref| <= (2^-8 + 2^-13) 4 v_scale`` and ``|lse - ref| <= 2^-8 + 2^-20 |ref|`` against
    float64 over the dequantised values on the host for every sequence and head.  Sizes of 0 mean the
    default workload (64 sequences of up to 8192 keys, 32 query heads on 8 KV heads: 1 GiB of K and V);
    ``splits`` 0 lets the library choose.  ``inject`` corrupts one element of each verified output
    (1 error per set); ``skip_verified_launch`` leaves the poison in place.

    Returns ``decode.decode_check``'s keys, with ``decode8_errors`` for the sum of ``o_errors`` and
    ``lse_errors``; ``max_err`` is the hashed set's largest ``|o - ref| / v_scale``."""
    lib = load()
    flags = (INJECT if inject else 0) | (SKIP_VERIFIED_LAUNCH if skip_verified_launch else 0)
    r, err = Decode8Result(), ctypes.create_string_buffer(256)
    if lib.amdgpu_decode8_check(int(device), int(batch), int(q_heads), int(kv_heads), int(seq), int(splits), int(iters), flags,
                                ctypes.byref(r), err, 256) != 0:
        raise RuntimeError("decode_check failed: " + err.value.decode(errors="replace"))
    lib.amdgpu_decode8_describe(ctypes.byref(r), err, 256)
    sets = {name: {"o_errors": int(r.o_errors[i]), "lse_errors": int(r.lse_errors[i]), "ms": float(r.ms[i])}
            for i, name in enumerate(SETS)}
    o_errors, lse_errors = sum(r.o_errors), sum(r.lse_errors)
    return {"ok": o_errors + lse_errors == 0, "error": err.value.decode(errors="replace"), "ms": sum(r.ms),
            "kv_gbps": float(r.kv_gbps), "o_errors": int(o_errors), "lse_errors": int(lse_errors),
            "decode8_errors": int(o_errors + lse_errors), "max_err": float(r.max_err), "max_lse_err": float(r.max_lse_err),
            "sets": sets, "batch": int(r.batch), "q_heads": int(r.q_heads), "kv_heads": int(r.kv_heads), "seq": int(r.seq),
            "splits": int(r.splits), "iters": int(r.iters)}


def main(argv=None) -> int:
    import argparse
    import json

    ap = argparse.ArgumentParser(description="The fp8 decode-attention check on one device; prints one JSON line.")
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
