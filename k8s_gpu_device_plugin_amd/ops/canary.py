"""Python face of the gfx950 health canary (``ops/canary.hip`` and the sources named below;
the C ABI mirrored here is declared in ``ops/canary_common.h``).

``run(device)`` loads ``libamdgpu_canary.so`` with ctypes (no torch needed) and runs
the HBM pattern test (``hbm.hip``), the MFMA exactness/throughput probe, the matrix-path check
(``gemm.hip``: an LDS-staged MFMA GEMM on exact integer data with ABFT row/column checksums), the
fp8 / bf8 / fp4 MFMA exactness and rate checks, the LDS march (``datapath.hip``), the
site probe (``sites.hip``: MFMA and vector-ALU exactness on every CU and SIMD, each
mismatch located), the fabric check (``fabric.hip``: a march through each XCD's L2, a
cross-XCD exchange and the global atomics) and the CU memory check (``cumem.hip``: a march
over each SIMD's vector register file and re-reads through each CU's vector L1) on
one HIP device (= one compute partition).  ``run_isolated(device)`` does the same in a child process so the
long-lived plugin daemon never creates a HIP context on GPUs it hands to pods.

CLI: ``python -m k8s_gpu_device_plugin_amd.ops.canary --device 0 [--bytes N]`` prints
one JSON line; ``--sites`` prints the site probe's coverage map instead, ``--fabric`` the
fabric check's per-XCD tables, ``--cu`` the CU memory check's per-site table, ``--host-link``
the host-link check (``ops/hostlink.py``: PCIe reads, writes, copies and system atomics), which
``--with-host-link`` / ``run(host_link=True)`` merges into the full run, ``--pace`` the pace
check (``ops/pace.py``: in-kernel clock and rate per XCD, CU and SIMD), which ``--with-pace`` /
``run(pace=True)`` merges likewise, ``--lds-path`` the LDS-path check (``ops/ldspath.py``: LDS
widths, atomics and transposed read per CU, every lane-crossing instruction per SIMD), which
``--with-lds-path`` / ``run(lds_path=True)`` merges likewise.  Missing library => loud ``RuntimeError`` (never a silent
pass).
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import os
import subprocess
import sys
from typing import NamedTuple

from ._sites import SITE_SLOTS, UNWRITTEN, decode_site, format_site, load_library  # noqa: F401

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libamdgpu_canary.so")


class CanaryResult(ctypes.Structure):
    _fields_ = [("ok", ctypes.c_int), ("device", ctypes.c_int), ("hbm_bytes", ctypes.c_ulonglong),
                ("hbm_errors", ctypes.c_ulonglong), ("mfma_errors", ctypes.c_ulonglong),
                ("write_gbps", ctypes.c_double), ("read_gbps", ctypes.c_double), ("mfma_tflops", ctypes.c_double),
                ("elapsed_ms", ctypes.c_double), ("num_cus", ctypes.c_int), ("arch", ctypes.c_char * 64),
                ("error", ctypes.c_char * 256), ("gemm_tflops", ctypes.c_double),
                ("gemm_errors", ctypes.c_ulonglong), ("fp8_tflops", ctypes.c_double),
                ("fp4_tflops", ctypes.c_double), ("lowp_errors", ctypes.c_ulonglong),
                ("lds_errors", ctypes.c_ulonglong), ("lds_bytes", ctypes.c_ulonglong),
                ("site_errors", ctypes.c_ulonglong), ("cus_reached", ctypes.c_int),
                ("simds_reached", ctypes.c_int), ("cus_unreached", ctypes.c_int), ("site_ms", ctypes.c_double),
                ("n_bad_sites", ctypes.c_int), ("bad_sites", ctypes.c_uint * 16),
                ("l2_errors", ctypes.c_ulonglong), ("xcd_errors", ctypes.c_ulonglong),
                ("atomic_errors", ctypes.c_ulonglong), ("l2_gbps", ctypes.c_double), ("fabric_ms", ctypes.c_double),
                ("xccs_reached", ctypes.c_int), ("xcd_pairs_reached", ctypes.c_int),
                ("xcd_pairs_unreached", ctypes.c_int)]


SITE_CHECKS = ("mfma", "lowp", "valu")


class SiteSlot(ctypes.Structure):
    _fields_ = [("waves", ctypes.c_uint), ("bad", ctypes.c_uint * 3)]


class SitesResult(ctypes.Structure):
    _fields_ = [("errors", ctypes.c_ulonglong * 3), ("unlocated_errors", ctypes.c_ulonglong),
                ("waves", ctypes.c_ulonglong), ("moved", ctypes.c_ulonglong), ("launches", ctypes.c_int),
                ("cus_reached", ctypes.c_int), ("simds_reached", ctypes.c_int), ("cus_expected", ctypes.c_int),
                ("n_bad", ctypes.c_int), ("bad_sites", ctypes.c_uint * 16), ("ms", ctypes.c_double)]


FABRIC_XCCS = 16
# the global-atomic forms of the fabric check, in the order of ops/fabric.hip
ATOMIC_OPS = ("u32_add", "u64_add", "i32_min", "u32_max", "u64_max", "and", "or", "xor", "f32_add", "f64_add",
              "pk_add_bf16", "pk_add_f16", "cas_inc", "ticket")
FABRIC_INJECT = ("l2", "xcd", "atomic")
ATOMIC_ELEMS = 2048
# element type of each operation's table: the packed forms as 16-bit patterns (low half first),
# cas_inc as its 64 words, ticket as the ticket word followed by seen[16384]
_ATOMIC_DTYPES = {"u64_add": "uint64", "u64_max": "uint64", "i32_min": "int32", "f32_add": "float32",
                  "f64_add": "float64", "pk_add_bf16": "uint16", "pk_add_f16": "uint16"}


class XccSlot(ctypes.Structure):
    _fields_ = [("blocks", ctypes.c_ulonglong), ("bytes", ctypes.c_ulonglong), ("bad", ctypes.c_ulonglong)]


class PairSlot(ctypes.Structure):
    _fields_ = [("reads", ctypes.c_ulonglong), ("bad", ctypes.c_ulonglong)]


class FabricResult(ctypes.Structure):
    _fields_ = [("l2_errors", ctypes.c_ulonglong), ("unlocated_errors", ctypes.c_ulonglong),
                ("xcd_errors", ctypes.c_ulonglong), ("atomic_errors", ctypes.c_ulonglong),
                ("moved", ctypes.c_ulonglong), ("atomic_bad", ctypes.c_ulonglong * len(ATOMIC_OPS)),
                ("march_read_bytes", ctypes.c_ulonglong), ("blocks", ctypes.c_int), ("slice_kb", ctypes.c_int),
                ("xccs_reached", ctypes.c_int), ("pairs_reached", ctypes.c_int), ("pairs_expected", ctypes.c_int),
                ("first_bad_slice", ctypes.c_int), ("first_bad_offset", ctypes.c_uint),
                ("first_bad_xcc", ctypes.c_int), ("first_bad_op", ctypes.c_int), ("first_bad_elem", ctypes.c_int),
                ("march_ms", ctypes.c_double), ("exchange_ms", ctypes.c_double), ("atomic_ms", ctypes.c_double)]


CU_INJECT = ("vgpr", "agpr", "l1")


class OptionalCheck(NamedTuple):
    """An opt-in check: a library and a Python face of its own, merged into ``run`` when asked for."""
    keyword: str   # of run() and run_isolated()
    stem: str      # "--<stem>": only this check; "--with-<stem>": the full run with it merged in
    module: str    # its Python face in ops/, imported when it runs
    function: str  # called as function(device, *args)
    args: tuple    # (keyword of run(), default, key of health.*) of each further argument; "--<keyword>" on the command line
    title: str     # "the pace check", for the help texts
    detail: str    # what it covers, for the help text of "--<stem>"
    keys: tuple    # (key in run()'s result, key of the check's result or a callable on it), in the order merged
    errors: tuple  # (label, key) pairs it adds to amdgpu_canary_errors
    switch: str    # the health.* option that turns it on


# In the order run() merges them.  run_isolated's flags, main's arguments and the metric labels go in the
# order the checks were added, which is the reverse.
OPTIONAL_CHECKS = (
    # lds_errors is already lds_march's count, so the width passes' is lds_width_errors
    OptionalCheck("lds_path", "lds-path", "ldspath", "ldspath_check", (),
                  "the LDS-path check", "LDS widths, atomics, lane swaps and the transposed read, per site",
                  (("ldspath_errors", "ldspath_errors"), ("lds_width_errors", "lds_errors"), ("lds_dma_errors", "dma_errors"),
                   ("lds_atomic_errors", "lds_atomic_errors"), ("lane_errors", "lane_errors"), ("tr_errors", "tr_errors"),
                   ("ldspath_ms", "ms"), ("ldspath_bad_sites", "bad_sites")),
                  (("lds_width", "lds_width_errors"), ("lds_dma", "lds_dma_errors"), ("lds_atomic", "lds_atomic_errors"),
                   ("lane", "lane_errors"), ("lds_tr", "tr_errors")),
                  "canaryLdsPath"),
    # wrong results fail the run; slowness is carried as figures and pace_note for the caller's floors
    OptionalCheck("pace", "pace", "pace", "pace_check", (),
                  "the pace check", "in-kernel clock and rate per XCD, CU and SIMD",
                  (("pace_errors", "pace_errors"), ("clock_mhz_min", "clock_mhz_min"), ("clock_mhz_max", "clock_mhz_max"),
                   ("clock_fraction", "clock_fraction"), ("xcd_pace_ratio", "xcd_pace_ratio"),
                   ("xcd_mem_ratio", "xcd_mem_ratio"), ("pace_slow_sites", "slow_sites"), ("pace_slow_xccs", "slow_xccs"),
                   ("pace_ms", "ms"), ("pace_note", "note")),
                  (("pace", "pace_errors"),),
                  "canaryPace"),
    OptionalCheck("host_link", "host-link", "hostlink", "host_link_check",
                  (("host_link_bytes", 64 << 20, "canaryHostLinkBytes"),),
                  "the host-link check", "PCIe reads, writes, copies and system atomics",
                  (("host_read_errors", "read_errors"), ("host_write_errors", "write_errors"),
                   ("host_copy_errors", lambda hl: hl["h2d_errors"] + hl["d2h_errors"]),
                   ("host_atomic_errors", "atomic_errors"), ("kernel_read_gbps", "kernel_read_gbps"),
                   ("kernel_write_gbps", "kernel_write_gbps"), ("copy_h2d_gbps", "copy_h2d_gbps"),
                   ("copy_d2h_gbps", "copy_d2h_gbps"), ("host_ms", "ms")),
                  (("host_read", "host_read_errors"), ("host_write", "host_write_errors"),
                   ("host_copy", "host_copy_errors"), ("host_atomic", "host_atomic_errors")),
                  "canaryHostLink"),
)
_LDS_PATH, _PACE, _HOST_LINK = OPTIONAL_CHECKS
# what the LDS-path check merges into run()'s result: (key there, key of ldspath_check)
LDS_PATH_KEYS = _LDS_PATH.keys
# what the pace check merges into run()'s result under the same name
PACE_KEYS = tuple(key for key, theirs in _PACE.keys if key == theirs)
# the rates the host-link check merges into run()'s result
HOST_LINK_RATES = tuple(key for key, _ in _HOST_LINK.keys if key.endswith("_gbps"))


class CuSlot(ctypes.Structure):
    _fields_ = [("waves", ctypes.c_uint), ("bad_vgpr", ctypes.c_uint), ("bad_agpr", ctypes.c_uint),
                ("bad_l1", ctypes.c_uint)]


class CuResult(ctypes.Structure):
    _fields_ = [("vgpr_errors", ctypes.c_ulonglong), ("agpr_errors", ctypes.c_ulonglong),
                ("l1_errors", ctypes.c_ulonglong), ("l1_fill_errors", ctypes.c_ulonglong),
                ("unlocated_errors", ctypes.c_ulonglong), ("moved", ctypes.c_ulonglong),
                ("waves", ctypes.c_ulonglong), ("l1_moved", ctypes.c_ulonglong), ("launches", ctypes.c_int),
                ("cus_reached", ctypes.c_int), ("simds_reached", ctypes.c_int), ("cus_expected", ctypes.c_int),
                ("l1_cus_reached", ctypes.c_int), ("regs_vgpr", ctypes.c_int), ("regs_agpr", ctypes.c_int),
                ("n_bad", ctypes.c_int), ("bad_sites", ctypes.c_uint * 16), ("reg_ms", ctypes.c_double),
                ("l1_ms", ctypes.c_double)]


def _declare(lib) -> None:
    lib.amdgpu_canary_run.argtypes = [ctypes.c_int, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(CanaryResult)]
    lib.amdgpu_canary_run.restype = ctypes.c_int
    lib.amdgpu_canary_device_count.restype = ctypes.c_int
    lib.amdgpu_canary_mfma_gemm.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                                            ctypes.c_int]
    lib.amdgpu_canary_mfma_gemm.restype = ctypes.c_int
    lib.amdgpu_canary_detects_corruption.argtypes = [ctypes.c_int, ctypes.c_ulonglong, ctypes.c_int]
    lib.amdgpu_canary_detects_corruption.restype = ctypes.c_longlong
    lib.amdgpu_canary_mfma_detects.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.amdgpu_canary_mfma_detects.restype = ctypes.c_longlong
    lib.amdgpu_canary_hbm_sweep.argtypes = [ctypes.c_int, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ulonglong)]
    lib.amdgpu_canary_hbm_sweep.restype = ctypes.c_int
    lib.amdgpu_canary_gemm.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                                       ctypes.c_int]
    lib.amdgpu_canary_gemm.restype = ctypes.c_int
    lib.amdgpu_canary_gemm_rate.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_canary_gemm_rate.restype = ctypes.c_int
    lib.amdgpu_canary_abft.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong),
                                       ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_canary_abft.restype = ctypes.c_int
    lib.amdgpu_canary_gemm_tile_map.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_int]
    lib.amdgpu_canary_gemm_tile_map.restype = ctypes.c_int
    lib.amdgpu_canary_lowp_check.argtypes = [ctypes.c_int] * 5
    lib.amdgpu_canary_lowp_check.restype = ctypes.c_longlong
    lib.amdgpu_canary_lowp_rate.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_double)]
    lib.amdgpu_canary_lowp_rate.restype = ctypes.c_int
    lib.amdgpu_canary_lds_check.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong)]
    lib.amdgpu_canary_lds_check.restype = ctypes.c_longlong
    lib.amdgpu_canary_lowp_gemm.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5 + \
        [ctypes.c_int] * 3 + [ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_canary_lowp_gemm.restype = ctypes.c_int
    lib.amdgpu_canary_sites.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(SiteSlot),
                                                             ctypes.POINTER(ctypes.c_uint), ctypes.c_int,
                                                             ctypes.POINTER(SitesResult), ctypes.c_char_p,
                                                             ctypes.c_int]
    lib.amdgpu_canary_sites.restype = ctypes.c_int
    lib.amdgpu_canary_fabric.argtypes = [ctypes.c_int] * 7 + [ctypes.POINTER(XccSlot), ctypes.POINTER(PairSlot),
                                                              ctypes.POINTER(ctypes.c_uint), ctypes.c_int,
                                                              ctypes.POINTER(FabricResult), ctypes.c_char_p,
                                                              ctypes.c_int]
    lib.amdgpu_canary_fabric.restype = ctypes.c_int
    lib.amdgpu_canary_fabric_describe.argtypes = [ctypes.POINTER(FabricResult), ctypes.POINTER(XccSlot),
                                                  ctypes.POINTER(PairSlot), ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_canary_fabric_describe.restype = ctypes.c_int
    lib.amdgpu_canary_atomic_expected.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    lib.amdgpu_canary_atomic_expected.restype = ctypes.c_int
    lib.amdgpu_canary_cu.argtypes = [ctypes.c_int] * 7 + [ctypes.POINTER(CuSlot), ctypes.POINTER(ctypes.c_uint),
                                                          ctypes.c_int, ctypes.POINTER(CuResult),
                                                          ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_canary_cu.restype = ctypes.c_int
    lib.amdgpu_canary_cu_describe.argtypes = [ctypes.POINTER(CuResult), ctypes.POINTER(CuSlot), ctypes.c_char_p,
                                              ctypes.c_int]
    lib.amdgpu_canary_cu_describe.restype = ctypes.c_int
    lib.amdgpu_canary_cu_regs.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.amdgpu_canary_cu_regs.restype = None
    lib.amdgpu_canary_cu_sizeof.argtypes = [ctypes.c_int]
    lib.amdgpu_canary_cu_sizeof.restype = ctypes.c_int


def load():
    return load_library(LIB_PATH, "build_canary", _declare)


def device_count() -> int:
    return load().amdgpu_canary_device_count()


def run(device: int = 0, hbm_bytes: int = 1 << 30, passes: int = 3, mfma_iters: int = 8192, host_link: bool = False,
        host_link_bytes: int = 64 << 20, pace: bool = False, lds_path: bool = False) -> dict:
    r = CanaryResult()
    rc = load().amdgpu_canary_run(int(device), int(hbm_bytes), int(passes), int(mfma_iters), ctypes.byref(r))
    out = {f[0]: getattr(r, f[0]) for f in CanaryResult._fields_}
    out["arch"] = r.arch.decode(errors="replace")
    out["error"] = r.error.decode(errors="replace")
    out["ok"] = bool(r.ok) and rc == 0
    out["bad_sites"] = [format_site(p) for p in r.bad_sites[:min(r.n_bad_sites, 16)]]
    # the CU memory check has its own entry point (amdgpu_canary_result is a fixed ABI):
    # same process, same device, merged into the same verdict
    try:
        cu = cu_check(device)
    except (RuntimeError, OSError) as e:
        out["ok"] = False
        out["error"] = out["error"] or str(e)
        return out
    out["reg_errors"] = cu["vgpr_errors"] + cu["agpr_errors"] + cu["unlocated_errors"]
    out["l1_errors"] = cu["l1_errors"]
    out["l1_fill_errors"] = cu["l1_fill_errors"]  # came from L2 / HBM: reported, not an L1 verdict
    out["cu_ms"] = cu["reg_ms"] + cu["l1_ms"]
    out["regs_marched"] = cu["regs_marched"]
    out["cu_bad_sites"] = cu["bad_sites"]
    if out["reg_errors"] or out["l1_errors"]:
        out["ok"] = False
        out["error"] = out["error"] or cu["error"]
    asked = {"lds_path": lds_path, "pace": pace, "host_link": host_link, "host_link_bytes": host_link_bytes}
    for check in OPTIONAL_CHECKS:
        if asked[check.keyword]:
            _merge(out, check, device, *(asked[arg] for arg, _, _ in check.args))
    return out


def _function(check: OptionalCheck):
    return getattr(importlib.import_module("." + check.module, __package__), check.function)


def _merge(out: dict, check: OptionalCheck, device: int, *args) -> None:
    """One opt-in check (a library of its own), same process and device, merged into ``run``'s
    verdict the way the CU memory check is."""
    try:
        p = _function(check)(device, *args)
    except (RuntimeError, OSError) as e:
        out["ok"] = False
        out["error"] = out["error"] or str(e)
        return
    for key, theirs in check.keys:
        out[key] = theirs(p) if callable(theirs) else p[theirs]
    if not p["ok"]:
        out["ok"] = False
        out["error"] = out["error"] or p["error"]


def cu_check(device: int = 0, blocks: int = 0, reps: int = 2, l1_kb: int = 16, l1_reps: int = 4, inject=None,
             inject_waves: int = 0) -> dict:
    """The two storage arrays next to the ALUs (``ops/cumem.hip``), as 4-wave workgroups whose
    waves record their site like the site probe's.  The register march: every lane keeps
    ``regs_vgpr`` values pinned in VGPRs and ``regs_agpr`` in AGPRs, all live at once (a wave
    is allocated its SIMD's whole 512-entry file), writes them, verifies them ascending, writes
    the complement and verifies descending, ``reps`` times.  The L1 march: each workgroup (one
    resident per CU) reads its ``l1_kb`` KiB slice with plain loads, then re-reads it
    ``l1_reps`` times, alternately reversed and forward.  ``blocks=0``: 2 workgroups per CU
    plus up to 3 top-up launches while a CU or SIMD is missing; ``blocks>0``: one launch.
    ``inject`` (``vgpr``, ``agpr`` or ``l1``) makes the first ``inject_waves`` waves (``l1``:
    workgroups) flip one bit of one value they then compare.

    Returns the totals (``vgpr_errors``, ``agpr_errors``, ``unlocated_errors``: wrong register
    words; ``l1_errors``: wrong re-read words; ``l1_fill_errors``: wrong words of the first
    read, which came from L2 or HBM), the coverage counts, ``regs_marched`` and
    ``reg_bytes_per_simd``, ``sites``, ``wave_sites`` / ``l1_wave_sites`` (the site of each
    wave of the first launch of either kernel), ``bad_sites`` and ``error`` (the canary's
    text for the first failing check)."""
    kind = -1 if inject is None else CU_INJECT.index(inject)
    lib = load()
    r = CuResult()
    table = (CuSlot * SITE_SLOTS)()
    n_waves = 4 * (int(blocks) if blocks > 0 else 2 * 1024)  # automatic: room for 1024 CUs
    wave_sites = (ctypes.c_uint * (2 * n_waves))()  # the register march's, then the L1 march's
    err = ctypes.create_string_buffer(256)
    rc = lib.amdgpu_canary_cu(int(device), int(blocks), int(reps), int(l1_kb), int(l1_reps), kind, int(inject_waves),
                              table, wave_sites, n_waves, ctypes.byref(r), err, 256)
    if rc != 0:
        raise RuntimeError("cu_check failed: " + err.value.decode(errors="replace"))
    out = {f: int(getattr(r, f)) for f in ("vgpr_errors", "agpr_errors", "l1_errors", "l1_fill_errors",
                                           "unlocated_errors", "moved", "waves", "l1_moved", "launches",
                                           "cus_reached", "simds_reached", "cus_expected", "l1_cus_reached",
                                           "regs_vgpr", "regs_agpr", "n_bad")}
    out["regs_marched"] = out["regs_vgpr"] + out["regs_agpr"]
    out["reg_bytes_per_simd"] = out["regs_marched"] * 256  # 64 lanes x 4 B per entry
    out["reg_ms"], out["l1_ms"] = r.reg_ms, r.l1_ms
    out["bad_sites"] = [format_site(p) for p in r.bad_sites[:min(r.n_bad, 16)]]
    out["sites"] = {format_site(p): {"waves": int(s.waves), "vgpr": int(s.bad_vgpr), "agpr": int(s.bad_agpr),
                                     "l1": int(s.bad_l1)}
                    for p, s in enumerate(table) if s.waves or s.bad_l1}
    out["wave_sites"] = [format_site(p) for p in wave_sites[:n_waves] if p != UNWRITTEN]  # unwritten: all-ones
    out["l1_wave_sites"] = [format_site(p) for p in wave_sites[n_waves:] if p != UNWRITTEN]
    lib.amdgpu_canary_cu_describe(ctypes.byref(r), table, err, 256)
    out["error"] = err.value.decode(errors="replace") if out["vgpr_errors"] or out["agpr_errors"] or \
        out["unlocated_errors"] or out["l1_errors"] else ""
    return out


def site_probe(device: int = 0, blocks: int = 0, ksteps: int = 4, inject=None, inject_waves: int = 0) -> dict:
    """Coverage map and fault location of the MFMA and vector-ALU exactness checks: 4-wave
    workgroups, one resident per CU, whose waves record the (xcc, se, sh, cu, simd) they ran
    on.  ``blocks=0``: 2 workgroups per CU plus up to 3 top-up launches while a CU or SIMD is
    missing; ``blocks>0``: one launch of that many.  ``inject`` (``mfma``, ``lowp`` or
    ``valu``) makes the first ``inject_waves`` waves compute that check on a perturbed
    operand.  Returns the totals, ``sites`` (every site a wave ran on) and ``wave_sites``
    (the site of each wave of the first launch)."""
    check = -1 if inject is None else SITE_CHECKS.index(inject)
    lib = load()
    r = SitesResult()
    table = (SiteSlot * SITE_SLOTS)()
    n_waves = 4 * (int(blocks) if blocks > 0 else 2 * 1024)  # automatic: room for 1024 CUs
    wave_sites = (ctypes.c_uint * n_waves)()
    err = ctypes.create_string_buffer(256)
    rc = lib.amdgpu_canary_sites(int(device), int(blocks), int(ksteps), check, int(inject_waves), table, wave_sites,
                                 n_waves, ctypes.byref(r), err, 256)
    if rc != 0:
        raise RuntimeError("site_probe failed: " + err.value.decode(errors="replace"))
    out = {name: int(r.errors[i]) for i, name in enumerate(SITE_CHECKS)}
    for f in ("unlocated_errors", "waves", "moved", "launches", "cus_reached", "simds_reached", "cus_expected"):
        out[f] = int(getattr(r, f))
    out["n_bad"] = int(r.n_bad)
    out["bad_sites"] = [format_site(p) for p in r.bad_sites[:min(r.n_bad, 16)]]
    out["ms"] = r.ms
    out["sites"] = {format_site(p): dict({"waves": int(s.waves)}, **{c: int(s.bad[i]) for i, c in enumerate(SITE_CHECKS)})
                    for p, s in enumerate(table) if s.waves}
    out["wave_sites"] = [format_site(p) for p in wave_sites if p != UNWRITTEN]  # unwritten entries stay all-ones
    return out


def fabric_check(device: int = 0, blocks: int = 0, slice_kb: int = 64, reps: int = 2, inject=None,
                 inject_op: str = "u32_add", inject_blocks: int = 0) -> dict:
    """What lies between a CU and HBM (``ops/fabric.hip``), in three launches of ``blocks``
    256-thread workgroups (0: one per CU).  The L2 march: each workgroup writes a slice of
    ``slice_kb`` KiB, reads it back ``reps`` times while it is resident in its XCD's L2, then
    does the same with the complement.  The exchange: every slice is verified again by a
    later launch, per (writer xcc, reader xcc).  The atomics: every global atomic form into
    tables the host predicts.  ``inject`` (``l2``, ``xcd`` or ``atomic``, the latter in
    operation ``inject_op``) makes the first ``inject_blocks`` workgroups plant a fault.

    Returns the totals (``l2_errors``, ``xcd_errors``, ``atomic_errors``, ``unlocated_errors``,
    ``moved``), ``xccs`` (``"xcc5"`` -> blocks, bytes, bad), ``pairs`` (``"xcc1>xcc6"``: written
    on xcc1, read on xcc6 -> reads, bad), ``slice_xcc`` (the xcc that wrote each slice),
    ``atomic`` (operation -> wrong elements), ``first_bad`` (``l2``: xcc, slice, offset;
    ``atomic``: op, element), ``error`` (the canary's text for the first failing check),
    ``l2_gbps`` (bytes the march read back over the march's whole device time: a lower
    bound) and ``ms``."""
    kind = -1 if inject is None else FABRIC_INJECT.index(inject)
    lib = load()
    r = FabricResult()
    xt = (XccSlot * FABRIC_XCCS)()
    pm = (PairSlot * (FABRIC_XCCS * FABRIC_XCCS))()
    n_slices = int(blocks) if blocks > 0 else 4096
    sx = (ctypes.c_uint * n_slices)()
    err = ctypes.create_string_buffer(256)
    rc = lib.amdgpu_canary_fabric(int(device), int(blocks), int(slice_kb), int(reps), kind,
                                  ATOMIC_OPS.index(inject_op), int(inject_blocks), xt, pm, sx, n_slices,
                                  ctypes.byref(r), err, 256)
    if rc != 0:
        raise RuntimeError("fabric_check failed: " + err.value.decode(errors="replace"))
    out = {f: int(getattr(r, f)) for f in ("l2_errors", "xcd_errors", "atomic_errors", "unlocated_errors", "moved",
                                           "blocks", "slice_kb", "xccs_reached", "pairs_reached", "pairs_expected")}
    out["xccs"] = {"xcc%d" % x: {"blocks": int(s.blocks), "bytes": int(s.bytes), "bad": int(s.bad)}
                   for x, s in enumerate(xt) if s.blocks}
    out["pairs"] = {"xcc%d>xcc%d" % divmod(c, FABRIC_XCCS): {"reads": int(p.reads), "bad": int(p.bad)}
                    for c, p in enumerate(pm) if p.reads}
    out["slice_xcc"] = [int(x) for x in sx[:r.blocks]]
    out["atomic"] = {op: int(r.atomic_bad[i]) for i, op in enumerate(ATOMIC_OPS)}
    out["first_bad"] = {
        "l2": None if r.first_bad_slice < 0 else {"xcc": r.first_bad_xcc, "slice": r.first_bad_slice,
                                                  "offset": int(r.first_bad_offset)},
        "atomic": None if r.first_bad_op < 0 else {"op": ATOMIC_OPS[r.first_bad_op], "element": r.first_bad_elem}}
    lib.amdgpu_canary_fabric_describe(ctypes.byref(r), xt, pm, err, 256)
    out["error"] = err.value.decode(errors="replace") if out["l2_errors"] or out["xcd_errors"] or \
        out["atomic_errors"] else ""
    out["l2_gbps"] = r.march_read_bytes / (r.march_ms * 1e-3) / 1e9 if r.march_ms > 0 else 0.0
    out["march_ms"], out["exchange_ms"], out["atomic_ms"] = r.march_ms, r.exchange_ms, r.atomic_ms
    out["ms"] = r.march_ms + r.exchange_ms + r.atomic_ms
    return out


def atomic_expected(op: str, blocks: int):
    """The table operation ``op`` (one of ``ATOMIC_OPS``) must hold after the fabric check's
    atomics ran as ``blocks`` workgroups, computed on the host (no GPU needed): a numpy array
    of 2048 elements (4096 16-bit patterns for the packed forms, low half first), the 64
    words of ``cas_inc``, or the ticket word followed by ``seen[16384]`` for ``ticket``."""
    import numpy as np

    buf = np.zeros(1 + 16384, dtype=np.uint32)
    n = load().amdgpu_canary_atomic_expected(ATOMIC_OPS.index(op), int(blocks), buf.ctypes.data, buf.nbytes)
    if n < 0:
        raise ValueError("atomic_expected(%s, %r): blocks must be in 1..4096" % (op, blocks))
    return buf.view(np.uint8)[:n].view(_ATOMIC_DTYPES.get(op, "uint32")).copy()


def detects_corruption(device: int = 0, hbm_bytes: int = 64 << 20, flips: int = 5) -> int:
    """Fault-injection check of the HBM verifier; returns the mismatches it found."""
    return int(load().amdgpu_canary_detects_corruption(int(device), int(hbm_bytes), int(flips)))


def mfma_detects_corruption(device: int = 0, inject_blocks: int = 3) -> int:
    """Fault-injection check of the MFMA exactness verifier; returns the wrong
    accumulator registers it found (0 expected with inject_blocks=0)."""
    return int(load().amdgpu_canary_mfma_detects(int(device), int(inject_blocks)))


# cbsz/blgp format codes of v_mfma_scale_f32_32x32x64_f8f6f4 (OCP formats); "fp8_unscaled" is
# v_mfma_f32_32x32x16_fp8_fp8
LOWP_FORMATS = {"fp8": 0, "bf8": 1, "fp4": 4, "fp8_unscaled": 8}


def lowp_check(device: int = 0, fmt: str = "fp8", ksteps: int = 4, vary_scale: bool = True,
               inject_blocks: int = 0) -> int:
    """Exactness of one low-precision MFMA form on small-integer operands with power-of-two
    block scales (2 single-wave blocks per CU, K = 64 * ksteps); returns the wrong
    accumulator registers (0 expected unless ``inject_blocks`` perturb an operand)."""
    rc = load().amdgpu_canary_lowp_check(int(device), LOWP_FORMATS[fmt], int(ksteps), int(bool(vary_scale)),
                                         int(inject_blocks))
    if rc < 0:
        raise RuntimeError("lowp_check(%s) failed on device %d" % (fmt, device))
    return int(rc)


def lowp_rate(device: int = 0, fmt: str = "fp8", iters: int = 2048) -> float:
    """Dense TFLOP/s of the block-scaled MFMA on ``fmt`` (fp8, bf8 or fp4)."""
    t = ctypes.c_double()
    if load().amdgpu_canary_lowp_rate(int(device), LOWP_FORMATS[fmt], int(iters), ctypes.byref(t)) != 0:
        raise RuntimeError("lowp_rate(%s) failed on device %d" % (fmt, device))
    return t.value


def lds_check(device: int = 0, inject_blocks: int = 0) -> tuple:
    """LDS march over every CU's whole LDS; returns (mismatches, bytes per workgroup)."""
    nbytes = ctypes.c_ulonglong()
    rc = load().amdgpu_canary_lds_check(int(device), int(inject_blocks), ctypes.byref(nbytes))
    if rc < 0:
        raise RuntimeError("lds_check failed on device %d" % device)
    return int(rc), int(nbytes.value)


def lowp_gemm(a_codes, bt_codes, a_scales, b_scales, fmt: str = "fp8", device: int = 0):
    """C = dequant(A) @ dequant(Bt).T through the block-scaled MFMA.  ``a_codes`` uint8 [M, K]
    and ``bt_codes`` uint8 [N, K] hold one OCP code per element (fp4 in the low nibble);
    ``a_scales`` [M, K/32], ``b_scales`` [N, K/32] are E8M0 exponents (127 = 1.0).
    M, N % 32 == 0, K % 64 == 0.  Returns float32 [M, N]."""
    import numpy as np

    a = np.ascontiguousarray(a_codes, dtype=np.uint8)
    bt = np.ascontiguousarray(bt_codes, dtype=np.uint8)
    sa = np.ascontiguousarray(a_scales, dtype=np.uint8)
    sb = np.ascontiguousarray(b_scales, dtype=np.uint8)
    (m, k), (nn, k2) = a.shape, bt.shape
    if k != k2 or sa.shape != (m, k // 32) or sb.shape != (nn, k // 32):
        raise ValueError("shapes do not match: A %s, Bt %s, scales %s / %s" % (a.shape, bt.shape, sa.shape, sb.shape))
    c = np.empty((m, nn), dtype=np.float32)
    err = ctypes.create_string_buffer(256)
    rc = load().amdgpu_canary_lowp_gemm(int(device), LOWP_FORMATS[fmt], a.ctypes.data, bt.ctypes.data,
                                        sa.ctypes.data, sb.ctypes.data, c.ctypes.data, m, nn, k, err, 256)
    if rc != 0:
        raise RuntimeError("lowp_gemm failed: " + err.value.decode(errors="replace"))
    return c


SWEEP_VARIANTS = {0: "u4 grid-stride", 1: "u8 grid-stride", 2: "u4 nontemporal", 3: "u8 nontemporal",
                  4: "u4 chunked", 5: "u8 chunked", 6: "u4 nt chunked", 7: "u16 grid-stride",
                  8: "u8 nt chunked", 9: "u2 nt chunked", 10: "u4 tile-stride (nt verify)",
                  11: "u8 tile-stride (nt verify)", 12: "u8 tile-stride"}


def hbm_sweep(device: int = 0, nbytes: int = 4 << 30, variants=tuple(SWEEP_VARIANTS), blocks_per_cu=(4, 8, 16),
              reps: int = 5) -> list:
    """Times write+verify for each access shape; returns rows of GB/s (HBM-resident buffer)."""
    rows = []
    for v in variants:
        for b in blocks_per_cu:
            w, r, e = ctypes.c_double(), ctypes.c_double(), ctypes.c_ulonglong()
            rc = load().amdgpu_canary_hbm_sweep(device, nbytes, v, b, reps, ctypes.byref(w), ctypes.byref(r),
                                                ctypes.byref(e))
            rows.append({"variant": SWEEP_VARIANTS[v], "blocks_per_cu": b, "write_gbps": round(w.value, 1),
                         "read_verify_gbps": round(r.value, 1), "errors": e.value, "rc": rc})
    return rows


def _bf16_operands(a_bits, b_bits, b_k_axis: int, error: str = None):
    """Two bf16 operands as contiguous uint16 arrays, A [M, K] and B with K on axis ``b_k_axis``:
    ``(a, b, m, n, k)``.  ``ValueError`` (with ``error`` as its text, if given) unless both are
    2-D and agree on K."""
    import numpy as np

    a, b = (np.ascontiguousarray(x, dtype=np.uint16) for x in (a_bits, b_bits))
    if error and (a.ndim != 2 or b.ndim != 2):
        raise ValueError(error)
    (m, k), (n, k2) = a.shape, b.shape[::1 if b_k_axis else -1]
    if k != k2:
        raise ValueError(error or "inner dimensions differ: %d vs %d" % (k, k2))
    return a, b, m, n, k


def mfma_gemm(a_bf16_bits, b_bf16_bits, device: int = 0):
    """C = A @ B through the canary's MFMA kernel.  ``a``/``b``: uint16 numpy arrays of
    bf16 bit patterns (row-major, M,N % 32 == 0, K % 16 == 0); returns float32 [M, N]."""
    import numpy as np

    a, b, m, nn, k = _bf16_operands(a_bf16_bits, b_bf16_bits, 0)
    c = np.empty((m, nn), dtype=np.float32)
    err = ctypes.create_string_buffer(256)
    rc = load().amdgpu_canary_mfma_gemm(int(device), a.ctypes.data, b.ctypes.data, c.ctypes.data, m, nn, k, err, 256)
    if rc != 0:
        raise RuntimeError("mfma_gemm failed: " + err.value.decode(errors="replace"))
    return c


# kernel ids of amdgpu_canary_gemm*: "auto" picks pingpong256s for >= 256 tiles of 256x256, else lds128; the
# pingpong256s_* entries are the ablations in profiles/gemm_r1/SUMMARY.md
GEMM_KERNELS = {"auto": 0, "lds128": 1, "pingpong256": 2, "pingpong256s": 3, "pingpong256s_b2": 4,
                "pingpong256s_b0": 5, "pingpong256s_b3": 6, "pingpong256s_g1early": 7, "pingpong256s_vwave": 8,
                "pingpong256s_group2": 9, "pingpong256s_group8": 10, "pingpong256s_noprio": 11}
# flags of amdgpu_canary_gemm_rate, as in canary_common.h
GEMM_INJECT, GEMM_RANDOM_DATA, GEMM_SKIP_VERIFIED_LAUNCH = 1, 2, 4


def _kernel_id(kernel) -> int:
    """A name of ``GEMM_KERNELS`` or a raw kernel id (the library refuses one it does not know)."""
    return GEMM_KERNELS[kernel] if isinstance(kernel, str) else int(kernel)


def gemm_tile_map(kernel, m: int, n: int):
    """Tile origin ``(m0, n0)`` of every workgroup of GEMM kernel ``kernel`` at an ``m`` x ``n``
    product, in workgroup order, from the kernels' own index arithmetic run on the host (no
    GPU needed): an int32 array [grid, 2].  ``ValueError`` for a shape the kernel refuses."""
    import numpy as np

    lib = load()
    grid = lib.amdgpu_canary_gemm_tile_map(_kernel_id(kernel), int(m), int(n), None, None, 0)
    if grid <= 0:
        raise ValueError("gemm_tile_map: shape (%d,%d) does not fit kernel %r" % (m, n, kernel))
    m0, n0 = np.full(grid, -1, dtype=np.int32), np.full(grid, -1, dtype=np.int32)
    lib.amdgpu_canary_gemm_tile_map(_kernel_id(kernel), int(m), int(n), m0.ctypes.data, n0.ctypes.data, grid)
    return np.stack([m0, n0], axis=1)


def gemm(a_bf16_bits, bt_bf16_bits, device: int = 0, kernel="auto"):
    """C = A @ Bt.T through the LDS-staged MFMA GEMM (the canary's matrix path).
    ``a``: uint16 [M, K] bf16 bit patterns, ``bt``: uint16 [N, K] (B transposed, K
    contiguous); K % 64 == 0 and M, N % 128 == 0 (``lds128``) or % 256 == 0
    (``pingpong256``; ``auto`` takes it when that gives >= 256 tiles).  Returns float32
    [M, N]."""
    import numpy as np

    a, bt, m, nn, k = _bf16_operands(a_bf16_bits, bt_bf16_bits, 1)
    c = np.empty((m, nn), dtype=np.float32)
    err = ctypes.create_string_buffer(256)
    rc = load().amdgpu_canary_gemm(int(device), a.ctypes.data, bt.ctypes.data, c.ctypes.data, m, nn, k,
                                   _kernel_id(kernel), err, 256)
    if rc != 0:
        raise RuntimeError("gemm failed: " + err.value.decode(errors="replace"))
    return c


def gemm_rate(device: int = 0, m: int = 4096, n: int = 4096, k: int = 4096, iters: int = 10,
              inject: bool = False, kernel="auto", random_data: bool = False,
              skip_verified_launch: bool = False) -> dict:
    """Matrix-path canary: timed LDS-staged MFMA GEMMs on exact integer data, then one more
    product written into a poisoned (all-NaN) C, and the ABFT row/column checksums of that
    one.  ``errors`` counts wrong rows + wrong columns.  ``inject`` corrupts one element of
    the verified product (2 expected); ``skip_verified_launch`` leaves the poison in place
    (``m + n`` expected).  ``random_data``: uniform bf16 operands in [-1, 1) instead (the
    rate a BLAS benchmark quotes; no checksum, ``errors`` is None)."""
    t, e = ctypes.c_double(), ctypes.c_ulonglong()
    err = ctypes.create_string_buffer(256)
    flags = ((GEMM_INJECT if inject else 0) | (GEMM_RANDOM_DATA if random_data else 0) |
             (GEMM_SKIP_VERIFIED_LAUNCH if skip_verified_launch else 0))
    rc = load().amdgpu_canary_gemm_rate(int(device), int(m), int(n), int(k), int(iters), flags, _kernel_id(kernel),
                                        ctypes.byref(t), ctypes.byref(e), err, 256)
    if rc != 0:
        raise RuntimeError("gemm_rate failed: " + err.value.decode(errors="replace"))
    return {"tflops": t.value, "errors": None if random_data else e.value, "shape": (m, n, k), "iters": iters,
            "kernel": kernel, "data": "random" if random_data else "integer"}


def abft(a_bf16_bits, bt_bf16_bits, c, device: int = 0) -> tuple:
    """The matrix path's verifier on its own: the ABFT verdict on a caller-supplied product.
    ``a``: uint16 [M, K] and ``bt``: uint16 [N, K] bf16 bit patterns of integers, ``c``:
    float32 [M, N]; any positive M, N and K <= 65536.  Returns ``(row_errors, col_errors)``:
    the rows and the columns whose checksum is off or that hold an element no healthy product
    holds (a fraction, a magnitude above 2^24, NaN, -0)."""
    import numpy as np

    c = np.ascontiguousarray(c, dtype=np.float32)
    mismatch = "shapes do not match: A %s, Bt %s, C %s" % (np.shape(a_bf16_bits), np.shape(bt_bf16_bits), c.shape)
    a, bt, m, n, k = _bf16_operands(a_bf16_bits, bt_bf16_bits, 1, mismatch)
    if c.shape != (m, n):
        raise ValueError(mismatch)
    rows, cols = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    err = ctypes.create_string_buffer(256)
    rc = load().amdgpu_canary_abft(int(device), a.ctypes.data, bt.ctypes.data, c.ctypes.data, m, n, k,
                                   ctypes.byref(rows), ctypes.byref(cols), err, 256)
    if rc != 0:
        raise RuntimeError("abft failed: " + err.value.decode(errors="replace"))
    return int(rows.value), int(cols.value)


def run_isolated(device: int, hbm_bytes: int = 256 << 20, timeout: float = 120.0, passes: int = 1,
                 host_link: bool = False, host_link_bytes: int = 64 << 20, pace: bool = False,
                 lds_path: bool = False) -> dict:
    """``run`` in a child process (its own HIP runtime, gone when it exits)."""
    cmd = [sys.executable, "-m", "k8s_gpu_device_plugin_amd.ops.canary", "--device", str(device),
           "--bytes", str(hbm_bytes), "--passes", str(passes)]
    asked = {"lds_path": lds_path, "pace": pace, "host_link": host_link, "host_link_bytes": host_link_bytes}
    for check in reversed(OPTIONAL_CHECKS):
        if asked[check.keyword]:
            cmd += ["--with-" + check.stem]
            for arg, _, _ in check.args:
                cmd += ["--" + arg.replace("_", "-"), str(asked[arg])]
    env = dict(os.environ)
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        return {"ok": False, "device": device, "error": "canary timed out after %.0fs" % timeout}
    for line in reversed(p.stdout.strip().splitlines()):
        try:
            res = json.loads(line)
        except ValueError:
            continue
        if isinstance(res, dict):  # the result line, not stray output that happens to parse
            if p.returncode != 0 and res.get("ok"):
                res = dict(res, ok=False, error="canary reported ok but exited %d: %s"
                           % (p.returncode, p.stderr[-300:]))
            return res
    return {"ok": False, "device": device, "error": "canary exited %d: %s" % (p.returncode, p.stderr[-500:])}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="MI355X partition health canary")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--mfma-iters", type=int, default=8192)
    ap.add_argument("--gemm", type=int, default=0, help="only the matrix-path GEMM, at this M=N=K")
    ap.add_argument("--gemm-iters", type=int, default=20)
    ap.add_argument("--gemm-kernel", choices=sorted(GEMM_KERNELS), default="auto")
    ap.add_argument("--gemm-random", action="store_true", help="random bf16 operands (rate only, no checksum)")
    ap.add_argument("--sites", action="store_true", help="only the site probe: the CU/SIMD coverage map")
    ap.add_argument("--fabric", action="store_true",
                    help="only the fabric check: L2 march, cross-XCD exchange, global atomics")
    ap.add_argument("--cu", action="store_true",
                    help="only the CU memory check: register-file march and L1 march, per site")
    for check in reversed(OPTIONAL_CHECKS):
        ap.add_argument("--" + check.stem, action="store_true", help="only %s: %s" % (check.title, check.detail))
        ap.add_argument("--with-" + check.stem, action="store_true", help="the full run, with %s merged in" % check.title)
        for arg, default, _ in check.args:
            ap.add_argument("--" + arg.replace("_", "-"), type=type(default), default=default)
    a = ap.parse_args(argv)
    for check in OPTIONAL_CHECKS:
        if getattr(a, check.keyword):
            res = _function(check)(a.device, *(getattr(a, arg) for arg, _, _ in check.args))
            print(json.dumps(res))
            return 0 if res["ok"] else 1
    if a.cu:
        res = cu_check(a.device)
        print(json.dumps(res))
        return 0 if not (res["vgpr_errors"] or res["agpr_errors"] or res["unlocated_errors"] or
                         res["l1_errors"]) else 1
    if a.fabric:
        res = fabric_check(a.device)
        print(json.dumps(res))
        return 0 if not (res["l2_errors"] or res["xcd_errors"] or res["atomic_errors"]) else 1
    if a.sites:
        res = site_probe(a.device)
        print(json.dumps(res))
        return 0 if not (res["mfma"] or res["lowp"] or res["valu"] or res["unlocated_errors"]) else 1
    if a.gemm:
        res = gemm_rate(a.device, a.gemm, a.gemm, a.gemm, a.gemm_iters, kernel=a.gemm_kernel,
                        random_data=a.gemm_random)
        print(json.dumps(res))
        return 0 if not res["errors"] else 1
    more = {}
    for check in OPTIONAL_CHECKS:
        on = getattr(a, "with_" + check.keyword)
        if on or check.args:  # a check with arguments is always spelt out; the others are named only when asked for
            more[check.keyword] = on
            more.update({arg: getattr(a, arg) for arg, _, _ in check.args})
    res = run(a.device, a.bytes, a.passes, a.mfma_iters, **more)
    print(json.dumps(res))
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
