"""The pace library's C ABI (``ops/pace/pace.h``, ``ops/pace/pace_host.h``): the sizes of the
structs ``ops/pace.py`` mirrors with ctypes, the exact set of exported entry points, the
build's list of sources and headers, arguments refused as text before any HIP call, and the
kernels' build contract (no scratch, no spills) from the compiler's resource-usage remarks.
``tests/test_canary_abi.py`` pins the canary library's own ABI, which this library must leave
alone."""
import ctypes
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

from k8s_gpu_device_plugin_amd import _build
from k8s_gpu_device_plugin_amd.ops import pace
from kernel_usage import kernel_resource_usage

EXPORTS = """
amdgpu_pace_run amdgpu_pace_reduce amdgpu_pace_describe amdgpu_pace_note amdgpu_pace_sizeof amdgpu_pace_default_iters
""".split()


@pytest.mark.parametrize("which, name, size", [(0, "Record", 32), (1, "SiteSlot", 24), (2, "XccSlot", 48),
                                               (3, "PaceResult", 400)])
def test_ctypes_mirror_has_the_size_the_library_reports(which, name, size):
    assert ctypes.sizeof(getattr(pace, name)) == size == pace.load().amdgpu_pace_sizeof(which)


def test_numpy_record_is_the_ctypes_record():
    dt = np.dtype(pace.RECORD_DTYPE)
    assert dt.itemsize == ctypes.sizeof(pace.Record)
    assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(pace.Record, n).offset) for n, _ in pace.Record._fields_]


def test_sizeof_refuses_an_unknown_struct():
    assert pace.load().amdgpu_pace_sizeof(4) == -1 and pace.load().amdgpu_pace_sizeof(-1) == -1


def _nm():
    llvm = os.path.join(_build.ROCM, "lib", "llvm", "bin", "llvm-nm")
    for path in (llvm, shutil.which("llvm-nm"), shutil.which("nm")):
        if path and os.path.exists(path):
            return path
    raise AssertionError("no nm: neither ROCm's llvm-nm nor a system nm")


def test_library_exports_exactly_the_entry_points():
    pace.load()  # builds the library if it is missing
    p = subprocess.run([_nm(), "-D", "--defined-only", _build.PACE_LIB], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    rows = [line.split() for line in p.stdout.splitlines()]
    text = sorted(r[2] for r in rows if len(r) == 3 and r[1] == "T" and not r[2].startswith("_Z"))
    assert text == sorted(EXPORTS)
    lib = ctypes.CDLL(_build.PACE_LIB)
    assert all(hasattr(lib, name) for name in EXPORTS)


def test_build_lists_cover_every_source_and_header_of_the_directory():
    listed = _build.PACE_SOURCES + _build.PACE_HEADERS
    assert len(set(listed)) == len(listed) and all(os.path.isfile(p) for p in listed)
    on_disk = glob.glob(os.path.join(_build.PACE_DIR, "*.hip")) + glob.glob(os.path.join(_build.PACE_DIR, "*.h"))
    own = [p for p in listed if os.path.dirname(p) == _build.PACE_DIR]
    assert sorted(os.path.realpath(p) for p in on_disk) == sorted(os.path.realpath(p) for p in own)
    # the canary's header-only helpers are dependencies, and stay sources of the canary library alone
    assert set(_build.CANARY_HEADERS) <= set(_build.PACE_HEADERS)
    assert not set(_build.PACE_SOURCES) & (set(_build.CANARY_SOURCES) | set(_build.HOSTLINK_SOURCES))
    assert len({os.path.dirname(p) for p in (_build.PACE_LIB, _build.CANARY_LIB, _build.HOSTLINK_LIB)}) == 3


def test_the_host_header_needs_no_hip():
    text = open(os.path.join(_build.PACE_DIR, "pace_host.h")).read()
    assert "hip/" not in text and "canary_" not in text


def test_default_iters_keeps_every_accumulator_exact():
    # |A . B| <= 16 * 4 * 4 per MFMA: iters * 256 must stay below 2^24
    assert 1 <= pace.default_iters() * 256 < 1 << 24


def test_bad_arguments_are_an_error_text_before_any_gpu_call():
    """Refused arguments never reach HIP, so this needs no GPU."""
    for kw in ({"iters": 65536}, {"iters": -1}, {"blocks": 4097}, {"blocks": -1}, {"slice_kb": 0}, {"slice_kb": 6},
               {"slice_kb": 16388}, {"blocks": 4096, "slice_kb": 2048}, {"slow_ratio": 0.5}, {"slow_ratio": float("nan")},
               {"inject": "slow_xcc", "inject_xcc": 16}, {"inject": "slow_xcc", "inject_factor": 17},
               {"inject": "slow_xcc", "inject_factor": 0}, {"inject": "slow_xcc", "iters": 16384, "inject_factor": 4},
               {"inject": "slow_waves", "iters": 32768, "inject_factor": 2, "inject_waves": 1},
               {"inject": "result", "inject_waves": -1}):
        with pytest.raises(RuntimeError, match="pace check: bad arguments"):
            pace.pace_check(**kw)
    with pytest.raises(ValueError):
        pace.pace_check(inject="fast")


def test_kernels_build_without_scratch_or_spills(tmp_path, monkeypatch):
    monkeypatch.setattr(_build, "CANARY_SOURCES", list(_build.PACE_SOURCES))  # the one source the helper compiles
    usage = kernel_resource_usage("pace.hip", tmp_path)
    kernels = {"pace_mfma": 1, "pace_fill": 1, "pace_mem": 1}
    for stem, count in kernels.items():
        assert sum(stem in name for name in usage) == count, sorted(usage)
    assert len(usage) == sum(kernels.values())
    for name, u in usage.items():
        assert u["ScratchSize"] == "0", (name, u)
        assert u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (name, u)
