"""The canary library's C ABI as a whole: the sizes of the structs that ``canary.py`` mirrors
with ctypes (``ops/canary_common.h`` pins the same numbers with ``static_assert``), the exact set
of exported entry points, and the build's list of sources and headers."""
import ctypes
import glob
import os
import shutil
import subprocess

import pytest

from k8s_gpu_device_plugin_amd import _build
from k8s_gpu_device_plugin_amd.ops import canary

EXPORTS = """
amdgpu_canary_abft amdgpu_canary_gemm_tile_map
amdgpu_canary_atomic_expected amdgpu_canary_atomic_op_name amdgpu_canary_cu amdgpu_canary_cu_describe
amdgpu_canary_cu_regs amdgpu_canary_cu_sizeof amdgpu_canary_datapaths amdgpu_canary_detects_corruption
amdgpu_canary_device_count amdgpu_canary_fabric amdgpu_canary_fabric_describe amdgpu_canary_format_site
amdgpu_canary_gemm amdgpu_canary_gemm_rate amdgpu_canary_hbm_sweep amdgpu_canary_lds_check
amdgpu_canary_lowp_check amdgpu_canary_lowp_gemm amdgpu_canary_lowp_rate amdgpu_canary_lowp_raw
amdgpu_canary_mfma_detects amdgpu_canary_mfma_gemm amdgpu_canary_run amdgpu_canary_sites
""".split()


@pytest.mark.parametrize("name, size", [("CanaryResult", 608), ("SiteSlot", 16), ("SitesResult", 144),
                                        ("XccSlot", 24), ("PairSlot", 16), ("FabricResult", 224), ("CuSlot", 16),
                                        ("CuResult", 176)])
def test_ctypes_mirror_has_the_size_the_header_pins(name, size):
    assert ctypes.sizeof(getattr(canary, name)) == size


def _nm():
    llvm = os.path.join(_build.ROCM, "lib", "llvm", "bin", "llvm-nm")
    for path in (llvm, shutil.which("llvm-nm"), shutil.which("nm")):
        if path and os.path.exists(path):
            return path
    raise AssertionError("no nm: neither ROCm's llvm-nm nor a system nm")


def test_library_exports_exactly_the_entry_points():
    canary.load()  # builds the library if it is missing
    p = subprocess.run([_nm(), "-D", "--defined-only", _build.CANARY_LIB], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    rows = [line.split() for line in p.stdout.splitlines()]
    text = sorted(r[2] for r in rows if len(r) == 3 and r[1] == "T" and not r[2].startswith("_Z"))
    assert text == sorted(EXPORTS)
    lib = ctypes.CDLL(_build.CANARY_LIB)
    assert all(hasattr(lib, name) for name in EXPORTS)


def test_build_lists_cover_every_source_and_header():
    listed = _build.CANARY_SOURCES + _build.CANARY_HEADERS
    assert len(set(listed)) == len(listed)
    for path in listed:
        assert os.path.isfile(path), path
    assert all(p.endswith(".hip") for p in _build.CANARY_SOURCES)
    assert all(p.endswith(".h") for p in _build.CANARY_HEADERS)
    ops = os.path.dirname(_build.CANARY_LIB)
    on_disk = glob.glob(os.path.join(ops, "*.hip")) + glob.glob(os.path.join(ops, "*.h"))
    assert sorted(os.path.realpath(p) for p in on_disk) == sorted(os.path.realpath(p) for p in listed)
