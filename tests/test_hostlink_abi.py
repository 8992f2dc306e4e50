"""The host-link library's C ABI (``ops/hostlink/hostlink.h``): the sizes of the structs
``ops/hostlink.py`` mirrors with ctypes, the exact set of exported entry points, the build's
list of sources and headers, and the kernels' build contract (no scratch, no spills) from the
compiler's resource-usage remarks.  ``tests/test_canary_abi.py`` pins the canary library's own
ABI, which this library must leave alone."""
import ctypes
import glob
import os
import shutil
import subprocess

import pytest

from k8s_gpu_device_plugin_amd import _build
from k8s_gpu_device_plugin_amd.ops import hostlink
from kernel_usage import kernel_resource_usage

EXPORTS = """
amdgpu_hostlink_run amdgpu_hostlink_describe amdgpu_hostlink_sizeof amdgpu_hostlink_tile_words
amdgpu_hostlink_pattern amdgpu_hostlink_verify amdgpu_hostlink_atomic_expected amdgpu_hostlink_atomic_compare
amdgpu_hostlink_atomic_op_name
""".split()


@pytest.mark.parametrize("which, name, size", [(0, "XccSlot", 40), (1, "HostLinkResult", 224)])
def test_ctypes_mirror_has_the_size_the_library_reports(which, name, size):
    assert ctypes.sizeof(getattr(hostlink, name)) == size == hostlink.load().amdgpu_hostlink_sizeof(which)


def test_sizeof_refuses_an_unknown_struct():
    assert hostlink.load().amdgpu_hostlink_sizeof(2) == -1


def _nm():
    llvm = os.path.join(_build.ROCM, "lib", "llvm", "bin", "llvm-nm")
    for path in (llvm, shutil.which("llvm-nm"), shutil.which("nm")):
        if path and os.path.exists(path):
            return path
    raise AssertionError("no nm: neither ROCm's llvm-nm nor a system nm")


def test_library_exports_exactly_the_entry_points():
    hostlink.load()  # builds the library if it is missing
    p = subprocess.run([_nm(), "-D", "--defined-only", _build.HOSTLINK_LIB], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    rows = [line.split() for line in p.stdout.splitlines()]
    text = sorted(r[2] for r in rows if len(r) == 3 and r[1] == "T" and not r[2].startswith("_Z"))
    assert text == sorted(EXPORTS)
    lib = ctypes.CDLL(_build.HOSTLINK_LIB)
    assert all(hasattr(lib, name) for name in EXPORTS)


def test_build_lists_cover_every_source_and_header_of_the_directory():
    listed = _build.HOSTLINK_SOURCES + _build.HOSTLINK_HEADERS
    assert len(set(listed)) == len(listed) and all(os.path.isfile(p) for p in listed)
    on_disk = glob.glob(os.path.join(_build.HOSTLINK_DIR, "*.hip")) + glob.glob(os.path.join(_build.HOSTLINK_DIR, "*.h"))
    own = [p for p in listed if os.path.dirname(p) == _build.HOSTLINK_DIR]
    assert sorted(os.path.realpath(p) for p in on_disk) == sorted(os.path.realpath(p) for p in own)
    # the canary's header-only helpers are dependencies, and stay sources of the canary library alone
    assert set(_build.CANARY_HEADERS) <= set(_build.HOSTLINK_HEADERS)
    assert not set(_build.HOSTLINK_SOURCES) & set(_build.CANARY_SOURCES)
    assert os.path.dirname(_build.HOSTLINK_LIB) != os.path.dirname(_build.CANARY_LIB)


def test_atomic_names_follow_the_python_list():
    lib = hostlink.load()
    names = [lib.amdgpu_hostlink_atomic_op_name(i).decode() for i in range(len(hostlink.ATOMIC_OPS))]
    assert names == [n.replace("_", " ") for n in hostlink.ATOMIC_OPS]
    assert lib.amdgpu_hostlink_atomic_op_name(len(hostlink.ATOMIC_OPS)) == b"?"
    assert [hostlink.tile_words(u) for u in (2, 4, 8)] == [512, 1024, 2048]
    assert hostlink.tile_words() in (512, 1024, 2048)  # the default is whichever one the measurements picked
    with pytest.raises(ValueError):
        hostlink.tile_words(3)


def test_bad_arguments_are_an_error_text_before_any_gpu_call():
    """Refused arguments never reach HIP, so this needs no GPU."""
    for kw in ({"nbytes": 0}, {"nbytes": 24}, {"reps": 0}, {"blocks": 4097}, {"unroll": 3}, {"atomic_blocks": 65},
               {"nbytes": 32, "inject": "read", "inject_n": 3}, {"host_adds": -1}):
        with pytest.raises(RuntimeError, match="host link check: bad arguments"):
            hostlink.host_link_check(**kw)


def test_kernels_build_without_scratch_or_spills(tmp_path, monkeypatch):
    monkeypatch.setattr(_build, "CANARY_SOURCES", list(_build.HOSTLINK_SOURCES))  # the one source the helper compiles
    usage = kernel_resource_usage("hostlink.hip", tmp_path)
    kernels = {"host_read": 3, "tile_fill": 3, "dev_verify": 1, "host_atomic": 1}  # one per UNROLL of the bulk kernels
    for stem, count in kernels.items():
        assert sum(stem in name for name in usage) == count, sorted(usage)
    assert len(usage) == sum(kernels.values())
    for name, u in usage.items():
        assert u["ScratchSize"] == "0", (name, u)
        assert u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (name, u)
