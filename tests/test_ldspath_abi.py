"""The LDS-path library's C ABI (``ops/ldspath/ldspath.h``, ``ops/ldspath/ldspath_host.h``): the
sizes of the structs ``ops/ldspath.py`` mirrors with ctypes, the exact set of exported entry
points, the build's list of sources and headers, arguments refused as text before any HIP
call, and the kernels' build contract from the compiler's own output: no scratch, no spills,
dynamic LDS only, and every instruction the check exists to exercise present in the kernels'
assembly (a compiler that narrows an access or folds a lane op away fails here instead of
silently changing what is tested).  ``tests/test_canary_abi.py`` pins the canary library's own
ABI, which this library must leave alone."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from k8s_gpu_device_plugin_amd import _build
from k8s_gpu_device_plugin_amd.ops import ldspath
from kernel_usage import kernel_resource_usage

EXPORTS = """
amdgpu_ldspath_run amdgpu_ldspath_reduce amdgpu_ldspath_lane_sources amdgpu_ldspath_lane_map amdgpu_ldspath_tr_map
amdgpu_ldspath_atomic_expected amdgpu_ldspath_describe amdgpu_ldspath_sizeof amdgpu_ldspath_ops
""".split()
KERNELS = {"dma_fill": 1, "lds_widths": 1, "lds_atomic": 1, "lane_xchg": 1, "lds_tr": 1}


@pytest.mark.parametrize("which, name, size", [(0, "Record", 208), (1, "LdsPathResult", 1904)])
def test_ctypes_mirror_has_the_size_the_library_reports(which, name, size):
    assert ctypes.sizeof(getattr(ldspath, name)) == size == ldspath.load().amdgpu_ldspath_sizeof(which)


def test_numpy_record_is_the_ctypes_record():
    dt = np.dtype(ldspath.RECORD_DTYPE)
    assert dt.itemsize == ctypes.sizeof(ldspath.Record)
    assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(ldspath.Record, n).offset) for n, _ in ldspath.Record._fields_]


def test_sizeof_and_ops_refuse_what_they_do_not_know():
    lib = ldspath.load()
    assert lib.amdgpu_ldspath_sizeof(2) == -1 and lib.amdgpu_ldspath_sizeof(-1) == -1
    assert lib.amdgpu_ldspath_ops(4, -1, None, 0) == -1 and lib.amdgpu_ldspath_ops(0, len(ldspath.LANE_OPS), None, 0) == -1
    assert lib.amdgpu_ldspath_ops(0, -1, None, 0) == len(ldspath.LANE_OPS) <= ldspath.SUBS
    assert lib.amdgpu_ldspath_ops(1, -1, None, 0) == len(ldspath.ATOMIC_FORMS) == 10


def _nm():
    llvm = os.path.join(_build.ROCM, "lib", "llvm", "bin", "llvm-nm")
    for path in (llvm, shutil.which("llvm-nm"), shutil.which("nm")):
        if path and os.path.exists(path):
            return path
    raise AssertionError("no nm: neither ROCm's llvm-nm nor a system nm")


def test_library_exports_exactly_the_entry_points():
    ldspath.load()  # builds the library if it is missing
    p = subprocess.run([_nm(), "-D", "--defined-only", _build.LDSPATH_LIB], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    rows = [line.split() for line in p.stdout.splitlines()]
    text = sorted(r[2] for r in rows if len(r) == 3 and r[1] == "T" and not r[2].startswith("_Z"))
    assert text == sorted(EXPORTS)
    lib = ctypes.CDLL(_build.LDSPATH_LIB)
    assert all(hasattr(lib, name) for name in EXPORTS)


def test_build_lists_cover_every_source_and_header_of_the_directory():
    listed = _build.LDSPATH_SOURCES + _build.LDSPATH_HEADERS
    assert len(set(listed)) == len(listed) and all(os.path.isfile(p) for p in listed)
    on_disk = glob.glob(os.path.join(_build.LDSPATH_DIR, "*.hip")) + glob.glob(os.path.join(_build.LDSPATH_DIR, "*.h"))
    own = [p for p in listed if os.path.dirname(p) == _build.LDSPATH_DIR]
    assert sorted(os.path.realpath(p) for p in on_disk) == sorted(os.path.realpath(p) for p in own)
    # the canary's header-only helpers are dependencies, and stay sources of the canary library alone
    assert set(_build.CANARY_HEADERS) <= set(_build.LDSPATH_HEADERS)
    others = set(_build.CANARY_SOURCES) | set(_build.HOSTLINK_SOURCES) | set(_build.PACE_SOURCES)
    assert not set(_build.LDSPATH_SOURCES) & others
    assert len({os.path.dirname(p) for p in (_build.LDSPATH_LIB, _build.PACE_LIB, _build.CANARY_LIB, _build.HOSTLINK_LIB)}) == 4


def test_the_host_header_needs_no_hip():
    text = open(os.path.join(_build.LDSPATH_DIR, "ldspath_host.h")).read()
    assert "hip/" not in text and "canary_" not in text


def test_bad_arguments_are_an_error_text_before_any_gpu_call():
    """Refused arguments never reach HIP, so this needs no GPU."""
    for kw in ({"blocks": -1}, {"blocks": 4097}, {"reps": 0}, {"reps": 65}, {"steps": 0}, {"steps": 65}, {"rounds": 0},
               {"rounds": 65}, {"inject": "lds", "inject_waves": -1}, {"inject_op": -1},
               {"inject": "atomic", "inject_op": 10, "inject_waves": 1},
               {"inject": "lane", "inject_op": len(ldspath.LANE_OPS), "inject_waves": 1}):
        with pytest.raises(RuntimeError, match="ldspath check: bad arguments"):
            ldspath.ldspath_check(**kw)
    with pytest.raises(ValueError):
        ldspath.ldspath_check(inject="everything")
    err = ctypes.create_string_buffer(256)
    out = (ctypes.c_uint * 8)()
    assert ldspath.load().amdgpu_ldspath_lane_sources(0, out, 8, err, 256) == -1
    assert err.value.decode().startswith("ldspath check: bad arguments")


def test_kernels_build_without_scratch_or_spills_and_with_dynamic_lds_only(tmp_path, monkeypatch):
    monkeypatch.setattr(_build, "CANARY_SOURCES", list(_build.LDSPATH_SOURCES))  # the one source the helper compiles
    usage = kernel_resource_usage("ldspath.hip", tmp_path)
    for stem, count in KERNELS.items():
        assert sum(stem in name for name in usage) == count, sorted(usage)
    assert len(usage) == sum(KERNELS.values())
    for name, u in usage.items():
        assert u["ScratchSize"] == "0", (name, u)
        assert u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (name, u)
        assert u["LDS Size"] == "0", (name, u)  # no static __shared__: the allocation is the launch's


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    """The device assembly of ldspath.hip, per kernel."""
    out = tmp_path_factory.mktemp("ldspath_asm") / "ldspath.s"
    p = subprocess.run([_build.hipcc_path(), "--offload-arch=" + _build.OFFLOAD_ARCH, "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", _build.LDSPATH_SOURCES[0], "-o", str(out)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    kernels, name = {}, None
    for line in open(out).read().splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = next((k for k in KERNELS if k in m.group(1)), None)
        elif line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            name = None
        if name and line.startswith("\t") and not line.startswith("\t."):
            kernels.setdefault(name, []).append(line.split(";")[0].strip())
    assert set(kernels) == set(KERNELS)
    return {k: "\n".join(v) for k, v in kernels.items()}


MUST_HAVE = {
    "lds_widths": [r"ds_read_b128\b", r"ds_write_b128\b", r"ds_read_b64\b", r"ds_write_b64\b", r"ds_read_b32\b",
                   r"ds_write_b32\b", r"ds_read_u16\b", r"ds_read_u8\b", r"ds_write_b16\b", r"ds_write_b8\b",
                   r"global_load_lds_dword\b", r"global_load_lds_dwordx4\b"],
    "lds_atomic": [r"ds_add_u32\b", r"ds_add_u64\b", r"ds_add_f32\b", r"ds_add_rtn_u32\b", r"ds_cmpst_rtn_b32\b",
                   r"ds_min_i32\b", r"ds_max_u32\b", r"ds_and_b32\b", r"ds_or_b32\b", r"ds_xor_b32\b"],
    "lane_xchg": [r"ds_bpermute_b32\b", r"ds_permute_b32\b", r"ds_swizzle_b32\b", r"v_permlane16_swap_b32",
                  r"v_permlane32_swap_b32", r"quad_perm:", r"row_shl:", r"row_shr:", r"row_ror:", r"row_mirror\b",
                  r"row_half_mirror\b", r"wave_shl:1", r"wave_rol:1", r"wave_shr:1", r"wave_ror:1", r"row_bcast:15",
                  r"row_bcast:31", r"row_mask:0x[0-9a-e]\b", r"bank_mask:0x[0-9a-e]\b", r"bound_ctrl:", r"v_readlane_b32\b",
                  r"v_writelane_b32\b", r"v_readfirstlane_b32\b"],
    "lds_tr": [r"ds_read_b64_tr_b16\b"],
}


@pytest.mark.parametrize("kernel", sorted(MUST_HAVE))
def test_the_kernels_contain_the_instructions_they_exist_to_exercise(assembly, kernel):
    text = assembly[kernel]
    missing = [pat for pat in MUST_HAVE[kernel] if not re.search(pat, text)]
    assert not missing, (kernel, missing)


def test_every_lane_op_of_the_table_is_in_the_assembly(assembly):
    """One instruction per table entry at the least: none was folded into another or away."""
    text = assembly["lane_xchg"]
    names = ldspath.LANE_OPS
    assert len(re.findall(r"ds_swizzle_b32\b", text)) >= sum(n.startswith("ds_swizzle") for n in names)
    assert len(re.findall(r"ds_permute_b32\b", text)) >= sum(n.startswith("ds_permute") for n in names)
    assert len(re.findall(r"_dpp\b", text)) >= sum(n.startswith("dpp ") for n in names)
    assert len(re.findall(r"v_writelane_b32\b", text)) >= sum(n.startswith("v_writelane") for n in names)
    assert len(re.findall(r"quad_perm:", text)) >= 3
