"""The vector-ALU library's C ABI (``ops/valu/valu.h``, ``ops/valu/valu_host.h``): the sizes of the
structs ``ops/valu.py`` mirrors, the exact set of exported entry points, the build wiring beside
``HIP_LIBS``, and the kernels' build contract from the compiler's own output: no scratch, no
spills, no static LDS, and every op's instruction (the table's own column) present in its group's
kernel, so a compiler that folds an op away fails here.  No GPU."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from k8s_gpu_device_plugin_amd import _build
from k8s_gpu_device_plugin_amd.ops import valu


@pytest.mark.parametrize("which, name, size", [(0, "Record", 272), (1, "ValuResult", 3080)])
def test_ctypes_mirror_has_the_size_the_library_reports(which, name, size):
    assert ctypes.sizeof(getattr(valu, name)) == size == valu.load().amdgpu_valu_sizeof(which)
    assert valu.load().amdgpu_valu_sizeof(9) == -1 and valu.load().amdgpu_valu_sizeof(-1) == -1
    constants = (valu.WAVES, valu.MAX_OPS, valu.GROUP_OPS, valu.MAX_GROUPS, valu.MAX_ROUNDS, valu.MAX_RESULTS, valu.INJECT_LANE)
    assert constants == tuple(valu.load().amdgpu_valu_sizeof(k) for k in range(2, 9))
    dt = np.dtype(valu.RECORD_DTYPE)
    assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(valu.Record, n).offset) for n, _ in valu.Record._fields_]


def test_library_exports_exactly_the_entry_points():
    valu.load()  # builds the library if it is missing
    nm = next(p for p in (os.path.join(_build.ROCM, "lib", "llvm", "bin", "llvm-nm"), shutil.which("llvm-nm"), shutil.which("nm"))
              if p and os.path.exists(p))
    p = subprocess.run([nm, "-D", "--defined-only", _build.VALU_LIB], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    rows = [line.split() for line in p.stdout.splitlines()]
    text = sorted(r[2] for r in rows if len(r) == 3 and r[1] == "T" and not r[2].startswith("_Z"))
    assert text == sorted("amdgpu_valu_" + n for n in valu.EXPORTS)


def test_the_library_stands_beside_the_table_of_the_canary_s_libraries(monkeypatch):
    assert [row["name"] for row in _build.HIP_LIBS] == ["canary", "hostlink", "pace", "ldspath"]
    listed = _build.VALU_SOURCES + _build.VALU_HEADERS
    on_disk = glob.glob(os.path.join(_build.VALU_DIR, "*.hip")) + glob.glob(os.path.join(_build.VALU_DIR, "*.h"))
    assert sorted(on_disk) == sorted(p for p in listed if os.path.dirname(p) == _build.VALU_DIR)
    assert set(_build.CANARY_HEADERS) <= set(_build.VALU_HEADERS) and valu.LIB_PATH == _build.VALU_LIB
    built = []
    monkeypatch.setattr(_build, "_build_hip_lib", lambda **kw: built.append(kw["name"]) or kw["lib"])
    monkeypatch.setattr(_build, "build_native", lambda **kw: None)
    monkeypatch.setattr(_build, "build_bench", lambda **kw: None)
    _build.build_all()
    assert "valu" not in built and len(built) == 4
    assert _build.main(["--valu"]) == 0 and built[4:] == ["valu"]
    assert _build.build_valu(verbose=False) == _build.VALU_LIB


def test_the_two_host_headers_need_no_hip(tmp_path):
    for name in ("valu_ops.h", "valu_host.h"):
        text = open(os.path.join(_build.VALU_DIR, name)).read()
        assert "hip/" not in text and "canary_" not in text, name
    assert '#include "../site.h"' in open(os.path.join(_build.VALU_DIR, "valu_host.h")).read()
    assert '#include "../canary_host.h"' in open(os.path.join(_build.VALU_DIR, "valu.h")).read()
    src = tmp_path / "host.cpp"
    src.write_text('#include "%s"\nint main() { return valu::kNumOps == 0; }\n' % os.path.join(_build.VALU_DIR, "valu_host.h"))
    p = subprocess.run([_build._cxx(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """One device-only compile of valu.hip: the kernel-resource-usage remarks and the assembly per kernel."""
    out = tmp_path_factory.mktemp("valu_asm") / "valu.s"
    p = subprocess.run([_build.hipcc_path(), "--offload-arch=" + _build.OFFLOAD_ARCH, "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", _build.VALU_SOURCES[0], "-o", str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    usage, name = {}, None
    for line in p.stdout.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:\[]*?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and name:
            usage[name][m.group(1)] = m.group(2)
    kernels, name = {}, None
    for line in open(out).read().splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
        elif line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            name = None
        if name and line.startswith("\t") and not line.startswith("\t."):
            kernels.setdefault(name, []).append(line.split(";")[0].strip())
    return usage, kernels


def test_kernels_build_without_scratch_spills_or_static_lds(compiled):
    usage, _ = compiled
    assert sum("valu_sweep" in n for n in usage) == len(valu.GROUPS) and sum("valu_raw" in n for n in usage) == 1
    assert len(usage) == len(valu.GROUPS) + 1
    for name, u in usage.items():
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0" and u["LDS Size"] == "0", (name, u)


def test_every_op_s_instruction_is_in_its_group_s_kernel(compiled):
    _, kernels = compiled
    raw = next(text for name, text in kernels.items() if "valu_raw" in name)
    missing = []
    for op, mnemonic, group in zip(valu.OPS, valu.MNEMONICS, valu.OP_GROUPS):
        sweep = next(text for name, text in kernels.items() if "valu_sweepILi%dE" % valu.GROUPS.index(group) in name)
        pattern = re.compile(re.escape(mnemonic) + r"(_e32|_e64|_sdwa|_dpp)?\b")
        missing += [(op, where) for where, text in (("sweep", sweep), ("raw", raw)) if not any(pattern.match(line) for line in text)]
    assert not missing, missing
