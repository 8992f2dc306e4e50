"""The block-scaled matrix-path library's C ABI (``ops/mxgemm/mxgemm.h``, ``ops/mxgemm/mxgemm_host.h``):
the size of the struct ``ops/mxgemm.py`` mirrors, the exact set of exported entry points, the build
wiring beside ``HIP_LIBS``, the host header's independence of HIP, the kernels' build contract from
the compiler's own output, and the host-only data functions.  No GPU."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from k8s_gpu_device_plugin_amd import _build
from k8s_gpu_device_plugin_amd.ops import mxgemm
from matforms_model import DECODE


def test_ctypes_mirror_has_the_size_the_library_reports():
    assert ctypes.sizeof(mxgemm.MxGemmResult) == 56 == mxgemm.load().amdgpu_mxgemm_sizeof(0)
    assert mxgemm.load().amdgpu_mxgemm_sizeof(1) == -1
    assert mxgemm.KERNELS == {1: {"tile": 128, "threads": 256, "lds_bytes": 65536},
                              2: {"tile": 256, "threads": 512, "lds_bytes": 131072}}


def test_library_exports_exactly_the_entry_points():
    mxgemm.load()  # builds the library if it is missing
    nm = next(p for p in (os.path.join(_build.ROCM, "lib", "llvm", "bin", "llvm-nm"), shutil.which("llvm-nm"), shutil.which("nm"))
              if p and os.path.exists(p))
    p = subprocess.run([nm, "-D", "--defined-only", _build.MXGEMM_LIB], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    rows = [line.split() for line in p.stdout.splitlines()]
    text = sorted(r[2] for r in rows if len(r) == 3 and r[1] == "T" and not r[2].startswith("_Z"))
    assert text == sorted("amdgpu_mxgemm_" + n for n in mxgemm.EXPORTS)


def test_the_library_stands_beside_the_table_of_the_canary_s_libraries(monkeypatch):
    assert [row["name"] for row in _build.HIP_LIBS] == ["canary", "hostlink", "pace", "ldspath"]
    listed = _build.MXGEMM_SOURCES + _build.MXGEMM_HEADERS
    on_disk = glob.glob(os.path.join(_build.MXGEMM_DIR, "*.hip")) + glob.glob(os.path.join(_build.MXGEMM_DIR, "*.h"))
    assert sorted(on_disk) == sorted(p for p in listed if os.path.dirname(p) == _build.MXGEMM_DIR)
    assert set(_build.CANARY_HEADERS) <= set(_build.MXGEMM_HEADERS) and mxgemm.LIB_PATH == _build.MXGEMM_LIB
    built = []
    monkeypatch.setattr(_build, "_build_hip_lib", lambda **kw: built.append(kw["name"]) or kw["lib"])
    monkeypatch.setattr(_build, "build_native", lambda **kw: None)
    monkeypatch.setattr(_build, "build_bench", lambda **kw: None)
    _build.build_all()
    assert "mxgemm" not in built and len(built) == 4
    assert _build.main(["--mxgemm"]) == 0 and built[4:] == ["mxgemm"]
    assert _build.main(["--valu"]) == 0 and _build.main(["--matforms"]) == 0 and built[5:] == ["valu", "matforms"]
    assert _build.main(["--matforms", "--mxgemm"]) == 0 and built[7:] == ["matforms", "mxgemm"]
    assert _build.build_mxgemm(verbose=False) == _build.MXGEMM_LIB


def test_the_host_header_needs_no_hip(tmp_path):
    assert "hip/" not in open(os.path.join(_build.MXGEMM_DIR, "mxgemm_host.h")).read()
    assert '#include "../canary_host.h"' in open(os.path.join(_build.MXGEMM_DIR, "mxgemm.h")).read()
    src = tmp_path / "host.cpp"
    src.write_text('#include "%s"\nint main() { return mxgemm::tile_k(mxgemm::kFp4) != 256; }\n'
                   % os.path.join(_build.MXGEMM_DIR, "mxgemm_host.h"))
    p = subprocess.run([_build._cxx(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]


def test_kernels_build_to_their_contract(tmp_path):
    """One device-only compile.  Every mx_gemm instance: no scratch, no spills, the whole double
    buffer as its static LDS, and, from the compiler's waves per SIMD over the block's waves, two
    workgroups per CU (id 1) or one (id 2); its assembly holds the scaled MFMA, the 16 B LDS DMA
    and the 16 B LDS read."""
    out = tmp_path / "mxgemm.s"
    p = subprocess.run([_build.hipcc_path(), "--offload-arch=" + _build.OFFLOAD_ARCH, "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", _build.MXGEMM_SOURCES[0], "-o", str(out)],
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
    asm = open(out).read()
    instances = {(fmt, tile): next(n for n in usage if "mx_gemmILi%dELi%dE" % (fmt, tile) in n)
                 for fmt in mxgemm.FORMATS.values() for tile in (128, 256)}
    assert len(instances) == sum("mx_gemm" in n for n in usage) == 6
    for (fmt, tile), name in instances.items():
        u = usage[name]
        print(name, {k: u[k] for k in ("VGPRs", "AGPRs", "LDS Size", "Occupancy")})
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (name, u)
        assert int(u["LDS Size"]) == 4 * tile * 128 and int(u["Occupancy"]) * 4 // (tile // 32) == 256 // tile, (name, u)
        body = asm[asm.index("\n" + name + ":"):asm.index(".end_amdhsa_kernel", asm.index("\n" + name + ":"))]
        for mnemonic in ("v_mfma_scale_f32_32x32x64_f8f6f4", "global_load_lds_dwordx4", "ds_read_b128"):
            assert re.search(r"^\s+" + mnemonic + r"\b", body, re.M), (name, mnemonic)


@pytest.mark.parametrize("fmt, enc", [("fp8", "e4m3"), ("bf8", "e5m2"), ("fp4", "e2m1")])
def test_pack_and_operands_against_numpy(fmt, enc):
    d = mxgemm.operands(6, 4, 128, fmt)
    for x, s, rows in (("a", "a_scales", 6), ("bt", "b_scales", 4)):
        codes, values = d[x + "_codes"], d[x + "_values"]
        assert codes.shape == values.shape == (rows, 128) and d[s].shape == (rows, 4) and set(d[s].ravel()) == {127, 128}
        assert np.array_equal(DECODE[enc](codes), values) and values.min() == -4 and values.max() == 4
        packed = mxgemm.pack(codes, fmt)
        assert np.array_equal(packed, codes[:, 0::2] | codes[:, 1::2] << 4 if fmt == "fp4" else codes)
    assert not np.array_equal(d["a_values"][:4], d["bt_values"]) and set(mxgemm.operands(4, 4, 64, fmt, False)["a_scales"].ravel()) == {127}
    assert mxgemm.tile_k(fmt) == (256 if fmt == "fp4" else 128) and mxgemm.pick(128, 128, 256, fmt) == 1
    assert mxgemm.pick(4096, 4096, 4096, fmt, 2) == 2 and mxgemm.pick(128, 128, 128, fmt) == (0 if fmt == "fp4" else 1)
    assert mxgemm.pick(128, 100, 256, fmt) == 0 and mxgemm.pick(128, 128, 131072, fmt) == 0 and mxgemm.pick(128, 128, 256, fmt, 2) == 0
    with pytest.raises(RuntimeError, match=r"mx matrix path: shape \(128,100,256\) does not fit"):
        mxgemm.mx_gemm(np.zeros((128, 256), np.uint8), np.zeros((100, 256), np.uint8), np.zeros((128, 8), np.uint8),
                       np.zeros((100, 8), np.uint8), fmt)
