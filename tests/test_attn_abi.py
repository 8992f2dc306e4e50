"""The attention-path library's C ABI (``ops/attn/attn.h``, ``ops/attn/attn_host.h``): the size of the
struct ``ops/attn.py`` mirrors, the exact set of exported entry points, the build wiring beside
``HIP_LIBS``, the host header's independence of HIP, the kernel's build contract from the compiler's
own output, and the host-only data functions.  No GPU."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from k8s_gpu_device_plugin_amd import _build
from k8s_gpu_device_plugin_amd.ops import attn


def test_ctypes_mirror_has_the_size_the_library_reports():
    assert ctypes.sizeof(attn.AttnResult) == 168 == attn.load().amdgpu_attn_sizeof(0)
    assert attn.load().amdgpu_attn_sizeof(1) == -1


def test_library_exports_exactly_the_entry_points():
    attn.load()  # builds the library if it is missing
    nm = next(p for p in (os.path.join(_build.ROCM, "lib", "llvm", "bin", "llvm-nm"), shutil.which("llvm-nm"), shutil.which("nm"))
              if p and os.path.exists(p))
    p = subprocess.run([nm, "-D", "--defined-only", _build.ATTN_LIB], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    rows = [line.split() for line in p.stdout.splitlines()]
    text = sorted(r[2] for r in rows if len(r) == 3 and r[1] == "T" and not r[2].startswith("_Z"))
    assert text == sorted("amdgpu_attn_" + n for n in attn.EXPORTS)


def test_the_library_stands_beside_the_table_of_the_canary_s_libraries(monkeypatch):
    assert [row["name"] for row in _build.HIP_LIBS] == ["canary", "hostlink", "pace", "ldspath"]
    listed = _build.ATTN_SOURCES + _build.ATTN_HEADERS
    on_disk = glob.glob(os.path.join(_build.ATTN_DIR, "*.hip")) + glob.glob(os.path.join(_build.ATTN_DIR, "*.h"))
    assert sorted(on_disk) == sorted(p for p in listed if os.path.dirname(p) == _build.ATTN_DIR)
    assert set(_build.CANARY_HEADERS) <= set(_build.ATTN_HEADERS) and attn.LIB_PATH == _build.ATTN_LIB
    built = []
    monkeypatch.setattr(_build, "_build_hip_lib", lambda **kw: built.append(kw["name"]) or kw["lib"])
    monkeypatch.setattr(_build, "build_native", lambda **kw: None)
    monkeypatch.setattr(_build, "build_bench", lambda **kw: None)
    _build.build_all()
    assert "attn" not in built and len(built) == 4
    assert _build.main(["--attn"]) == 0 and built[4:] == ["attn"]
    assert _build.main(["--attn", "--mxgemm", "--matforms"]) == 0 and built[5:] == ["matforms", "mxgemm", "attn"]
    assert _build.build_attn(verbose=False) == _build.ATTN_LIB


def test_the_host_header_needs_no_hip(tmp_path):
    assert "hip/" not in open(os.path.join(_build.ATTN_DIR, "attn_host.h")).read()
    assert '#include "../canary_host.h"' in open(os.path.join(_build.ATTN_DIR, "attn.h")).read()
    src = tmp_path / "host.cpp"
    src.write_text('#include "%s"\nint main() { return attn::match_key(5, 1) != 128 + 26 || !attn::shape_ok(1, 128, 64, 0); }\n'
                   % os.path.join(_build.ATTN_DIR, "attn_host.h"))
    p = subprocess.run([_build._cxx(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]


def test_kernel_builds_to_its_contract(tmp_path):
    """One device-only compile.  attn_fwd: no scratch, no spills, the double-buffered K and V images as
    its static LDS, two workgroups of four waves per CU, and in its body the bf16 MFMA, the 16 B LDS
    DMA and the exponential."""
    out = tmp_path / "attn.s"
    p = subprocess.run([_build.hipcc_path(), "--offload-arch=" + _build.OFFLOAD_ARCH, "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", _build.ATTN_SOURCES[0], "-o", str(out)],
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
    (name,) = [n for n in usage if "attn_fwd" in n]
    u = usage[name]
    print(name, {k: u[k] for k in ("VGPRs", "AGPRs", "LDS Size", "Occupancy")})
    assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", u
    assert int(u["LDS Size"]) == 65536 and int(u["Occupancy"]) * 4 // 4 == 2, u
    asm = open(out).read()
    body = asm[asm.index("\n" + name + ":"):asm.index(".end_amdhsa_kernel", asm.index("\n" + name + ":"))]
    for mnemonic in ("v_mfma_f32_32x32x16_bf16", "global_load_lds_dwordx4", "v_exp_f32"):
        assert re.search(r"^\s+" + mnemonic + r"(_e32|_e64)?\b", body, re.M), mnemonic  # the assembler's encoding suffix


def bf16(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


@pytest.mark.parametrize("name", attn.SETS[:2])
@pytest.mark.parametrize("sq, sk, causal", [(128, 64, False), (256, 192, False), (128, 320, True), (256, 256, True)])
def test_expected_is_the_mean_of_v_over_the_top_keys(name, sq, sk, causal):
    """The T_i rule in numpy: the visible keys of highest score, the integer sum of V over them in
    float32, one float32 division by their number; lse is the log of that number plus the score."""
    q, k, v = (bf16(x) for x in attn.operands(name, 2, sq, sk))
    o, lse = attn.expected(name, 2, sq, sk, causal)
    assert np.abs(v).max() == 4 and np.array_equal(v, np.round(v)) and (name == "routed" or not q.any())
    s = np.einsum("hid,hjd->hij", q, k)
    hidden = np.arange(sk)[None, :] > np.arange(sq)[:, None] + (sk - sq) if causal else np.zeros((sq, sk), bool)
    s = np.where(hidden, -np.inf, s)
    top = s == s.max(axis=2, keepdims=True)
    assert set(np.unique(s[np.isfinite(s)])) <= {0.0, 4096.0}
    assert name != "routed" or (top.sum(axis=2).min() == 1 and 1 < top.sum(axis=2).max() <= sk)  # matches, and rows without one
    want = np.einsum("hij,hjd->hid", top, v).astype(np.float32) / top.sum(axis=2)[:, :, None].astype(np.float32)
    assert want.dtype == np.float32 and np.array_equal(o.view(np.uint32), want.view(np.uint32))
    assert np.allclose(lse, np.log(top.sum(axis=2)) + s.max(axis=2) / np.sqrt(128.0), rtol=0, atol=1e-12)


def test_bad_shapes_are_refused_with_a_text_before_any_launch():
    z = lambda *shape: np.zeros(shape, np.uint16)  # noqa: E731
    with pytest.raises(RuntimeError, match=r"attention path: shape \(3,100,256\) does not fit"):
        attn.attention(z(3, 100, 128), z(3, 256, 128), z(3, 256, 128))
    with pytest.raises(RuntimeError, match=r"attention path: shape \(1,256,128\) does not fit .*Sk >= Sq when causal"):
        attn.attention(z(1, 256, 128), z(1, 128, 128), z(1, 128, 128), causal=True)
    with pytest.raises(RuntimeError, match=r"attention path: shape \(1,128,96\) does not fit"):
        attn.attention_check(0, 1, 128, 96)
    with pytest.raises(ValueError):
        attn.expected("hashed", 1, 128, 128)
