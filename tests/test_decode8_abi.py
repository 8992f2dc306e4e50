"""The fp8 decode-attention library's C ABI (``ops/decode8/decode8.h``, ``ops/decode8/decode8_host.h``): the
size of the struct ``ops/decode8.py`` mirrors, the exact set of exported entry points, the build wiring
beside ``HIP_LIBS``, the host header's independence of HIP, the kernels' build contract from the
compiler's own output, the host-only data functions and the refusals.  No GPU."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from k8s_gpu_device_plugin_amd import _build
from k8s_gpu_device_plugin_amd.ops import decode8


def test_ctypes_mirror_has_the_size_the_library_reports():
    assert ctypes.sizeof(decode8.Decode8Result) == 168 == decode8.load().amdgpu_decode8_sizeof(0)
    assert decode8.load().amdgpu_decode8_sizeof(1) == -1


def test_library_exports_exactly_the_entry_points():
    decode8.load()  # builds the library if it is missing
    nm = next(p for p in (os.path.join(_build.ROCM, "lib", "llvm", "bin", "llvm-nm"), shutil.which("llvm-nm"), shutil.which("nm"))
              if p and os.path.exists(p))
    p = subprocess.run([nm, "-D", "--defined-only", _build.DECODE8_LIB], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    rows = [line.split() for line in p.stdout.splitlines()]
    text = sorted(r[2] for r in rows if len(r) == 3 and r[1] == "T" and not r[2].startswith("_Z"))
    assert text == sorted("amdgpu_decode8_" + n for n in decode8.EXPORTS)


def test_the_library_stands_beside_the_table_of_the_canary_s_libraries(monkeypatch):
    assert [row["name"] for row in _build.HIP_LIBS] == ["canary", "hostlink", "pace", "ldspath"]
    listed = _build.DECODE8_SOURCES + _build.DECODE8_HEADERS
    on_disk = glob.glob(os.path.join(_build.DECODE8_DIR, "*.hip")) + glob.glob(os.path.join(_build.DECODE8_DIR, "*.h"))
    assert sorted(on_disk) == sorted(p for p in listed if os.path.dirname(p) == _build.DECODE8_DIR)
    assert set(_build.CANARY_HEADERS) <= set(_build.DECODE8_HEADERS) and decode8.LIB_PATH == _build.DECODE8_LIB
    shared = os.path.join(_build.DECODE_DIR, "decode_host.h")  # the staleness rule sees the header it reuses
    assert any(os.path.samefile(h, shared) for h in _build.DECODE8_HEADERS)
    built = []
    monkeypatch.setattr(_build, "_build_hip_lib", lambda **kw: built.append(kw["name"]) or kw["lib"])
    monkeypatch.setattr(_build, "build_native", lambda **kw: None)
    monkeypatch.setattr(_build, "build_bench", lambda **kw: None)
    _build.build_all()
    assert "decode8" not in built and len(built) == 4
    assert _build.main(["--decode8"]) == 0 and built[4:] == ["decode8"]
    assert _build.main(["--decode8", "--decode"]) == 0 and built[5:] == ["decode", "decode8"]
    assert _build.build_decode8(verbose=False) == _build.DECODE8_LIB


def test_the_host_header_needs_no_hip(tmp_path):
    host = open(os.path.join(_build.DECODE8_DIR, "decode8_host.h")).read()
    assert "hip/" not in host and '#include "../decode/decode_host.h"' in host
    assert '#include "../canary_host.h"' in open(os.path.join(_build.DECODE8_DIR, "decode8.h")).read()
    src = tmp_path / "host.cpp"
    src.write_text('#include "%s"\nint main() { return decode8::fp8_value(0x7E) != 448.f || decode8::quarter_code(-3) != 0xB4 || '
                   'decode8::scale_ok(0.f) || decode8::kPageBytes != 2048; }\n' % os.path.join(_build.DECODE8_DIR, "decode8_host.h"))
    p = subprocess.run([_build._cxx(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]


def test_kernels_build_to_their_contract():
    """One device-only compile.  Both kernels: no scratch, no spills.  kv8_split: KV8_STAGES x 32 KiB of
    static LDS (two stages as built); kv8_combine: none."""
    p = subprocess.run([_build.hipcc_path(), "--offload-arch=" + _build.OFFLOAD_ARCH, "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", _build.DECODE8_SOURCES[0], "-o", os.devnull],
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
    for kernel, lds in (("kv8_split", 2 * 32768), ("kv8_combine", 0)):
        (name,) = [n for n in usage if kernel in n]
        u = usage[name]
        print(name, {k: u[k] for k in ("VGPRs", "AGPRs", "LDS Size", "Occupancy")})
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", u
        assert int(u["LDS Size"]) == lds, u


# the 256 e4m3 values: bias 7, subnormals below 2^-6, 0x7F / 0xFF NaN
E4M3 = np.array([(-1.0) ** (c >> 7) * (np.nan if c & 0x7F == 0x7F else
                                       (c & 7) / 8 * 2.0 ** -6 if (c >> 3) & 15 == 0 else (1 + (c & 7) / 8) * 2.0 ** (((c >> 3) & 15) - 7))
                 for c in range(256)])


@pytest.mark.parametrize("name", decode8.SETS[:2])
@pytest.mark.parametrize("batch, hq, hkv, seq", [(1, 1, 1, 1), (3, 4, 2, 77), (2, 16, 1, 300), (5, 8, 8, 129)])
def test_expected_is_the_scaled_mean_of_v_over_the_top_keys(name, batch, hq, hkv, seq):
    """The T rule in numpy over the pages gathered through the table and decoded with the table above:
    the visible keys of highest score, the integer sum of V over them in float32, one float32 division
    by their number, one float32 multiply by v_scale; lse is the log of that number plus the scaled score."""
    q, kc, vc, ks, vs, table, lens = decode8.operands(name, batch, hq, hkv, seq)
    o, lse = decode8.expected(name, batch, hq, hkv, seq)
    used, g = table[table >= 0], hq // hkv
    assert lens[0] == seq and (batch < 2 or lens[1] % 2) and ((lens >= max(1, seq // 2)) & (lens <= seq)).all()
    assert len(set(used)) == len(used) == sum(-(-n // 16) for n in lens) and (len(used) < 3 or (np.diff(used) != 1).any())
    assert set(ks) <= {1.0, 0.5} and set(vs) <= {0.25, 1.0, 2.0} and (hkv < 2 or (ks[0] != ks[1] and vs[0] != vs[1]))
    assert not ((kc == 0x80) | (vc == 0x80)).any()  # zero is always code 0x00
    for b in range(batch):
        gather = lambda c: E4M3[c[table[b, :-(-lens[b] // 16)]]].transpose(1, 0, 2, 3).reshape(hkv, -1, 128)[:, :lens[b]]  # noqa: E731
        k, v = gather(kc) * ks[:, None, None], gather(vc)
        assert np.abs(v).max() <= 4 and np.array_equal(v, np.round(v)) and not np.isnan(k).any()  # no NaN code among the visible keys
        s = np.einsum("hd,hjd->hj", (q[b].astype(np.uint32) << 16).view(np.float32).astype(np.float64), k.repeat(g, 0))
        top = s == s.max(axis=1, keepdims=True)
        assert set(np.unique(s)) <= {0.0, 2048.0, 4096.0}
        want = np.einsum("hj,hjd->hd", top, v.repeat(g, 0)).astype(np.float32) / top.sum(axis=1)[:, None].astype(np.float32) \
            * vs.repeat(g)[:, None]
        assert want.dtype == np.float32 and np.array_equal(o[b].view(np.uint32), want.view(np.uint32))
        assert np.allclose(lse[b], np.log(top.sum(axis=1)) + s.max(axis=1) / np.sqrt(128.0), rtol=0, atol=1e-12)


@pytest.mark.parametrize("lens, entry, hq, splits, k_scale, text", [
    ([0], 0, 2, 0, 1.0, r"decode8 path: seq_lens\[0\] = 0 does not fit \("),
    ([33], 0, 2, 0, 1.0, r"decode8 path: seq_lens\[0\] = 33 does not fit \(.*2 pages"),
    ([32], 4, 2, 0, 1.0, r"decode8 path: block_table\[0\]\[1\] = 4 does not fit \(pages 0 \.\. 3\)"),
    ([32], 0, 3, 0, 1.0, r"decode8 path: shape \(1,3/1,4 pages,2 per sequence\) does not fit \("),
    ([32], 0, 2, 65, 1.0, r"decode8 path: splits 65 does not fit \(0 \.\. 64\)"),
    ([32], 0, 2, 0, float("nan"), r"decode8 path: k_scale\[0\] = nan does not fit \(finite, > 0\)"),
    ([32], 0, 2, 0, 0.0, r"decode8 path: k_scale\[0\] = 0 does not fit \(finite, > 0\)"),
])
def test_bad_calls_are_refused_with_a_text_before_any_launch(lens, entry, hq, splits, k_scale, text):
    z = lambda *shape: np.zeros(shape, np.uint8)  # noqa: E731
    with pytest.raises(RuntimeError, match=text):
        decode8.decode_attention(np.zeros((1, hq, 128), np.uint16), z(4, 1, 16, 128), z(4, 1, 16, 128), [k_scale], [1.0],
                                 [[0, entry]], lens, splits=splits)
