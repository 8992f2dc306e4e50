"""The decode-attention library's C ABI (``ops/decode/decode.h``, ``ops/decode/decode_host.h``): the size
of the struct ``ops/decode.py`` mirrors, the exact set of exported entry points, the build wiring beside
``HIP_LIBS``, the host header's independence of HIP, the kernels' build contract from the compiler's
own output, the host-only data functions and the refusals.  No GPU."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from k8s_gpu_device_plugin_amd import _build
from k8s_gpu_device_plugin_amd.ops import decode


def test_ctypes_mirror_has_the_size_the_library_reports():
    assert ctypes.sizeof(decode.DecodeResult) == 168 == decode.load().amdgpu_decode_sizeof(0)
    assert decode.load().amdgpu_decode_sizeof(1) == -1


def test_library_exports_exactly_the_entry_points():
    decode.load()  # builds the library if it is missing
    nm = next(p for p in (os.path.join(_build.ROCM, "lib", "llvm", "bin", "llvm-nm"), shutil.which("llvm-nm"), shutil.which("nm"))
              if p and os.path.exists(p))
    p = subprocess.run([nm, "-D", "--defined-only", _build.DECODE_LIB], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    rows = [line.split() for line in p.stdout.splitlines()]
    text = sorted(r[2] for r in rows if len(r) == 3 and r[1] == "T" and not r[2].startswith("_Z"))
    assert text == sorted("amdgpu_decode_" + n for n in decode.EXPORTS)


def test_the_library_stands_beside_the_table_of_the_canary_s_libraries(monkeypatch):
    assert [row["name"] for row in _build.HIP_LIBS] == ["canary", "hostlink", "pace", "ldspath"]
    listed = _build.DECODE_SOURCES + _build.DECODE_HEADERS
    on_disk = glob.glob(os.path.join(_build.DECODE_DIR, "*.hip")) + glob.glob(os.path.join(_build.DECODE_DIR, "*.h"))
    assert sorted(on_disk) == sorted(p for p in listed if os.path.dirname(p) == _build.DECODE_DIR)
    assert set(_build.CANARY_HEADERS) <= set(_build.DECODE_HEADERS) and decode.LIB_PATH == _build.DECODE_LIB
    built = []
    monkeypatch.setattr(_build, "_build_hip_lib", lambda **kw: built.append(kw["name"]) or kw["lib"])
    monkeypatch.setattr(_build, "build_native", lambda **kw: None)
    monkeypatch.setattr(_build, "build_bench", lambda **kw: None)
    _build.build_all()
    assert "decode" not in built and len(built) == 4
    assert _build.main(["--decode"]) == 0 and built[4:] == ["decode"]
    assert _build.main(["--decode", "--attn", "--matforms"]) == 0 and built[5:] == ["matforms", "attn", "decode"]
    assert _build.build_decode(verbose=False) == _build.DECODE_LIB


def test_the_host_header_needs_no_hip(tmp_path):
    host = open(os.path.join(_build.DECODE_DIR, "decode_host.h")).read()
    assert "hip/" not in host and "attn_host.h" not in host
    assert '#include "../canary_host.h"' in open(os.path.join(_build.DECODE_DIR, "decode.h")).read()
    src = tmp_path / "host.cpp"
    src.write_text('#include "%s"\nint main() { return decode::match_key(5, 1) != 128 + 26 || !decode::shape_ok(1, 8, 2, 1, 1) || '
                   'decode::tiles_per_split(300, 2) != 2; }\n' % os.path.join(_build.DECODE_DIR, "decode_host.h"))
    p = subprocess.run([_build._cxx(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]


def test_kernels_build_to_their_contract():
    """One device-only compile.  Both kernels: no scratch, no spills.  decode_split: the four waves'
    double-buffered slices as its static LDS, one workgroup per CU."""
    p = subprocess.run([_build.hipcc_path(), "--offload-arch=" + _build.OFFLOAD_ARCH, "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", _build.DECODE_SOURCES[0], "-o", os.devnull],
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
    for kernel, lds in (("decode_split", 131072), ("decode_combine", 0)):
        (name,) = [n for n in usage if kernel in n]
        u = usage[name]
        print(name, {k: u[k] for k in ("VGPRs", "AGPRs", "LDS Size", "Occupancy")})
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", u
        assert int(u["LDS Size"]) == lds, u


def bf16(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


@pytest.mark.parametrize("name", decode.SETS[:2])
@pytest.mark.parametrize("batch, hq, hkv, seq", [(1, 1, 1, 1), (3, 4, 2, 77), (2, 16, 1, 300), (5, 8, 8, 129)])
def test_expected_is_the_mean_of_v_over_the_top_keys(name, batch, hq, hkv, seq):
    """The T rule in numpy over the pages gathered through the table: the visible keys of highest
    score, the integer sum of V over them in float32, one float32 division by their number; lse is
    the log of that number plus the scaled score."""
    q, kc, vc, table, lens = decode.operands(name, batch, hq, hkv, seq)
    o, lse = decode.expected(name, batch, hq, hkv, seq)
    used = table[table >= 0]
    assert lens[0] == seq and (batch < 2 or lens[1] % 2) and ((lens >= max(1, seq // 2)) & (lens <= seq)).all()
    assert len(set(used)) == len(used) == sum(-(-n // 16) for n in lens) and (len(used) < 3 or (np.diff(used) != 1).any())
    for b in range(batch):
        k = bf16(kc[table[b, :-(-lens[b] // 16)]]).transpose(1, 0, 2, 3).reshape(hkv, -1, 128)[:, :lens[b]].repeat(hq // hkv, 0)
        v = bf16(vc[table[b, :-(-lens[b] // 16)]]).transpose(1, 0, 2, 3).reshape(hkv, -1, 128)[:, :lens[b]].repeat(hq // hkv, 0)
        assert np.abs(v).max() <= 4 and np.array_equal(v, np.round(v))  # no NaN of the unwritten rest among the visible keys
        s = np.einsum("hd,hjd->hj", bf16(q[b]), k)
        top = s == s.max(axis=1, keepdims=True)
        assert set(np.unique(s)) <= {0.0, 4096.0}
        want = np.einsum("hj,hjd->hd", top, v).astype(np.float32) / top.sum(axis=1)[:, None].astype(np.float32)
        assert want.dtype == np.float32 and np.array_equal(o[b].view(np.uint32), want.view(np.uint32))
        assert np.allclose(lse[b], np.log(top.sum(axis=1)) + s.max(axis=1) / np.sqrt(128.0), rtol=0, atol=1e-12)


@pytest.mark.parametrize("lens, entry, hq, splits, text", [
    ([0], 0, 2, 0, r"decode path: seq_lens\[0\] = 0 does not fit \("),
    ([33], 0, 2, 0, r"decode path: seq_lens\[0\] = 33 does not fit \(.*2 pages"),
    ([32], 4, 2, 0, r"decode path: block_table\[0\]\[1\] = 4 does not fit \(pages 0 \.\. 3\)"),
    ([32], 0, 3, 0, r"decode path: shape \(1,3/1,4 pages,2 per sequence\) does not fit \("),
    ([32], 0, 2, 65, r"decode path: splits 65 does not fit \(0 \.\. 64\)"),
])
def test_bad_calls_are_refused_with_a_text_before_any_launch(lens, entry, hq, splits, text):
    z = lambda *shape: np.zeros(shape, np.uint16)  # noqa: E731
    with pytest.raises(RuntimeError, match=text):
        decode.decode_attention(z(1, hq, 128), z(4, 1, 16, 128), z(4, 1, 16, 128), [[0, entry]], lens, splits=splits)
