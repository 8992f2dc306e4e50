"""The site vocabulary every located check shares: ``ops/site.h`` under a sanitizer as
a program of its own, and ``ops/_sites.py`` against it.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import pytest

from k8s_gpu_device_plugin_amd import _build
from k8s_gpu_device_plugin_amd.ops import _sites, canary, ldspath, pace

# every field alone at its maximum, all together, and one mixed site
FIELDS = [dict(xcc=15), dict(se=7), dict(sh=1), dict(cu=15), dict(simd=3), dict(xcc=15, se=7, sh=1, cu=15, simd=3),
          dict(xcc=3, se=1, sh=0, cu=7, simd=2)]


def _pack(fields):
    return _sites.pack_site(**{"xcc": 0, **fields})


def test_sanitized_selftest_program(tmp_path):
    """Host code under AddressSanitizer and UBSan as a program of its own: nothing sanitized
    is loaded into Python."""
    cxx = shutil.which(_build._cxx())
    assert cxx, "no C++ compiler"
    src = os.path.join(_build.HARNESS_DIR, "site_selftest.cpp")
    exe = str(tmp_path / "site_selftest")
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + _build.OPS_DIR,
                        src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
           "PATH": "/usr/bin:/bin"}  # as tests/test_native_selftest.py runs its program
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", p.stdout[-3000:]


def test_the_site_header_needs_no_hip_and_no_other_header_of_the_project():
    """pace_host.h and ldspath_host.h include it and must keep compiling without HIP."""
    text = open(os.path.join(_build.OPS_DIR, "site.h")).read()
    assert "hip/" not in text and '#include "' not in text
    assert os.path.join(_build.OPS_DIR, "site.h") in _build.CANARY_HEADERS


def _c_format_site(packed: int) -> str:
    buf = ctypes.create_string_buffer(64)
    lib = canary.load()
    lib.amdgpu_canary_format_site.argtypes = [ctypes.c_uint, ctypes.c_char_p, ctypes.c_int]
    lib.amdgpu_canary_format_site.restype = ctypes.c_int
    n = lib.amdgpu_canary_format_site(packed, buf, 64)
    assert n == len(buf.value)
    return buf.value.decode()


@pytest.mark.parametrize("packed", [0, _sites.SITE_SLOTS - 1] + [_pack(f) for f in FIELDS])
def test_c_and_python_format_a_site_alike(packed):
    text = _sites.format_site(packed)
    assert _c_format_site(packed) == text
    assert _sites.format_site(packed, simd=False) == text.rsplit("/", 1)[0] and text.rsplit("/", 1)[1].startswith("simd")


@pytest.mark.parametrize("fields", FIELDS)
def test_pack_and_decode_round_trip(fields):
    whole = dict(dict(xcc=0, se=0, sh=0, cu=0, simd=0), **fields)
    packed = _pack(fields)
    assert 0 <= packed < _sites.SITE_SLOTS
    assert _sites.decode_site(packed) == whole
    assert _sites.pack_site(**_sites.decode_site(packed)) == packed


def test_pack_decode_round_trip_over_the_whole_table():
    assert all(_sites.pack_site(**_sites.decode_site(p)) == p for p in range(_sites.SITE_SLOTS))
    assert _sites.pack_site(16, 8, 2, 16, 4) == 0  # a field past its width is cut, never spills into its neighbour


def test_the_faces_share_one_vocabulary():
    for mod in (canary, pace, ldspath):
        assert mod.format_site is _sites.format_site and mod.SITE_SLOTS == _sites.SITE_SLOTS == 1 << 14
    assert pace.pack_site is ldspath.pack_site is _sites.pack_site and canary.decode_site is _sites.decode_site
    assert pace.UNWRITTEN == ldspath.UNWRITTEN == _sites.UNWRITTEN == 0xFFFFFFFF
    assert _sites.xcc_names(0) == [] and _sites.xcc_names(0b100001) == ["xcc0", "xcc5"]
    assert _sites.xcc_names(1 << 15) == ["xcc15"]


def test_load_library_loads_once_and_declares_once(tmp_path, monkeypatch):
    seen = []
    path = canary.LIB_PATH
    canary.load()  # builds it if it is missing
    monkeypatch.setattr(_sites, "_libs", {})
    a = _sites.load_library(path, "build_canary", seen.append)
    b = _sites.load_library(path, "build_canary", seen.append)
    assert a is b and seen == [a]
    # a missing file is built by the named recipe before it is opened
    built = []
    monkeypatch.setattr(_build, "build_nothing", lambda verbose=True: built.append(verbose), raising=False)
    with pytest.raises(OSError):
        _sites.load_library(str(tmp_path / "libmissing.so"), "build_nothing", seen.append)
    assert built == [False] and len(seen) == 1


def test_as_records():
    import numpy as np

    empty = _sites.as_records(None, pace.RECORD_DTYPE, pace.records)
    assert empty.size == 0 and empty.dtype == np.dtype(pace.RECORD_DTYPE)
    rows = [(5, 5, 64, 2, 2, 0), (9, 8, 1, 1, 1, 3)]
    from_rows = _sites.as_records(rows, pace.RECORD_DTYPE, pace.records)
    assert from_rows.tolist() == rows and from_rows.flags["C_CONTIGUOUS"]
    taken = _sites.as_records(from_rows[::-1], pace.RECORD_DTYPE, pace.records)  # a structured array is not re-read as rows
    assert taken.tolist() == rows[::-1] and taken.flags["C_CONTIGUOUS"]
