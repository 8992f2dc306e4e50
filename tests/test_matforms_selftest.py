"""The matrix-forms check's host side (``ops/matforms/matforms_forms.h``,
``ops/matforms/matforms_host.h``) without a GPU: every form emulated from its operand map, and
the reduction on hand-built records, by a stand-alone program under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

from k8s_gpu_device_plugin_amd import _build


def test_sanitized_selftest_program(tmp_path):
    """Host code as a program of its own: nothing sanitized is loaded into Python."""
    cxx = shutil.which(_build._cxx())
    assert cxx, "no C++ compiler"
    src = os.path.join(_build.HARNESS_DIR, "matforms_selftest.cpp")
    exe = str(tmp_path / "matforms_selftest")
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + _build.OPS_DIR,
                        src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
           "PATH": "/usr/bin:/bin"}  # as tests/test_canary_forms.py runs its program
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", p.stdout[-3000:]
