"""The MFMA forms (``ops/mfma_forms.h``) without a GPU: the operand maps and the reference
emulated by a stand-alone program under AddressSanitizer and UBSan, and the build contract of
the three sources whose kernels are made of the forms (``canary.hip``, ``datapath.hip``,
``sites.hip``), read from the compiler's resource-usage remarks."""
import os
import shutil
import subprocess

import pytest

from kernel_usage import kernel_resource_usage
from k8s_gpu_device_plugin_amd import _build


def test_sanitized_selftest_program(tmp_path):
    """Every form emulated from its operand map must give what the kernels compare with.  Host
    code as a program of its own: nothing sanitized is loaded into Python."""
    cxx = shutil.which(_build._cxx())
    assert cxx, "no C++ compiler"
    src = os.path.join(_build.HARNESS_DIR, "forms_selftest.cpp")
    exe = str(tmp_path / "forms_selftest")
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + _build.OPS_DIR,
                        src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
           "PATH": "/usr/bin:/bin"}  # as tests/test_canary_site.py runs its program
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", p.stdout[-3000:]


def test_the_forms_header_needs_no_hip_and_rebuilds_every_library():
    text = open(os.path.join(_build.OPS_DIR, "mfma_forms.h")).read()
    assert "hip/" not in text and '#include "' not in text
    assert os.path.join(_build.OPS_DIR, "mfma_forms.h") in _build.CANARY_HEADERS
    assert all(os.path.join(_build.OPS_DIR, "mfma_forms.h") in row["headers"] for row in _build.HIP_LIBS)


# (VGPRs, AGPRs, occupancy in waves per SIMD) of every kernel of the three sources, by a fragment
# of its mangled name: the numbers of the commit before the forms were written once, taken from a
# build of that commit with kernel_resource_usage's own command.  The rate kernels were
# mfma_rate and lowp_rate<FMT> there and are instances of rate_chain<F> now.
PINNED = {
    "canary.hip": {
        "10mfma_exactE": (32, 16, 8),
        "10rate_chainINS_8FormBf16E": (33, 32, 7),             # was mfma_rate
    },
    "datapath.hip": {
        "9fp8_exactE": (45, 16, 8),
        "9lds_marchE": (24, 0, 8),
        "10rate_chainINS_10FormScaledILi0E": (68, 32, 4),      # was lowp_rate<0>
        "10rate_chainINS_10FormScaledILi1E": (68, 32, 4),      # was lowp_rate<1>
        "10rate_chainINS_10FormScaledILi4E": (70, 32, 4),      # was lowp_rate<4>
        "10lowp_exactILi0E": (150, 16, 3),
        "10lowp_exactILi1E": (150, 16, 3),
        "10lowp_exactILi4E": (148, 16, 3),
        "9lowp_gemmILi0E": (32, 16, 8),
        "9lowp_gemmILi1E": (32, 16, 8),
        "9lowp_gemmILi4E": (38, 16, 8),
        "8lowp_rawILi0E": (22, 16, 8),
        "8lowp_rawILi1E": (22, 16, 8),
        "8lowp_rawILi4E": (51, 16, 7),
    },
    "sites.hip": {
        "10site_probeE": (162, 16, 2),
    },
}


@pytest.mark.parametrize("source", sorted(PINNED))
def test_kernels_build_without_scratch_and_no_worse_than_pinned(source, tmp_path):
    """No kernel spills, and none needs more registers or fits fewer waves than before the
    shared forms: how a helper is spelt moves the allocator (see the comments in
    ``mfma_forms.h`` and ``canary_common.h``), so the verdict is the compiler's."""
    usage = kernel_resource_usage(source, tmp_path)
    pinned = PINNED[source]
    for fragment in pinned:
        assert sum(fragment in name for name in usage) == 1, (fragment, sorted(usage))
    for name, u in sorted(usage.items()):
        match = [v for fragment, v in pinned.items() if fragment in name]
        assert len(match) == 1, "a kernel without pinned numbers, or with two: %s" % name
        vgprs, agprs, occupancy = match[0]
        print("%s: %s" % (name, u))
        assert int(u["ScratchSize"]) == 0 and int(u["VGPRs Spill"]) == 0
        assert int(u["Occupancy"]) >= occupancy
        assert int(u["VGPRs"]) <= vgprs and int(u["AGPRs"]) <= agprs
