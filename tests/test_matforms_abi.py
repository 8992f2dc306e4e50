"""The matrix-forms library's C ABI (``ops/matforms/matforms.h``, ``ops/matforms/matforms_host.h``):
the sizes of the structs ``ops/matforms.py`` mirrors with ctypes, the exact set of exported
entry points, the build's list of sources and headers, arguments refused as text before any
HIP call, and the kernels' build contract from the compiler's own output: no scratch, no
spills, and the MFMA instruction of every form of the table present in that form's kernels (a
compiler that folds a form away fails here).  The library stands beside the table of the
canary's libraries: ``HIP_LIBS`` keeps its four rows and ``build_all`` does not build it."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import matforms_model as model
from k8s_gpu_device_plugin_amd import _build
from k8s_gpu_device_plugin_amd.ops import matforms

EXPORTS = ["amdgpu_matforms_" + name for name in """
run reduce raw operands expected inject_expected map forms form_ints encode describe sizeof
""".split()]
KERNELS = ("form_sweep", "raw_mfma", "form_rate")  # one instance of each per form


@pytest.mark.parametrize("which, name, size", [(0, "Record", 80), (1, "MatFormsResult", 848)])
def test_ctypes_mirror_has_the_size_the_library_reports(which, name, size):
    assert ctypes.sizeof(getattr(matforms, name)) == size == matforms.load().amdgpu_matforms_sizeof(which)


def test_numpy_record_is_the_ctypes_record():
    dt = np.dtype(matforms.RECORD_DTYPE)
    assert dt.itemsize == ctypes.sizeof(matforms.Record)
    assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(matforms.Record, n).offset) for n, _ in matforms.Record._fields_]


def test_sizeof_and_the_table_refuse_what_they_do_not_know():
    lib = matforms.load()
    n = len(matforms.FORMS)
    assert lib.amdgpu_matforms_sizeof(2) == -1 and lib.amdgpu_matforms_sizeof(-1) == -1
    assert lib.amdgpu_matforms_forms(-1, 0, None, 0) == n <= matforms.MAX_FORMS
    assert lib.amdgpu_matforms_forms(n, 0, None, 0) == -1 and lib.amdgpu_matforms_forms(0, 3, None, 0) == -1
    assert lib.amdgpu_matforms_forms(0, 0, None, 0) == len(matforms.FORMS[0])
    assert lib.amdgpu_matforms_inject_expected(n, 0) == -1 and lib.amdgpu_matforms_inject_expected(0, -1) == -1
    assert lib.amdgpu_matforms_form_ints(n, (ctypes.c_uint * 12)()) == -1
    with pytest.raises(ValueError):
        matforms.form_index("fp64_32")
    with pytest.raises(ValueError):
        matforms.operands(0, 0, 9)
    assert len(matforms.FORMS) == len(matforms.FORM_TEXTS) == len(matforms.INSTRUCTIONS) == len(set(matforms.FORMS))
    # the forms whose map the guide or the project's own measurements give are all there
    assert {"bf16_16", "f32_32", "f32_16", "f64_16", "mxfp8fp4_32"} <= set(matforms.FORMS)


def _nm():
    llvm = os.path.join(_build.ROCM, "lib", "llvm", "bin", "llvm-nm")
    for path in (llvm, shutil.which("llvm-nm"), shutil.which("nm")):
        if path and os.path.exists(path):
            return path
    raise AssertionError("no nm: neither ROCm's llvm-nm nor a system nm")


def test_library_exports_exactly_the_entry_points():
    matforms.load()  # builds the library if it is missing
    p = subprocess.run([_nm(), "-D", "--defined-only", _build.MATFORMS_LIB], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    rows = [line.split() for line in p.stdout.splitlines()]
    text = sorted(r[2] for r in rows if len(r) == 3 and r[1] == "T" and not r[2].startswith("_Z"))
    assert text == sorted(EXPORTS) == sorted("amdgpu_matforms_" + n for n in matforms.EXPORTS)
    lib = ctypes.CDLL(_build.MATFORMS_LIB)
    assert all(hasattr(lib, name) for name in EXPORTS)


def test_build_lists_cover_every_source_and_header_of_the_directory():
    listed = _build.MATFORMS_SOURCES + _build.MATFORMS_HEADERS
    assert len(set(listed)) == len(listed) and all(os.path.isfile(p) for p in listed)
    on_disk = glob.glob(os.path.join(_build.MATFORMS_DIR, "*.hip")) + glob.glob(os.path.join(_build.MATFORMS_DIR, "*.h"))
    own = [p for p in listed if os.path.dirname(p) == _build.MATFORMS_DIR]
    assert sorted(os.path.realpath(p) for p in on_disk) == sorted(os.path.realpath(p) for p in own)
    assert set(_build.CANARY_HEADERS) <= set(_build.MATFORMS_HEADERS)
    others = set(_build.CANARY_SOURCES) | set(_build.HOSTLINK_SOURCES) | set(_build.PACE_SOURCES) | set(_build.LDSPATH_SOURCES)
    assert not set(_build.MATFORMS_SOURCES) & others
    assert matforms.LIB_PATH == _build.MATFORMS_LIB
    assert len({os.path.dirname(row["lib"]) for row in _build.HIP_LIBS} | {_build.MATFORMS_DIR}) == len(_build.HIP_LIBS) + 1


def test_the_library_stands_beside_the_table_of_the_canary_s_libraries(monkeypatch):
    """Nothing calls the check automatically yet: adding its row to ``HIP_LIBS`` (and to
    ``canary.OPTIONAL_CHECKS``) belongs with the tests that pin those tables."""
    assert [row["name"] for row in _build.HIP_LIBS] == ["canary", "hostlink", "pace", "ldspath"]
    built = []
    monkeypatch.setattr(_build, "_build_hip_lib", lambda **kw: built.append(kw["name"]) or kw["lib"])
    monkeypatch.setattr(_build, "build_native", lambda **kw: None)
    monkeypatch.setattr(_build, "build_bench", lambda **kw: None)
    _build.build_all()
    assert _build.main([]) == 0
    assert "matforms" not in built and len(built) == 8
    assert _build.main(["--matforms"]) == 0 and built[8:] == ["matforms"]
    assert _build.build_matforms(verbose=False) == _build.MATFORMS_LIB and built[9:] == ["matforms"]


def test_the_two_host_headers_need_no_hip():
    for name in ("matforms_forms.h", "matforms_host.h"):
        text = open(os.path.join(_build.MATFORMS_DIR, name)).read()
        assert "hip/" not in text and "canary_" not in text, name
    assert '#include "../site.h"' in open(os.path.join(_build.MATFORMS_DIR, "matforms_host.h")).read()
    assert '#include "../canary_host.h"' in open(os.path.join(_build.MATFORMS_DIR, "matforms.h")).read()


def test_bad_arguments_are_an_error_text_before_any_gpu_call():
    """Refused arguments never reach HIP, so this needs no GPU."""
    for kw in ({"blocks": -1}, {"blocks": 4097}, {"ksteps": 0}, {"ksteps": 9}, {"forms": []}, {"inject_form": "i8_32", "inject_waves": -1},
               {"forms": ["f64_16"], "inject_form": "i8_32", "inject_waves": 1}, {"rates": True, "rate_iters": -1}):
        with pytest.raises(RuntimeError, match="matrix form check: bad arguments"):
            matforms.matrix_forms_check(**kw)
    with pytest.raises(ValueError):
        matforms.matrix_forms_check(forms=["everything"])
    zeros = np.zeros((1, 64, 8), dtype=np.uint32)
    err = ctypes.create_string_buffer(256)
    assert matforms.load().amdgpu_matforms_raw(0, len(matforms.FORMS), zeros.ctypes.data, zeros.ctypes.data, zeros.ctypes.data,
                                               zeros.ctypes.data, zeros.ctypes.data, 1, err, 256) == -1
    assert err.value.decode().startswith("matrix form check: bad arguments")
    with pytest.raises(ValueError):
        matforms.raw("i8_32", zeros[:, :32], zeros)


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """One device-only compile of matforms.hip: the kernel-resource-usage remarks per kernel, and
    the assembly per kernel."""
    out = tmp_path_factory.mktemp("matforms_asm") / "matforms.s"
    p = subprocess.run([_build.hipcc_path(), "--offload-arch=" + _build.OFFLOAD_ARCH, "-O3", "-std=c++17", "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", _build.MATFORMS_SOURCES[0], "-o", str(out)],
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
            name = m.group(1) if any(k in m.group(1) for k in KERNELS) else None
        elif line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            name = None
        if name and line.startswith("\t") and not line.startswith("\t."):
            kernels.setdefault(name, []).append(line.split(";")[0].strip())
    return usage, {k: "\n".join(v) for k, v in kernels.items()}


def test_kernels_build_without_scratch_or_spills(compiled):
    usage, _ = compiled
    n = len(matforms.FORMS)
    for stem in KERNELS:
        assert sum(stem in name for name in usage) == n, (stem, sorted(usage))
    assert len(usage) == len(KERNELS) * n
    for name, u in usage.items():
        assert u["ScratchSize"] == "0", (name, u)
        assert u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (name, u)
        assert u["LDS Size"] == "0", (name, u)  # no static __shared__: the allocation is the launch's


MX_CODE = {"e4m3": 0, "e5m2": 1, "e2m3": 2, "e3m2": 3, "e2m1": 4}  # cbsz / blgp of the scaled instruction


def test_every_form_s_instruction_is_in_its_kernels_assembly(compiled):
    _, kernels = compiled
    wrong = []
    for index, (form, instruction) in enumerate(zip(matforms.FORMS, matforms.INSTRUCTIONS)):
        assert instruction == model.FORMS[form]["instruction"]
        pattern = re.escape(instruction) + r"\b"
        tag = "%d%sE" % (len(_class_name(form)), _class_name(form))  # the form's class in the mangled name
        mine = {name: text for name, text in kernels.items() if tag in name}
        if len(mine) != len(KERNELS):
            wrong.append((form, "kernels", sorted(mine)))
        for name, text in mine.items():
            found = [line for line in text.splitlines() if re.search(pattern, line)]
            if model.FORMS[form]["scaled"]:  # the formats are modifiers; the assembler leaves a zero one out
                a, b = (MX_CODE[e] for e in model.FORMS[form]["enc"])
                found = [line for line in found
                         if (re.search(r"cbsz:%d\b" % a, line) if a else "cbsz:" not in line)
                         and (re.search(r"blgp:%d\b" % b, line) if b else "blgp:" not in line)]
            if not found:
                wrong.append((form, name))
    assert not wrong, wrong


def _class_name(form):
    return {"f16_32": "FormF16_32", "f16_16": "FormF16_16", "bf16_16": "FormBf16_16", "i8_32": "FormI8_32", "i8_16": "FormI8_16",
            "f32_32": "FormF32_32", "f32_16": "FormF32_16", "f64_16": "FormF64_16", "fp8_16": "FormFp8_16",
            "bf8fp8_32": "FormBf8Fp8_32", "mxfp6_32": "FormMxFp6_32", "mxbf6_32": "FormMxBf6_32",
            "mxfp8fp4_32": "FormMxFp8Fp4_32", "mxfp8_16": "FormMxFp8_16", "mxfp4_16": "FormMxFp4_16"}[form]
