"""The compiler's own account of every kernel of one HIP source: its kernel-resource-usage
remarks, so a build contract (no scratch, an occupancy, an LDS size) is read from the build and
a compiler upgrade cannot change it silently."""
import re
import subprocess

from k8s_gpu_device_plugin_amd import _build


def kernel_resource_usage(source_suffix, tmp_path):
    """Compiles the one canary source whose path ends in ``source_suffix`` for the package's
    offload architecture; returns ``{mangled kernel name: {remark name: value string}}``, e.g.
    ``usage[name]["ScratchSize"] == "0"``."""
    src = [s for s in _build.CANARY_SOURCES if s.endswith(source_suffix)]
    assert len(src) == 1
    p = subprocess.run([_build.hipcc_path(), "--offload-arch=" + _build.OFFLOAD_ARCH, "-O3", "-std=c++17", "-fPIC",
                        "-c", "-Rpass-analysis=kernel-resource-usage", src[0], "-o", str(tmp_path / "usage.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
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
    return usage
