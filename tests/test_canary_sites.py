"""Site probe, host side: packed-site decoding, the per-check canary metrics and the
place of a failure in the start-up canary's log line."""
import logging
import time

import pytest

from k8s_gpu_device_plugin_amd.ops import canary
from k8s_gpu_device_plugin_amd.plugin.kubelet_stub import KubeletStub
from k8s_gpu_device_plugin_amd.plugin.manager import PluginManager


def _pack(xcc, se, sh, cu, simd):
    """The site as ops/sites.hip packs it.  From the documented registers: HW_ID has SIMD_ID
    at 5:4, CU_ID 11:8, SH_ID 12, SE_ID 15:13; XCC_ID has the XCC at 3:0.  HW_ID bits 15:4 are
    read as one field, so CU/SH/SE (HW_ID 15:8) land above the 2 SIMD bits and the XCC on top."""
    hw_id = (simd << 4) | (cu << 8) | (sh << 12) | (se << 13)
    field = (hw_id >> 4) & 0xFFF  # bits 15:4
    return (field & 3) | (((field >> 4) & 0xFF) << 2) | ((xcc & 0xF) << 10)


@pytest.mark.parametrize("fields", [
    dict(xcc=0, se=0, sh=0, cu=0, simd=0),
    dict(xcc=15, se=7, sh=1, cu=15, simd=3),  # the maximum of every field
    dict(xcc=15, se=0, sh=0, cu=0, simd=0),
    dict(xcc=0, se=7, sh=0, cu=0, simd=0),
    dict(xcc=0, se=0, sh=1, cu=0, simd=0),
    dict(xcc=0, se=0, sh=0, cu=15, simd=0),
    dict(xcc=0, se=0, sh=0, cu=0, simd=3),
    dict(xcc=3, se=1, sh=0, cu=7, simd=2),
])
def test_decode_and_format_site(fields):
    packed = _pack(**fields)
    assert 0 <= packed < canary.SITE_SLOTS
    assert canary.decode_site(packed) == fields
    assert canary.format_site(packed) == "xcc%(xcc)d/se%(se)d/sh%(sh)d/cu%(cu)d/simd%(simd)d" % fields
    assert _pack(**canary.decode_site(packed)) == packed  # round trip


def test_site_strings_are_distinct_over_the_whole_table():
    assert canary.format_site(_pack(3, 1, 0, 7, 2)) == "xcc3/se1/sh0/cu7/simd2"
    assert len({canary.format_site(p) for p in range(canary.SITE_SLOTS)}) == canary.SITE_SLOTS


def _result(**extra):
    r = {"ok": True, "device": 0, "error": "", "hbm_errors": 0, "mfma_errors": 0, "gemm_errors": 0,
         "lowp_errors": 0, "lds_errors": 0, "write_gbps": 6100.0, "read_gbps": 5900.0, "mfma_tflops": 1800.0}
    r.update(extra)
    return r


def _error_samples(m):
    rows = [x for x in m._canary_lines() if x.startswith("amdgpu_canary_errors{")]
    return {x.split('check="')[1].split('"')[0]: int(x.rsplit(" ", 1)[1]) for x in rows}


def test_canary_lines_carry_site_checks_only_when_present(make_cfg):
    m = PluginManager(make_cfg())
    m.canary_results[(0, 0)] = (time.time(), _result(site_errors=5, cus_unreached=2))
    got = _error_samples(m)
    assert got["site"] == 5 and got["unreached"] == 2
    assert set(got) == {"hbm", "mfma", "gemm", "lowp", "lds", "site", "unreached"}
    m.canary_results[(0, 0)] = (time.time(), _result())
    assert set(_error_samples(m)) == {"hbm", "mfma", "gemm", "lowp", "lds"}


class _Records(logging.Handler):
    def __init__(self):
        super().__init__(logging.DEBUG)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def test_startup_canary_log_names_the_site(make_cfg, plugin_dir, monkeypatch):
    from k8s_gpu_device_plugin_amd.plugin import manager as manager_mod
    why = "site check: 5 wrong results at xcc3/se1/sh0/cu7/simd2 (+1 more site)"

    def run_isolated(device, nbytes, timeout=120.0):
        if device != 9:
            return {"ok": True, "device": device, "error": ""}
        return {"ok": False, "device": device, "error": why, "site_errors": 5,
                "bad_sites": ["xcc3/se1/sh0/cu7/simd2", "xcc3/se1/sh0/cu7/simd3"]}
    monkeypatch.setattr(canary, "run_isolated", run_isolated)
    rec = _Records()
    manager_mod.log.addHandler(rec)
    level = manager_mod.log.level
    manager_mod.log.setLevel(logging.INFO)
    m = t = None
    try:
        with KubeletStub(plugin_dir) as k:
            m = PluginManager(make_cfg(fixture="2gpu_cpx_nps2", migStrategy="single", health={"canaryOnStart": True}))
            t = m.start_background()
            k.wait_for_registrations(1)
            deadline = time.monotonic() + 10
            while time.monotonic() < deadline and (m._start_pending or not m.counters.get("canary_failures")):
                time.sleep(0.02)
            failed = [x for x in rec.lines if x.startswith("start-up canary failed")]
            assert len(failed) == 1, rec.lines
            assert "partition 1" in failed[0] and "xcc3/se1/sh0/cu7/simd2" in failed[0] and why in failed[0]
            assert 'check="site"} 5' in "\n".join(m._canary_lines())
    finally:
        manager_mod.log.removeHandler(rec)
        manager_mod.log.setLevel(level)
        if m is not None:
            m.stop()
            t.join(10)
