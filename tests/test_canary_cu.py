"""CU memory check, host side: the register march's build contract (no scratch, occupancy 1,
at least 448 of 512 entries), the C ABI, argument validation, the error text, how
``canary.run`` merges the check into its verdict, the per-check metrics, the CLI and the
start-up canary's log line."""
import ctypes
import json
import logging
import time

import pytest

from kernel_usage import kernel_resource_usage
from k8s_gpu_device_plugin_amd.ops import canary
from k8s_gpu_device_plugin_amd.plugin.kubelet_stub import KubeletStub
from k8s_gpu_device_plugin_amd.plugin.manager import PluginManager


def _site(xcc, se, sh, cu, simd):
    return simd | (cu << 2) | (sh << 6) | (se << 7) | (xcc << 10)


def _regs():
    nv, na = ctypes.c_int(), ctypes.c_int()
    canary.load().amdgpu_canary_cu_regs(ctypes.byref(nv), ctypes.byref(na))
    return nv.value, na.value


# ---- build contract --------------------------------------------------------------------
def test_reg_march_builds_without_scratch_at_occupancy_one(tmp_path):
    """The march is a register-file test only while no marched value lives in scratch memory
    and a wave is allocated the SIMD's whole file: both are read from the compiler's own
    resource-usage remarks, so a compiler upgrade cannot change them silently."""
    usage = kernel_resource_usage("cumem.hip", tmp_path)
    march = [u for n, u in usage.items() if "reg_march" in n]
    assert len(march) == 1, sorted(usage)
    u = march[0]
    nv, na = _regs()
    print("reg_march: %s; NV %d, NA %d" % (u, nv, na))
    assert int(u["ScratchSize"]) == 0
    assert int(u["Occupancy"]) == 1
    assert int(u["VGPRs Spill"]) == 0
    assert int(u["AGPRs"]) >= na and int(u["VGPRs"]) >= nv
    assert nv + na >= 448 and nv <= 256 and na <= 256


# ---- C ABI -----------------------------------------------------------------------------
def test_library_exports_the_cu_symbols_and_sizes_agree():
    lib = canary.load()
    for sym in ("amdgpu_canary_cu", "amdgpu_canary_cu_describe", "amdgpu_canary_cu_regs", "amdgpu_canary_cu_sizeof"):
        assert hasattr(lib, sym)
    assert lib.amdgpu_canary_cu_sizeof(0) == ctypes.sizeof(canary.CuSlot) == 16
    assert lib.amdgpu_canary_cu_sizeof(1) == ctypes.sizeof(canary.CuResult)
    assert lib.amdgpu_canary_cu_sizeof(2) == -1
    assert canary.CU_INJECT == ("vgpr", "agpr", "l1")


@pytest.mark.parametrize("kw", [dict(l1_kb=6), dict(l1_kb=36), dict(l1_kb=0), dict(reps=0), dict(reps=65),
                                dict(blocks=5000), dict(blocks=-1), dict(l1_reps=0), dict(l1_reps=65),
                                dict(inject_waves=-1)])
def test_bad_arguments_are_refused_before_any_hip_call(kw):
    """The message is the validator's: a HIP call on a machine without a GPU would have
    produced HIP's error string instead."""
    with pytest.raises(RuntimeError, match=r"cu_check failed: cu check: bad arguments \(blocks "):
        canary.cu_check(**kw)


def test_inject_kind_out_of_range_is_refused():
    lib = canary.load()
    for kind in (3, -2):
        r, err = canary.CuResult(), ctypes.create_string_buffer(256)
        assert lib.amdgpu_canary_cu(0, 1, 1, 4, 1, kind, 1, None, None, 0, ctypes.byref(r), err, 256) == -1
        assert err.value.decode().startswith("cu check: bad arguments") and "inject %d/1" % kind in err.value.decode()
    r, err = canary.CuResult(), ctypes.create_string_buffer(256)
    assert lib.amdgpu_canary_cu(0, 1, 1, 4, 1, -1, 0, None, None, 5, ctypes.byref(r), err, 256) == -1  # len, no buffer
    assert (r.regs_vgpr, r.regs_agpr) == _regs()
    with pytest.raises(ValueError):
        canary.cu_check(inject="sgpr")


# ---- the error text --------------------------------------------------------------------
def _describe(r, table):
    buf = ctypes.create_string_buffer(256)
    n = canary.load().amdgpu_canary_cu_describe(ctypes.byref(r), table, buf, 256)
    assert n == len(buf.value)
    return buf.value.decode()


def test_describe_names_the_site_the_kind_and_further_sites():
    table = (canary.CuSlot * canary.SITE_SLOTS)()
    r = canary.CuResult()
    assert _describe(r, table) == ""
    table[_site(3, 1, 0, 7, 2)].bad_agpr = 2
    table[_site(5, 0, 0, 1, 0)].bad_agpr = 1
    r.agpr_errors = 3
    assert _describe(r, table) == "register check: 3 wrong words at xcc3/se1/sh0/cu7/simd2 (agpr; +1 more site)"
    table[_site(5, 0, 0, 1, 0)].bad_agpr = 0
    r.agpr_errors = 2
    assert _describe(r, table) == "register check: 2 wrong words at xcc3/se1/sh0/cu7/simd2 (agpr)"
    table[_site(3, 1, 0, 7, 2)].bad_agpr = 0
    table[_site(3, 1, 0, 7, 2)].bad_vgpr = 1
    table[_site(6, 2, 0, 4, 1)].bad_vgpr = 1
    table[_site(7, 3, 0, 8, 3)].bad_agpr = 4
    r.agpr_errors, r.vgpr_errors, r.unlocated_errors = 4, 2, 1
    assert _describe(r, table) == "register check: 7 wrong words at xcc3/se1/sh0/cu7/simd2 (vgpr+agpr; +2 more sites)"
    table = (canary.CuSlot * canary.SITE_SLOTS)()
    r = canary.CuResult()
    r.vgpr_errors = 1
    table[_site(0, 0, 0, 0, 1)].bad_vgpr = 1
    assert _describe(r, table) == "register check: 1 wrong words at xcc0/se0/sh0/cu0/simd1 (vgpr)"
    r = canary.CuResult()
    r.unlocated_errors = 4
    assert _describe(r, (canary.CuSlot * canary.SITE_SLOTS)()) == "register check: 4 wrong words at an unknown site"


def test_describe_names_the_cu_of_an_l1_error_after_the_register_check():
    table = (canary.CuSlot * canary.SITE_SLOTS)()
    r = canary.CuResult()
    table[_site(3, 1, 0, 7, 0)].bad_l1 = 1
    table[_site(3, 1, 0, 7, 3)].bad_l1 = 1  # two SIMDs, one CU
    r.l1_errors = 2
    assert _describe(r, table) == "l1 check: 2 wrong words at xcc3/se1/sh0/cu7"
    table[_site(4, 0, 0, 2, 1)].bad_l1 = 5
    r.l1_errors = 7
    assert _describe(r, table) == "l1 check: 7 wrong words at xcc3/se1/sh0/cu7 (+1 more cu)"
    r.l1_fill_errors = 9  # not a verdict: no text of its own
    table[_site(1, 0, 0, 0, 0)].bad_vgpr = 1
    r.vgpr_errors = 1
    assert _describe(r, table).startswith("register check: 1 wrong words at xcc1/se0/sh0/cu0/simd0 (vgpr)")
    r = canary.CuResult()
    r.l1_fill_errors = 9
    assert _describe(r, (canary.CuSlot * canary.SITE_SLOTS)()) == ""


# ---- run() merges the check ------------------------------------------------------------
class _Lib:
    """Stands in for the library's amdgpu_canary_run: fills the result like a run would."""

    def __init__(self, ok=1, error=b""):
        self.ok, self.error, self.calls = ok, error, 0

    def amdgpu_canary_run(self, device, nbytes, passes, iters, ref):
        self.calls += 1
        r = ref._obj
        r.ok, r.device, r.error, r.num_cus, r.site_errors = self.ok, device, self.error, 256, 0 if self.ok else 5
        return 0 if self.ok else 1


def _cu_result(**extra):
    r = {"vgpr_errors": 0, "agpr_errors": 0, "l1_errors": 0, "l1_fill_errors": 0, "unlocated_errors": 0, "moved": 0,
         "regs_marched": 480, "reg_ms": 0.25, "l1_ms": 0.5, "bad_sites": [], "error": ""}
    r.update(extra)
    return r


def _run_with(monkeypatch, cu, lib=None):
    lib = lib or _Lib()
    calls = []

    def cu_check(device=0, **kw):
        calls.append((device, kw))
        if isinstance(cu, Exception):
            raise cu
        return cu
    monkeypatch.setattr(canary, "load", lambda: lib)
    monkeypatch.setattr(canary, "cu_check", cu_check)
    out = canary.run(2, 64 << 20, 1, 256)
    assert calls == [(2, {})] and lib.calls == 1  # same device, the check's own defaults
    return out


def test_run_merges_a_clean_cu_check(monkeypatch):
    out = _run_with(monkeypatch, _cu_result())
    assert out["ok"] is True and out["error"] == "" and out["device"] == 2 and out["num_cus"] == 256
    assert (out["reg_errors"], out["l1_errors"], out["l1_fill_errors"]) == (0, 0, 0)
    assert out["cu_ms"] == 0.75 and out["regs_marched"] == 480 and out["cu_bad_sites"] == []
    assert out["bad_sites"] == []  # the site probe's list keeps its meaning


@pytest.mark.parametrize("counts, reg, l1", [(dict(vgpr_errors=2), 2, 0), (dict(agpr_errors=1), 1, 0),
                                             (dict(unlocated_errors=3), 3, 0),
                                             (dict(vgpr_errors=1, agpr_errors=1, unlocated_errors=1), 3, 0),
                                             (dict(l1_errors=4), 0, 4)])
def test_run_fails_on_register_or_l1_errors(monkeypatch, counts, reg, l1):
    why = "register check: 3 wrong words at xcc3/se1/sh0/cu7/simd2 (agpr; +1 more site)"
    out = _run_with(monkeypatch, _cu_result(error=why, bad_sites=["xcc3/se1/sh0/cu7/simd2"], **counts))
    assert out["ok"] is False and out["error"] == why
    assert (out["reg_errors"], out["l1_errors"]) == (reg, l1)
    assert out["cu_bad_sites"] == ["xcc3/se1/sh0/cu7/simd2"]


def test_run_keeps_an_earlier_error_text(monkeypatch):
    first = b"site check: 5 wrong results at xcc0/se0/sh0/cu1/simd0"
    out = _run_with(monkeypatch, _cu_result(vgpr_errors=1, error="register check: 1 wrong words at ..."),
                    lib=_Lib(ok=0, error=first))
    assert out["ok"] is False and out["error"] == first.decode() and out["reg_errors"] == 1
    out = _run_with(monkeypatch, _cu_result(), lib=_Lib(ok=0, error=first))  # a clean check does not mend a failed run
    assert out["ok"] is False and out["error"] == first.decode() and out["reg_errors"] == 0


def test_fill_errors_alone_do_not_fail_the_run(monkeypatch):
    out = _run_with(monkeypatch, _cu_result(l1_fill_errors=7))
    assert out["ok"] is True and out["error"] == "" and out["l1_fill_errors"] == 7 and out["l1_errors"] == 0


def test_run_fails_when_the_cu_check_raises(monkeypatch):
    out = _run_with(monkeypatch, RuntimeError("cu_check failed: cu check: reg_march: unspecified launch failure"))
    assert out["ok"] is False
    assert out["error"] == "cu_check failed: cu check: reg_march: unspecified launch failure"
    assert "reg_errors" not in out and "l1_errors" not in out


# ---- metrics, CLI, log line ------------------------------------------------------------
def _result(**extra):
    r = {"ok": True, "device": 0, "error": "", "hbm_errors": 0, "mfma_errors": 0, "gemm_errors": 0,
         "lowp_errors": 0, "lds_errors": 0, "write_gbps": 6100.0, "read_gbps": 5900.0, "mfma_tflops": 1800.0}
    r.update(extra)
    return r


def _error_samples(m):
    rows = [x for x in m._canary_lines() if x.startswith("amdgpu_canary_errors{")]
    return {x.split('check="')[1].split('"')[0]: int(x.rsplit(" ", 1)[1]) for x in rows}


def test_canary_lines_carry_reg_and_l1_only_when_present(make_cfg):
    m = PluginManager(make_cfg())
    m.canary_results[(0, 0)] = (time.time(), _result(reg_errors=3, l1_errors=2, l1_fill_errors=9))
    got = _error_samples(m)
    assert (got["reg"], got["l1"]) == (3, 2)
    assert set(got) == {"hbm", "mfma", "gemm", "lowp", "lds", "reg", "l1"}
    m.canary_results[(0, 0)] = (time.time(), _result(reg_errors=0, l1_errors=0))
    assert _error_samples(m)["reg"] == 0 and _error_samples(m)["l1"] == 0
    m.canary_results[(0, 0)] = (time.time(), _result())
    assert set(_error_samples(m)) == {"hbm", "mfma", "gemm", "lowp", "lds"}


@pytest.mark.parametrize("counts, rc", [((0, 0, 0, 0), 0), ((1, 0, 0, 0), 1), ((0, 2, 0, 0), 1), ((0, 0, 3, 0), 1),
                                        ((0, 0, 0, 4), 1)])
def test_cu_cli_prints_json_and_fails_on_any_error(monkeypatch, capsys, counts, rc):
    calls = []

    def cu_check(device=0, **kw):
        calls.append((device, kw))
        return _cu_result(vgpr_errors=counts[0], agpr_errors=counts[1], unlocated_errors=counts[2],
                          l1_errors=counts[3], l1_fill_errors=6, sites={"xcc0/se0/sh0/cu0/simd0": {"waves": 2}})
    monkeypatch.setattr(canary, "cu_check", cu_check)
    assert canary.main(["--cu", "--device", "2"]) == rc
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1
    assert json.loads(out[0])["sites"] == {"xcc0/se0/sh0/cu0/simd0": {"waves": 2}}
    assert calls == [(2, {})]


def test_cu_cli_passes_with_fill_errors_only(monkeypatch, capsys):
    monkeypatch.setattr(canary, "cu_check", lambda device=0, **kw: _cu_result(l1_fill_errors=6))
    assert canary.main(["--cu"]) == 0
    assert json.loads(capsys.readouterr().out)["l1_fill_errors"] == 6


class _Records(logging.Handler):
    def __init__(self):
        super().__init__(logging.DEBUG)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def test_startup_canary_log_names_the_register_site(make_cfg, plugin_dir, monkeypatch):
    from k8s_gpu_device_plugin_amd.plugin import manager as manager_mod
    why = "register check: 3 wrong words at xcc3/se1/sh0/cu7/simd2 (agpr; +1 more site)"

    def run_isolated(device, nbytes, timeout=120.0):
        if device != 9:
            return {"ok": True, "device": device, "error": "", "reg_errors": 0, "l1_errors": 0}
        return {"ok": False, "device": device, "error": why, "reg_errors": 3, "l1_errors": 0, "l1_fill_errors": 0}
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
            assert "partition 1" in failed[0] and "xcc3/se1/sh0/cu7/simd2 (agpr" in failed[0] and why in failed[0]
            lines = "\n".join(m._canary_lines())
            assert 'check="reg"} 3' in lines and 'check="l1"} 0' in lines
    finally:
        manager_mod.log.removeHandler(rec)
        manager_mod.log.setLevel(level)
        if m is not None:
            m.stop()
            t.join(10)
