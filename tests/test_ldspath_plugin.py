"""The LDS-path check above the library, no GPU: how ``canary.run`` merges it, the flags
``run_isolated`` and the CLI pass on (alone and with the pace check's and the host link's), the
config key, the plugin's call shape with the option off and on, and the metric lines."""
import json
import subprocess

import pytest

from k8s_gpu_device_plugin_amd import config as config_mod
from k8s_gpu_device_plugin_amd.metrics import families
from k8s_gpu_device_plugin_amd.ops import canary, hostlink, ldspath, pace
from k8s_gpu_device_plugin_amd.plugin.manager import PluginManager

MERGED = {"ldspath_errors", "lds_width_errors", "lds_dma_errors", "lds_atomic_errors", "lane_errors", "tr_errors",
          "ldspath_ms", "ldspath_bad_sites"}
PACE_MERGED = {"pace_errors", "clock_mhz_min", "clock_mhz_max", "clock_fraction", "xcd_pace_ratio", "xcd_mem_ratio",
               "pace_slow_sites", "pace_slow_xccs", "pace_ms", "pace_note"}
BAD_TEXT = "lane check: 4 wrong words in dpp row_ror:3 at xcc3/se1/sh0/cu7/simd2 (+1 more site)"
CHECKS = {"lds_width", "lds_dma", "lds_atomic", "lane", "lds_tr"}


class _Lib:
    """Stands in for the canary library's amdgpu_canary_run."""

    def __init__(self, ok=1, error=b""):
        self.ok, self.error = ok, error

    def amdgpu_canary_run(self, device, nbytes, passes, iters, ref):
        r = ref._obj
        r.ok, r.device, r.error, r.num_cus = self.ok, device, self.error, 256
        return 0 if self.ok else 1


def _cu_result():
    return {"vgpr_errors": 0, "agpr_errors": 0, "l1_errors": 0, "l1_fill_errors": 0, "unlocated_errors": 0, "moved": 0,
            "regs_marched": 480, "reg_ms": 0.25, "l1_ms": 0.5, "bad_sites": [], "error": ""}


def _lds_result(**extra):
    r = {"ldspath_errors": 0, "lds_errors": 0, "dma_errors": 0, "lds_atomic_errors": 0, "lane_errors": 0, "tr_errors": 0,
         "unlocated_errors": 0, "ms": 0.6, "bad_sites": [], "error": "", "ok": True}
    r.update(extra)
    return r


def _pace_result():
    return {"pace_errors": 0, "mfma_errors": 0, "mem_errors": 0, "unlocated_errors": 0, "clock_mhz_min": 2090.0,
            "clock_mhz_max": 2110.0, "clock_fraction": 0.87, "xcd_pace_ratio": 0.99, "xcd_mem_ratio": 0.95,
            "slow_sites": [], "slow_xccs": [], "ms": 0.8, "note": "", "error": "", "ok": True}


def _hl_result():
    return {"read_errors": 0, "write_errors": 0, "h2d_errors": 0, "d2h_errors": 0, "atomic_errors": 0,
            "kernel_read_gbps": 51.0, "kernel_write_gbps": 51.5, "copy_h2d_gbps": 54.0, "copy_d2h_gbps": 56.0,
            "ms": 8.5, "error": "", "ok": True}


@pytest.fixture
def fake_run(monkeypatch):
    """canary.run over a fake library and fake CU, LDS-path, pace and host-link checks."""
    calls = []

    def install(result, lib=None):
        def ldspath_check(device=0, **kw):
            calls.append(("lds", device, kw))
            if isinstance(result, Exception):
                raise result
            return result

        def pace_check(device=0, **kw):
            calls.append(("pace", device, kw))
            return _pace_result()

        def host_link_check(device=0, nbytes=64 << 20, **kw):
            calls.append(("host", device, nbytes, kw))
            return _hl_result()
        monkeypatch.setattr(canary, "load", lambda: lib or _Lib())
        monkeypatch.setattr(canary, "cu_check", lambda device=0, **kw: _cu_result())
        monkeypatch.setattr(ldspath, "ldspath_check", ldspath_check)
        monkeypatch.setattr(pace, "pace_check", pace_check)
        monkeypatch.setattr(hostlink, "host_link_check", host_link_check)
        return calls
    return install


# ---- canary.run --------------------------------------------------------------------------
def test_run_without_the_option_is_todays_run(fake_run):
    calls = fake_run(RuntimeError("must not be called"))
    out = canary.run(2, 64 << 20, 1, 256)
    assert calls == [] and out["ok"] is True and not MERGED & set(out)
    assert canary.run(2, 64 << 20, 1, 256, lds_path=False) == out
    assert out["lds_errors"] == 0  # lds_march's count, as before


def test_run_merges_a_clean_check_under_exactly_the_stated_keys(fake_run):
    calls = fake_run(_lds_result())
    plain = canary.run(2, 64 << 20, 1, 256)
    out = canary.run(2, 64 << 20, 1, 256, lds_path=True)
    assert calls == [("lds", 2, {})]  # same device, the check's own defaults
    assert set(out) - set(plain) == MERGED and {k: out[k] for k in plain} == plain
    assert out["ok"] is True and out["error"] == ""
    assert [out[k] for k in sorted(MERGED)] == [0, 0, 0, 0, [], 0, 0.6, 0]


def test_run_keeps_lds_marchs_count_apart_from_the_width_passes(fake_run):
    fake_run(_lds_result(ok=False, error="lds check: 2 wrong words at xcc0/se0/sh0/cu1 (pass 1, 128-bit store; first at offset 0x0)",
                         ldspath_errors=2, lds_errors=2, bad_sites=["xcc0/se0/sh0/cu1/simd0"]))
    out = canary.run(0, 64 << 20, 1, 256, lds_path=True)
    assert (out["lds_errors"], out["lds_width_errors"], out["ldspath_errors"]) == (0, 2, 2)
    assert out["ldspath_bad_sites"] == ["xcc0/se0/sh0/cu1/simd0"] and out["ok"] is False


def test_run_runs_the_check_before_pace_and_the_host_link(fake_run):
    calls = fake_run(_lds_result())
    out = canary.run(2, 64 << 20, 1, 256, host_link=True, host_link_bytes=1 << 20, pace=True, lds_path=True)
    assert [c[0] for c in calls] == ["lds", "pace", "host"]
    assert MERGED | PACE_MERGED <= set(out) and out["ok"] is True


def test_run_fails_on_errors_with_the_checks_text(fake_run):
    fake_run(_lds_result(ok=False, error=BAD_TEXT, ldspath_errors=4, lane_errors=4))
    out = canary.run(0, 64 << 20, 1, 256, lds_path=True)
    assert out["ok"] is False and out["error"] == BAD_TEXT and out["lane_errors"] == 4 and out["ldspath_errors"] == 4


def test_run_keeps_an_earlier_error_text(fake_run):
    first = b"site check: 5 wrong results at xcc0/se0/sh0/cu1/simd0"
    fake_run(_lds_result(ok=False, error=BAD_TEXT, ldspath_errors=4, lane_errors=4), lib=_Lib(ok=0, error=first))
    out = canary.run(0, 64 << 20, 1, 256, lds_path=True)
    assert out["ok"] is False and out["error"] == first.decode() and out["lane_errors"] == 4


def test_run_fails_when_the_check_raises(fake_run):
    why = "ldspath_check failed: ldspath check: launch: out of memory"
    fake_run(RuntimeError(why))
    out = canary.run(0, 64 << 20, 1, 256, lds_path=True)
    assert out["ok"] is False and out["error"] == why and not MERGED & set(out)
    assert out["reg_errors"] == 0  # the checks before it are still reported


# ---- run_isolated and the CLI ------------------------------------------------------------
@pytest.fixture
def child(monkeypatch):
    cmds = []

    def run(cmd, **kw):
        cmds.append(cmd)
        return subprocess.CompletedProcess(cmd, 0, stdout=json.dumps({"ok": True, "device": 3}) + "\n", stderr="")
    monkeypatch.setattr(canary.subprocess, "run", run)
    return cmds


def test_run_isolated_adds_the_flag_only_when_asked(child):
    assert canary.run_isolated(3, 128 << 20, 30.0)["ok"] is True
    assert canary.run_isolated(3, 128 << 20, 30.0, lds_path=False)["ok"] is True
    base = child[0]
    assert child[1] == base and not any("lds" in a for a in base)
    canary.run_isolated(3, 128 << 20, 30.0, lds_path=True)
    assert child[2] == base + ["--with-lds-path"]
    canary.run_isolated(3, 128 << 20, 30.0, host_link=True, host_link_bytes=1 << 20, pace=True, lds_path=True)
    assert child[3] == base + ["--with-host-link", "--host-link-bytes", str(1 << 20), "--with-pace", "--with-lds-path"]
    canary.run_isolated(3, 128 << 20, 30.0, pace=True)
    assert child[4] == base + ["--with-pace"]


@pytest.mark.parametrize("result, rc", [(_lds_result(), 0), (_lds_result(ok=False, error=BAD_TEXT, ldspath_errors=4), 1)])
def test_lds_path_cli_runs_only_that_check(monkeypatch, capsys, result, rc):
    calls = []
    monkeypatch.setattr(ldspath, "ldspath_check", lambda device=0, **kw: calls.append((device, kw)) or result)
    monkeypatch.setattr(canary, "run", lambda *a, **kw: pytest.fail("--lds-path must not start the full run"))
    assert canary.main(["--lds-path", "--device", "2"]) == rc
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and json.loads(out[0]) == result and calls == [(2, {})]


def test_full_run_cli_passes_the_option_only_when_asked(monkeypatch, capsys):
    calls = []
    monkeypatch.setattr(canary, "run", lambda *a, **kw: calls.append((a, kw)) or {"ok": True})
    base = ["--device", "1", "--bytes", "1024", "--passes", "1"]
    assert canary.main(base) == 0
    assert canary.main(base + ["--with-lds-path"]) == 0
    assert canary.main(base + ["--with-lds-path", "--with-pace", "--with-host-link", "--host-link-bytes", "4096"]) == 0
    capsys.readouterr()
    assert calls[0] == ((1, 1024, 1, 8192), {"host_link": False, "host_link_bytes": 64 << 20})
    assert calls[1] == ((1, 1024, 1, 8192), {"host_link": False, "host_link_bytes": 64 << 20, "lds_path": True})
    assert calls[2] == ((1, 1024, 1, 8192), {"host_link": True, "host_link_bytes": 4096, "pace": True, "lds_path": True})


# ---- config ------------------------------------------------------------------------------
def test_config_default_and_validation(make_cfg):
    assert make_cfg().health.canaryLdsPath is False
    assert make_cfg(health={"canaryLdsPath": True}).health.canaryLdsPath is True
    assert make_cfg(health={"canaryldspath": "yes"}).health.canaryLdsPath is True  # keys match without case, bools are coerced
    assert make_cfg(health={"canaryLdsPath": 0}).health.canaryLdsPath is False
    assert "canaryLdsPath" in {f.name for f in config_mod.dataclasses.fields(config_mod.HealthConfig)}
    assert not any(f.startswith("canaryMinLds") or f.startswith("canaryMinLane") for f in vars(make_cfg().health))  # no floors


# ---- the plugin --------------------------------------------------------------------------
def _full_result(**extra):
    r = {"ok": True, "device": 0, "error": "", "hbm_errors": 0, "mfma_errors": 0, "gemm_errors": 0, "lowp_errors": 0,
         "lds_errors": 0, "write_gbps": 6100.0, "read_gbps": 5900.0, "mfma_tflops": 1800.0}
    r.update(extra)
    return r


def _lds_keys(**extra):
    r = {"ldspath_errors": 0, "lds_width_errors": 0, "lds_dma_errors": 0, "lds_atomic_errors": 0, "lane_errors": 0,
         "tr_errors": 0, "ldspath_ms": 0.6, "ldspath_bad_sites": []}
    r.update(extra)
    return r


def _checks(m):
    return {x.split('check="')[1].split('"')[0] for x in m._canary_lines() if x.startswith("amdgpu_canary_errors{")}


def test_plugin_off_keeps_the_old_call_shape_and_adds_no_metric_lines(make_cfg, monkeypatch):
    seen = []

    def run_isolated(device, nbytes, timeout=120.0):  # the three-parameter fake of the older tests
        seen.append((device, nbytes, timeout))
        return _full_result(device=device)
    monkeypatch.setattr(canary, "run_isolated", run_isolated)
    m = PluginManager(make_cfg(health={"canaryBytes": 1 << 20, "canaryTimeoutS": 7.0}))
    res = m._run_canary(0, 0, 3)
    assert seen == [(3, 1 << 20, 7.0)] and res["ok"] is True
    assert _checks(m) == {"hbm", "mfma", "gemm", "lowp", "lds"} and not CHECKS & _checks(m)


@pytest.fixture
def plugin_on(make_cfg, monkeypatch):
    def make(result, **health):
        seen = []

        def run_isolated(device, nbytes, timeout=120.0, **kw):
            seen.append((device, nbytes, timeout, kw))
            return result
        monkeypatch.setattr(canary, "run_isolated", run_isolated)
        cfg = make_cfg(health=dict({"canaryLdsPath": True, "canaryBytes": 1 << 20, "canaryTimeoutS": 7.0}, **health))
        return PluginManager(cfg), seen
    return make


def test_plugin_on_passes_the_option_and_exports_the_checks(plugin_on):
    m, seen = plugin_on(_full_result(**_lds_keys()))
    res = m._run_canary(0, 0, 3)
    assert seen == [(3, 1 << 20, 7.0, {"lds_path": True})] and res["ok"] is True
    assert _checks(m) == {"hbm", "mfma", "gemm", "lowp", "lds"} | CHECKS
    lines = m._canary_lines()
    for check in sorted(CHECKS):
        assert 'amdgpu_canary_errors{gpu="0",partition="0",check="%s"} 0' % check in lines


def test_plugin_on_with_pace_and_the_host_link_passes_every_keyword(plugin_on):
    m, seen = plugin_on(_full_result(**_lds_keys()), canaryPace=True, canaryHostLink=True, canaryHostLinkBytes=1 << 20)
    m._run_canary(0, 0, 3)
    assert seen == [(3, 1 << 20, 7.0, {"host_link": True, "host_link_bytes": 1 << 20, "pace": True, "lds_path": True})]


def test_plugin_on_an_error_count_fails_the_verdict_with_the_checks_text(plugin_on):
    m, _ = plugin_on(_full_result(ok=False, error=BAD_TEXT, **_lds_keys(ldspath_errors=4, lane_errors=4)))
    res = m._run_canary(1, 0, 0)
    assert res["ok"] is False and res["error"] == BAD_TEXT
    lines = m._canary_lines()
    assert 'amdgpu_canary_errors{gpu="1",partition="0",check="lane"} 4' in lines
    assert 'amdgpu_canary_errors{gpu="1",partition="0",check="lds_tr"} 0' in lines
    assert 'amdgpu_canary_last_ok{gpu="1",partition="0"} 0' in lines


def test_the_family_help_names_the_new_checks():
    fam = families.family_of("amdgpu_canary_errors")
    assert "health.canaryLdsPath" in fam.help
    for check in CHECKS:
        assert check in fam.help, check
    assert "health.canaryLdsPath" in families.markdown()
