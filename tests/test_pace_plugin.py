"""The pace check above the library, no GPU: how ``canary.run`` merges it, the flags
``run_isolated`` and the CLI pass on (alone and with the host link's), the config keys and
their validation, the plugin's call shape with the option off, on and on with the host link,
the two floors with their texts and order, and the metric lines."""
import json
import subprocess

import pytest

from k8s_gpu_device_plugin_amd import config as config_mod
from k8s_gpu_device_plugin_amd.metrics import families
from k8s_gpu_device_plugin_amd.ops import canary, hostlink, pace
from k8s_gpu_device_plugin_amd.plugin.manager import PluginManager

MERGED = {"pace_errors", "clock_mhz_min", "clock_mhz_max", "clock_fraction", "xcd_pace_ratio", "xcd_mem_ratio",
          "pace_slow_sites", "pace_slow_xccs", "pace_ms", "pace_note"}
HOST_MERGED = {"host_read_errors", "host_write_errors", "host_copy_errors", "host_atomic_errors", "kernel_read_gbps",
               "kernel_write_gbps", "copy_h2d_gbps", "copy_d2h_gbps", "host_ms"}
BAD_TEXT = "pace check: 3 wrong results at xcc3/se1/sh0/cu7/simd2 (+1 more site)"
NOTE = "pace: xcc5 ran 1210 MHz beside a median of 2105 (ratio 0.57)"


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


def _pace_result(**extra):
    r = {"pace_errors": 0, "mfma_errors": 0, "mem_errors": 0, "unlocated_errors": 0, "clock_mhz_min": 2090.0,
         "clock_mhz_max": 2110.0, "clock_fraction": 0.87, "xcd_pace_ratio": 0.99, "xcd_mem_ratio": 0.95,
         "slow_sites": [], "slow_xccs": [], "ms": 0.8, "note": "", "error": "", "ok": True}
    r.update(extra)
    return r


def _hl_result():
    return {"read_errors": 0, "write_errors": 0, "h2d_errors": 0, "d2h_errors": 0, "atomic_errors": 0,
            "kernel_read_gbps": 51.0, "kernel_write_gbps": 51.5, "copy_h2d_gbps": 54.0, "copy_d2h_gbps": 56.0,
            "ms": 8.5, "error": "", "ok": True}


@pytest.fixture
def fake_run(monkeypatch):
    """canary.run over a fake library, a fake CU check, a fake pace check and a fake host-link check."""
    calls = []

    def install(result, lib=None):
        def pace_check(device=0, **kw):
            calls.append(("pace", device, kw))
            if isinstance(result, Exception):
                raise result
            return result

        def host_link_check(device=0, nbytes=64 << 20, **kw):
            calls.append(("host", device, nbytes, kw))
            return _hl_result()
        monkeypatch.setattr(canary, "load", lambda: lib or _Lib())
        monkeypatch.setattr(canary, "cu_check", lambda device=0, **kw: _cu_result())
        monkeypatch.setattr(pace, "pace_check", pace_check)
        monkeypatch.setattr(hostlink, "host_link_check", host_link_check)
        return calls
    return install


# ---- canary.run --------------------------------------------------------------------------
def test_run_without_pace_is_todays_run(fake_run):
    calls = fake_run(RuntimeError("must not be called"))
    out = canary.run(2, 64 << 20, 1, 256)
    assert calls == [] and out["ok"] is True and not MERGED & set(out)
    assert canary.run(2, 64 << 20, 1, 256, pace=False) == out


def test_run_merges_a_clean_pace_check(fake_run):
    calls = fake_run(_pace_result(slow_sites=["xcc1/se0/sh0/cu2/simd3"], slow_xccs=["xcc5"], note=NOTE))
    plain = canary.run(2, 64 << 20, 1, 256)
    out = canary.run(2, 64 << 20, 1, 256, pace=True)
    assert calls == [("pace", 2, {})]  # same device, the check's own defaults
    assert set(out) - set(plain) == MERGED and {k: out[k] for k in plain} == plain
    assert out["ok"] is True and out["error"] == ""  # slowness alone does not fail the run
    assert (out["pace_errors"], out["clock_mhz_min"], out["clock_mhz_max"], out["clock_fraction"]) == (0, 2090.0, 2110.0, 0.87)
    assert (out["xcd_pace_ratio"], out["xcd_mem_ratio"], out["pace_ms"], out["pace_note"]) == (0.99, 0.95, 0.8, NOTE)
    assert out["pace_slow_sites"] == ["xcc1/se0/sh0/cu2/simd3"] and out["pace_slow_xccs"] == ["xcc5"]


def test_run_runs_the_pace_check_before_the_host_link(fake_run):
    calls = fake_run(_pace_result())
    out = canary.run(2, 64 << 20, 1, 256, host_link=True, host_link_bytes=1 << 20, pace=True)
    assert [c[0] for c in calls] == ["pace", "host"] and calls[1] == ("host", 2, 1 << 20, {})
    assert MERGED | HOST_MERGED <= set(out) and out["ok"] is True


def test_run_fails_on_pace_errors_with_the_checks_text(fake_run):
    fake_run(_pace_result(ok=False, error=BAD_TEXT, pace_errors=3, mfma_errors=3))
    out = canary.run(0, 64 << 20, 1, 256, pace=True)
    assert out["ok"] is False and out["error"] == BAD_TEXT and out["pace_errors"] == 3


def test_run_keeps_an_earlier_error_text(fake_run):
    first = b"site check: 5 wrong results at xcc0/se0/sh0/cu1/simd0"
    fake_run(_pace_result(ok=False, error=BAD_TEXT, pace_errors=3), lib=_Lib(ok=0, error=first))
    out = canary.run(0, 64 << 20, 1, 256, pace=True)
    assert out["ok"] is False and out["error"] == first.decode() and out["pace_errors"] == 3


def test_run_fails_when_the_pace_check_raises(fake_run):
    why = "pace_check failed: pace check: pace_mfma: out of memory"
    fake_run(RuntimeError(why))
    out = canary.run(0, 64 << 20, 1, 256, pace=True)
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
    assert canary.run_isolated(3, 128 << 20, 30.0, pace=False)["ok"] is True
    base = child[0]
    assert child[1] == base and not any("pace" in a for a in base)
    canary.run_isolated(3, 128 << 20, 30.0, pace=True)
    assert child[2] == base + ["--with-pace"]
    canary.run_isolated(3, 128 << 20, 30.0, host_link=True, host_link_bytes=1 << 20, pace=True)
    assert child[3] == base + ["--with-host-link", "--host-link-bytes", str(1 << 20), "--with-pace"]
    canary.run_isolated(3, 128 << 20, 30.0, host_link=True)
    assert child[4] == base + ["--with-host-link", "--host-link-bytes", str(64 << 20)]


@pytest.mark.parametrize("result, rc", [(_pace_result(), 0), (_pace_result(slow_xccs=["xcc5"], note=NOTE), 0),
                                        (_pace_result(ok=False, error=BAD_TEXT, pace_errors=3), 1)])
def test_pace_cli_runs_only_that_check(monkeypatch, capsys, result, rc):
    calls = []
    monkeypatch.setattr(pace, "pace_check", lambda device=0, **kw: calls.append((device, kw)) or result)
    monkeypatch.setattr(canary, "run", lambda *a, **kw: pytest.fail("--pace must not start the full run"))
    assert canary.main(["--pace", "--device", "2"]) == rc
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and json.loads(out[0]) == result and calls == [(2, {})]


def test_full_run_cli_passes_pace_only_when_asked(monkeypatch, capsys):
    calls = []
    monkeypatch.setattr(canary, "run", lambda *a, **kw: calls.append((a, kw)) or {"ok": True})
    base = ["--device", "1", "--bytes", "1024", "--passes", "1"]
    assert canary.main(base) == 0
    assert canary.main(base + ["--with-pace"]) == 0
    assert canary.main(base + ["--with-pace", "--with-host-link", "--host-link-bytes", "4096"]) == 0
    capsys.readouterr()
    assert calls[0] == ((1, 1024, 1, 8192), {"host_link": False, "host_link_bytes": 64 << 20})
    assert calls[1] == ((1, 1024, 1, 8192), {"host_link": False, "host_link_bytes": 64 << 20, "pace": True})
    assert calls[2] == ((1, 1024, 1, 8192), {"host_link": True, "host_link_bytes": 4096, "pace": True})


# ---- config ------------------------------------------------------------------------------
def test_config_defaults_and_validation(make_cfg):
    h = make_cfg().health
    assert (h.canaryPace, h.canaryMinClockMhz, h.canaryMinXcdPaceRatio) == (False, 0.0, 0.0)
    h = make_cfg(health={"canaryPace": True, "canaryMinClockMhz": 1500, "canaryMinXcdPaceRatio": 0.8}).health
    assert (h.canaryPace, h.canaryMinClockMhz, h.canaryMinXcdPaceRatio) == (True, 1500, 0.8)
    assert make_cfg(health={"canaryMinXcdPaceRatio": 1}).health.canaryMinXcdPaceRatio == 1
    for bad in (-0.1, 1.01, 2, float("nan")):
        with pytest.raises(config_mod.ConfigError, match="canaryMinXcdPaceRatio"):
            make_cfg(health={"canaryMinXcdPaceRatio": bad})
    for bad in (-1, float("nan")):
        with pytest.raises(config_mod.ConfigError, match="canaryMinClockMhz"):
            make_cfg(health={"canaryMinClockMhz": bad})


# ---- the plugin --------------------------------------------------------------------------
def _full_result(**extra):
    r = {"ok": True, "device": 0, "error": "", "hbm_errors": 0, "mfma_errors": 0, "gemm_errors": 0, "lowp_errors": 0,
         "lds_errors": 0, "write_gbps": 6100.0, "read_gbps": 5900.0, "mfma_tflops": 1800.0}
    r.update(extra)
    return r


def _pace_keys(**extra):
    r = {"pace_errors": 0, "clock_mhz_min": 1210.0, "clock_mhz_max": 2110.0, "clock_fraction": 0.5,
         "xcd_pace_ratio": 0.57, "xcd_mem_ratio": 0.91, "pace_slow_sites": [], "pace_slow_xccs": ["xcc5"],
         "pace_ms": 0.8, "pace_note": NOTE}
    r.update(extra)
    return r


def _host_keys():
    return {"host_read_errors": 0, "host_write_errors": 0, "host_copy_errors": 0, "host_atomic_errors": 0,
            "kernel_read_gbps": 51.0, "kernel_write_gbps": 51.5, "copy_h2d_gbps": 54.0, "copy_d2h_gbps": 21.4, "host_ms": 8.5}


def _samples(m, family):
    return [x for x in m._canary_lines() if x.startswith(family + "{")]


def test_plugin_off_keeps_the_old_call_shape_and_adds_no_metric_lines(make_cfg, monkeypatch):
    seen = []

    def run_isolated(device, nbytes, timeout=120.0):  # the three-parameter fake of the older tests
        seen.append((device, nbytes, timeout))
        return _full_result(device=device)
    monkeypatch.setattr(canary, "run_isolated", run_isolated)
    m = PluginManager(make_cfg(health={"canaryBytes": 1 << 20, "canaryTimeoutS": 7.0, "canaryMinClockMhz": 1500,
                                       "canaryMinXcdPaceRatio": 0.8}))
    res = m._run_canary(0, 0, 3)
    assert seen == [(3, 1 << 20, 7.0)] and res["ok"] is True  # the floors need the check: nothing to judge
    lines = m._canary_lines()
    assert not any("pace" in x or "amdgpu_canary_clock_mhz" in x for x in lines)
    assert {x.split('check="')[1].split('"')[0] for x in _samples(m, "amdgpu_canary_errors")} == \
        {"hbm", "mfma", "gemm", "lowp", "lds"}


@pytest.fixture
def plugin_on(make_cfg, monkeypatch):
    def make(result, **health):
        seen = []

        def run_isolated(device, nbytes, timeout=120.0, **kw):
            seen.append((device, nbytes, timeout, kw))
            return result
        monkeypatch.setattr(canary, "run_isolated", run_isolated)
        cfg = make_cfg(health=dict({"canaryPace": True, "canaryBytes": 1 << 20, "canaryTimeoutS": 7.0}, **health))
        return PluginManager(cfg), seen
    return make


def test_plugin_on_passes_the_option_and_exports_the_keys(plugin_on):
    m, seen = plugin_on(_full_result(**_pace_keys()))
    res = m._run_canary(0, 0, 3)
    assert seen == [(3, 1 << 20, 7.0, {"pace": True})] and res["ok"] is True  # slow, but no floor is set
    lines = m._canary_lines()
    assert 'amdgpu_canary_errors{gpu="0",partition="0",check="pace"} 0' in lines
    assert _samples(m, "amdgpu_canary_clock_mhz") == ['amdgpu_canary_clock_mhz{gpu="0",partition="0",stat="min"} 1210',
                                                      'amdgpu_canary_clock_mhz{gpu="0",partition="0",stat="max"} 2110']
    assert _samples(m, "amdgpu_canary_xcd_pace_ratio") == [
        'amdgpu_canary_xcd_pace_ratio{gpu="0",partition="0",path="clock"} 0.570',
        'amdgpu_canary_xcd_pace_ratio{gpu="0",partition="0",path="mem"} 0.910']
    assert "# TYPE amdgpu_canary_clock_mhz gauge" in lines and "# TYPE amdgpu_canary_xcd_pace_ratio gauge" in lines
    assert not any(x.startswith("amdgpu_canary_host_gbps") for x in lines)
    for name, labels in (("amdgpu_canary_clock_mhz", ("gpu", "partition", "stat")),
                         ("amdgpu_canary_xcd_pace_ratio", ("gpu", "partition", "path"))):
        fam = families.family_of(name)
        assert fam is not None and fam.labels == labels and fam.type == "gauge" and fam in families.OPT_IN_FAMILIES
        assert "`%s`" % name in families.markdown()


def test_plugin_on_with_the_host_link_passes_both_sets_of_keywords(plugin_on):
    m, seen = plugin_on(_full_result(**_pace_keys(), **_host_keys()), canaryHostLink=True, canaryHostLinkBytes=1 << 20)
    assert m._run_canary(0, 0, 3)["ok"] is True
    assert seen == [(3, 1 << 20, 7.0, {"host_link": True, "host_link_bytes": 1 << 20, "pace": True})]
    assert _samples(m, "amdgpu_canary_host_gbps") and _samples(m, "amdgpu_canary_clock_mhz")


def test_plugin_on_an_error_count_fails_the_verdict_with_the_checks_text(plugin_on):
    m, _ = plugin_on(_full_result(ok=False, error=BAD_TEXT, **_pace_keys(pace_errors=3)), canaryMinClockMhz=1)
    res = m._run_canary(1, 0, 0)
    assert res["ok"] is False and res["error"] == BAD_TEXT
    assert 'amdgpu_canary_errors{gpu="1",partition="0",check="pace"} 3' in m._canary_lines()
    assert 'amdgpu_canary_last_ok{gpu="1",partition="0"} 0' in m._canary_lines()


def test_plugin_floors_their_texts_and_their_order(plugin_on):
    floor = "below the canary performance floor: "
    m, _ = plugin_on(_full_result(**_pace_keys()), canaryMinClockMhz=1500)
    res = m._run_canary(0, 0, 0)
    assert res["ok"] is False and res["error"] == floor + "clock 1210 MHz < 1500"
    m, _ = plugin_on(_full_result(**_pace_keys()), canaryMinClockMhz=1210)
    assert m._run_canary(0, 0, 0)["ok"] is True
    m, _ = plugin_on(_full_result(**_pace_keys()), canaryMinXcdPaceRatio=0.8)
    assert m._run_canary(0, 0, 0)["error"] == floor + "slowest XCD at 0.57 of the median < 0.8"
    # the smaller of the two ratios is judged
    m, _ = plugin_on(_full_result(**_pace_keys(xcd_pace_ratio=0.99, xcd_mem_ratio=0.62)), canaryMinXcdPaceRatio=0.8)
    assert m._run_canary(0, 0, 0)["error"] == floor + "slowest XCD at 0.62 of the median < 0.8"
    m, _ = plugin_on(_full_result(**_pace_keys()), canaryMinXcdPaceRatio=0.57)
    assert m._run_canary(0, 0, 0)["ok"] is True
    m, _ = plugin_on(_full_result(**_pace_keys()), canaryMinXcdPaceRatio=0, canaryMinClockMhz=0)
    assert m._run_canary(0, 0, 0)["ok"] is True
    # with the other floors: one text, in the order HBM, MFMA, host link, clock, XCD pace
    m, _ = plugin_on(_full_result(**_pace_keys(), **_host_keys()), canaryHostLink=True, canaryMinHostGbps=40,
                     canaryMinHbmGbps=7000, canaryMinClockMhz=1500, canaryMinXcdPaceRatio=0.8)
    assert m._run_canary(0, 0, 0)["error"] == floor + ("HBM 5900 GB/s < 7000, host link 21 GB/s < 40, clock 1210 MHz < 1500, "
                                                       "slowest XCD at 0.57 of the median < 0.8")
    # a child that reported no pace figures at all (an older tree, a crash before the check) is below any floor
    m, _ = plugin_on(_full_result(), canaryMinClockMhz=1500, canaryMinXcdPaceRatio=0.8)
    assert m._run_canary(0, 0, 0)["error"] == floor + "clock 0 MHz < 1500, slowest XCD at 0.00 of the median < 0.8"


def test_prestart_path_uses_the_same_call(plugin_on):
    m, seen = plugin_on(_full_result(**_pace_keys()))
    m.load_plugins()
    try:
        ids = [d.id for d in m.plugins[0].devices()][:1]
        assert m._prestart_check(ids) == ""
        assert seen and all(kw == {"pace": True} for *_, kw in seen)
    finally:
        m.exporter.stop()
        m.monitor.stop()
