"""The host-link check above the library, no GPU: how ``canary.run`` merges it, the flags
``run_isolated`` and the CLI pass on, the config keys and their validation, the plugin's call
shape with the option off and on, the performance floor and the metric lines."""
import json
import subprocess
import time

import pytest

from k8s_gpu_device_plugin_amd import config as config_mod
from k8s_gpu_device_plugin_amd.metrics import families
from k8s_gpu_device_plugin_amd.ops import canary, hostlink
from k8s_gpu_device_plugin_amd.plugin.manager import PluginManager

MERGED = {"host_read_errors", "host_write_errors", "host_copy_errors", "host_atomic_errors", "kernel_read_gbps",
          "kernel_write_gbps", "copy_h2d_gbps", "copy_d2h_gbps", "host_ms"}
READ_TEXT = "host read check: 3 wrong words read on xcc5 (first at offset 0x1a40)"


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


def _hl_result(**extra):
    r = {"read_errors": 0, "write_errors": 0, "h2d_errors": 0, "d2h_errors": 0, "atomic_errors": 0,
         "kernel_read_gbps": 51.0, "kernel_write_gbps": 51.5, "copy_h2d_gbps": 54.0, "copy_d2h_gbps": 56.0,
         "ms": 8.5, "error": "", "ok": True}
    r.update(extra)
    return r


@pytest.fixture
def fake_run(monkeypatch):
    """canary.run over a fake library, a fake CU check and a fake host-link check."""
    calls = []

    def install(hl, lib=None):
        def host_link_check(device=0, nbytes=64 << 20, **kw):
            calls.append((device, nbytes, kw))
            if isinstance(hl, Exception):
                raise hl
            return hl
        monkeypatch.setattr(canary, "load", lambda: lib or _Lib())
        monkeypatch.setattr(canary, "cu_check", lambda device=0, **kw: _cu_result())
        monkeypatch.setattr(hostlink, "host_link_check", host_link_check)
        return calls
    return install


# ---- canary.run --------------------------------------------------------------------------
def test_run_without_host_link_is_todays_run(fake_run):
    calls = fake_run(RuntimeError("must not be called"))
    out = canary.run(2, 64 << 20, 1, 256)
    assert calls == [] and out["ok"] is True and not MERGED & set(out)
    assert canary.run(2, 64 << 20, 1, 256, host_link=False) == out


def test_run_merges_a_clean_host_link_check(fake_run):
    calls = fake_run(_hl_result())
    plain = canary.run(2, 64 << 20, 1, 256)
    out = canary.run(2, 64 << 20, 1, 256, host_link=True, host_link_bytes=1 << 20)
    assert calls == [(2, 1 << 20, {})]  # same device, the bytes asked for, the check's own defaults
    assert set(out) - set(plain) == MERGED and {k: out[k] for k in plain} == plain
    assert out["ok"] is True and out["error"] == "" and out["host_ms"] == 8.5
    assert (out["kernel_read_gbps"], out["kernel_write_gbps"], out["copy_h2d_gbps"], out["copy_d2h_gbps"]) == \
        (51.0, 51.5, 54.0, 56.0)
    canary.run(2, 64 << 20, 1, 256, host_link=True)
    assert calls[-1] == (2, 64 << 20, {})


@pytest.mark.parametrize("counts, merged", [
    (dict(read_errors=3), dict(host_read_errors=3)), (dict(write_errors=2), dict(host_write_errors=2)),
    (dict(h2d_errors=1), dict(host_copy_errors=1)), (dict(d2h_errors=4), dict(host_copy_errors=4)),
    (dict(h2d_errors=1, d2h_errors=2), dict(host_copy_errors=3)), (dict(atomic_errors=4), dict(host_atomic_errors=4))])
def test_run_fails_on_any_host_link_error(fake_run, counts, merged):
    fake_run(_hl_result(ok=False, error=READ_TEXT, **counts))
    out = canary.run(0, 64 << 20, 1, 256, host_link=True)
    assert out["ok"] is False and out["error"] == READ_TEXT
    want = {"host_read_errors": 0, "host_write_errors": 0, "host_copy_errors": 0, "host_atomic_errors": 0, **merged}
    assert {k: out[k] for k in want} == want


def test_run_keeps_an_earlier_error_text(fake_run):
    first = b"site check: 5 wrong results at xcc0/se0/sh0/cu1/simd0"
    fake_run(_hl_result(ok=False, error=READ_TEXT, read_errors=3), lib=_Lib(ok=0, error=first))
    out = canary.run(0, 64 << 20, 1, 256, host_link=True)
    assert out["ok"] is False and out["error"] == first.decode() and out["host_read_errors"] == 3


def test_run_fails_when_the_host_link_check_raises(fake_run):
    why = "host_link_check failed: host link check: hipHostMalloc of the pinned buffer: out of memory"
    fake_run(RuntimeError(why))
    out = canary.run(0, 64 << 20, 1, 256, host_link=True)
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


def test_run_isolated_adds_the_flags_only_when_asked(child):
    assert canary.run_isolated(3, 128 << 20, 30.0)["ok"] is True
    assert canary.run_isolated(3, 128 << 20, 30.0, host_link=False, host_link_bytes=1 << 20)["ok"] is True
    base = child[0]
    assert child[1] == base and not any("host-link" in a for a in base)
    assert base[base.index("--device") + 1] == "3" and base[base.index("--bytes") + 1] == str(128 << 20)
    canary.run_isolated(3, 128 << 20, 30.0, host_link=True, host_link_bytes=1 << 20)
    assert child[2] == base + ["--with-host-link", "--host-link-bytes", str(1 << 20)]
    canary.run_isolated(3, 128 << 20, 30.0, host_link=True)
    assert child[3] == base + ["--with-host-link", "--host-link-bytes", str(64 << 20)]


@pytest.mark.parametrize("result, rc", [(_hl_result(), 0), (_hl_result(ok=False, error=READ_TEXT, read_errors=3), 1),
                                        (_hl_result(ok=False, atomic_errors=1, error="host atomic check: ..."), 1)])
def test_host_link_cli_runs_only_that_check(monkeypatch, capsys, result, rc):
    calls = []
    monkeypatch.setattr(hostlink, "host_link_check", lambda device=0, nbytes=64 << 20, **kw: calls.append(
        (device, nbytes, kw)) or result)
    monkeypatch.setattr(canary, "run", lambda *a, **kw: pytest.fail("--host-link must not start the full run"))
    assert canary.main(["--host-link", "--device", "2", "--host-link-bytes", str(1 << 20)]) == rc
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and json.loads(out[0]) == result and calls == [(2, 1 << 20, {})]
    assert canary.main(["--host-link"]) == rc and calls[-1] == (0, 64 << 20, {})


def test_full_run_cli_passes_the_host_link_options(monkeypatch, capsys):
    calls = []
    monkeypatch.setattr(canary, "run", lambda *a, **kw: calls.append((a, kw)) or {"ok": True})
    assert canary.main(["--device", "1", "--bytes", "1024", "--passes", "1"]) == 0
    assert canary.main(["--device", "1", "--bytes", "1024", "--passes", "1", "--with-host-link", "--host-link-bytes",
                        "4096"]) == 0
    capsys.readouterr()
    assert calls[0] == ((1, 1024, 1, 8192), {"host_link": False, "host_link_bytes": 64 << 20})
    assert calls[1] == ((1, 1024, 1, 8192), {"host_link": True, "host_link_bytes": 4096})


# ---- config ------------------------------------------------------------------------------
def test_config_defaults_and_validation(make_cfg):
    h = make_cfg().health
    assert (h.canaryHostLink, h.canaryHostLinkBytes, h.canaryMinHostGbps) == (False, 64 << 20, 0.0)
    h = make_cfg(health={"canaryHostLink": True, "canaryHostLinkBytes": 16, "canaryMinHostGbps": 40}).health
    assert (h.canaryHostLink, h.canaryHostLinkBytes, h.canaryMinHostGbps) == (True, 16, 40)
    for bad in (0, -16, 8, 24, (64 << 20) + 8):
        with pytest.raises(config_mod.ConfigError, match="canaryHostLinkBytes"):
            make_cfg(health={"canaryHostLinkBytes": bad})
    with pytest.raises(config_mod.ConfigError, match="canaryMinHostGbps"):
        make_cfg(health={"canaryMinHostGbps": -1})


# ---- the plugin --------------------------------------------------------------------------
def _full_result(**extra):
    r = {"ok": True, "device": 0, "error": "", "hbm_errors": 0, "mfma_errors": 0, "gemm_errors": 0, "lowp_errors": 0,
         "lds_errors": 0, "write_gbps": 6100.0, "read_gbps": 5900.0, "mfma_tflops": 1800.0}
    r.update(extra)
    return r


def _host_keys(**extra):
    r = {"host_read_errors": 0, "host_write_errors": 0, "host_copy_errors": 0, "host_atomic_errors": 0,
         "kernel_read_gbps": 51.0, "kernel_write_gbps": 51.5, "copy_h2d_gbps": 54.0, "copy_d2h_gbps": 21.4, "host_ms": 8.5}
    r.update(extra)
    return r


def _samples(m, family):
    return [x for x in m._canary_lines() if x.startswith(family + "{")]


def test_plugin_off_keeps_the_old_call_shape_and_adds_no_metric_lines(make_cfg, monkeypatch):
    seen = []

    def run_isolated(device, nbytes, timeout=120.0):  # the three-parameter fake of the older tests
        seen.append((device, nbytes, timeout))
        return _full_result(device=device)
    monkeypatch.setattr(canary, "run_isolated", run_isolated)
    m = PluginManager(make_cfg(health={"canaryBytes": 1 << 20, "canaryTimeoutS": 7.0, "canaryMinHostGbps": 40}))
    res = m._run_canary(0, 0, 3)
    assert seen == [(3, 1 << 20, 7.0)] and res["ok"] is True  # the floor needs the check: nothing to judge
    lines = m._canary_lines()
    assert not any("host" in x for x in lines)
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
        cfg = make_cfg(health=dict({"canaryHostLink": True, "canaryBytes": 1 << 20, "canaryTimeoutS": 7.0}, **health))
        return PluginManager(cfg), seen
    return make


def test_plugin_on_passes_the_options_and_exports_the_keys(plugin_on):
    m, seen = plugin_on(_full_result(**_host_keys()), canaryHostLinkBytes=1 << 20)
    res = m._run_canary(0, 0, 3)
    assert seen == [(3, 1 << 20, 7.0, {"host_link": True, "host_link_bytes": 1 << 20})] and res["ok"] is True
    errors = {x.split('check="')[1].split('"')[0]: int(x.rsplit(" ", 1)[1]) for x in _samples(m, "amdgpu_canary_errors")}
    assert {k: v for k, v in errors.items() if k.startswith("host_")} == \
        {"host_read": 0, "host_write": 0, "host_copy": 0, "host_atomic": 0}
    rates = {x.split('path="')[1].split('"')[0]: float(x.rsplit(" ", 1)[1]) for x in _samples(m, "amdgpu_canary_host_gbps")}
    assert rates == {"kernel_read": 51.0, "kernel_write": 51.5, "copy_h2d": 54.0, "copy_d2h": 21.4}
    assert all(x.startswith('amdgpu_canary_host_gbps{gpu="0",partition="0",path="') for x in
               _samples(m, "amdgpu_canary_host_gbps"))
    lines = m._canary_lines()
    assert "# TYPE amdgpu_canary_host_gbps gauge" in lines
    fam = families.family_of("amdgpu_canary_host_gbps")
    assert fam is not None and fam.labels == ("gpu", "partition", "path") and fam.type == "gauge"
    assert "`amdgpu_canary_host_gbps`" in families.markdown()


def test_plugin_on_an_error_count_fails_the_verdict_with_the_checks_text(plugin_on):
    m, _ = plugin_on(_full_result(ok=False, error=READ_TEXT, **_host_keys(host_read_errors=3)), canaryMinHostGbps=1)
    res = m._run_canary(1, 0, 0)
    assert res["ok"] is False and res["error"] == READ_TEXT
    assert 'amdgpu_canary_errors{gpu="1",partition="0",check="host_read"} 3' in m._canary_lines()
    assert 'amdgpu_canary_last_ok{gpu="1",partition="0"} 0' in m._canary_lines()


def test_plugin_host_floor_judges_the_slowest_of_the_four_rates(plugin_on):
    m, _ = plugin_on(_full_result(**_host_keys()), canaryMinHostGbps=40)
    res = m._run_canary(0, 0, 0)
    assert res["ok"] is False and res["error"] == "below the canary performance floor: host link 21 GB/s < 40"
    m, _ = plugin_on(_full_result(**_host_keys()), canaryMinHostGbps=21)
    assert m._run_canary(0, 0, 0)["ok"] is True
    m, _ = plugin_on(_full_result(**_host_keys()), canaryMinHostGbps=0)
    assert m._run_canary(0, 0, 0)["ok"] is True
    # with the other floors: one text, in the order HBM, MFMA, host link
    m, _ = plugin_on(_full_result(**_host_keys()), canaryMinHostGbps=40, canaryMinHbmGbps=7000)
    assert m._run_canary(0, 0, 0)["error"] == \
        "below the canary performance floor: HBM 5900 GB/s < 7000, host link 21 GB/s < 40"
    # a child that reported no rates at all (an older tree, a crash before the check) is below any floor
    m, _ = plugin_on(_full_result(), canaryMinHostGbps=40)
    assert m._run_canary(0, 0, 0)["error"] == "below the canary performance floor: host link 0 GB/s < 40"


def test_prestart_path_uses_the_same_call(plugin_on):
    m, seen = plugin_on(_full_result(**_host_keys()))
    m.load_plugins()
    try:
        ids = [d.id for d in m.plugins[0].devices()][:1]
        assert m._prestart_check(ids) == ""
        assert seen and all(kw == {"host_link": True, "host_link_bytes": 64 << 20} for *_, kw in seen)
    finally:
        m.exporter.stop()
        m.monitor.stop()
