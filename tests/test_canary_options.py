"""The table of the canary's opt-in checks (``canary.OPTIONAL_CHECKS``) against everything that
reads it, for every subset of the checks: the child's command line and what ``main`` makes of
it, what ``run`` merges and in which order, the verdict rule, the plugin's keywords and the
metric labels.  And the table of the HIP libraries in ``_build``.  No GPU: the checks are fakes."""
import itertools
import json
import subprocess
import time

import pytest

from k8s_gpu_device_plugin_amd import _build
from k8s_gpu_device_plugin_amd.ops import canary, hostlink, ldspath, pace
from k8s_gpu_device_plugin_amd.plugin.manager import PluginManager

CHECKS = canary.OPTIONAL_CHECKS
SUBSETS = [c for n in range(len(CHECKS) + 1) for c in itertools.combinations(CHECKS, n)]
# what each check merges into run()'s result, in the order run() has always merged it
MERGED = {
    "lds_path": ["ldspath_errors", "lds_width_errors", "lds_dma_errors", "lds_atomic_errors", "lane_errors", "tr_errors",
                 "ldspath_ms", "ldspath_bad_sites"],
    "pace": ["pace_errors", "clock_mhz_min", "clock_mhz_max", "clock_fraction", "xcd_pace_ratio", "xcd_mem_ratio",
             "pace_slow_sites", "pace_slow_xccs", "pace_ms", "pace_note"],
    "host_link": ["host_read_errors", "host_write_errors", "host_copy_errors", "host_atomic_errors", "kernel_read_gbps",
                  "kernel_write_gbps", "copy_h2d_gbps", "copy_d2h_gbps", "host_ms"],
}
# the (label, key) pairs of amdgpu_canary_errors as PluginManager._canary_lines listed them before the table
ERROR_LABELS = (("hbm", "hbm_errors"), ("mfma", "mfma_errors"), ("gemm", "gemm_errors"),
                ("lowp", "lowp_errors"), ("lds", "lds_errors"), ("site", "site_errors"),
                ("unreached", "cus_unreached"), ("l2", "l2_errors"), ("xcd", "xcd_errors"),
                ("atomic", "atomic_errors"), ("xcd_unreached", "xcd_pairs_unreached"),
                ("reg", "reg_errors"), ("l1", "l1_errors"), ("host_read", "host_read_errors"),
                ("host_write", "host_write_errors"), ("host_copy", "host_copy_errors"),
                ("host_atomic", "host_atomic_errors"), ("pace", "pace_errors"),
                ("lds_width", "lds_width_errors"), ("lds_dma", "lds_dma_errors"),
                ("lds_atomic", "lds_atomic_errors"), ("lane", "lane_errors"), ("lds_tr", "tr_errors"))
RESULTS = {
    "lds_path": {"ldspath_errors": 0, "lds_errors": 11, "dma_errors": 12, "lds_atomic_errors": 13, "lane_errors": 14,
                 "tr_errors": 15, "ms": 0.6, "bad_sites": ["xcc0/se0/sh0/cu1/simd0"], "error": "", "ok": True},
    "pace": {"pace_errors": 0, "clock_mhz_min": 2090.0, "clock_mhz_max": 2110.0, "clock_fraction": 0.87,
             "xcd_pace_ratio": 0.99, "xcd_mem_ratio": 0.95, "slow_sites": ["xcc1/se0/sh0/cu0/simd0"], "slow_xccs": ["xcc1"],
             "ms": 0.8, "note": "pace: a note", "error": "", "ok": True},
    "host_link": {"read_errors": 1, "write_errors": 2, "h2d_errors": 3, "d2h_errors": 4, "atomic_errors": 5,
                  "kernel_read_gbps": 51.0, "kernel_write_gbps": 51.5, "copy_h2d_gbps": 54.0, "copy_d2h_gbps": 56.0,
                  "ms": 8.5, "error": "", "ok": True},
}
FUNCTIONS = {"lds_path": (ldspath, "ldspath_check"), "pace": (pace, "pace_check"), "host_link": (hostlink, "host_link_check")}


def _ids(subset):
    return "+".join(c.keyword for c in subset) or "none"


class _Lib:
    """Stands in for the canary library's amdgpu_canary_run."""

    def __init__(self, ok=1, error=b""):
        self.ok, self.error = ok, error

    def amdgpu_canary_run(self, device, nbytes, passes, iters, ref):
        r = ref._obj
        r.ok, r.device, r.error, r.num_cus = self.ok, device, self.error, 256
        return 0 if self.ok else 1


@pytest.fixture
def fake_checks(monkeypatch):
    """canary.run over a fake library and a fake CU check; every optional check is a fake that
    records its call and returns ``RESULTS`` (or raises what ``failing`` names for it)."""
    calls = []

    def install(failing=None, lib=None):
        def fake(keyword):
            def check(device=0, *args, **kw):
                calls.append((keyword, device, args, kw))
                if failing and keyword in failing:
                    raise failing[keyword]
                return dict(RESULTS[keyword])
            return check
        for keyword, (mod, name) in FUNCTIONS.items():
            monkeypatch.setattr(mod, name, fake(keyword))
        monkeypatch.setattr(canary, "load", lambda: lib or _Lib())
        monkeypatch.setattr(canary, "cu_check", lambda device=0, **kw: {
            "vgpr_errors": 0, "agpr_errors": 0, "l1_errors": 0, "l1_fill_errors": 0, "unlocated_errors": 0, "moved": 0,
            "regs_marched": 480, "reg_ms": 0.25, "l1_ms": 0.5, "bad_sites": [], "error": ""})
        return calls
    return install


def test_the_table_is_the_three_checks_in_merge_order():
    assert [c.keyword for c in CHECKS] == ["lds_path", "pace", "host_link"]
    assert [c.stem for c in CHECKS] == ["lds-path", "pace", "host-link"]
    assert [(c.module, c.function) for c in CHECKS] == [(m.__name__.rsplit(".", 1)[1], f) for m, f in
                                                        (FUNCTIONS[c.keyword] for c in CHECKS)]
    assert [[a[0] for a in c.args] for c in CHECKS] == [[], [], ["host_link_bytes"]]
    assert [c.switch for c in CHECKS] == ["canaryLdsPath", "canaryPace", "canaryHostLink"]
    assert {c.keyword: [k for k, _ in c.keys] for c in CHECKS} == MERGED
    # the names other modules read are views of the table
    assert canary.LDS_PATH_KEYS == CHECKS[0].keys
    assert canary.PACE_KEYS == tuple(MERGED["pace"][:6])
    assert canary.HOST_LINK_RATES == ("kernel_read_gbps", "kernel_write_gbps", "copy_h2d_gbps", "copy_d2h_gbps")


@pytest.mark.parametrize("subset", SUBSETS, ids=_ids)
def test_the_childs_command_line_asks_main_for_exactly_that_subset(subset, monkeypatch, capsys):
    """run_isolated's command line, parsed by main, reaches run with the subset's keywords on, its
    arguments as given, and nothing else but the host link's two keywords, which main has always
    spelt out (off, with the default size) when the check was not asked for."""
    cmds, calls = [], []

    def child(cmd, **kw):
        cmds.append(cmd)
        return subprocess.CompletedProcess(cmd, 0, stdout=json.dumps({"ok": True, "device": 3}) + "\n", stderr="")
    monkeypatch.setattr(canary.subprocess, "run", child)
    monkeypatch.setattr(canary, "run", lambda *a, **kw: calls.append((a, kw)) or {"ok": True})
    asked = {c.keyword: True for c in subset}
    if "host_link" in asked:
        asked["host_link_bytes"] = 3 << 20
    assert canary.run_isolated(3, 128 << 20, 30.0, **asked)["ok"] is True
    cmd = cmds[0]
    assert cmd[1:3] == ["-m", "k8s_gpu_device_plugin_amd.ops.canary"]
    flags = {a for a in cmd[3:] if a.startswith("--")}
    assert flags == {"--device", "--bytes", "--passes"} | {"--with-" + c.stem for c in subset} | \
        {"--" + a[0].replace("_", "-") for c in subset for a in c.args}
    assert canary.main(cmd[3:]) == 0
    capsys.readouterr()
    (args, kw), = calls
    assert args == (3, 128 << 20, 1, 8192)
    off = {} if "host_link" in asked else {"host_link": False, "host_link_bytes": 64 << 20}
    assert kw == dict(asked, **off)


@pytest.mark.parametrize("subset", SUBSETS, ids=_ids)
def test_run_merges_exactly_that_subset_in_table_order(subset, fake_checks):
    calls = fake_checks()
    plain = canary.run(2, 64 << 20, 1, 256)
    assert calls == []
    asked = {c.keyword: True for c in subset}
    out = canary.run(2, 64 << 20, 1, 256, host_link_bytes=3 << 20, **asked)
    assert [c[0] for c in calls] == [c.keyword for c in subset]  # table order, whatever order they were named in
    assert all(c[1] == 2 and c[3] == {} for c in calls)
    assert [c[2] for c in calls] == [((3 << 20,) if c.keyword == "host_link" else ()) for c in subset]
    assert list(out) == list(plain) + [k for c in subset for k in MERGED[c.keyword]]
    assert {k: out[k] for k in plain} == plain and out["ok"] is True and out["error"] == ""
    if "lds_path" in asked:
        assert (out["lds_width_errors"], out["lds_dma_errors"], out["ldspath_ms"]) == (11, 12, 0.6)
        assert out["ldspath_bad_sites"] == ["xcc0/se0/sh0/cu1/simd0"] and out["lds_errors"] == 0  # lds_march's own count
    if "pace" in asked:
        assert (out["pace_slow_sites"], out["pace_slow_xccs"]) == (["xcc1/se0/sh0/cu0/simd0"], ["xcc1"])
        assert (out["pace_ms"], out["pace_note"], out["clock_mhz_min"]) == (0.8, "pace: a note", 2090.0)
    if "host_link" in asked:
        assert (out["host_read_errors"], out["host_write_errors"], out["host_copy_errors"], out["host_atomic_errors"]) == \
            (1, 2, 3 + 4, 5)
        assert (out["copy_d2h_gbps"], out["host_ms"]) == (56.0, 8.5)


@pytest.mark.parametrize("subset", SUBSETS[1:], ids=_ids)
def test_a_check_that_raises_clears_ok_and_sets_error_only_if_it_was_empty(subset, fake_checks):
    asked = {c.keyword: True for c in subset}
    failing = {c.keyword: RuntimeError("%s failed: out of memory" % c.function) for c in subset}
    fake_checks(failing)
    out = canary.run(0, 64 << 20, 1, 256, **asked)
    assert out["ok"] is False and out["error"] == "%s failed: out of memory" % subset[0].function  # the first one's
    assert not {k for keys in MERGED.values() for k in keys} & set(out) and out["reg_errors"] == 0
    first = b"site check: 5 wrong results at xcc0/se0/sh0/cu1/simd0"
    fake_checks(failing, lib=_Lib(ok=0, error=first))
    out = canary.run(0, 64 << 20, 1, 256, **asked)
    assert out["ok"] is False and out["error"] == first.decode()
    # OSError is caught like RuntimeError (a library that does not load); anything else is a bug and propagates
    fake_checks({subset[-1].keyword: OSError("cannot open shared object file")})
    out = canary.run(0, 64 << 20, 1, 256, **asked)
    assert out["ok"] is False and out["error"] == "cannot open shared object file"
    every = {k for keys in MERGED.values() for k in keys}
    assert [k for k in out if k in every] == [k for c in subset[:-1] for k in MERGED[c.keyword]]  # the others still merge
    fake_checks({subset[0].keyword: KeyError("ms")})
    with pytest.raises(KeyError):
        canary.run(0, 64 << 20, 1, 256, **asked)


@pytest.mark.parametrize("keyword", list(MERGED))
def test_a_check_that_reports_errors_fails_the_run_with_its_text(keyword, fake_checks, monkeypatch):
    fake_checks()
    monkeypatch.setitem(RESULTS, keyword, dict(RESULTS[keyword], ok=False, error="its own text"))
    out = canary.run(0, 64 << 20, 1, 256, **{keyword: True})
    assert out["ok"] is False and out["error"] == "its own text" and set(MERGED[keyword]) <= set(out)


@pytest.mark.parametrize("subset", SUBSETS, ids=_ids)
def test_the_plugin_passes_the_subsets_keywords_from_health(subset, make_cfg, monkeypatch):
    seen = []

    def run_isolated(device, nbytes, timeout=120.0, **kw):
        seen.append((device, nbytes, timeout, kw))
        return {"ok": True, "device": device, "error": ""}
    monkeypatch.setattr(canary, "run_isolated", run_isolated)
    health = {c.switch: True for c in subset}
    health.update({"canaryBytes": 1 << 20, "canaryTimeoutS": 7.0, "canaryHostLinkBytes": 2 << 20})
    m = PluginManager(make_cfg(health=health))
    m._run_canary(0, 0, 3)
    want = {c.keyword: True for c in subset}
    if "host_link" in want:
        want["host_link_bytes"] = 2 << 20
    assert seen == [(3, 1 << 20, 7.0, want)]


def test_the_metric_labels_are_the_old_list_in_the_old_order(make_cfg):
    m = PluginManager(make_cfg())
    result = {key: i for i, (_, key) in enumerate(ERROR_LABELS)}
    m.canary_results[(0, 1)] = (time.time(), dict(result, ok=True))
    got = [x for x in m._canary_lines() if x.startswith("amdgpu_canary_errors{")]
    assert got == ['amdgpu_canary_errors{gpu="0",partition="1",check="%s"} %d' % (label, i)
                   for i, (label, _) in enumerate(ERROR_LABELS)]
    assert len(ERROR_LABELS) == 23 and [p for c in reversed(CHECKS) for p in c.errors] == list(ERROR_LABELS[13:])
    # a run without the optional checks carries none of their labels
    base = {key: 0 for _, key in ERROR_LABELS[:13]}
    m.canary_results[(0, 1)] = (time.time(), dict(base, ok=True))
    got = [x.split('check="')[1].split('"')[0] for x in m._canary_lines() if x.startswith("amdgpu_canary_errors{")]
    assert got == [label for label, _ in ERROR_LABELS[:13]]


# ---- the build table ---------------------------------------------------------------------
def test_hip_libs_names_the_four_libraries():
    assert [row["name"] for row in _build.HIP_LIBS] == ["canary", "hostlink", "pace", "ldspath"]
    assert [row["lib"] for row in _build.HIP_LIBS] == [_build.CANARY_LIB, _build.HOSTLINK_LIB, _build.PACE_LIB,
                                                       _build.LDSPATH_LIB]
    assert [row["lib"] for row in _build.HIP_LIBS] == [canary.LIB_PATH, hostlink.LIB_PATH, pace.LIB_PATH, ldspath.LIB_PATH]
    for row, sources, headers in zip(_build.HIP_LIBS,
                                     (_build.CANARY_SOURCES, _build.HOSTLINK_SOURCES, _build.PACE_SOURCES,
                                      _build.LDSPATH_SOURCES),
                                     (_build.CANARY_HEADERS, _build.HOSTLINK_HEADERS, _build.PACE_HEADERS,
                                      _build.LDSPATH_HEADERS)):
        assert row["sources"] == sources and row["headers"] == headers
        assert set(row) == {"name", "lib", "sources", "headers"}
    assert all(callable(getattr(_build, "build_" + row["name"])) for row in _build.HIP_LIBS)


@pytest.mark.parametrize("entry", ["build_all", "main"])
def test_every_hip_library_is_built_once(entry, monkeypatch, capsys):
    """build_all() and the command line go through the table: one hipcc line per library, in
    table order, each written to <lib>.tmp and then renamed, and one "built" line each."""
    ran, renamed = [], []
    monkeypatch.setattr(_build, "build_native", lambda **kw: None)
    monkeypatch.setattr(_build, "build_bench", lambda **kw: None)
    monkeypatch.setattr(_build, "hipcc_path", lambda: "/nowhere/hipcc")
    monkeypatch.setattr(_build, "_run", lambda cmd, what: ran.append((cmd, what)))
    monkeypatch.setattr(_build.os, "replace", lambda a, b: renamed.append((a, b)))
    if entry == "build_all":
        _build.build_all(force=True)
    else:
        assert _build.main(["--force"]) == 0
    assert [what for _, what in ran] == ["hipcc canary", "hipcc hostlink", "hipcc pace", "hipcc ldspath"]
    for (cmd, _), row in zip(ran, _build.HIP_LIBS):
        assert cmd == ["/nowhere/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wall", "-o",
                       row["lib"] + ".tmp"] + row["sources"]
    assert renamed == [(row["lib"] + ".tmp", row["lib"]) for row in _build.HIP_LIBS]
    assert capsys.readouterr().out.splitlines() == [
        "built k8s_gpu_device_plugin_amd/ops/libamdgpu_canary.so",
        "built k8s_gpu_device_plugin_amd/ops/hostlink/libamdgpu_hostlink.so",
        "built k8s_gpu_device_plugin_amd/ops/pace/libamdgpu_pace.so",
        "built k8s_gpu_device_plugin_amd/ops/ldspath/libamdgpu_ldspath.so"]


def test_an_up_to_date_library_is_left_alone_and_no_canary_skips_them_all(monkeypatch):
    ran = []
    monkeypatch.setattr(_build, "build_native", lambda **kw: None)
    monkeypatch.setattr(_build, "build_bench", lambda **kw: None)
    monkeypatch.setattr(_build, "hipcc_path", lambda: "/nowhere/hipcc")
    monkeypatch.setattr(_build, "_run", lambda cmd, what: ran.append(what))
    monkeypatch.setattr(_build, "_stale", lambda target, deps: False)
    _build.build_all()
    assert _build.main(["--no-canary", "--force"]) == 0
    assert ran == []
    monkeypatch.setattr(_build, "hipcc_path", lambda: None)
    with pytest.raises(RuntimeError, match="hipcc not found"):
        _build.build_pace()
