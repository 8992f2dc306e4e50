"""Pace check of the gfx950 canary (``ops/pace/pace.hip``) on a real MI355X: the clock every
XCD ran and the cycles every SIMD needed per MFMA, measured inside the kernels, reach every CU
and SIMD with zero errors; injected extra work is found at exactly the XCD or the sites that
did it; an injected wrong result is an error at its site.

What a healthy device measures (``docs/CANARY.md``, "Pace", Measured) is not asserted here:
the only bounds are the ones arithmetic gives, a clock no higher than the part's maximum and no
fewer than 32 cycles per MFMA."""
import statistics

import pytest

pytestmark = pytest.mark.gpu

MFMA_ISSUE_CYCLES = 32  # v_mfma_f32_32x32x16_bf16 back to back on one SIMD; stamps only add


def _check(**kw):
    from k8s_gpu_device_plugin_amd.ops import pace
    return pace.pace_check(**kw)


@pytest.fixture(scope="module")
def healthy():
    return _check()


def _xcc(site):
    return site.split("/", 1)[0]


def _slow_through_sites(r, slow_ratio):
    """The slow set recomputed from ``sites`` (``slow_sites`` lists only the first 16)."""
    timed = {s: v["cycles_per_mfma"] for s, v in r["sites"].items() if v["cycles_per_mfma"] > 0}
    median = statistics.median(timed.values())
    return {s for s, c in timed.items() if c > slow_ratio * median}


def test_healthy_defaults_cover_every_cu_and_simd(healthy):
    r = healthy
    print("pace: launches %d, waves %d, moved %d, mfma %.3f ms, fill %.3f ms, mem %.3f ms, iters %d, slice %d KiB; "
          "clock %.0f..%.0f MHz of %.0f (fraction %.3f), cycles per MFMA %.2f / %.2f / %.2f, ratios clock %.4f mem %.4f; "
          "slow sites %d, slow xccs %s, note %r"
          % (r["launches"], r["waves"], r["moved"], r["mfma_ms"], r["fill_ms"], r["mem_ms"], r["iters"], r["slice_kb"],
             r["clock_mhz_min"], r["clock_mhz_max"], r["clock_max_mhz"], r["clock_fraction"], r["cycles_per_mfma_min"],
             r["cycles_per_mfma_median"], r["cycles_per_mfma_max"], r["xcd_pace_ratio"], r["xcd_mem_ratio"],
             r["n_slow"], r["slow_xccs"], r["note"]))
    for x, v in sorted(r["xccs"].items()):
        print("  %-5s clock %7.1f MHz  cycles/MFMA %6.2f  %7.2f us/MiB  waves %4d  blocks %3d  bad %d"
              % (x, v["clock_mhz"], v["cycles_per_mfma"], v["us_per_mib"], v["waves"], v["blocks"], v["bad"]))
    assert r["pace_errors"] == 0 and r["error"] == "" and r["ok"] is True
    assert (r["mfma_errors"], r["mem_errors"], r["unlocated_errors"]) == (0, 0, 0) and r["bad_sites"] == []
    assert r["cus_reached"] == r["cus_expected"] > 0
    assert r["simds_reached"] == 4 * r["cus_reached"]
    assert 1 <= r["launches"] <= 4
    assert r["waves"] + r["moved"] == r["launches"] * 2 * r["cus_expected"] * 4
    assert sum(s["waves"] for s in r["sites"].values()) == r["waves"]
    assert len(r["wave_sites"]) == 2 * r["cus_expected"] * 4 and len(r["mem_wave_sites"]) == r["cus_expected"] * 4
    assert r["mem_waves"] + r["mem_moved"] == r["cus_expected"] * 4
    assert r["tick_mhz"] > 0 and r["clock_max_mhz"] > 0
    for x, v in r["xccs"].items():
        # above the part's maximum means wrong arithmetic; 2 % is the counter granularity at this run length
        assert 0 < v["clock_mhz"] <= 1.02 * r["clock_max_mhz"], (x, v)
    for s, v in r["sites"].items():
        assert v["cycles_per_mfma"] >= MFMA_ISSUE_CYCLES, (s, v)
    assert r["clock_mhz_min"] == min(v["clock_mhz"] for v in r["xccs"].values())
    assert r["clock_mhz_max"] == max(v["clock_mhz"] for v in r["xccs"].values())
    assert 0 < r["xcd_pace_ratio"] <= 1.0 and 0 < r["xcd_mem_ratio"] <= 1.0
    assert r["mfma_ms"] > 0 and r["mem_ms"] > 0 and r["ms"] >= r["mfma_ms"] + r["mem_ms"]


def test_injected_slow_xcc_is_found_in_both_stages(healthy):
    """Every wave on one XCD does four times the work it records.  Margin: 4 x the work, less
    what the loop's prologue and the stamps cost, is at least 3 x; slow_ratio 2.0 is below that."""
    xccs = sorted(healthy["xccs"])
    inj = xccs[len(xccs) // 2]
    r = _check(blocks=16, iters=256, slice_kb=64, slow_ratio=2.0, inject="slow_xcc", inject_xcc=int(inj[3:]),
               inject_factor=4)
    print("slow_xcc %s: %s" % (inj, {x: (round(v["cycles_per_mfma"], 1), round(v["us_per_mib"], 1), round(v["clock_mhz"]))
                                     for x, v in sorted(r["xccs"].items())}))
    assert r["pace_errors"] == 0 and r["error"] == "" and r["launches"] == 1
    assert r["waves"] + r["moved"] == 64
    on_it = {s for s in r["sites"] if _xcc(s) == inj}
    assert on_it, "16 workgroups did not reach %s" % inj
    if len(xccs) == 1:
        assert r["slow_xccs"] == []
        # every site did 4 x the work at no fewer than 32 cycles each
        assert all(v["cycles_per_mfma"] >= 3 * MFMA_ISSUE_CYCLES for v in r["sites"].values())
        return
    assert r["slow_xccs"] == [inj]
    assert r["slow_xccs_by"] == {"clock": [], "cycles": [inj], "mem": [inj]}
    assert _slow_through_sites(r, 2.0) == on_it
    assert set(r["slow_sites"]) <= on_it and r["n_slow"] == len(on_it)
    others = [v["cycles_per_mfma"] for x, v in r["xccs"].items() if x != inj]
    ratio = r["xccs"][inj]["cycles_per_mfma"] / statistics.median(others)
    mem_ratio = r["xccs"][inj]["us_per_mib"] / statistics.median(v["us_per_mib"] for x, v in r["xccs"].items() if x != inj)
    print("wave time on %s against the others: mfma %.2f x, mem %.2f x" % (inj, ratio, mem_ratio))
    assert ratio >= 3
    assert r["mem_xcc"] == inj and r["xcd_mem_ratio"] < 0.5 and "us per MiB" in r["note"]


def test_injected_slow_waves_are_exactly_the_slow_sites():
    r = _check(blocks=8, iters=256, slice_kb=64, slow_ratio=2.0, inject="slow_waves", inject_waves=3)
    print("slow_waves: %s of %s" % (r["slow_sites"], r["wave_sites"][:4]))
    assert r["pace_errors"] == 0 and r["moved"] == 0 and len(r["wave_sites"]) == 32
    assert set(r["slow_sites"]) == set(r["wave_sites"][:3]) and r["n_slow"] == 3
    assert len({s.rsplit("/", 1)[0] for s in r["wave_sites"][:4]}) == 1  # one workgroup, one CU
    assert r["slow_xccs_by"]["clock"] == [] and r["slow_xccs_by"]["mem"] == []


def test_injected_wrong_result_is_an_error_at_its_site():
    r = _check(blocks=8, iters=256, slice_kb=64, slow_ratio=2.0, inject="result", inject_waves=3)
    print("result: %s, %r" % (r["bad_sites"], r["error"]))
    bad = {s for s, v in r["sites"].items() if v["bad"]}
    assert bad == set(r["wave_sites"][:3]) == set(r["bad_sites"]) and r["moved"] == 0
    assert r["mfma_errors"] == r["pace_errors"] > 0 and r["mem_errors"] == 0 and r["ok"] is False
    assert r["error"].startswith("pace check: %d wrong result" % r["mfma_errors"])
    assert r["n_slow"] == 0 and r["slow_sites"] == [] and r["slow_xccs"] == []


def test_smallest_shapes():
    """One workgroup, one iteration (the loop body never runs), a 4 KiB slice (the tail rows only)."""
    r = _check(blocks=1, iters=1, slice_kb=4)
    assert r["waves"] == 4 and r["moved"] == 0 and r["pace_errors"] == 0 and r["simds_reached"] == 4
    assert r["xcd_pace_ratio"] == 1.0 and r["slow_xccs"] == [] and r["mem_waves"] == 4
    r = _check(blocks=3, iters=2, slice_kb=20)  # one whole tile of 16 KiB, then a tail row
    assert r["waves"] == 12 and r["pace_errors"] == 0 and r["mem_waves"] == 12


def test_run_merges_the_check_only_when_asked():
    from k8s_gpu_device_plugin_amd.ops import canary
    merged = {"pace_errors", "clock_mhz_min", "clock_mhz_max", "clock_fraction", "xcd_pace_ratio", "xcd_mem_ratio",
              "pace_slow_sites", "pace_slow_xccs", "pace_ms", "pace_note"}
    plain = canary.run(0, 64 << 20, 1, 256)
    assert plain["ok"], plain["error"]
    assert not merged & set(plain)
    r = canary.run(0, 64 << 20, 1, 256, pace=True)
    assert r["ok"], r["error"]
    assert set(r) - set(plain) == merged
    assert r["pace_errors"] == 0 and 0 < r["clock_mhz_min"] <= r["clock_mhz_max"] and r["pace_ms"] > 0
    assert 0 < r["xcd_pace_ratio"] <= 1.0 and 0 < r["xcd_mem_ratio"] <= 1.0
