"""The pace check's host reduction (``ops/pace/pace_host.h``, reached through ``pace.reduce``)
against an independent numpy model on synthetic records, no GPU: located and moved records,
per-site and per-XCD medians, the two ratios, slow sites and slow XCDs at their boundaries, one
XCD, an empty XCD, and the texts.  ``tests/native/pace_selftest.cpp`` runs the same header
under AddressSanitizer and UBSan as a program of its own."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from k8s_gpu_device_plugin_amd import _build
from k8s_gpu_device_plugin_amd.ops import pace

TICK_MHZ = 100.0
CLOCK_MAX = 2400.0
ITERS_WORK = 4096  # MFMAs a record stands for
MIB = 1 << 20


def site(xcc, cu=0, simd=0, se=0, sh=0):
    return pace.pack_site(xcc, se, sh, cu, simd)


def mfma_rec(s, cpm=32.0, mhz=2100.0, bad=0, last=None, work=ITERS_WORK):
    """A record of `work` MFMAs at `cpm` cycles each on a clock of `mhz`."""
    cycles = int(round(cpm * work))
    ticks = int(round(cycles / mhz * TICK_MHZ))
    return (s, s if last is None else last, cycles, ticks, work, bad)


def mem_block(s_cu, us_per_mib=40.0, nbytes=MIB, bad=(0, 0, 0, 0), moved_wave=None):
    """The four records of one memory workgroup on the CU of `s_cu` (simd bits ignored)."""
    ticks = int(round(us_per_mib * nbytes / MIB * TICK_MHZ))
    rows = []
    for w in range(4):
        s = (s_cu & ~3) | w
        rows.append((s, s ^ (4 if moved_wave == w else 0), ticks * 21, ticks + w, nbytes, bad[w]))
    return rows


# ---- the independent model -----------------------------------------------------------------
def med(values):
    v = sorted(values)
    n = len(v)
    if n == 0:
        return 0.0
    return v[n // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2


def model(mfma, mem=(), slow_ratio=1.5, tick=TICK_MHZ, clock_max=CLOCK_MAX):
    by_site, out = {}, {"unlocated_errors": 0, "mfma_errors": 0, "mem_errors": 0, "moved": 0, "waves": 0}
    for s0, s1, cycles, ticks, work, bad in mfma:
        if s0 == pace.UNWRITTEN:
            continue
        if s0 != s1:
            out["moved"] += 1
            out["unlocated_errors"] += bad
            continue
        out["waves"] += 1
        out["mfma_errors"] += bad
        slot = by_site.setdefault(s0, {"cpm": [], "mhz": [], "waves": 0, "bad": 0})
        slot["waves"] += 1
        slot["bad"] += bad
        if cycles and ticks and work:
            slot["cpm"].append(cycles / work)
            slot["mhz"].append(cycles / ticks * tick)
    sites = {s: {"cycles_per_mfma": med(v["cpm"]), "clock_mhz": med(v["mhz"]), "waves": v["waves"], "bad": v["bad"]}
             for s, v in by_site.items()}
    timed = {s: v for s, v in sites.items() if by_site[s]["cpm"]}
    site_median = med([v["cycles_per_mfma"] for v in timed.values()])
    slow = sorted(s for s, v in timed.items() if v["cycles_per_mfma"] > slow_ratio * site_median)
    xccs = {}
    for x in range(16):
        mhz = [m for s, v in by_site.items() if s >> 10 == x for m in v["mhz"]]
        if mhz:
            xccs[x] = {"clock_mhz": med(mhz),
                       "cycles_per_mfma": med([v["cycles_per_mfma"] for s, v in timed.items() if s >> 10 == x])}
    us = {}
    for i, (s0, s1, cycles, ticks, work, bad) in enumerate(mem):
        if s0 == pace.UNWRITTEN:
            continue
        if s0 != s1:
            out["unlocated_errors"] += bad
            continue
        out["mem_errors"] += bad
        if i % 4 == 0 and cycles and ticks and work:
            us.setdefault(s0 >> 10, []).append(ticks / tick / (work / MIB))
    us = {x: med(v) for x, v in us.items()}
    clocks = [v["clock_mhz"] for v in xccs.values()]
    out["clock_mhz_min"], out["clock_mhz_max"] = (min(clocks), max(clocks)) if clocks else (0.0, 0.0)
    out["clock_fraction"] = out["clock_mhz_min"] / clock_max if clocks else 0.0
    clock_median, cpm_median, us_median = med(clocks), med([v["cycles_per_mfma"] for v in xccs.values()]), med(us.values())
    many, many_mem = len(xccs) > 1, len(us) > 1
    out["xcd_pace_ratio"] = min(clocks) / clock_median if many else 1.0
    out["xcd_mem_ratio"] = us_median / max(us.values()) if many_mem else 1.0
    by = {"clock": [x for x, v in xccs.items() if many and v["clock_mhz"] < clock_median / slow_ratio],
          "cycles": [x for x, v in xccs.items() if many and v["cycles_per_mfma"] > cpm_median * slow_ratio],
          "mem": [x for x, v in us.items() if many_mem and v > us_median * slow_ratio]}
    out["slow_xccs_by"] = {k: ["xcc%d" % x for x in sorted(v)] for k, v in by.items()}
    out["slow_xccs"] = ["xcc%d" % x for x in sorted(set(by["clock"]) | set(by["cycles"]) | set(by["mem"]))]
    out["pace_errors"] = out["mfma_errors"] + out["mem_errors"] + out["unlocated_errors"]
    out["n_slow"] = len(slow)
    out["slow_sites"] = [pace.format_site(s) for s in slow[:16]]
    out["sites"] = {pace.format_site(s): v for s, v in sites.items()}
    out["xccs"] = {"xcc%d" % x: dict(v, us_per_mib=us.get(x, 0.0)) for x, v in xccs.items()}
    return out


def check(mfma, mem=(), slow_ratio=1.5):
    """pace.reduce against the model on every figure both hold; returns pace.reduce's result."""
    got = pace.reduce(pace.records(mfma), TICK_MHZ, CLOCK_MAX, slow_ratio, pace.records(mem) if len(mem) else None)
    want = model(mfma, mem, slow_ratio)
    for key in ("unlocated_errors", "mfma_errors", "mem_errors", "pace_errors", "moved", "waves", "n_slow", "slow_sites",
                "slow_xccs", "slow_xccs_by"):
        assert got[key] == want[key], key
    for key in ("clock_mhz_min", "clock_mhz_max", "clock_fraction", "xcd_pace_ratio", "xcd_mem_ratio"):
        assert got[key] == pytest.approx(want[key], rel=1e-12), key
    assert set(got["sites"]) == set(want["sites"])
    for s, v in want["sites"].items():
        assert got["sites"][s] == pytest.approx(v, rel=1e-12), s
    for x, v in want["xccs"].items():
        assert {k: got["xccs"][x][k] for k in v} == pytest.approx(v, rel=1e-12), x
    assert got["ok"] is (got["pace_errors"] == 0)
    return got


def balanced(xccs=8, cus=4, waves=2):
    """`waves` records on every SIMD of `cus` CUs of `xccs` XCDs, and one memory workgroup per CU."""
    mfma = [mfma_rec(site(x, c, s)) for _ in range(waves) for x in range(xccs) for c in range(cus) for s in range(4)]
    mem = [row for x in range(xccs) for c in range(cus) for row in mem_block(site(x, c))]
    return mfma, mem


# ---- the cases -------------------------------------------------------------------------------
def test_balanced_table_has_ratios_of_exactly_one_and_nothing_slow():
    mfma, mem = balanced()
    r = check(mfma, mem)
    assert r["xcd_pace_ratio"] == 1.0 and r["xcd_mem_ratio"] == 1.0
    assert r["slow_xccs"] == [] and r["slow_sites"] == [] and r["n_slow"] == 0 and r["note"] == "" and r["error"] == ""
    assert r["xccs_reached"] == 8 and r["cus_reached"] == 32 and r["simds_reached"] == 128 and r["mem_cus_reached"] == 32
    assert r["clock_mhz_min"] == r["clock_mhz_max"] and r["clock_fraction"] == pytest.approx(r["clock_mhz_min"] / CLOCK_MAX)
    assert abs(r["clock_mhz_min"] - 2100.0) < 1.0  # the tick count is a whole number
    assert all(v["cycles_per_mfma"] == 32.0 for v in r["sites"].values())
    assert all(v["us_per_mib"] == 40.0 and v["blocks"] == 4 for v in r["xccs"].values())
    assert r["pace_xcc"] is not None  # some XCD is the slowest even when all agree


def test_one_xcd_at_half_the_clock():
    mfma, mem = balanced()
    # the same cycles per MFMA over twice the ticks
    mfma = [(s0, s1, c, t * 2 if s0 >> 10 == 5 else t, w, b) for s0, s1, c, t, w, b in mfma]
    r = check(mfma, mem)
    assert r["xcd_pace_ratio"] == pytest.approx(0.5, rel=1e-12) and r["xcd_mem_ratio"] == 1.0
    assert r["slow_xccs"] == ["xcc5"] and r["slow_xccs_by"] == {"clock": ["xcc5"], "cycles": [], "mem": []}
    assert r["pace_xcc"] == "xcc5" and r["n_slow"] == 0  # cycles per MFMA did not change
    fast = r["xccs"]["xcc0"]["clock_mhz"]
    assert r["note"] == "pace: xcc5 ran %.0f MHz beside a median of %.0f (ratio 0.50)" % (fast / 2, fast)
    assert r["ok"] is True and r["error"] == ""  # slowness is reported, not failed
    assert r["clock_fraction"] == pytest.approx(fast / 2 / CLOCK_MAX)


def test_one_xcd_at_twice_the_memory_time():
    mfma, mem = balanced()
    mem = [row for x in range(8) for c in range(4) for row in mem_block(site(x, c), 80.0 if x == 2 else 40.0)]
    r = check(mfma, mem)
    assert r["xcd_mem_ratio"] == pytest.approx(0.5) and r["xcd_pace_ratio"] == 1.0
    assert r["slow_xccs"] == ["xcc2"] and r["slow_xccs_by"]["mem"] == ["xcc2"] and r["mem_xcc"] == "xcc2"
    assert r["note"] == "pace: xcc2 took 80.0 us per MiB beside a median of 40.0 (ratio 0.50)"


def test_one_site_at_twice_the_cycles_is_alone_in_slow_sites():
    mfma, mem = balanced()
    slow = site(3, 2, 1)
    mfma = [mfma_rec(s0, 64.0) if s0 == slow else row for row in mfma for s0 in row[:1]]
    r = check(mfma, mem)
    assert r["slow_sites"] == [pace.format_site(slow)] == ["xcc3/se0/sh0/cu2/simd1"] and r["n_slow"] == 1
    assert r["slow_xccs"] == []  # one site of sixteen does not move its XCD's median
    assert r["note"] == "pace: xcc3/se0/sh0/cu2/simd1 took 64.0 cycles per MFMA beside a median of 32.0"


def test_seventeen_slow_sites_sixteen_listed():
    mfma, mem = balanced(cus=8)  # 256 sites
    slow = sorted(site(x, c, s) for x in range(8) for c in range(8) for s in range(4))[5::15][:17]
    mfma = [mfma_rec(row[0], 70.0) if row[0] in slow else row for row in mfma]
    r = check(mfma, mem)
    assert r["n_slow"] == 17 and len(r["slow_sites"]) == 16
    assert r["slow_sites"] == [pace.format_site(s) for s in slow[:16]]
    assert r["note"].endswith("(+16 more sites)")


def test_moved_records_lose_their_timings_and_their_bad_is_unlocated():
    mfma, mem = balanced()
    a, b = site(1, 1, 1), site(1, 1, 2)
    mfma += [mfma_rec(a, 500.0, 300.0, bad=3, last=b), mfma_rec(site(6), 32.0, bad=2)]
    mem += mem_block(site(4, 3), 400.0, bad=(0, 5, 0, 0), moved_wave=1)  # wave 1 moved: its 5 are unlocated
    mem += mem_block(site(7, 1), 900.0, bad=(1, 0, 0, 0), moved_wave=0)  # wave 0 moved: the workgroup is not timed
    r = check(mfma, mem)
    assert (r["moved"], r["unlocated_errors"], r["mfma_errors"], r["mem_errors"]) == (1, 3 + 5 + 1, 2, 0)
    assert r["pace_errors"] == 11 and r["ok"] is False
    assert r["n_slow"] == 0 and r["slow_xccs"] == [] and r["xcd_mem_ratio"] == pytest.approx(1.0)
    assert r["sites"][pace.format_site(a)]["cycles_per_mfma"] == 32.0
    assert r["mem_moved"] == 2 and r["xccs"]["xcc7"]["blocks"] == 4 and r["xccs"]["xcc4"]["blocks"] == 5
    assert r["error"] == "pace check: 2 wrong results at xcc6/se0/sh0/cu0/simd0" and r["bad_sites"] == ["xcc6/se0/sh0/cu0/simd0"]


def test_error_texts():
    mfma, mem = balanced()
    r = check(mfma + [mfma_rec(site(3, 7, 2, se=1), bad=3), mfma_rec(site(4), bad=1)], mem)
    assert r["error"] == "pace check: 4 wrong results at xcc3/se1/sh0/cu7/simd2 (+1 more site)"
    r = check(mfma, mem + mem_block(site(5, 9), bad=(1, 0, 1, 0)))
    assert r["error"] == "pace check: 2 wrong words read on xcc5" and r["xccs"]["xcc5"]["bad"] == 2
    r = check(mfma, mem + mem_block(site(5, 9), bad=(1, 0, 0, 0)) + mem_block(site(6, 9), bad=(0, 0, 0, 2)))
    assert r["error"] == "pace check: 3 wrong words read on xcc5 (+1 more xcc)"
    r = check(mfma + [mfma_rec(site(0), bad=1, last=site(1))], mem)
    assert r["error"] == "pace check: 1 wrong result at an unknown site" and r["ok"] is False


def test_single_xcd_has_ratios_of_one_and_no_slow_xcd_but_sites_can_be_slow():
    mfma, mem = balanced(xccs=1, cus=8)
    slow = site(0, 5, 3)
    mfma = [mfma_rec(row[0], 100.0, 900.0) if row[0] == slow else row for row in mfma]
    r = check(mfma, mem)
    assert r["xcd_pace_ratio"] == 1.0 and r["xcd_mem_ratio"] == 1.0 and r["slow_xccs"] == []
    assert r["pace_xcc"] is None and r["mem_xcc"] is None and r["xccs_reached"] == 1
    assert r["slow_sites"] == [pace.format_site(slow)]
    assert r["clock_mhz_min"] == r["clock_mhz_max"] > 0


def test_an_empty_xcd_is_left_out():
    mfma, mem = balanced()
    mfma = [row for row in mfma if row[0] >> 10 != 4]
    mem = [row for row in mem if row[0] >> 10 != 4]
    r = check(mfma, mem)
    assert "xcc4" not in r["xccs"] and r["xccs_reached"] == 7 and r["mem_xccs_reached"] == 7
    assert r["xcd_pace_ratio"] == 1.0 and r["slow_xccs"] == [] and r["clock_mhz_min"] > 0
    # an XCD with memory records alone has no clock, and does not count as the slowest
    r = check(mfma, mem + mem_block(site(4, 0)))
    assert r["xccs"]["xcc4"]["clock_mhz"] == 0.0 and r["xccs"]["xcc4"]["us_per_mib"] == 40.0 and r["clock_mhz_min"] > 0


def test_no_records_at_all():
    r = pace.reduce(np.zeros(0, dtype=pace.RECORD_DTYPE), TICK_MHZ, CLOCK_MAX)
    assert r["waves"] == 0 and r["xccs"] == {} and r["sites"] == {} and r["ok"] is True
    assert (r["xcd_pace_ratio"], r["xcd_mem_ratio"], r["clock_mhz_min"], r["clock_fraction"]) == (1.0, 1.0, 0.0, 0.0)
    unwritten = [(pace.UNWRITTEN, pace.UNWRITTEN, 2**64 - 1, 2**64 - 1, pace.UNWRITTEN, pace.UNWRITTEN)] * 8
    assert check(unwritten, unwritten)["waves"] == 0


@pytest.mark.parametrize("slow_ratio", [1.5, 2.0])
def test_exactly_at_the_ratio_is_not_slow(slow_ratio):
    mfma, mem = balanced()
    at, above = site(1, 1, 1), site(2, 2, 2)
    edge = 32.0 * slow_ratio  # exact in binary, as is the record's cycles / work
    mfma = [mfma_rec(row[0], edge) if row[0] == at else mfma_rec(row[0], edge + 1 / 64) if row[0] == above else row
            for row in mfma]
    r = check(mfma, mem, slow_ratio)
    assert r["slow_sites"] == [pace.format_site(above)]
    # XCDs: 2100 MHz against 2100 / slow_ratio exactly, and one tick more; 40 us against 40 x slow_ratio
    base, _ = balanced()
    cycles = 21 * 4096  # 2100 MHz over 4096 ticks
    slow_ticks = int(4096 * slow_ratio)
    recs = [(s0, s1, cycles, slow_ticks if s0 >> 10 == 3 else slow_ticks + 1 if s0 >> 10 == 6 else 4096, w, b)
            for s0, s1, _, _, w, b in base]
    mem = [row for x in range(8) for c in range(4) for row in
           mem_block(site(x, c), 40.0 * slow_ratio if x == 1 else 40.0 * slow_ratio + 0.01 if x == 2 else 40.0)]
    r = check(recs, mem, slow_ratio)
    assert r["slow_xccs_by"] == {"clock": ["xcc6"], "cycles": [], "mem": ["xcc2"]}
    assert r["xccs"]["xcc3"]["clock_mhz"] == 2100.0 / slow_ratio


def test_even_and_odd_medians():
    s = site(2, 3, 1)
    odd = [mfma_rec(s, c) for c in (40.0, 32.0, 36.0)]
    even = odd + [mfma_rec(s, 33.0)]
    assert check(odd)["sites"][pace.format_site(s)]["cycles_per_mfma"] == 36.0
    assert check(even)["sites"][pace.format_site(s)]["cycles_per_mfma"] == 34.5
    # over XCDs: two XCDs, the median is their mean, so the slower one is at 2 x 0.5 / 1.5 of it
    two = [mfma_rec(site(0), mhz=2000.0), mfma_rec(site(1), mhz=1000.0)]
    r = check(two)
    assert r["xcd_pace_ratio"] == pytest.approx(1000.0 / 1500.0, rel=1e-3) and r["pace_xcc"] == "xcc1"
    three = two + [mfma_rec(site(2), mhz=1600.0)]
    assert check(three)["xcd_pace_ratio"] == pytest.approx(1000.0 / 1600.0, rel=1e-3)


def test_zero_counters_are_located_but_not_timed():
    s = site(1)
    r = check([(s, s, 0, 0, 16, 2), mfma_rec(site(2))])
    assert r["sites"][pace.format_site(s)] == {"cycles_per_mfma": 0.0, "clock_mhz": 0.0, "waves": 1, "bad": 2}
    assert r["mfma_errors"] == 2 and r["xccs_reached"] == 1 and r["n_slow"] == 0


def test_reduce_refuses_bad_arguments():
    good = pace.records([mfma_rec(site(0))])
    for kw in ({"tick_mhz": 0.0}, {"tick_mhz": float("nan")}, {"clock_max_mhz": -1.0}, {"slow_ratio": 0.99},
               {"slow_ratio": float("nan")}):
        args = dict({"tick_mhz": TICK_MHZ, "clock_max_mhz": CLOCK_MAX, "slow_ratio": 1.5}, **kw)
        with pytest.raises(ValueError, match="pace.reduce: bad arguments"):
            pace.reduce(good, **args)
    with pytest.raises(ValueError):
        pace.reduce(pace.records([(1 << 14, 1 << 14, 1, 1, 1, 0)]), TICK_MHZ, CLOCK_MAX)  # no such site
    with pytest.raises(ValueError):
        pace.reduce(good, TICK_MHZ, CLOCK_MAX, 1.5, pace.records(mem_block(site(0))[:3]))  # not four per workgroup
    assert pace.reduce(good, TICK_MHZ, 0.0)["clock_fraction"] == 0.0  # a device that reports no maximum


# ---- the stand-alone sanitized program ---------------------------------------------------
def test_sanitized_selftest_program(tmp_path):
    """Host code under AddressSanitizer and UBSan as a program of its own: nothing sanitized
    is loaded into Python."""
    cxx = shutil.which(_build._cxx())
    assert cxx, "no C++ compiler"
    src = os.path.join(_build.HARNESS_DIR, "pace_selftest.cpp")
    exe = str(tmp_path / "pace_selftest")
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + _build.PACE_DIR,
                        src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
           "PATH": "/usr/bin:/bin"}  # as tests/test_native_selftest.py runs its program
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", p.stdout[-3000:]
