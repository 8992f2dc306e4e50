"""Site probe of the gfx950 canary (``ops/sites.hip``) on a real MI355X: the MFMA and
vector-ALU exactness checks reach every CU and SIMD, and an injected fault is reported at
the site of the waves that computed it."""
import pytest

pytestmark = pytest.mark.gpu

CHECKS = ("mfma", "lowp", "valu")


@pytest.fixture(scope="module")
def canary_run():
    from k8s_gpu_device_plugin_amd.ops import canary
    return canary.run(0, hbm_bytes=64 << 20, passes=1, mfma_iters=256)


def _cu(site):
    return site.rsplit("/", 1)[0]  # xcc/se/sh/cu without the simd


def test_healthy_map_covers_every_cu_and_simd(canary_run):
    from k8s_gpu_device_plugin_amd.ops import canary
    r = canary.site_probe(ksteps=1)
    print("site probe: launches %d, moved %d, waves %d, %.3f ms, CUs %d/%d, SIMDs %d"
          % (r["launches"], r["moved"], r["waves"], r["ms"], r["cus_reached"], r["cus_expected"], r["simds_reached"]))
    assert [r[c] for c in CHECKS] == [0, 0, 0] and r["unlocated_errors"] == 0
    assert r["n_bad"] == 0 and r["bad_sites"] == []
    assert r["cus_reached"] == r["cus_expected"] == canary_run["num_cus"]
    assert r["simds_reached"] == 4 * r["cus_reached"]
    assert 1 <= r["launches"] <= 4
    assert len(r["sites"]) == r["simds_reached"]
    assert sum(s["waves"] for s in r["sites"].values()) == r["waves"]
    assert r["waves"] + r["moved"] == r["launches"] * 2 * r["cus_expected"] * 4
    xccs = {int(s.split("/")[0][3:]) for s in r["sites"]}
    assert all(x < 8 for x in xccs) and len(xccs) in (1, 2, 4, 8)  # SPX, DPX, QPX or CPX
    assert len(r["wave_sites"]) == 2 * r["cus_expected"] * 4


@pytest.mark.parametrize("check", CHECKS)
def test_injected_fault_is_located(check):
    from k8s_gpu_device_plugin_amd.ops import canary
    r = canary.site_probe(blocks=8, ksteps=1, inject=check, inject_waves=3)
    print("inject %s: %s, moved %d" % (check, {c: r[c] for c in CHECKS}, r["moved"]))
    assert r[check] > 0
    assert [r[c] for c in CHECKS if c != check] == [0, 0]
    assert r["launches"] == 1 and r["waves"] + r["moved"] == 32 and len(r["wave_sites"]) == 32
    bad = {s for s, v in r["sites"].items() if v["mfma"] or v["lowp"] or v["valu"]}
    assert bad == set(r["wave_sites"][:3])
    assert set(r["bad_sites"]) == bad and r["n_bad"] == len(bad)
    assert len({_cu(s) for s in r["wave_sites"][0:4]}) == 1  # one workgroup, one CU


def test_smallest_grid():
    from k8s_gpu_device_plugin_amd.ops import canary
    r = canary.site_probe(blocks=1, ksteps=1)
    assert r["waves"] == 4 and r["moved"] == 0
    assert len({_cu(s) for s in r["sites"]}) == 1
    assert [r[c] for c in CHECKS] == [0, 0, 0]


def test_canary_run_reports_sites(canary_run):
    r = canary_run
    assert r["ok"], r
    assert r["site_errors"] == 0 and r["cus_unreached"] == 0 and r["bad_sites"] == []
    assert r["site_ms"] > 0
    assert r["cus_reached"] == r["num_cus"] and r["simds_reached"] == 4 * r["num_cus"]
