"""CU memory check of the gfx950 canary (``ops/cumem.hip``) on a real MI355X: the register
file march and the L1 march reach every CU and SIMD with zero errors, and an injected flip
is counted exactly once per injected wave or workgroup, at the site it ran on."""
import pytest

pytestmark = pytest.mark.gpu

COUNTS = ("vgpr_errors", "agpr_errors", "l1_errors", "l1_fill_errors", "unlocated_errors")


@pytest.fixture(scope="module")
def canary_run():
    from k8s_gpu_device_plugin_amd.ops import canary
    return canary.run(0, 64 << 20, 1, 256)


@pytest.fixture(scope="module")
def healthy():
    from k8s_gpu_device_plugin_amd.ops import canary
    return canary.cu_check()


def _cu(site):
    return site.rsplit("/", 1)[0]  # xcc/se/sh/cu without the simd


def _bad(r):
    return {s for s, v in r["sites"].items() if v["vgpr"] or v["agpr"] or v["l1"]}


def test_healthy_defaults_cover_every_cu_and_simd(healthy, canary_run):
    r = healthy
    print("cu check: launches %d, moved %d (l1 %d), waves %d, reg %.3f ms, l1 %.3f ms, CUs %d/%d (l1 %d), SIMDs %d, "
          "%d + %d registers" % (r["launches"], r["moved"], r["l1_moved"], r["waves"], r["reg_ms"], r["l1_ms"],
                                 r["cus_reached"], r["cus_expected"], r["l1_cus_reached"], r["simds_reached"],
                                 r["regs_vgpr"], r["regs_agpr"]))
    assert [r[c] for c in COUNTS] == [0, 0, 0, 0, 0]
    assert r["n_bad"] == 0 and r["bad_sites"] == [] and r["error"] == ""
    assert r["cus_reached"] == r["cus_expected"] == canary_run["num_cus"]
    assert r["simds_reached"] == 4 * r["cus_reached"]
    assert 1 <= r["launches"] <= 4
    assert r["waves"] + r["moved"] == r["launches"] * 2 * r["cus_expected"] * 4
    assert r["regs_marched"] >= 448 and r["regs_marched"] == r["regs_vgpr"] + r["regs_agpr"]
    assert r["reg_bytes_per_simd"] == 256 * r["regs_marched"]
    assert r["l1_cus_reached"] == r["cus_expected"]
    assert sum(s["waves"] for s in r["sites"].values()) == r["waves"]
    assert len(r["wave_sites"]) == len(r["l1_wave_sites"]) == 2 * r["cus_expected"] * 4


@pytest.mark.parametrize("kind", ("vgpr", "agpr", "l1"))
def test_injected_flip_is_counted_once_and_located(kind):
    from k8s_gpu_device_plugin_amd.ops import canary
    r = canary.cu_check(blocks=8, reps=1, l1_kb=4, l1_reps=1, inject=kind, inject_waves=3)
    print("inject %s: %s, moved %d / %d, bad %s" % (kind, {c: r[c] for c in COUNTS}, r["moved"], r["l1_moved"],
                                                    r["bad_sites"]))
    assert r["launches"] == 1 and r["waves"] + r["moved"] == 32
    assert len(r["wave_sites"]) == 32 and len(r["l1_wave_sites"]) == 32
    if kind == "l1":
        assert r["l1_errors"] == 3
        assert [r[c] for c in COUNTS if c != "l1_errors"] == [0, 0, 0, 0]
        assert {_cu(s) for s in _bad(r)} == {_cu(r["l1_wave_sites"][4 * b]) for b in range(3)}
        assert "l1 check: 3 wrong words at " in r["error"]
    else:
        assert r[kind + "_errors"] + r["unlocated_errors"] == 3
        assert [r[c] for c in COUNTS if c not in (kind + "_errors", "unlocated_errors")] == [0, 0, 0]
        assert _bad(r) == set(r["wave_sites"][:3])
        assert all(r["sites"][s][kind] == 1 for s in _bad(r))
        assert r["error"].startswith("register check: 3 wrong words at ") and "(" + kind in r["error"]
    assert set(r["bad_sites"]) == _bad(r) and r["n_bad"] == len(_bad(r))
    assert len({_cu(s) for s in r["wave_sites"][0:4]}) == 1  # one workgroup, one CU
    assert len({_cu(s) for s in r["l1_wave_sites"][0:4]}) == 1


def test_smallest_shapes():
    """One workgroup, a 4 KiB slice: 256 16-B words, so exactly one load per thread per pass."""
    from k8s_gpu_device_plugin_amd.ops import canary
    r = canary.cu_check(blocks=1, reps=1, l1_kb=4, l1_reps=1)
    assert r["waves"] == 4 and r["moved"] == 0 and r["launches"] == 1
    assert len({_cu(s) for s in r["sites"]}) == 1 and r["simds_reached"] == 4 and r["l1_cus_reached"] == 1
    assert [r[c] for c in COUNTS] == [0, 0, 0, 0, 0]


def test_whole_l1_slice():
    """l1_kb=32: the upper edge, a slice as large as the L1 itself."""
    from k8s_gpu_device_plugin_amd.ops import canary
    r = canary.cu_check(l1_kb=32, l1_reps=1)
    assert [r[c] for c in COUNTS] == [0, 0, 0, 0, 0]
    assert r["l1_cus_reached"] == r["cus_expected"]


def test_canary_run_merges_the_cu_check(canary_run, healthy):
    r = canary_run
    assert r["ok"], r
    assert r["reg_errors"] == 0 and r["l1_errors"] == 0 and r["l1_fill_errors"] == 0 and r["cu_bad_sites"] == []
    assert r["cu_ms"] > 0
    assert r["regs_marched"] == healthy["regs_marched"]
