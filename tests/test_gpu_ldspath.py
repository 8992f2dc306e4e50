"""LDS-path check of the gfx950 canary (``ops/ldspath/ldspath.hip``) on a real MI355X: the
march at every access width, the LDS atomics, every lane-crossing op and the transposed read
reach every CU and SIMD with zero errors; what the hardware's lanes receive equals the numpy
model op for op; and each injected fault shows as exactly the predicted count, in exactly
that counter, at exactly the sites that injected it."""
import pytest

import ldspath_model as model

pytestmark = pytest.mark.gpu

COUNTERS = ("lds_errors", "dma_errors", "lds_atomic_errors", "lane_errors", "tr_errors", "unlocated_errors")


def _check(**kw):
    from k8s_gpu_device_plugin_amd.ops import ldspath
    return ldspath.ldspath_check(**kw)


def _cu(site):
    return site.rsplit("/", 1)[0]


@pytest.fixture(scope="module")
def healthy():
    return _check()


def test_healthy_defaults_cover_every_cu_and_simd(healthy):
    from k8s_gpu_device_plugin_amd.ops import canary
    r = healthy
    print("ldspath: launches %d, waves %d, moved %d, lds %d bytes; widths %.3f ms, atomic %.3f ms, lane %.3f ms, tr %.3f ms"
          % (r["launches"], r["waves"], r["moved"], r["lds_bytes"], r["widths_ms"], r["atomic_ms"], r["lane_ms"], r["tr_ms"]))
    assert all(r[k] == 0 for k in COUNTERS + ("ldspath_errors", "plain_errors", "subword_errors", "conflict_errors"))
    assert r["ok"] is True and r["error"] == "" and r["bad_sites"] == [] and not any(r["bad_by"].values())
    assert r["cus_reached"] == r["cus_expected"] > 0
    assert r["simds_reached"] == 4 * r["cus_reached"]
    assert 1 <= r["launches"] <= 4
    launched = r["launches"] * 2 * r["cus_expected"] * 4
    assert r["waves"] + r["moved"] == launched
    for stage in ("widths", "atomic", "lane", "tr"):  # every stage ran the same grid, and every wave left a record
        assert r["stage_waves"][stage] + r["stage_moved"][stage] == launched, stage
        assert len(r["wave_sites"][stage]) == 2 * r["cus_expected"] * 4, stage
    assert r["lds_bytes"] == canary.lds_check(0)[1] >= 128 * 1024  # (mismatches, bytes per workgroup)
    assert r["ms"] > 0 and all(r[k] > 0 for k in ("widths_ms", "atomic_ms", "lane_ms", "tr_ms"))
    # one workgroup, one CU: the four waves of a workgroup sit on the four SIMDs of one CU
    first = r["wave_sites"]["lane"][:4]
    assert len({_cu(s) for s in first}) == 1 and len(set(first)) == 4


def test_what_the_lanes_receive_equals_the_model_for_every_op():
    """One wave, one launch: the test that ties the table to the hardware."""
    from k8s_gpu_device_plugin_amd.ops import ldspath
    got = ldspath.lane_sources()
    assert len(got) == len(ldspath.LANE_OPS)
    wrong = []
    for k, name in enumerate(ldspath.LANE_OPS):
        want = [[0 if c == model.ZERO else int(c) for c in out] for out in model.lane_op(name)]
        if got[k] != want:
            wrong.append((name, got[k], want))
    assert not wrong, wrong


INJECTED = [("lds", 0, "lds_errors", "widths", "128-bit store"), ("subword", 0, "lds_errors", "widths", "8-bit store"),
            ("dma", 0, "dma_errors", "widths", "dma fill"), ("lane", 20, "lane_errors", "lane", "dpp row_ror:3"),
            ("lane", 33, "lane_errors", "lane", "v_permlane16_swap"), ("tr", 0, "tr_errors", "tr", "tr")]


@pytest.mark.parametrize("kind, op, counter, stage, sub", INJECTED)
def test_an_injected_wrong_word_is_one_error_per_wave_at_its_site(kind, op, counter, stage, sub):
    r = _check(blocks=8, reps=1, steps=1, rounds=1, inject=kind, inject_waves=3, inject_op=op)
    print(kind, op, r["error"], r["bad_sites"], r["wave_sites"][stage][:4])
    assert r["moved"] == 0 and r["stage_moved"][stage] == 0 and r["launches"] == 1 and r["waves"] == 32
    assert {k: r[k] for k in COUNTERS} == {k: 3 if k == counter else 0 for k in COUNTERS}
    assert r["ldspath_errors"] == 3 and r["ok"] is False
    assert r["bad_by"] == {s: ({sub: 3} if s == stage else {}) for s in ("widths", "atomic", "lane", "tr")}
    assert set(r["bad_sites"]) == set(r["wave_sites"][stage][:3]) and len(r["bad_sites"]) == 3
    assert r["error"] == r["texts"][stage] != "" and sum(t != "" for t in r["texts"].values()) == 1
    if stage == "widths":
        assert "(pass %d, %s; first at offset 0x" % ({"lds": 1, "subword": 4, "dma": 5}[kind], sub) in r["error"]
        assert r["error"].startswith("lds dma check: 3 wrong words at " if kind == "dma" else "lds check: 3 wrong words at ")
    elif stage == "lane":
        assert r["error"].startswith("lane check: 3 wrong words in %s at " % sub) and r["error"].endswith("(+2 more sites)")
    else:
        assert r["error"].startswith("lds transpose check: 3 wrong elements at ")


@pytest.mark.parametrize("form", range(10))
def test_an_injected_atomic_operand_is_one_wrong_element_per_workgroup_in_that_form(form):
    from k8s_gpu_device_plugin_amd.ops import ldspath
    name = ldspath.ATOMIC_FORMS[form]
    r = _check(blocks=8, reps=1, steps=1, rounds=1, inject="atomic", inject_waves=3, inject_op=form)
    print(name, r["error"], r["bad_sites"])
    assert {k: r[k] for k in COUNTERS} == {k: 3 if k == "lds_atomic_errors" else 0 for k in COUNTERS}
    assert r["bad_by"]["atomic"] == {name: 3} and r["stage_moved"]["atomic"] == 0
    # the element thread 3 hit in step 0 is compared by one thread of each of the first 3 workgroups
    sites = r["wave_sites"]["atomic"]
    assert {_cu(s) for s in r["bad_sites"]} == {_cu(sites[4 * b]) for b in range(3)} and len(r["bad_sites"]) == 3
    assert r["error"].startswith("lds atomic check: 3 wrong elements in %s at " % name)
    if name != "ticket":  # which ticket thread 3 drew is the hardware's choice
        element = model.atomic_index(form, 3, 0)
        assert "(first at %d;" % element in r["error"]


def test_smallest_shapes_and_more_repetitions():
    r = _check(blocks=1, reps=1, steps=1, rounds=1)
    assert r["waves"] == 4 and r["moved"] == 0 and r["ldspath_errors"] == 0 and r["simds_reached"] == 4 and r["cus_reached"] == 1
    r = _check(blocks=3, reps=2, steps=8, rounds=8)
    assert r["waves"] == 12 and r["ldspath_errors"] == 0 and r["stage_waves"] == {s: 12 for s in ("widths", "atomic", "lane", "tr")}


def test_run_merges_the_check_only_when_asked():
    from k8s_gpu_device_plugin_amd.ops import canary
    merged = {"ldspath_errors", "lds_width_errors", "lds_dma_errors", "lds_atomic_errors", "lane_errors", "tr_errors",
              "ldspath_ms", "ldspath_bad_sites"}
    plain = canary.run(0, 64 << 20, 1, 256)
    assert plain["ok"], plain["error"]
    assert not merged & set(plain)
    r = canary.run(0, 64 << 20, 1, 256, lds_path=True)
    assert r["ok"], r["error"]
    assert set(r) - set(plain) == merged
    assert all(r[k] == 0 for k in merged - {"ldspath_ms", "ldspath_bad_sites"}) and r["ldspath_bad_sites"] == [] and r["ldspath_ms"] > 0
