"""The matrix-forms check (``ops/matforms/matforms.hip``) on a real MI355X: every form of the
table reaches every CU and SIMD with zero errors; the hardware's own account of each operand
map (one-hot operands through single-wave MFMAs) is the table's partition; random in-range raw
codes multiply to exactly what the numpy model's decoders give; and each injected fault shows
as exactly the predicted count, in exactly that form, at exactly the sites that injected it."""
import math

import numpy as np
import pytest

import matforms_model as model

pytestmark = pytest.mark.gpu

FORMS = list(model.FORMS)  # test_matforms_model.py holds the table to the same list


def _check(**kw):
    from k8s_gpu_device_plugin_amd.ops import matforms
    return matforms.matrix_forms_check(**kw)


def _cu(site):
    return site.rsplit("/", 1)[0]


@pytest.fixture(scope="module")
def healthy():
    return _check()


def test_healthy_defaults_cover_every_cu_and_simd_with_every_form(healthy):
    r = healthy
    print("matforms: launches %d, waves %d, moved %d, %.3f ms: %s"
          % (r["launches"], r["waves"], r["moved"], r["ms"], {k: round(v, 3) for k, v in r["form_ms"].items()}))
    assert r["forms"] == FORMS
    assert all(v == 0 for v in r["errors"].values()) and r["unlocated_errors"] == 0 and r["matforms_errors"] == 0
    assert r["ok"] is True and r["error"] == "" and r["bad_sites"] == [] and r["bad_by"] == {} and r["n_bad"] == 0
    assert r["cus_reached"] == r["cus_expected"] > 0
    assert r["simds_reached"] == 4 * r["cus_reached"]
    assert 1 <= r["launches"] <= 4
    per_form = r["launches"] * 2 * r["cus_expected"] * 4
    assert r["blocks"] == 2 * r["cus_expected"] and r["ksteps"] == 4 and r["vary_scale"] == 1
    assert r["waves"] + r["moved"] == per_form * len(FORMS)
    assert r["ms"] > 0 and r["tflops"] == {}
    for form in FORMS:  # every form ran the same grid, and every wave left a record
        assert r["form_waves"][form] <= per_form and r["form_ms"][form] > 0
        sites = r["wave_sites"][form]
        assert len(sites) == 2 * r["cus_expected"] * 4, form
        # one workgroup, one CU: its four waves sit on the four SIMDs of one CU
        assert len({_cu(s) for s in sites[:4]}) == 1 and len(set(sites[:4])) == 4, (form, sites[:4])
    assert sum(r["form_waves"].values()) == r["waves"]


@pytest.mark.parametrize("ksteps", [1, 3])
@pytest.mark.parametrize("vary_scale", [False, True])
def test_small_grid_at_the_smallest_depths(ksteps, vary_scale):
    """One and three MFMAs, scales fixed and varied: the smallest shapes at which a map, a
    k-step stride or a scale block can still be wrong."""
    r = _check(blocks=8, ksteps=ksteps, vary_scale=vary_scale)
    assert r["launches"] == 1 and r["waves"] + r["moved"] == 32 * len(FORMS) and r["moved"] == 0
    assert r["matforms_errors"] == 0 and all(v == 0 for v in r["errors"].values()) and r["ok"]
    assert r["form_waves"] == {f: 32 for f in FORMS}
    # a site counts as reached once every selected form has run there: eight workgroups of one form
    # reach at most eight CUs, eight of each of fifteen forms need not share any
    assert r["simds_reached"] <= 32 and r["cus_reached"] <= 8
    one = _check(blocks=8, ksteps=ksteps, vary_scale=vary_scale, forms=[FORMS[-1]])
    assert one["simds_reached"] == 4 * one["cus_reached"] and 1 <= one["cus_reached"] <= 8 and one["matforms_errors"] == 0


@pytest.mark.parametrize("form", FORMS)
def test_an_injected_operand_is_the_predicted_count_in_that_form_at_its_site(form):
    from k8s_gpu_device_plugin_amd.ops import matforms
    r = _check(blocks=8, inject_form=form, inject_waves=3)
    want = [matforms.inject_expected(form, w) for w in range(3)]
    print(form, want, r["error"], r["bad_sites"], r["wave_sites"][form][:4])
    assert all(w > 0 for w in want)  # the first three waves' data: each has a B element to meet
    assert r["moved"] == 0 and r["launches"] == 1 and r["unlocated_errors"] == 0
    assert r["errors"] == {f: sum(want) if f == form else 0 for f in FORMS}
    assert r["matforms_errors"] == sum(want) and r["ok"] is False
    assert set(r["bad_by"]) == {form} and r["bad_by"][form]["sites"] == 3
    assert set(r["bad_sites"]) == set(r["wave_sites"][form][:3]) and len(r["bad_sites"]) == 3 == r["n_bad"]
    text = matforms.form_info(form)["text"]
    assert r["error"].startswith("matrix form check: %d wrong results in %s at " % (sum(want), text))
    assert r["error"].endswith("(+2 more sites)") and r["bad_by"][form]["first_site"] in r["error"]
    # each wave on its own: the count is that wave's
    one = _check(blocks=8, forms=[form], inject_form=form, inject_waves=1)
    assert one["errors"] == {form: want[0]} and one["bad_sites"] == one["wave_sites"][form][:1]


@pytest.mark.parametrize("form", FORMS)
def test_the_hardware_s_operand_map_is_the_table_s_partition(form):
    """The test a wrong map cannot pass: rows and columns, which A and B elements share a k, and
    which k-block each lane's scale byte scales, read from the hardware with one-hot operands."""
    from k8s_gpu_device_plugin_amd.ops import matforms
    hw = matforms.operand_map(form)
    assert matforms.map_mismatches(form, hw) == []
    f = model.FORMS[form]  # ... and the model's own statement of the map, k for k up to the labels
    m, elems, K = f["m"], f["elems"], f["k"]
    a_k = np.array([[f["map"][0](lane // m, j, elems, K) for j in range(elems)] for lane in range(64)])
    b_k = np.array([[f["map"][1](lane // m, j, elems, K) for j in range(elems)] for lane in range(64)])
    pairs = set(zip(np.asarray(hw["a_class"]).ravel().tolist(), a_k.ravel().tolist())) | \
        set(zip(np.asarray(hw["b_class"]).ravel().tolist(), b_k.ravel().tolist()))
    assert len(pairs) == K == len({c for c, _ in pairs}) == len({k for _, k in pairs})


@pytest.mark.parametrize("form", FORMS)
def test_random_in_range_codes_multiply_to_the_model_s_product(form):
    """One tile of random raw codes of integers in [-R, R] (both zeros, every encoding of a
    value), scales 2^0 or 2^1: the reference is exact, so no element is left out and nothing is
    tolerated."""
    from k8s_gpu_device_plugin_amd.ops import matforms
    f = model.FORMS[form]
    rng = np.random.default_rng(0xF0 + FORMS.index(form))
    a = model.pack(model.random_codes(rng, f["enc"][0], f["r"], (1, 64, f["elems"])), model.BITS[f["enc"][0]])
    b = model.pack(model.random_codes(rng, f["enc"][1], f["r"], (1, 64, f["elems"])), model.BITS[f["enc"][1]])
    sa, sb = (rng.integers(127, 129, (1, 64)).astype(np.uint32) for _ in range(2))
    want = model.product(form, a, b, sa, sb)
    assert np.abs(want).max() < 2 ** model.ACC_BITS[f["acc"]] and np.abs(want).max() > 0
    got = model.read_accumulators(form, matforms.raw(form, a, b, sa, sb)[0])
    assert np.array_equal(got, want), (form, np.argwhere(got != want)[:8].tolist())


def test_rates_are_reported_for_every_form():
    r = _check(blocks=8, rates=True)
    print("matforms rates (TFLOP/s, i8 TOP/s):", {k: round(v, 1) for k, v in r["tflops"].items()})
    assert sorted(r["tflops"]) == sorted(FORMS) and r["ok"]
    assert all(math.isfinite(v) and v > 0 for v in r["tflops"].values())
