"""The matrix-forms check without a GPU: the words a wave feeds its MFMAs
(``matforms.operands``), decoded and multiplied by the independent numpy model
(``matforms_model.py``), must give the library's integer reference (``matforms.expected``)
element for element; every integer of a form's range must survive its code; the range must
keep every partial sum exact; and the injection must change exactly the predicted elements."""
import numpy as np
import pytest

import matforms_model as model
from k8s_gpu_device_plugin_amd.ops import matforms

FORMS = sorted(model.FORMS)


def test_the_table_is_the_model_s_list_of_forms():
    assert sorted(matforms.FORMS) == FORMS
    for name in matforms.FORMS:
        info, f = matforms.form_info(name), model.FORMS[name]
        assert (info["m"], info["k"], info["elems"], info["r"], bool(info["scaled"])) == (f["m"], f["k"], f["elems"], f["r"], f["scaled"])
        assert info["instruction"] == f["instruction"]
        assert (info["bits_a"], info["bits_b"]) == tuple(model.BITS[e] for e in f["enc"])
        assert ("f32", "i32", "f64")[info["acc_kind"]] == f["acc"] and info["acc"] == (16 if f["m"] == 32 else 4)
    offsets = [matforms.form_info(n)["key_offset"] for n in matforms.FORMS]
    # apart from one another and from the canary's own forms (0, 0x77 << 20, 1..5 << 20)
    assert len(set(offsets)) == len(offsets) and all(o >> 20 > 0x77 for o in offsets)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ksteps", [1, 3, 8])
@pytest.mark.parametrize("vary", [False, True])
def test_decoded_operands_multiply_to_the_reference(form, ksteps, vary):
    for key in (0, 5, (3 << 14) | 2047):
        a, b, sa, sb = matforms.operands(form, key, ksteps, vary)
        got = model.product(form, a, b, sa, sb)
        want = matforms.expected(form, key, ksteps, vary)
        assert np.array_equal(got, want.astype(np.float64)), (form, key)
        assert np.abs(want).max() > 0
        if model.FORMS[form]["scaled"]:
            assert set(np.unique(sa)) | set(np.unique(sb)) == ({127, 128} if vary else {127})
        else:
            assert np.array_equal(want, matforms.expected(form, key, ksteps, not vary))


def _codes(form, which, values):
    """``matforms.encode`` over many values, through the library directly."""
    import ctypes
    lib, f, code = matforms.load(), matforms.form_index(form), ctypes.c_ulonglong()
    out = np.zeros(len(values), dtype=np.uint64)
    for i, v in enumerate(values):
        assert lib.amdgpu_matforms_encode(f, which, v, ctypes.byref(code)) == model.BITS[model.FORMS[form]["enc"][which]]
        out[i] = code.value
    return out


@pytest.mark.parametrize("form", FORMS)
def test_every_integer_of_the_range_round_trips_through_the_form_s_code(form):
    f = model.FORMS[form]
    r = f["r"]
    values = range(-r, r + 1)  # every integer, the 2^21 + 1 of f64 included
    for which in (0, 1):
        if which == 1 and f["enc"][1] == f["enc"][0] and r > 512:
            continue  # the same encoder twice: once is every integer
        codes = _codes(form, which, values)
        assert codes.max() < 2 ** model.BITS[f["enc"][which]] or model.BITS[f["enc"][which]] == 64
        assert np.array_equal(model.DECODE[f["enc"][which]](codes), np.arange(-r, r + 1, dtype=np.float64)), (form, which)
        assert matforms.encode(form, which, r) == int(codes[-1])
    for v in (-r - 1, r + 1):
        with pytest.raises(ValueError):
            matforms.encode(form, 0, v)


@pytest.mark.parametrize("form", FORMS)
def test_the_range_keeps_every_partial_sum_exact(form):
    """Every integer in [-R, R] is a value of the operand type (the round trip above), and the
    largest partial sum, K x 8 steps x R^2 x 4 for the two varied scales, stays below 2^24 for
    f32 accumulators, 2^31 for i32 and 2^53 for f64: exact in any order, no tolerance.  The
    factor 4 stands for the E8M0 scales and applies where a form has them: read onto the
    unscaled forms as well, the ranges the check was given (128 for f16 / bf16 16x16x32, 512
    for f32) meet or pass 2^24, although no product of theirs is ever scaled."""
    f = model.FORMS[form]
    assert model.largest_sum(form) < 2 ** model.ACC_BITS[f["acc"]]
    assert model.MAX_KSTEPS == matforms.MAX_KSTEPS
    for key in (1, 77):  # and the reference itself stays inside it
        assert np.abs(matforms.expected(form, key, 8, True)).max() <= model.largest_sum(form)
    with pytest.raises(ValueError):
        matforms.expected(form, 0, 9)
    info = matforms.form_info(form)
    assert info["r"] == f["r"] and all(2 * info["r"] < 2 ** model.BITS[e] for e in f["enc"])


@pytest.mark.parametrize("form", FORMS)
def test_inject_expected_is_the_model_s_count_of_changed_elements(form):
    seen = set()
    for wave in range(12):
        for ksteps, vary in ((1, False), (3, True)):
            clean = model.product(form, *matforms.operands(form, wave, ksteps, vary))
            hit = model.product(form, *matforms.operands(form, wave, ksteps, vary, inject=True))
            changed = clean != hit
            assert changed.sum() == matforms.inject_expected(form, wave), (form, wave)
            assert not changed[1:].any()  # lane 0 holds row 0
            # one A element moved by one: the operand stays in range and decodes to an integer
            a = matforms.operands(form, wave, 1, vary, inject=True)[0]
            f = model.FORMS[form]
            va = model.DECODE[f["enc"][0]](model.unpack(a, model.BITS[f["enc"][0]], f["elems"]))
            assert np.abs(va).max() <= f["r"] and np.array_equal(va, np.round(va))
        seen.add(matforms.inject_expected(form, wave))
    assert max(seen) > 0


def test_operand_map_comparison_accepts_the_table_and_refuses_another_map():
    """``map_mismatches`` on a map written from the table itself (any relabelling of k), and on
    one with two elements exchanged: the comparison the GPU test relies on can fail."""
    for form in ("bf16_16", "mxfp8fp4_32"):
        info, t = matforms.form_info(form), matforms.table_map(form)
        relabel = np.random.default_rng(1).permutation(info["k"])
        line = np.repeat((np.arange(64) % info["m"])[:, None], info["elems"], axis=1)
        hw = {"a_row": line.tolist(), "b_col": line.tolist(), "a_class": relabel[t["a_k"]].tolist(), "b_class": relabel[t["b_k"]].tolist()}
        if info["scaled"]:
            blocks = [{lane % info["m"]: sorted(int(relabel[k]) for k in range(32 * (lane // info["m"]), 32 * (lane // info["m"]) + 32))}
                      for lane in range(64)]
            hw["scale_a"], hw["scale_b"] = blocks, [dict(b) for b in blocks]
        assert matforms.map_mismatches(form, hw) == []
        hw["b_class"][0][0], hw["b_class"][0][1] = hw["b_class"][0][1], hw["b_class"][0][0]
        assert matforms.map_mismatches(form, hw) != []
