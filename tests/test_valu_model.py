"""The vector-ALU check's host side against the independent model (``tests/valu_model.py``): every
exact op's expected digests, the operand rules, the reduction with its consensus rule, and the
arguments refused before any HIP call.  No GPU."""
import pytest

import valu_model as model
from k8s_gpu_device_plugin_amd.ops import valu
from k8s_gpu_device_plugin_amd.ops._sites import pack_site

EXACT_OPS = [op for op in valu.OPS if valu.op_info(op)["cls"] == "exact"]
SITES = [pack_site(1, 2, 0, 3, simd) for simd in range(4)] + [pack_site(2, 0, 1, 5, 0)]


def test_the_model_covers_the_table():
    assert sorted(EXACT_OPS) == sorted(list(model.EXACT) + list(model.WIDE)) and 60 <= len(valu.OPS) <= valu.MAX_OPS
    assert set(model.APPROX) < {op for op in valu.OPS if valu.op_info(op)["cls"] == "consensus"}
    assert valu.GROUPS == ("int", "bit", "f32", "f64", "f16", "cvt", "approx")


@pytest.mark.parametrize("op", EXACT_OPS)
def test_expected_is_the_fold_of_the_model_over_the_operands(op):
    info = valu.op_info(op)
    for seed in (1, 0xBEEF):
        for rounds in (1, 3):
            a, b, c = valu.operands(op, seed, rounds)
            for kind, words in zip(info["kinds"], (a, b, c)):
                assert all(model.operand_floats_ok(kind, int(w)) for w in words.ravel()), (seed, rounds, kind)
            if info["wide"] and info["kinds"][0] == "enc_seed":
                assert all(model.operand_floats_ok("f32", int(x)) for x in valu.expand(op, int(a[0, 5]), int(c[0, 5])))
            res = model.results(op, a, b, c, valu.expand)
            assert all(len(w) == info["results"] and model.result_floats_ok(info["rkind"], w) for r in res for w in r)
            assert (valu.fold(res) == valu.expected(op, seed, rounds)).all(), (seed, rounds)


def _rec(site, bad=(), digest=(), last=None):
    return (site, site if last is None else last, dict(bad), dict(digest))


def test_reduce_on_hand_built_records():
    sdot4, exp2 = valu.op_info("sdot4"), valu.op_info("exp2_f32")
    ops = ["sdot4", "exp2_f32"]
    good = {exp2["slot"]: 0xABCD}
    clean = [_rec(s) for s in SITES] + [_rec(s, digest=good) for s in SITES]
    of = ["int"] * 5 + ["approx"] * 5
    r = valu.reduce(clean, of, ops)
    assert r["ok"] and r["valu_errors"] == 0 and r["waves"] == 10 and r["simds_reached"] == 5 and r["cus_reached"] == 2
    assert r["unjudged"] == [] and r["error"] == ""
    # one bad exact op at one site
    rows = list(clean)
    rows[2] = _rec(SITES[2], bad={sdot4["slot"]: 5})
    r = valu.reduce(rows, of, ops)
    assert not r["ok"] and r["errors"] == {"sdot4": 5, "exp2_f32": 0} and r["group_errors"] == {"int": 5, "approx": 0}
    assert r["error"] == "vector ALU check: 5 wrong results in sdot4 at xcc1/se2/sh0/cu3/simd2"
    assert r["bad_sites"] == ["xcc1/se2/sh0/cu3/simd2"]
    # a moved wave: its errors are unlocated and fail the check
    rows = list(clean)
    rows[1] = _rec(SITES[1], bad={sdot4["slot"]: 2}, last=SITES[0])
    r = valu.reduce(rows, of, ops)
    assert not r["ok"] and r["moved"] == 1 and r["unlocated_errors"] == 2 and r["errors"]["sdot4"] == 0
    assert r["error"] == "vector ALU check: 2 wrong results at an unknown site"
    # a consensus op with one dissenting record
    rows = list(clean)
    rows[9] = _rec(SITES[4], digest={exp2["slot"]: 0xABCE})
    r = valu.reduce(rows, of, ops)
    assert r["errors"]["exp2_f32"] == 1 and r["bad_sites"] == ["xcc2/se0/sh1/cu5/simd0"] and r["unjudged"] == []
    assert r["error"] == "vector ALU check: 1 wrong result in exp2_f32 at xcc2/se0/sh1/cu5/simd0"


@pytest.mark.parametrize("digests", [(1, 2), (1, 1, 2, 2), (1, 1, 2, 3)], ids=["two records", "split evenly", "no majority"])
def test_a_consensus_op_without_a_majority_is_unjudged(digests):
    slot = valu.op_info("rcp_f32")["slot"]
    r = valu.reduce([_rec(SITES[i], digest={slot: d}) for i, d in enumerate(digests)], ["approx"] * len(digests), ["rcp_f32"])
    assert r["ok"] and r["unjudged"] == ["rcp_f32"] and r["errors"] == {"rcp_f32": 0}


def test_bad_arguments_are_an_error_text_before_any_gpu_call():
    for kw in ({"blocks": -1}, {"blocks": 4097}, {"rounds": 0}, {"rounds": 17}, {"ops": []}, {"inject_op": "sdot4", "inject_waves": -1},
               {"ops": ["bfrev"], "inject_op": "sdot4", "inject_waves": 1}):
        with pytest.raises(RuntimeError, match="vector ALU check: bad arguments"):
            valu.valu_check(**kw)
    with pytest.raises(ValueError):
        valu.valu_check(ops=["everything"])
    with pytest.raises(ValueError):
        valu.expected("exp2_f32")  # no host reference for a consensus op
    with pytest.raises(ValueError):
        valu.operands("sdot4", 1, 17)
    with pytest.raises(ValueError):
        valu.reduce([_rec(1 << 14)], ["int"], ["sdot4"])
    with pytest.raises(ValueError):
        valu.reduce([_rec(SITES[0])], ["f64"], ["sdot4"])
