"""The vector-ALU check on the GPU: the healthy run, the smallest shapes, every exact op's raw
results against the independent model (``tests/valu_model.py``), the transcendentals against
float64, and fault injection."""
import numpy as np
import pytest

import valu_model as model
from k8s_gpu_device_plugin_amd.ops import valu

pytestmark = pytest.mark.gpu

EXACT_OPS = [op for op in valu.OPS if valu.op_info(op)["cls"] == "exact"]
# Twice the largest error measured on an MI355X over valu.operands(op, valu.SEED, 16), in ulps of
# the result type, at least 1 (profiles/valu/approx_ulp.json; measured: 0.6212, 0.9910, 0.8270,
# 0.7940, 0.8338, 8.624, 1.952, 2.1027e8, 2.2062e8, and 0.4995, 0.4998, 0.4998 for the f16 three).
# v_rcp_f64 and v_rsq_f64 are seeds of about 25 bits.
ULP_BOUND = {"exp2_f32": 1.242, "log2_f32": 1.982, "rcp_f32": 1.654, "rsq_f32": 1.588, "sqrt_raw_f32": 1.668,
             "sin_f32": 17.25, "cos_f32": 3.905, "rcp_f64": 4.2054e8, "rsq_f64": 4.4124e8,
             "exp2_f16": 1.0, "log2_f16": 1.0, "rcp_f16": 1.0}


def test_healthy_defaults():
    r = valu.valu_check()
    assert r["ok"] and r["valu_errors"] == 0 and r["error"] == "" and not any(r["errors"].values()), r["error"]
    assert r["cus_reached"] == r["cus_expected"] and r["simds_reached"] == 4 * r["cus_reached"]
    assert 1 <= r["launches"] <= 4 and r["unjudged"] == [] and r["rounds"] == valu.ROUNDS
    assert r["ops"] == list(valu.OPS) and set(r["group_ms"]) == set(valu.GROUPS)
    for group, sites in r["wave_sites"].items():  # the first four waves: the four SIMDs of one CU
        assert len({s.rsplit("/", 1)[0] for s in sites[:4]}) == 1 and len(set(sites[:4])) == 4, (group, sites[:4])


@pytest.mark.parametrize("rounds, ops", [(1, None), (3, None), (3, ["cvt_pk_fp8_f32", "cvt_f32_bf8"])],
                         ids=["one round", "three rounds", "one group"])
def test_smallest_shapes(rounds, ops):
    r = valu.valu_check(blocks=8, rounds=rounds, ops=ops)
    groups = len(valu.GROUPS) if ops is None else 1
    assert r["ok"] and r["valu_errors"] == 0 and r["launches"] == 1, r["error"]
    assert r["waves"] + r["moved"] == 32 * groups and len(r["group_ms"]) == groups
    assert all(len(sites) == 32 for sites in r["wave_sites"].values())


@pytest.mark.parametrize("op", EXACT_OPS)
def test_raw_results_are_the_model_s(op):
    a, b, c = valu.operands(op, valu.SEED, 2)
    got = valu.raw(op, a, b, c)
    want = np.array(model.results(op, a, b, c, valu.expand), dtype=np.uint32)
    assert got.shape == want.shape and (got == want).all(), np.argwhere((got != want).any(axis=2))[:8].tolist()


@pytest.mark.parametrize("op", sorted(ULP_BOUND))
def test_transcendentals_stay_within_their_ulp_bound(op):
    a, _, _ = valu.operands(op, valu.SEED, 16)
    got = valu.raw(op, a)
    worst = max(model.approx_error_ulp(op, int(x), words) for x, words in zip(a.ravel(), got.reshape(-1, got.shape[2])))
    print("%s: largest error %.4g ulp (bound %.4g)" % (op, worst, ULP_BOUND[op]))
    assert worst <= ULP_BOUND[op]


@pytest.mark.parametrize("op", ["sdot4", "bitop3_ca", "div_f32", "sqrt_f64", "pk_fma_f16", "cvt_scalef32_pk_fp4_f32", "exp2_f32"])
def test_injection_is_reported_at_the_sites_of_the_first_three_waves(op):
    r = valu.valu_check(inject_op=op, inject_waves=3)
    first = r["wave_sites"][valu.op_info(op)["group"]][:3]
    assert not r["ok"] and r["valu_errors"] == 3 and r["unlocated_errors"] == 0
    assert {k: v for k, v in r["errors"].items() if v} == {op: 3}
    assert sorted(r["bad_sites"]) == sorted(first) and r["bad_by"][op]["sites"] == 3
    assert r["error"].startswith("vector ALU check: 3 wrong results in %s at %s" % (op, r["bad_sites"][0]))
