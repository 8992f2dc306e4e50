"""The attention-path check on a GPU (``ops/attn``): the fused kernel against float64 numpy softmax
attention on every element, the exact data sets bit for bit, and the check's fault injection.

The bounds are derived, not measured: P is rounded to bf16 (2^-9 relative per term) and the row sum
may be taken from the rounded values (2^-9 again), so ``|o - ref| <= 2^-8 max|V|`` and
``|lse - ref| <= 2^-8 + 2^-20 |ref|``."""
import numpy as np
import pytest

from k8s_gpu_device_plugin_amd.ops import attn

pytestmark = pytest.mark.gpu


def to_bits(x):
    """float -> bf16 bit patterns, round to nearest even."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bits(b):
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def reference(q, k, v, causal):
    s = np.einsum("hid,hjd->hij", q, k) / np.sqrt(128.0)
    if causal:
        i, j = np.arange(q.shape[1])[:, None], np.arange(k.shape[1])[None, :]
        s = np.where(j <= i + (k.shape[1] - q.shape[1]), s, -np.inf)
    m = s.max(axis=2, keepdims=True)
    p = np.exp(s - m)
    l = p.sum(axis=2, keepdims=True)
    return np.einsum("hij,hjd->hid", p / l, v), (m + np.log(l))[:, :, 0]


def assert_within_bounds(qb, kb, vb, causal):
    q, k, v = from_bits(qb), from_bits(kb), from_bits(vb)
    o, lse = attn.attention(qb, kb, vb, causal=causal)
    ref_o, ref_lse = reference(q, k, v, causal)
    o_err, lse_err = np.abs(o - ref_o).max(), np.abs(lse - ref_lse)
    print("max |o - ref| %.3g of %.3g, max |lse - ref| %.3g" % (o_err, np.abs(v).max() / 256, lse_err.max()))
    assert o_err <= np.abs(v).max() / 256
    assert (lse_err <= 2.0 ** -8 + 2.0 ** -20 * np.abs(ref_lse)).all()


@pytest.mark.parametrize("h, sq, sk, causal", [
    (1, 128, 64, False),    # prologue only
    (1, 128, 128, False),   # both buffers
    (1, 128, 192, False),   # buffer parity wraps
    (3, 256, 320, False),   # several query blocks and heads
    (1, 128, 128, True),    # a diagonal tile in every block
    (2, 256, 256, True),    # skipped tiles
    (1, 128, 320, True),    # the offset Sk - Sq
])
def test_attention_against_float64_on_random_inputs(h, sq, sk, causal):
    rng = np.random.default_rng(h * 1000003 + sq * 1009 + sk + causal)
    qb, kb, vb = (to_bits(rng.standard_normal((h, n, 128))) for n in (sq, sk, sk))
    assert_within_bounds(qb, kb, vb, causal)


def test_a_late_peak_rescales_the_accumulators():
    """Query i scores about 40 above everything else at one key of the last tile, so the running
    maximum moves there and everything accumulated before shrinks by 2^-57."""
    rng = np.random.default_rng(7)
    q, k = np.zeros((1, 128, 128)), 0.5 * rng.standard_normal((1, 256, 128))
    i = np.arange(128)
    q[0, i, i] = 22.75
    k[0, 192 + (5 * i) % 64, i] = 20.0  # 22.75 * 20 / sqrt(128) = 40.2
    assert_within_bounds(to_bits(q), to_bits(k), to_bits(rng.integers(-4, 5, (1, 256, 128))), False)


@pytest.mark.parametrize("name", attn.SETS[:2])
@pytest.mark.parametrize("sk, causal", [(192, False), (320, True)])
def test_exact_sets_are_bit_equal_to_the_closed_form(name, sk, causal):
    q, k, v = attn.operands(name, 2, 256, sk)
    want_o, want_lse = attn.expected(name, 2, 256, sk, causal)
    o, lse = attn.attention(q, k, v, causal=causal)
    assert np.array_equal(o.view(np.uint32), want_o.view(np.uint32))
    assert (np.abs(lse - want_lse) <= 2.0 ** -8 + 2.0 ** -20 * np.abs(want_lse)).all()


@pytest.mark.parametrize("causal", [False, True])
def test_attention_check_and_its_fault_injection(causal):
    h, s = 4, 256
    r = attn.attention_check(0, h, s, s, causal, iters=2)
    print("hashed max_err %.3g of %.3g, max_lse_err %.3g" % (r["max_err"], 2.0 ** -6, r["max_lse_err"]))
    assert r["ok"] and r["error"] == "" and r["attn_errors"] == r["o_errors"] == r["lse_errors"] == 0, r
    assert (r["heads"], r["seq_q"], r["seq_k"], r["causal"]) == (h, s, s, causal) and r["tflops"] > 0 and r["ms"] > 0
    r = attn.attention_check(0, h, s, s, causal, iters=1, inject=True)
    assert not r["ok"] and [r["sets"][n]["o_errors"] for n in attn.SETS] == [1, 1, 1] and r["lse_errors"] == 0, r
    assert r["error"] == "attention path: 1 wrong element in uniform (first at head 2, row 255, d 5; %s4x256x256)" % (
        "causal, " if causal else "")
    r = attn.attention_check(0, h, s, s, causal, iters=1, skip_verified_launch=True)
    for name in attn.SETS[:2]:
        assert r["sets"][name] == {"o_errors": h * s * 128, "lse_errors": h * s, "ms": r["sets"][name]["ms"]}, r
    assert r["sets"]["hashed"]["o_errors"] == h * 8 * 128 and r["sets"]["hashed"]["lse_errors"] == h * 8
