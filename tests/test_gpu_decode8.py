"""The fp8 decode-attention check on a GPU (``ops/decode8``): the two kernels against float64 numpy
softmax attention over the gathered, dequantised pages on every element, the exact data sets bit
for bit, and the check's fault injection.

The bounds are derived, not measured (``decode8_host.h``): e4m3 -> bf16 is exact, P is rounded to
bf16 (2^-9 relative per term, once more for the sum), and the fp32 steps (the folded score factor on
base-2 scores of at most 130, the merges, the division, the ``v_scale`` multiply) stay below 2^-13:
``|o - ref| <= (2^-8 + 2^-13) max|V| v_scale`` and ``|lse - ref| <= 2^-8 + 2^-20 |ref|``."""
import numpy as np
import pytest

from k8s_gpu_device_plugin_amd.ops import decode8

pytestmark = pytest.mark.gpu

# the 256 e4m3 values: bias 7, subnormals below 2^-6, 0x7F / 0xFF NaN
E4M3 = np.array([(-1.0) ** (c >> 7) * (np.nan if c & 0x7F == 0x7F else
                                       (c & 7) / 8 * 2.0 ** -6 if (c >> 3) & 15 == 0 else (1 + (c & 7) / 8) * 2.0 ** (((c >> 3) & 15) - 7))
                 for c in range(256)])


def to_bits(x):
    """float -> bf16 bit patterns, round to nearest even."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def codes(rng, shape, top=0x47):
    """Random e4m3 codes: sign bit free, low 7 bits <= top (0x47: |x| <= 3.75), so never a NaN code."""
    return (rng.integers(0, top + 1, shape) | (rng.integers(0, 2, shape) << 7)).astype(np.uint8)


def assert_within_bounds(rng, q, k, v, lens, splits, k_scale=None):
    """``q`` [B, Hq, 128] in float, ``k`` and ``v`` [B, Hkv, S, 128] as codes, behind a shuffled table
    with three spare pages; every byte no visible key owns is 0xFF.  Every element of o and lse."""
    hq, hkv = q.shape[1], k.shape[1]
    ks = np.float32(0.37) + np.float32(0.11) * np.arange(hkv, dtype=np.float32) if k_scale is None else np.full(hkv, k_scale, np.float32)
    vs = np.float32(1.7) - np.float32(0.3) * np.arange(hkv, dtype=np.float32)
    pages = [-(-n // 16) for n in lens]
    order = rng.permutation(sum(pages) + 3)
    kc, vc = (np.full((len(order), hkv, 16, 128), 0xFF, np.uint8) for _ in range(2))
    table, at = np.full((len(lens), max(pages)), -1, np.int32), 0
    for b, n in enumerate(lens):
        table[b, :pages[b]] = order[at:at + pages[b]]
        at += pages[b]
        for j in range(n):
            kc[table[b, j // 16], :, j % 16], vc[table[b, j // 16], :, j % 16] = k[b, :, j], v[b, :, j]
    o, lse = decode8.decode_attention(to_bits(q), kc, vc, ks, vs, table, lens, splits=splits)
    qf = (to_bits(q).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    kf, vf = E4M3[k] * ks.astype(np.float64)[None, :, None, None], E4M3[v] * vs.astype(np.float64)[None, :, None, None]
    for b, n in enumerate(lens):
        s = np.einsum("hd,hjd->hj", qf[b], kf[b, :, :n].repeat(hq // hkv, 0)) / np.sqrt(128.0)
        assert np.abs(s).max() * np.log2(np.e) <= 130  # what the small term of the bound was derived for
        m = s.max(axis=1, keepdims=True)
        p = np.exp(s - m)
        ref_o = np.einsum("hj,hjd->hd", p / p.sum(axis=1, keepdims=True), vf[b, :, :n].repeat(hq // hkv, 0))
        ref_lse = (m + np.log(p.sum(axis=1, keepdims=True)))[:, 0]
        bound = (2.0 ** -8 + 2.0 ** -13) * np.abs(E4M3[v]).max() * vs.astype(np.float64).repeat(hq // hkv)[:, None]
        o_err, lse_err = np.abs(o[b] - ref_o), np.abs(lse[b] - ref_lse)
        print("seq %d: max |o - ref| / bound %.3g, max |lse - ref| %.3g of %.3g" % (b, (o_err / bound).max(), lse_err.max(), 2.0 ** -8))
        assert (o_err <= bound).all()
        assert (lse_err <= 2.0 ** -8 + 2.0 ** -20 * np.abs(ref_lse)).all()


@pytest.mark.parametrize("lens, hq, hkv, splits", [
    ([1], 4, 1, 1),      # one key; three waves empty
    ([16], 4, 1, 1),     # a whole page
    ([17], 4, 1, 1),     # one key into the second page
    ([33], 4, 1, 1),     # the second wave
    ([128], 4, 1, 1),    # a whole tile
    ([129], 4, 1, 1),    # the second tile: both stages
    ([300], 4, 1, 1),    # stage parity wraps
    ([300], 4, 1, 2),    # partitions of 2 tiles and 1
    ([300], 4, 1, 3),
    ([300], 4, 1, 8),    # empty partitions
    ([300], 2, 2, 2),    # G = 1, two KV heads
    ([300], 16, 1, 2),   # G = 16
    ([1, 129, 300, 77], 8, 2, 3),   # a mixed batch, two KV heads
    ([1, 129, 300, 77], 8, 2, 0),   # ... and the library's choice of splits
])
def test_decode_attention_against_float64_on_random_codes(lens, hq, hkv, splits):
    rng = np.random.default_rng(sum(lens) * 1009 + hq * 101 + hkv * 11 + splits)
    q = rng.standard_normal((len(lens), hq, 128))
    k, v = (codes(rng, (len(lens), hkv, max(lens), 128)) for _ in range(2))
    assert_within_bounds(rng, q, k, v, lens, splits)


def test_a_late_peak_rescales_both_merges():
    """Head g scores about 40 above everything else at key 290 + g: the second wave of the last of
    three partitions.  The first wave's state shrinks by about 2^-57 in the merge through LDS, the
    first two partitions' states in the merge through HBM."""
    rng = np.random.default_rng(7)
    q, k = np.zeros((1, 4, 128)), codes(rng, (1, 1, 300, 128), top=0x38)  # |x| <= 1
    g = np.arange(4)
    q[0, g, g] = 22.75
    k[0, 0, 290 + g, g] = 0x5A  # 20 = 1.25 * 2^4; 22.75 * 20 / sqrt(128) = 40.2
    assert E4M3[0x5A] == 20.0
    assert_within_bounds(rng, q, k, codes(rng, (1, 1, 300, 128)), [300], 3, k_scale=1.0)


@pytest.mark.parametrize("name", decode8.SETS[:2])
@pytest.mark.parametrize("splits", [1, 3])
def test_exact_sets_are_bit_equal_to_the_closed_form(name, splits):
    q, kc, vc, ks, vs, table, lens = decode8.operands(name, 4, 8, 2, 300)  # lengths in 150 .. 300, one of them odd
    want_o, want_lse = decode8.expected(name, 4, 8, 2, 300)
    o, lse = decode8.decode_attention(q, kc, vc, ks, vs, table, lens, splits=splits)
    assert np.array_equal(o.view(np.uint32), want_o.view(np.uint32))
    assert (np.abs(lse - want_lse) <= 2.0 ** -8 + 2.0 ** -20 * np.abs(want_lse)).all()


def test_decode_check_and_its_fault_injection():
    b, hq, hkv, s = 4, 8, 2, 300
    r = decode8.decode_check(0, b, hq, hkv, s, splits=3, iters=2)
    print("hashed max_err / v_scale %.3g of %.3g, max_lse_err %.3g" % (r["max_err"], (2.0 ** -8 + 2.0 ** -13) * 4, r["max_lse_err"]))
    assert r["ok"] and r["error"] == "" and r["decode8_errors"] == r["o_errors"] == r["lse_errors"] == 0, r
    assert (r["batch"], r["q_heads"], r["kv_heads"], r["seq"], r["splits"]) == (b, hq, hkv, s, 3) and r["kv_gbps"] > 0 and r["ms"] > 0
    r = decode8.decode_check(0, b, hq, hkv, s, splits=3, iters=1, inject=True)
    assert not r["ok"] and [r["sets"][n]["o_errors"] for n in decode8.SETS] == [1, 1, 1] and r["lse_errors"] == 0, r
    assert r["error"] == "decode8 path: 1 wrong element in uniform (first at seq 2, head 7, d 5; 4x8/2x300, 3 splits)"
    r = decode8.decode_check(0, b, hq, hkv, s, splits=3, iters=1, skip_verified_launch=True)
    for name in decode8.SETS:
        assert r["sets"][name] == {"o_errors": b * hq * 128, "lse_errors": b * hq, "ms": r["sets"][name]["ms"]}, r
