"""The block-scaled matrix path (``ops/mxgemm``) on a real MI355X: ``mx_gemm`` against numpy
references (int64 on integers, bit for bit; one-hot operands that put every element and every scale
byte in its place; float64 on random codes and scales), and the check itself with its two fault
injections.  Every case runs for each format and each kernel id; T is the kernel's tile edge and
BK the k of one K-tile."""
import numpy as np
import pytest

from matforms_model import DECODE, e8m0

pytestmark = pytest.mark.gpu

ENC = {"fp8": "e4m3", "bf8": "e5m2", "fp4": "e2m1"}
ONE = {"fp8": 0x38, "bf8": 0x3C, "fp4": 0x2}  # the code of 1.0
CASES = [(fmt, kernel) for fmt in ENC for kernel in (1, 2)]
both = pytest.mark.parametrize("fmt, kernel", CASES)


def _shape(fmt, kernel, tm, tn, tk):
    from k8s_gpu_device_plugin_amd.ops import mxgemm
    t = mxgemm.KERNELS[kernel]["tile"]
    return tm * t, tn * t, tk * mxgemm.tile_k(fmt)


def _random_codes(rng, shape, fmt):  # as tests/test_gpu_datapath.py: every finite code of the format
    if fmt == "fp4":
        return rng.integers(0, 16, size=shape, dtype=np.uint8)
    c = rng.integers(0, 256, size=shape, dtype=np.uint8)
    bad = (c & 0x7F) == 0x7F if fmt == "fp8" else (c & 0x7C) == 0x7C
    return np.where(bad, c & 0x83, c).astype(np.uint8)


def _bits(c):
    return np.ascontiguousarray(c, dtype=np.float32).view(np.uint32)


@both
@pytest.mark.parametrize("tiles", [(1, 1, 1), (1, 1, 2), (1, 1, 3), (9, 1, 1), (2, 3, 2)])
def test_integer_product_is_bit_exact(fmt, kernel, tiles):
    """Integers in [-4, 4], scales of 2^0 or 2^1, against an int64 product with the shifts: the
    prologue alone, both buffer parities, 9 tiles (xcd_remap with a remainder), a 2 x 3 grid."""
    from k8s_gpu_device_plugin_amd.ops import mxgemm
    m, n, k = _shape(fmt, kernel, *tiles)
    rng = np.random.default_rng(m + 7 * n + 13 * k + len(fmt) + kernel)
    dec = DECODE[ENC[fmt]](np.arange(16 if fmt == "fp4" else 256))
    code_of = np.array([int(np.flatnonzero(dec == v)[0]) for v in range(-4, 5)], dtype=np.uint8)
    av, bv = rng.integers(-4, 5, size=(m, k)), rng.integers(-4, 5, size=(n, k))
    sa = rng.integers(127, 129, size=(m, k // 32), dtype=np.uint8)
    sb = rng.integers(127, 129, size=(n, k // 32), dtype=np.uint8)
    c = mxgemm.mx_gemm(code_of[av + 4], code_of[bv + 4], sa, sb, fmt=fmt, kernel=kernel)
    ref = (av << np.repeat(sa.astype(np.int64) - 127, 32, axis=1)) @ (bv << np.repeat(sb.astype(np.int64) - 127, 32, axis=1)).T
    wrong = np.argwhere(_bits(c) != _bits(ref))
    assert wrong.size == 0, (len(wrong), wrong[:4], c[tuple(wrong[0])], ref[tuple(wrong[0])])


@both
@pytest.mark.parametrize("tiles", [(1, 1, 3), (3, 3, 2)])
def test_every_element_and_every_scale_byte_is_in_its_place(fmt, kernel, tiles):
    """A one-hot A (1.0 at k = i % K, unit scales) copies column i % K of the random Bt, times its
    scale, into row i of C, and a one-hot Bt does the same with A: one product plus zeros, so the
    result is exact.  The accumulators start at +0 and -0 + +0 is +0, hence the ``+ 0.0``."""
    from k8s_gpu_device_plugin_amd.ops import mxgemm
    m, n, k = _shape(fmt, kernel, *tiles)
    rng = np.random.default_rng(3 * m + n + k + len(fmt) + kernel)
    for rows, others, swapped in ((m, n, False), (n, m, True)):
        at = np.arange(rows) % k
        hot = np.zeros((rows, k), dtype=np.uint8)
        hot[np.arange(rows), at] = ONE[fmt]
        unit = np.full((rows, k // 32), 127, dtype=np.uint8)
        x = _random_codes(rng, (others, k), fmt)
        sx = rng.integers(124, 131, size=(others, k // 32), dtype=np.uint8)
        c = mxgemm.mx_gemm(x, hot, sx, unit, fmt, kernel=kernel) if swapped else mxgemm.mx_gemm(hot, x, unit, sx, fmt, kernel=kernel)
        expect = (DECODE[ENC[fmt]](x[:, at]) * e8m0(sx[:, at // 32])).T + 0.0  # [rows, others]
        expect = expect.T if swapped else expect
        wrong = np.argwhere(_bits(c) != _bits(expect))
        assert wrong.size == 0, (swapped, len(wrong), wrong[:4], c[tuple(wrong[0])], expect[tuple(wrong[0])])


@both
@pytest.mark.parametrize("tiles", [(1, 1, 2), (2, 3, 3)])
def test_random_codes_and_scales_match_float64(fmt, kernel, tiles):
    """Every finite code and scales of 2^-3 .. 2^3 against the float64 product of the decoded
    operands, under the bounds ``test_lowp_gemm_matches_torch_fp32`` holds the same instruction to
    (profiles/r2/lowp_numerics.md): 1e-3 of sum|a||b| for the 8-bit formats, 1e-5 for fp4."""
    from k8s_gpu_device_plugin_amd.ops import mxgemm
    m, n, k = _shape(fmt, kernel, *tiles)
    rng = np.random.default_rng(m * 1000 + n * 10 + k + len(fmt) + kernel)
    a, bt = _random_codes(rng, (m, k), fmt), _random_codes(rng, (n, k), fmt)
    sa = rng.integers(124, 131, size=(m, k // 32), dtype=np.uint8)
    sb = rng.integers(124, 131, size=(n, k // 32), dtype=np.uint8)
    c = mxgemm.mx_gemm(a, bt, sa, sb, fmt=fmt, kernel=kernel)
    af = DECODE[ENC[fmt]](a) * np.repeat(e8m0(sa), 32, axis=1)
    bf = DECODE[ENC[fmt]](bt) * np.repeat(e8m0(sb), 32, axis=1)
    err = np.abs(c - af @ bf.T) / np.maximum(np.abs(af) @ np.abs(bf).T, 1e-30)
    print("mx_gemm %s kernel %d %dx%dx%d: max error %.3g of sum|a||b|" % (fmt, kernel, m, n, k, err.max()))
    assert err.max() < (1e-5 if fmt == "fp4" else 1e-3), (err.max(), np.unravel_index(err.argmax(), err.shape))


@both
@pytest.mark.parametrize("tiles", [(1, 1, 1), (3, 2, 3)])
def test_check_is_clean_and_counts_both_injections(fmt, kernel, tiles):
    from k8s_gpu_device_plugin_amd.ops import mxgemm
    m, n, k = _shape(fmt, kernel, *tiles)
    clean = mxgemm.mx_gemm_check(0, m, n, k, fmt=fmt, iters=1, kernel=kernel)
    assert clean["ok"] and clean["mxgemm_errors"] == 0 and clean["error"] == "" and clean["kernel"] == kernel, clean
    hit = mxgemm.mx_gemm_check(0, m, n, k, fmt=fmt, iters=1, kernel=kernel, inject=True)
    assert not hit["ok"] and (hit[fmt]["row_errors"], hit[fmt]["col_errors"]) == (1, 1), hit
    assert hit["error"] == "mx matrix path: 1 wrong row and 1 wrong column in %s (kernel %d, %dx%dx%d)" % (fmt, kernel, m, n, k)
    skipped = mxgemm.mx_gemm_check(0, m, n, k, fmt=fmt, iters=1, kernel=kernel, skip_verified_launch=True)
    assert skipped["mxgemm_errors"] == m + n, skipped


def test_the_default_call_passes_and_reports_a_rate_for_each_format():
    from k8s_gpu_device_plugin_amd.ops import canary, mxgemm
    r = mxgemm.mx_gemm_check()
    assert r["ok"] and r["error"] == "", r
    for fmt in ENC:
        print("mx_gemm %s 4096^3 kernel %d: %.0f TFLOP/s; register-resident chain %.0f"
              % (fmt, r["kernel"], r[fmt]["tflops"], canary.lowp_rate(0, fmt, 2048)))
        assert r[fmt]["tflops"] > 0
