"""The matrix path of the canary on a real MI355X, every comparison exact.

Bit-exact GEMM: every kernel id of ``canary.GEMM_KERNELS`` (and ``mfma_gemm``) on integer
operands against an int64 numpy product, element by element, at the smallest shapes that reach
each mechanism (K-tile counts 1-5 and 16, grids with an XCD-remap remainder, ragged raster
groups).  ABFT: every id through ``gemm_rate`` clean, with one injected element and with the
verified launch skipped; and the verifier alone (``canary.abft``) against corruptions whose
verdict is known by construction or predicted by the numpy model of ``tests/abft_model.py``.

numpy references only: torch's HIP runtime and the canary's cannot own the device in one process
(see ``test_lds_gemm_rate_and_abft`` in ``tests/test_gpu.py``)."""
import functools

import numpy as np
import pytest

import abft_model as model
from k8s_gpu_device_plugin_amd.ops import canary

pytestmark = pytest.mark.gpu

IDS_256 = list(range(2, 12))
# (256, 256, K): K-tile counts 1-5 and 16 = the prologue with and without tile 1, the first
# stage_ah1(t + 1) at t = 1, both buffer parities, retire's vmcnt(0) tail against its steady count;
# 9 tiles (9x1): xcd_remap with a remainder and a ragged group for 2, 4 and 8; 10 tiles (5x2); 3x3; one tile row
SHAPES_256 = [(256, 256, k) for k in (64, 128, 192, 256, 320, 1024)] + \
    [(2304, 256, 64), (1280, 512, 128), (768, 768, 128), (256, 1024, 192)]
SHAPES_128 = [(128, 128, 64), (128, 128, 128), (128, 128, 192), (1152, 128, 64), (640, 256, 128), (384, 384, 256)]
SHAPES_MFMA = [(32, 32, 16), (96, 64, 48), (64, 160, 256)]
BOUNDS = (4, 16)  # the canary's own operand range; [-16, 16] with K <= 1024 keeps |C| <= 2^18


@functools.lru_cache(maxsize=None)
def _random_case(shape, bound):
    """(A bits [M, K], Bt bits [N, K], reference): computed once, shared by every kernel id."""
    m, n, k = shape
    assert bound * bound * k <= 1 << 24
    rng = np.random.default_rng(m * 7919 + n * 131 + k + bound)
    a = rng.integers(-bound, bound + 1, size=(m, k), dtype=np.int64)
    bt = rng.integers(-bound, bound + 1, size=(n, k), dtype=np.int64)
    ref = (a.astype(np.int64) @ bt.T.astype(np.int64)).astype(np.float32)
    out = (model.bf16_bits(a), model.bf16_bits(bt), ref)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _one_hot_case(shape, hot):
    """The structured case: one operand one-hot at column (row index % K), the other a position
    code in [-125, 125], so C[i][j] = Bt[j][i % K] (hot = "a") or A[i][j % K] (hot = "b") and a
    wrong row, k chunk or swizzle shows as a foreign code.  Returns int arrays and the reference."""
    m, n, k = shape
    cols = np.arange(k)[None, :]

    def code(rows):
        return ((np.arange(rows)[:, None] * k + cols) % 251 - 125).astype(np.int64)

    def one_hot(rows):
        return (cols == (np.arange(rows) % k)[:, None]).astype(np.int64)

    a, bt = (one_hot(m), code(n)) if hot == "a" else (code(m), one_hot(n))
    ref = (a.astype(np.int64) @ bt.T.astype(np.int64)).astype(np.float32)
    want = bt[:, np.arange(m) % k].T if hot == "a" else a[:, np.arange(n) % k]
    assert (ref == want).all()
    for x in (a, bt, ref):
        x.setflags(write=False)
    return a, bt, ref


def _assert_bit_exact(c, ref, tile, what, explain=None):
    wrong = np.argwhere(c.view(np.uint32) != ref.view(np.uint32))
    if len(wrong) == 0:
        return
    i, j = (int(x) for x in wrong[0])
    tiles = sorted({(int(r) // tile, int(q) // tile) for r, q in wrong})
    msg = ("%s: %d of %d elements wrong; first at (row %d, col %d) = %d-tile (%d, %d) offset (%d, %d): got %r "
           "(0x%08x), want %r (0x%08x); tiles with a wrong element: %s"
           % (what, len(wrong), c.size, i, j, tile, i // tile, j // tile, i % tile, j % tile, float(c[i, j]),
              int(c.view(np.uint32)[i, j]), float(ref[i, j]), int(ref.view(np.uint32)[i, j]), tiles[:12]))
    if explain is not None:
        msg += "; " + explain(i, j, float(c[i, j]))
    print(msg)
    pytest.fail(msg)


def _foreign_code(a, bt, hot):
    """Where the value a wrong element holds lives in the coded operand: names the fault."""
    k = a.shape[1]

    def explain(i, j, got):
        coded, row, col = (bt, j, i % k) if hot == "a" else (a, i, j % k)
        in_row = [int(x) for x in np.flatnonzero(coded[row] == got)[:8]]
        in_col = [int(x) for x in np.flatnonzero(coded[:, col] == got)[:8]]
        return ("the %s operand holds the got value in its row %d at k = %s (wanted k = %d: 16 B chunk %d of "
                "K-tile %d) and in column k = %d at rows %s (wanted row %d)"
                % ("Bt" if hot == "a" else "A", row, in_row, col, (col % 64) // 8, col // 64, col, in_col, row))
    return explain


# ---- bit-exact GEMM --------------------------------------------------------------------------
@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("shape", SHAPES_256, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("kid", IDS_256)
def test_gemm256_kernels_are_bit_exact_on_integers(kid, shape, bound):
    a, bt, ref = _random_case(shape, bound)
    c = canary.gemm(a, bt, device=0, kernel=kid)
    _assert_bit_exact(c, ref, 256, "kernel %d, shape %s, operands in [-%d, %d]" % (kid, shape, bound, bound))


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("shape", SHAPES_128, ids=lambda s: "%dx%dx%d" % s)
def test_gemm_lds_is_bit_exact_on_integers(shape, bound):
    a, bt, ref = _random_case(shape, bound)
    c = canary.gemm(a, bt, device=0, kernel=1)
    _assert_bit_exact(c, ref, 128, "kernel 1, shape %s, operands in [-%d, %d]" % (shape, bound, bound))


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("shape", SHAPES_MFMA, ids=lambda s: "%dx%dx%d" % s)
def test_mfma_gemm_is_bit_exact_on_integers(shape, bound):
    a, bt, ref = _random_case(shape, bound)
    c = canary.mfma_gemm(a, np.ascontiguousarray(bt.T), device=0)  # B [K, N] row-major
    _assert_bit_exact(c, ref, 32, "mfma_gemm, shape %s, operands in [-%d, %d]" % (shape, bound, bound))


@pytest.mark.parametrize("hot", ["a", "b"])
@pytest.mark.parametrize("shape", [(256, 256, 320), (768, 768, 128)], ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("kid", IDS_256)
def test_gemm256_kernels_move_every_operand_element_to_its_place(kid, shape, hot):
    a, bt, ref = _one_hot_case(shape, hot)
    c = canary.gemm(model.bf16_bits(a), model.bf16_bits(bt), device=0, kernel=kid)
    _assert_bit_exact(c, ref, 256, "kernel %d, shape %s, one-hot %s" % (kid, shape, hot), _foreign_code(a, bt, hot))


@pytest.mark.parametrize("hot", ["a", "b"])
@pytest.mark.parametrize("shape", [(128, 128, 192), (384, 384, 256)], ids=lambda s: "%dx%dx%d" % s)
def test_gemm_lds_moves_every_operand_element_to_its_place(shape, hot):
    a, bt, ref = _one_hot_case(shape, hot)
    c = canary.gemm(model.bf16_bits(a), model.bf16_bits(bt), device=0, kernel=1)
    _assert_bit_exact(c, ref, 128, "kernel 1, shape %s, one-hot %s" % (shape, hot), _foreign_code(a, bt, hot))


@pytest.mark.parametrize("hot", ["a", "b"])
@pytest.mark.parametrize("shape", [(96, 64, 48), (64, 160, 256)], ids=lambda s: "%dx%dx%d" % s)
def test_mfma_gemm_moves_every_operand_element_to_its_place(shape, hot):
    a, bt, ref = _one_hot_case(shape, hot)
    c = canary.mfma_gemm(model.bf16_bits(a), np.ascontiguousarray(model.bf16_bits(bt).T), device=0)
    _assert_bit_exact(c, ref, 32, "mfma_gemm, shape %s, one-hot %s" % (shape, hot), _foreign_code(a, bt, hot))


# ---- ABFT on the canary's own integer data, every kernel id ---------------------------------------
# id 1 also at the first two shapes halved to 128-multiples that no 256-tile kernel takes
RATE_CASES = [(kid, shape) for kid in range(1, 12) for shape in [(256, 256, 64), (768, 512, 320), (2304, 256, 128)]] + \
    [(1, (128, 128, 64)), (1, (384, 256, 320))]


@pytest.mark.parametrize("kid, shape", RATE_CASES, ids=lambda v: "%dx%dx%d" % v if isinstance(v, tuple) else str(v))
def test_abft_of_every_kernel_clean_injected_and_unwritten(kid, shape):
    m, n, _ = shape
    clean = canary.gemm_rate(0, *shape, iters=1, kernel=kid)
    assert clean["errors"] == 0, clean
    bad = canary.gemm_rate(0, *shape, iters=1, kernel=kid, inject=True)
    assert bad["errors"] == 2, bad
    # the product that is verified is written after the poison: without that launch the
    # verifier sees the poison in every row and every column
    unwritten = canary.gemm_rate(0, *shape, iters=1, kernel=kid, skip_verified_launch=True)
    assert unwritten["errors"] == m + n, unwritten


# ---- ABFT sensitivity: the verifier alone, no GEMM kernel involved ---------------------------------
def _check_cases(a, bt, cases):
    misses = []
    n_cases = 0
    for label, bad_c, want in cases:
        got = canary.abft(a, bt, bad_c, device=0)
        n_cases += 1
        if got != want:
            misses.append("%s: got %s, want %s" % (label, got, want))
    print("%d cases, %d missed" % (n_cases, len(misses)))
    assert not misses, "%d of %d cases: %s" % (len(misses), n_cases, "; ".join(misses[:12]))


@pytest.mark.parametrize("shape, bound", model.DATASETS)
def test_abft_verdict_on_hand_built_corruptions(shape, bound):
    """Clean (0, 0); one element replaced by +-1, +-0.5, 2^-20, NaN, +-Inf, -0 or its neighbour's
    value (1, 1); +1 and -1 in one row (0, 2), in one column (2, 0); and the rectangle of +d -d
    -d +d, which cancels in both of its rows and both of its columns: (0, 0), the limit inherent
    to row and column checksums."""
    a, bt, c = model.dataset(shape, bound)
    _check_cases(a, bt, model.hand_built_cases(c))


@pytest.mark.parametrize("shape, bound", model.SWEEP_DATASETS)
def test_abft_sees_every_bit_of_an_element(shape, bound):
    """Each of the 32 bits of a zero, of the largest element, of the corners and of the elements
    either side of index 63/64 and 255/256: one flipped bit is one wrong row and one wrong column."""
    a, bt, c = model.dataset(shape, bound)
    _check_cases(a, bt, model.bit_sweep_cases(c))


@pytest.mark.parametrize("shape, bound", [((65, 130, 257), 4), ((300, 70, 1000), 64)])
def test_abft_verdict_on_random_corruptions_matches_the_model(shape, bound):
    a, bt, c = model.dataset(shape, bound)
    cases = []
    for seed in range(20):
        bad_c = model.random_corruption(c, np.random.default_rng(100 + seed))
        cases.append(("seed %d" % (100 + seed), bad_c, model.verdict(a, bt, bad_c)))
    assert len({want for _, _, want in cases}) >= 3  # the draw is varied, not twenty times (1, 1)
    _check_cases(a, bt, cases)
