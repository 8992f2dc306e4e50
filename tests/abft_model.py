"""A numpy model of the matrix path's ABFT verdict (``gemm_abft`` in ``ops/gemm.hip``), and the
operand and corruption builders that ``tests/test_canary_gemm.py`` (CPU: checks the model on
cases whose answer is known by construction) and ``tests/test_gpu_gemm.py`` (GPU: uses the model
as the oracle of ``canary.abft``) share.

The verdict: a row (column) of C is wrong when the int64 sum of its elements differs from the
checksum predicted from A and Bt, or when it holds an element that no healthy product holds: one
that is not an integer, has a magnitude above 2^24, is NaN or Inf, or is -0.  Such elements stay
out of the sum.  The answer is (wrong rows, wrong columns)."""
import numpy as np


def bf16_bits(ints):
    """bf16 bit patterns (uint16) of an integer array; exact for |v| <= 256."""
    v = np.asarray(ints)
    assert np.abs(v).max(initial=0) <= 256
    return (v.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_ints(bits):
    """The integers the checksum kernels read from bf16 bit patterns (truncation, as they do)."""
    f = (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)
    return np.trunc(f).astype(np.int64)


def exact_product(a_ints, bt_ints):
    """C = A @ Bt.T in int64, as float32 (exact while |C| <= 2^24)."""
    c = np.asarray(a_ints, dtype=np.int64) @ np.asarray(bt_ints, dtype=np.int64).T
    assert np.abs(c).max(initial=0) <= 1 << 24
    return c.astype(np.float32)


def healthy(c):
    """Elementwise: an integer of magnitude <= 2^24 that is not -0 (decided on bit patterns
    and exact float64 arithmetic, so no flush-to-zero or compare mode matters)."""
    c = np.asarray(c, dtype=np.float32)
    bits = c.view(np.uint32)
    wide = c.astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(wide) & (np.abs(wide) <= float(1 << 24)) & (wide == np.trunc(wide))
    return ok & (bits != np.uint32(0x80000000))


def verdict(a_bits, bt_bits, c):
    """(wrong rows, wrong columns) of C [M, N] for A [M, K] and Bt [N, K] given as bf16 bits."""
    a, bt = bf16_ints(a_bits), bf16_ints(bt_bits)
    c = np.asarray(c, dtype=np.float32)
    assert c.shape == (a.shape[0], bt.shape[0]) and a.shape[1] == bt.shape[1]
    ok = healthy(c)
    summed = np.where(ok, c, np.float32(0)).astype(np.int64)
    want_rows = a @ bt.sum(axis=0)
    want_cols = bt @ a.sum(axis=0)
    rows = (summed.sum(axis=1) != want_rows) | ~ok.all(axis=1)
    cols = (summed.sum(axis=0) != want_cols) | ~ok.all(axis=0)
    return int(rows.sum()), int(cols.sum())


def operands(m, n, k, lo, hi, seed):
    """Integer A [m, k] (row 0 all zero, so row 0 of C is all zeros) and Bt [n, k] in [lo, hi]."""
    rng = np.random.default_rng(seed)
    a = rng.integers(lo, hi + 1, size=(m, k), dtype=np.int64)
    bt = rng.integers(lo, hi + 1, size=(n, k), dtype=np.int64)
    a[0, :] = 0
    return a, bt


def flip_bit(c, i, j, bit):
    """A copy of C with one bit of element (i, j) flipped."""
    out = np.array(c, dtype=np.float32, copy=True)
    out.view(np.uint32)[i, j] ^= np.uint32(1) << np.uint32(bit)
    return out


def replace(c, i, j, value):
    """A copy of C with element (i, j) replaced; ``value`` keeps its bit pattern (NaN, -0)."""
    out = np.array(c, dtype=np.float32, copy=True)
    out[i, j] = np.float32(value)
    return out


def same_bits(x, y):
    return np.float32(x).view(np.uint32) == np.float32(y).view(np.uint32)


# the replacements of the sensitivity tests; "neighbour" stands for the value of the element to the
# right (to the left in the last column, the one below in a one-column product)
REPLACEMENTS = (1.0, -1.0, 0.5, -0.5, 2.0 ** -20, float("nan"), float("inf"), float("-inf"), -0.0, "neighbour")


def neighbour_value(c, i, j):
    m, n = c.shape
    if n > 1:
        return c[i, j + 1 if j + 1 < n else j - 1]
    return c[i + 1 if i + 1 < m else i - 1, j] if m > 1 else c[i, j]


def sweep_elements(c):
    """The elements of the bit sweep: a zero, the largest magnitude, the two corners, and one
    either side of index 63/64 and 255/256 on both axes where the shape has them."""
    m, n = c.shape
    zeros = np.argwhere(c == 0)
    assert len(zeros), "the operands are built so that row 0 of C is zero"
    z = zeros[len(zeros) // 2]
    big = np.unravel_index(np.abs(c).argmax(), c.shape)
    out = [(int(z[0]), int(z[1])), (int(big[0]), int(big[1])), (0, 0), (m - 1, n - 1)]
    for edge in (63, 64, 255, 256):
        if edge < m:
            out.append((edge, min(edge, n - 1)))
        if edge < n:
            out.append((min(edge, m - 1), edge))
    return list(dict.fromkeys(out))


# (shape, operand range): the products the sensitivity tests corrupt.  The shapes cross
# gemm_colsum's 64-row slab and 256-wide k blocks and gemm_abft's 256-stride loops with a
# remainder on every axis; [-64, 64] at K = 1000 keeps |C| <= 2^22.
DATASETS = (((1, 1, 1), 4), ((65, 130, 257), 4), ((128, 128, 64), 4), ((300, 70, 1000), 4), ((300, 70, 1000), 64))
SWEEP_DATASETS = (((128, 128, 64), 4), ((65, 130, 257), 4))  # the bit sweep runs on these only


def dataset(shape, bound):
    """(A bits, Bt bits, exact C) of one of DATASETS, seeded by the shape and the range."""
    m, n, k = shape
    a, bt = operands(m, n, k, -bound, bound, seed=m * 1000003 + n * 1009 + k * 7 + bound)
    return bf16_bits(a), bf16_bits(bt), exact_product(a, bt)


def hand_built_cases(c):
    """(label, corrupted C, (wrong rows, wrong columns)) whose answer is known by construction:
    the clean product, every replacement at every sweep element, a +1 / -1 pair in one row and
    in one column, and the rectangle +d -d / -d +d that no row or column checksum can see."""
    m, n = c.shape
    yield "clean", c, (0, 0)
    for (i, j) in sweep_elements(c):
        for r in REPLACEMENTS:
            value = neighbour_value(c, i, j) if isinstance(r, str) else r
            want = (0, 0) if same_bits(value, c[i, j]) else (1, 1)
            yield "C[%d][%d] = %r" % (i, j, r), replace(c, i, j, value), want
    i, j = m // 2, n // 2
    if n >= 2:
        pair = np.array(c, copy=True)
        pair[i, 0] += 1
        pair[i, n - 1] -= 1
        yield "+1 and -1 in row %d" % i, pair, (0, 2)
    if m >= 2:
        pair = np.array(c, copy=True)
        pair[0, j] += 1
        pair[m - 1, j] -= 1
        yield "+1 and -1 in column %d" % j, pair, (2, 0)
    if m >= 2 and n >= 2:
        for d in (1, 7):
            rect = np.array(c, copy=True)
            rect[0, 0] += d
            rect[0, n - 1] -= d
            rect[m - 1, 0] -= d
            rect[m - 1, n - 1] += d
            yield "rectangle of +-%d" % d, rect, (0, 0)


def bit_sweep_cases(c):
    """(label, C with one bit of one sweep element flipped, (1, 1)) for all 32 bit positions."""
    for (i, j) in sweep_elements(c):
        for bit in range(32):
            yield "bit %d of C[%d][%d] = %r" % (bit, i, j, float(c[i, j])), flip_bit(c, i, j, bit), (1, 1)


def random_corruption(c, rng):
    """1-6 elements of C corrupted in a way drawn from `rng`: integer offsets (which may cancel
    along a row or a column), bit flips, fractions and special values."""
    out = np.array(c, dtype=np.float32, copy=True)
    m, n = out.shape
    rows = rng.integers(0, m, size=2)
    cols = rng.integers(0, n, size=2)
    for _ in range(int(rng.integers(1, 7))):
        # few distinct rows and columns, so that offsets meet in one and sometimes cancel
        i, j = int(rows[rng.integers(0, 2)]), int(cols[rng.integers(0, 2)])
        kind = int(rng.integers(0, 4))
        if kind == 0:
            out[i, j] += np.float32(int(rng.integers(-3, 4)))
        elif kind == 1:
            out.view(np.uint32)[i, j] ^= np.uint32(1) << np.uint32(int(rng.integers(0, 32)))
        elif kind == 2:
            out[i, j] += np.float32(rng.choice([0.5, -0.25, 2.0 ** -20]))
        else:
            out[i, j] = np.float32(rng.choice([np.nan, np.inf, -np.inf, -0.0, 3.0e7]))
    return out
