"""The matrix path of the canary (``ops/gemm.hip``) as far as it can be checked without a GPU:
the build contract of the LDS-staged kernels, the tile maps of every GEMM kernel id (the kernels' own index arithmetic, run on the host by
``amdgpu_canary_gemm_tile_map``), the shape validators of ``gemm``, ``gemm_rate`` and ``abft``
(refused by their own message, so before any HIP call), and the numpy model of the ABFT verdict
that ``tests/test_gpu_gemm.py`` uses as the oracle of the device verifier."""
import ctypes

import numpy as np
import pytest

import abft_model as model
from kernel_usage import kernel_resource_usage
from k8s_gpu_device_plugin_amd.ops import canary

IDS = sorted(v for v in canary.GEMM_KERNELS.values() if v != 0)
GROUP = {9: 2, 10: 8}  # tile rows per raster group; 4 for every other 256x256 kernel


def _tile(kid):
    return 128 if kid == 1 else 256


def _grids():
    return [(bm, bn) for bm in range(1, 25) for bn in range(1, 25)] + [(64, 3), (3, 64), (1, 200)]


def _xcd_remap(block, nblocks):
    """Workgroup `block` runs on XCD block % 8 as that XCD's (block // 8)-th; the XCDs take
    contiguous chunks of the tile order, the first nblocks % 8 of them one tile longer."""
    xcd, q, r = block % 8, nblocks // 8, nblocks % 8
    start = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return start + block // 8


# ---- build contract ------------------------------------------------------------------------
def test_gemm_kernels_build_without_scratch_at_occupancy_two(tmp_path):
    """What the LDS-staged kernels' schedules assume, read from the compiler's own resource-usage
    remarks: nothing spills, the one LDS array is 2 buffers x 2 operands x 16 KiB (gemm_lds) or
    2 x 64 KiB (the 256x256 kernels: one block per CU), and a 512-thread block's 8 waves fit the
    CU as 2 per SIMD of a 512-entry register file."""
    usage = kernel_resource_usage("gemm.hip", tmp_path)
    lds128 = [n for n in usage if "gemm_lds" in n]
    staged = [n for n in usage if "gemm256s" in n]
    whole = [n for n in usage if "gemm256" in n and n not in staged]
    assert (len(lds128), len(whole), len(staged)) == (1, 1, 9), sorted(usage)
    for name in lds128 + whole + staged:
        u = usage[name]
        print("%s: %s" % (name, u))
        assert int(u["ScratchSize"]) == 0
        assert int(u["SGPRs Spill"]) == 0 and int(u["VGPRs Spill"]) == 0
        assert int(u["LDS Size"]) == (65536 if name in lds128 else 131072)
        if name not in lds128:
            assert int(u["VGPRs"]) + int(u["AGPRs"]) <= 256
        assert int(u["Occupancy"]) == 2


# ---- tile maps ---------------------------------------------------------------------------
def test_ids_are_1_to_11():
    assert IDS == list(range(1, 12))


@pytest.mark.parametrize("kid", IDS)
def test_tile_map_is_a_permutation_of_the_tile_set(kid):
    t = _tile(kid)
    for bm, bn in _grids():
        m, n = bm * t, bn * t
        origins = canary.gemm_tile_map(kid, m, n)
        assert origins.shape == (bm * bn, 2), (kid, bm, bn)
        m0, n0 = origins[:, 0], origins[:, 1]
        assert (m0 % t == 0).all() and (n0 % t == 0).all(), (kid, bm, bn)
        assert m0.min() >= 0 and n0.min() >= 0 and m0.max() + t <= m and n0.max() + t <= n, (kid, bm, bn)
        seen = np.zeros((bm, bn), dtype=np.int64)
        np.add.at(seen, (m0 // t, n0 // t), 1)
        assert (seen == 1).all(), "kernel %d, %dx%d tiles: tiles hit %s times" % (kid, bm, bn, np.unique(seen))


@pytest.mark.parametrize("kid", [k for k in IDS if k != 1])
def test_raster_groups_hold_their_tile_rows(kid):
    """With the XCD remap undone, run g of group * nbn consecutive workgroups covers exactly the
    tile rows [g * group, (g + 1) * group) (fewer in a ragged last group): the rows of a run
    span at most `group`, which is what keeps an XCD's neighbours on shared A panels."""
    group = GROUP.get(kid, 4)
    for bm, bn in _grids():
        origins = canary.gemm_tile_map(kid, bm * 256, bn * 256)
        by_wg = np.full((bm * bn, 2), -1, dtype=np.int64)
        for block in range(bm * bn):
            by_wg[_xcd_remap(block, bm * bn)] = origins[block]
        assert (by_wg >= 0).all()
        for g in range((bm + group - 1) // group):
            run = by_wg[g * group * bn:(g + 1) * group * bn]
            rows = run[:, 0] // 256
            assert rows.min() == g * group and rows.max() == min((g + 1) * group, bm) - 1, (kid, bm, bn, g)
            assert rows.max() - rows.min() < group


def test_lds128_tiles_are_row_major_under_the_remap():
    for bm, bn in [(1, 1), (3, 3), (9, 1), (5, 2), (2, 13)]:
        origins = canary.gemm_tile_map(1, bm * 128, bn * 128)
        for block in range(bm * bn):
            wg = _xcd_remap(block, bm * bn)
            assert tuple(origins[block]) == ((wg // bn) * 128, (wg % bn) * 128)


def test_auto_kernel_maps_like_the_kernel_it_picks():
    assert (canary.gemm_tile_map("auto", 4096, 4096) == canary.gemm_tile_map("pingpong256s", 4096, 4096)).all()
    assert (canary.gemm_tile_map("auto", 1024, 1024) == canary.gemm_tile_map("lds128", 1024, 1024)).all()


@pytest.mark.parametrize("kid, m, n", [(1, 130, 128), (1, 128, 64), (2, 128, 256), (3, 256, 384), (9, 256, 128),
                                       (12, 256, 256), (-1, 256, 256), (3, 0, 256), (3, 256, -256)])
def test_tile_map_refuses_what_pick_gemm_refuses(kid, m, n):
    assert canary.load().amdgpu_canary_gemm_tile_map(kid, m, n, None, None, 0) == 0
    with pytest.raises(ValueError):
        canary.gemm_tile_map(kid, m, n)


def test_tile_map_fills_no_more_than_len():
    m0, n0 = np.full(8, -7, dtype=np.int32), np.full(8, -7, dtype=np.int32)
    assert canary.load().amdgpu_canary_gemm_tile_map(3, 1024, 1024, m0.ctypes.data, n0.ctypes.data, 5) == 16
    assert (m0[5:] == -7).all() and (n0[5:] == -7).all() and (m0[:5] >= 0).all()


# ---- shape refusals: the validator's own message, so no HIP call was made ------------------
GEMM_REFUSAL = "does not fit kernel"
BAD_TILE_SHAPES = [(1, (130, 128, 64)), (1, (128, 192 + 1, 64)), (1, (64, 128, 64)),
                   (2, (128, 256, 64)), (3, (256, 384, 64)), (4, (384, 256, 64)), (5, (256, 257, 64)),
                   (6, (255, 256, 64)), (7, (512, 128, 64)), (8, (128, 128, 64)), (9, (640, 256, 64)),
                   (10, (256, 640, 64)), (11, (384, 384, 64)),
                   (1, (128, 128, 32)), (3, (256, 256, 96)), (3, (256, 256, 65)), (2, (256, 256, 1)),  # K % 64
                   (12, (256, 256, 64)), (-1, (256, 256, 64)), (99, (256, 256, 64)),                   # unknown id
                   (3, (0, 256, 64)), (3, (256, 0, 64)), (1, (128, 128, 0))]                           # zero sizes


@pytest.mark.parametrize("kid, shape", BAD_TILE_SHAPES)
def test_gemm_refuses_the_shape_itself(kid, shape):
    m, n, k = shape
    a, bt = np.zeros((m, k), dtype=np.uint16), np.zeros((n, k), dtype=np.uint16)
    with pytest.raises(RuntimeError, match=GEMM_REFUSAL):
        canary.gemm(a, bt, device=0, kernel=kid)


@pytest.mark.parametrize("kid, shape", BAD_TILE_SHAPES + [(3, (256, 256, 65536 + 64)), (1, (128, 128, 1 << 20))])
def test_gemm_rate_refuses_the_shape_itself(kid, shape):
    with pytest.raises(RuntimeError, match=GEMM_REFUSAL):
        canary.gemm_rate(0, *shape, iters=1, kernel=kid)


@pytest.mark.parametrize("iters", [0, -1])
def test_gemm_rate_refuses_less_than_one_iteration(iters):
    with pytest.raises(RuntimeError, match=GEMM_REFUSAL + r".*iters >= 1"):
        canary.gemm_rate(0, 256, 256, 64, iters=iters, kernel=3)


@pytest.mark.parametrize("shape", [(-128, 128, 64), (128, -128, 64), (128, 128, -64), (-256, -256, -64)])
def test_negative_sizes_are_refused_at_the_c_abi(shape):
    lib = canary.load()
    err = ctypes.create_string_buffer(256)
    t, e = ctypes.c_double(), ctypes.c_ulonglong()
    for kid in (0, 1, 3):
        assert lib.amdgpu_canary_gemm(0, None, None, None, *shape, kid, err, 256) == -1
        assert GEMM_REFUSAL in err.value.decode()
        assert lib.amdgpu_canary_gemm_rate(0, *shape, 1, 0, kid, ctypes.byref(t), ctypes.byref(e), err, 256) == -1
        assert GEMM_REFUSAL in err.value.decode()
    rows, cols = ctypes.c_ulonglong(7), ctypes.c_ulonglong(7)
    assert lib.amdgpu_canary_abft(0, None, None, None, *shape, ctypes.byref(rows), ctypes.byref(cols), err, 256) == -1
    assert "must be positive" in err.value.decode() and (rows.value, cols.value) == (0, 0)


@pytest.mark.parametrize("shape", [(0, 4, 4), (4, 0, 4), (4, 4, 0), (2, 2, 65537), (1, 1, 1 << 17)])
def test_abft_refuses_the_shape_itself(shape):
    m, n, k = shape
    a, bt = np.zeros((m, k), dtype=np.uint16), np.zeros((n, k), dtype=np.uint16)
    with pytest.raises(RuntimeError, match="abft shape .* must be positive with K <= 65536"):
        canary.abft(a, bt, np.zeros((m, n), dtype=np.float32))


def test_abft_refuses_arrays_that_do_not_belong_together():
    a, bt = np.zeros((4, 8), dtype=np.uint16), np.zeros((6, 8), dtype=np.uint16)
    with pytest.raises(ValueError):
        canary.abft(a, bt, np.zeros((6, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        canary.abft(a, np.zeros((6, 7), dtype=np.uint16), np.zeros((4, 6), dtype=np.float32))


# ---- the model of the verdict ----------------------------------------------------------------
def test_bf16_round_trip_of_the_operand_ranges():
    v = np.arange(-256, 257)
    assert (model.bf16_ints(model.bf16_bits(v)) == v).all()
    assert model.bf16_bits(np.array([1, -2]))[0] == 0x3F80 and model.bf16_bits(np.array([1, -2]))[1] == 0xC000


def test_healthy_elements():
    good = np.array([0.0, 1.0, -1.0, 3.0, 2.0 ** 24, -(2.0 ** 24), 65536.0], dtype=np.float32)
    bad = np.array([-0.0, 0.5, -0.5, 2.0 ** -20, 1.5, 2.0 ** 24 + 2, 3.0e7, np.nan, np.inf, -np.inf, 1e-45,
                    8388607.5], dtype=np.float32)
    assert model.healthy(good).all()
    assert not model.healthy(bad).any()


@pytest.mark.parametrize("shape, bound", model.DATASETS)
def test_model_on_hand_built_cases(shape, bound):
    a, bt, c = model.dataset(shape, bound)
    assert (c[0] == 0).all() and c.shape == shape[:2]
    n_cases = 0
    for label, bad_c, want in model.hand_built_cases(c):
        assert model.verdict(a, bt, bad_c) == want, label
        n_cases += 1
    assert n_cases >= 1 + len(model.REPLACEMENTS)


@pytest.mark.parametrize("shape, bound", model.DATASETS)
def test_model_sees_every_bit_of_an_element(shape, bound):
    a, bt, c = model.dataset(shape, bound)
    for label, bad_c, want in model.bit_sweep_cases(c):
        assert model.verdict(a, bt, bad_c) == want, label


def test_truncating_sums_would_miss_what_the_model_sees():
    """The blind spot this verdict closes: a checksum of truncated elements passes every
    corruption that leaves the integer part alone."""
    a, bt, c = model.dataset((128, 128, 64), 4)
    i, j = 5, 7
    bad_c = model.replace(c, i, j, c[i, j] + np.float32(0.5 if c[i, j] >= 0 else -0.5))
    assert (np.trunc(bad_c) == c).all()
    assert model.verdict(a, bt, bad_c) == (1, 1)
    assert model.verdict(a, bt, model.replace(c, 0, 3, -0.0)) == (1, 1)
    assert model.verdict(a, bt, model.replace(c, 0, 3, 2.0 ** -20)) == (1, 1)


def test_random_corruptions_are_reproducible_and_varied():
    a, bt, c = model.dataset((65, 130, 257), 4)
    verdicts = [model.verdict(a, bt, model.random_corruption(c, np.random.default_rng(100 + s))) for s in range(20)]
    again = [model.verdict(a, bt, model.random_corruption(c, np.random.default_rng(100 + s))) for s in range(20)]
    assert verdicts == again
    assert len(set(verdicts)) >= 3 and all(r <= 2 and k <= 2 for r, k in verdicts)
