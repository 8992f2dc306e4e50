"""Host model of the host-link check (``ops/hostlink/hostlink_host.h``), no GPU: the pattern,
the host verifier and the atomics' expected tables against independent numpy models, the
acceptance rules of the order-dependent forms, and the stand-alone sanitized self-test."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from k8s_gpu_device_plugin_amd import _build
from k8s_gpu_device_plugin_amd.ops import hostlink

TILE = 1024  # 16-byte words of one tile at UNROLL 4; the host verifier itself knows no tile


# ---- pattern -----------------------------------------------------------------------------
def model_pattern(idx0, n, seed):
    idx = np.arange(n, dtype=np.uint64) + np.uint64(idx0)
    lo, hi = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32)
    b = lo * np.uint32(0x9E3779B1) ^ (hi + np.full(n, seed, dtype=np.uint32)) * np.uint32(0x85EBCA77)
    return np.stack([b, b ^ np.uint32(0xA5A5A5A5), ~b, b * np.uint32(3) + np.uint32(0x6A09E667)], axis=1)


@pytest.mark.parametrize("idx0, n", [(0, 1), (0, 4097), ((1 << 32) - 1500, 3000), ((3 << 32) - 1, 2), (1 << 40, 1025)])
@pytest.mark.parametrize("seed", [0, 0x48520000, 0xFFFFFFFF])
def test_pattern_matches_the_numpy_model(idx0, n, seed):
    got = hostlink.pattern_words(idx0, n, seed)
    assert got.shape == (n, 4) and got.dtype == np.uint32
    assert np.array_equal(got, model_pattern(idx0, n, seed))


@pytest.mark.parametrize("idx0", [0, (1 << 32) - 30000])
def test_no_two_words_of_a_range_are_equal(idx0):
    p = hostlink.pattern_words(idx0, 60000, hostlink.SEEDS["write"])
    assert len(np.unique(p, axis=0)) == len(p)
    assert len(np.unique(p[:, 0])) == len(p)  # already the first 32 bits differ
    # every bit of a 16-byte word takes both values over the range
    assert np.all(np.bitwise_or.reduce(p, axis=0) == 0xFFFFFFFF) and np.all(np.bitwise_and.reduce(p, axis=0) == 0)


def test_the_stage_seeds_give_different_buffers():
    bufs = [hostlink.pattern_words(0, 64, s) for s in hostlink.SEEDS.values()]
    assert all(not np.any(a[:, 0] == b[:, 0]) for i, a in enumerate(bufs) for b in bufs[i + 1:])


# ---- host verifier -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, TILE // 2, TILE // 2 + 1, TILE, TILE + 1])  # one word; one tile (+ 16 B) at UNROLL 2, 4
def test_host_verify_counts_hand_built_corruptions(n):
    seed = hostlink.SEEDS["d2h"]
    clean = hostlink.pattern_words(0, n, seed)
    assert hostlink.host_verify(clean, seed) == (0, -1)
    bad = clean.copy()
    bad[0, 0] ^= 1  # one bit in the first word
    assert hostlink.host_verify(bad, seed) == (1, 0)
    bad = clean.copy()
    bad[n - 1, 3] ^= 1 << 31  # one bit in the last word
    assert hostlink.host_verify(bad, seed) == (1, (n - 1) * 16 + 12)
    bad = clean.copy()
    bad[n - 1, 1] ^= 1 << 9  # two words of one 16-byte group
    bad[n - 1, 2] ^= 1 << 9
    assert hostlink.host_verify(bad, seed) == (2, (n - 1) * 16 + 4)
    if n > 1:
        bad = clean.copy()
        bad[[0, n // 2, n - 1], 2] = 0xDEADBEEF
        want = int(np.sum(bad != clean))
        assert want == 3 and hostlink.host_verify(bad, seed) == (3, 8)
    assert hostlink.host_verify(clean, seed + 1)[0] == 4 * n  # another seed: every 32-bit word differs
    with pytest.raises(ValueError):
        hostlink.host_verify(np.zeros(5, dtype=np.uint32), seed)


# ---- atomics -----------------------------------------------------------------------------
U32_ADD, U64_ADD, TICKET, CAS_INC, SWAP = range(5)
MASK = np.uint64(0xFFFFFFFFFFFFFFFF)


def fmix64(x):
    x = np.asarray(x, dtype=np.uint64).copy()
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xff51afd7ed558ccd)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xc4ceb9fe1a85ec53)
    x ^= x >> np.uint64(33)
    return x


def row_hash(op, wave):
    return fmix64(np.uint64(((op + 1) << 56) ^ (1 << 55)) ^ (np.asarray(wave, dtype=np.uint64) << np.uint64(8))) \
        & np.uint64(0xFFFFFFFF)


def operand_hash(op, gid):
    return fmix64(np.uint64((op + 1) << 56) ^ (np.asarray(gid, dtype=np.uint64) << np.uint64(8)))


def swap_token(wave):
    return (0x70C5 << 48) | (wave + 1)


def swap_initial():
    return [(0x1717 << 48) | s for s in range(hostlink.SWAP_SLOTS)]


def model_expected(op, blocks, host_adds=0, order=None):
    """The table as the device lays it out; ``order``: the order in which the waves of swap run."""
    threads, waves = blocks * 256, blocks * 4
    gid = np.arange(threads, dtype=np.uint64)
    if op in (U32_ADD, U64_ADD):
        elem = ((row_hash(op, gid >> np.uint64(6)) & np.uint64(15)) * np.uint64(64) + (gid & np.uint64(63))).astype(np.int64)
        t = np.arange(1024, dtype=np.uint64)
        np.add.at(t, elem, operand_hash(op, gid))
        if op == U32_ADD:
            return (t & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        i = np.arange(host_adds, dtype=np.uint64)
        np.add.at(t, (fmix64(np.uint64(0xC0 << 56) ^ i) & np.uint64(1023)).astype(np.int64),
                  fmix64(np.uint64(0xC1 << 56) ^ i))
        return t
    w = np.arange(waves, dtype=np.uint64)
    if op == TICKET:
        t = np.zeros(1 + hostlink.MAX_WAVES, dtype=np.uint32)
        t[0] = waves
        t[1:1 + waves] = 1
        return t
    if op == CAS_INC:
        t = np.zeros(64, dtype=np.uint64)
        np.add.at(t, (row_hash(op, w) & np.uint64(63)).astype(np.int64),
                  np.uint64(1) + (operand_hash(op, w * np.uint64(64)) & np.uint64(7)))
        return t
    slots, back = swap_initial(), [0] * hostlink.MAX_WAVES
    where = (row_hash(op, w) & np.uint64(63)).astype(np.int64)
    for wave in (range(waves) if order is None else order):
        back[wave], slots[where[wave]] = slots[where[wave]], swap_token(wave)
    return np.array(slots + back, dtype=np.uint64)


@pytest.mark.parametrize("blocks", [1, 13, 64])
@pytest.mark.parametrize("host_adds", [0, 1024])
@pytest.mark.parametrize("op", range(5))
def test_atomic_expected_matches_the_numpy_model(op, blocks, host_adds):
    name = hostlink.ATOMIC_OPS[op]
    got = hostlink.atomic_expected(name, blocks, host_adds)
    want = model_expected(op, blocks, host_adds)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert hostlink.atomic_wrong(name, blocks, want, host_adds) == (0, -1)


def test_host_adds_change_only_the_u64_add_table():
    for name in hostlink.ATOMIC_OPS:
        same = np.array_equal(hostlink.atomic_expected(name, 13, 0), hostlink.atomic_expected(name, 13, 1024))
        assert same == (name != "u64_add")
    # a table without the host's adds is wrong where the host added
    without = hostlink.atomic_expected("u64_add", 13, 0)
    bad, first = hostlink.atomic_wrong("u64_add", 13, without, host_adds=1024)
    assert bad == int(np.sum(without != hostlink.atomic_expected("u64_add", 13, 1024))) and 600 < bad <= 1024 and first >= 0


@pytest.mark.parametrize("blocks", [1, 13, 64])
def test_swap_accepts_every_order_and_rejects_a_duplicated_or_missing_token(blocks):
    waves = blocks * 4
    rng = np.random.default_rng(blocks)
    orders = [list(range(waves)), list(range(waves))[::-1]] + [list(rng.permutation(waves)) for _ in range(20)]
    tables = [model_expected(SWAP, blocks, order=o) for o in orders]
    assert all(hostlink.atomic_wrong("swap", blocks, t) == (0, -1) for t in tables)
    if waves > 4:
        assert any(not np.array_equal(t, tables[0]) for t in tables[1:])  # the orders do differ in their outcome
    t = tables[-1].copy()
    lost = int(t[hostlink.SWAP_SLOTS])
    t[hostlink.SWAP_SLOTS] = t[hostlink.SWAP_SLOTS + 1]  # wave 0 got what wave 1 got: one value twice, one lost
    bad, first = hostlink.atomic_wrong("swap", blocks, t)
    tokens = [swap_token(w) for w in range(waves)]
    where = tokens.index(lost) if lost in tokens else hostlink.MAX_WAVES + swap_initial().index(lost)
    assert (bad, first) == (1, where)
    t = tables[-1].copy()
    held = int(np.flatnonzero(t == np.uint64(swap_token(waves - 1)))[0])
    t[held] = 0  # the last wave's token is nowhere
    assert hostlink.atomic_wrong("swap", blocks, t) == (1, waves - 1)
    t = tables[-1].copy()
    t[held] = np.uint64(swap_token(waves - 1) ^ (1 << 40))  # ... or arrived with a flipped bit
    assert hostlink.atomic_wrong("swap", blocks, t) == (1, waves - 1)
    if waves < hostlink.MAX_WAVES:
        t = tables[-1].copy()
        t[hostlink.SWAP_SLOTS + waves] = 7  # an entry no wave owns must stay 0
        assert hostlink.atomic_wrong("swap", blocks, t) == (1, waves)


@pytest.mark.parametrize("blocks", [1, 13, 64])
def test_ticket_rule_rejects_a_duplicated_or_missing_ticket(blocks):
    waves = blocks * 4
    good = model_expected(TICKET, blocks)
    assert hostlink.atomic_wrong("ticket", blocks, good) == (0, -1)  # whichever wave took which ticket
    t = good.copy()
    t[1 + waves - 1], t[1] = 0, 2  # two waves were given ticket 0, nobody the last one
    assert hostlink.atomic_wrong("ticket", blocks, t) == (2, 1)
    t = good.copy()
    t[0] = waves - 1  # an add was lost
    assert hostlink.atomic_wrong("ticket", blocks, t) == (1, 0)
    if waves < hostlink.MAX_WAVES:
        t = good.copy()
        t[1 + waves] = 1  # a ticket past the last wave
        assert hostlink.atomic_wrong("ticket", blocks, t) == (1, 1 + waves)


def test_atomic_tables_refuse_bad_arguments():
    for blocks in (0, 65):
        with pytest.raises(ValueError):
            hostlink.atomic_expected("u32_add", blocks)
    with pytest.raises(ValueError):
        hostlink.atomic_wrong("swap", 4, np.zeros(10, dtype=np.uint64))
    with pytest.raises(ValueError):
        hostlink.atomic_expected("f32_add", 4)


# ---- the stand-alone sanitized program ---------------------------------------------------
def test_sanitized_selftest_program(tmp_path):
    """Host code under AddressSanitizer and UBSan as a program of its own: nothing sanitized
    is loaded into Python."""
    cxx = shutil.which(_build._cxx())
    assert cxx, "no C++ compiler"
    src = os.path.join(_build.HARNESS_DIR, "hostlink_selftest.cpp")
    exe = str(tmp_path / "hostlink_selftest")
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + _build.HOSTLINK_DIR,
                        src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
           "PATH": "/usr/bin:/bin"}  # as tests/test_native_selftest.py runs its program
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", p.stdout[-3000:]
