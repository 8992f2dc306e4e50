"""Fabric check, host side: the reference tables of the global atomics against an
independent numpy model, the order-independence bounds of the packed operands, the per-check
canary metrics, the place of a failure in the start-up canary's log line and the CLI."""
import json
import logging
import time

import numpy as np
import pytest

from k8s_gpu_device_plugin_amd.ops import canary
from k8s_gpu_device_plugin_amd.plugin.kubelet_stub import KubeletStub
from k8s_gpu_device_plugin_amd.plugin.manager import PluginManager

# ---- the documented (op, thread, step) -> (element, operand) map, written again in numpy ----
# (docs/CANARY.md, "The atomics' operands"; ops/fabric.hip atomic_elem / atomic_operand)
OPS = ("u32_add", "u64_add", "i32_min", "u32_max", "u64_max", "and", "or", "xor", "f32_add", "f64_add",
       "pk_add_bf16", "pk_add_f16", "cas_inc", "ticket")
STEPS, ELEMS, DENSE_WAVES, MAX_WAVES = 8, 2048, 512, 16384
U64 = np.uint64


def _fmix64(x):
    """MurmurHash3's 64-bit finalizer."""
    x = np.asarray(x, dtype=U64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U64(33)
        x *= U64(0xff51afd7ed558ccd)
        x ^= x >> U64(33)
        x *= U64(0xc4ceb9fe1a85ec53)
        x ^= x >> U64(33)
    return x


def _grid(blocks):
    """(thread id, step) of every lane-operation: [threads, STEPS] each."""
    gid = np.arange(blocks * 256, dtype=U64)[:, None]
    step = np.arange(STEPS, dtype=U64)[None, :]
    return np.broadcast_arrays(gid, step)


def _row_hash(op, wave, step):
    return _fmix64((U64(op + 1) << U64(56)) ^ (U64(1) << U64(55)) ^ (wave << U64(8)) ^ step) & U64(0xFFFFFFFF)


def _elem(op, gid, step):
    return ((_row_hash(op, gid >> U64(6), step) & U64(31)) * U64(64) + (gid & U64(63))).astype(np.int64)


def _hash(op, gid, step):
    return _fmix64((U64(op + 1) << U64(56)) ^ (gid << U64(8)) ^ step)


def _bit_sel(elem):
    e = elem.astype(U64)
    sel = _fmix64((U64(0xB175) << U64(40)) ^ e) & U64(0xFFFFFFFF)
    return (sel & ~(U64(1) << (e & U64(31))) & U64(0xFFFFFFFF)).astype(np.uint32)


def _packed_operands(name, h32, dense):
    """(low, high) non-negative integer operands of a packed form."""
    a, b = h32, h32 >> np.uint32(8)
    if name == "pk_add_bf16":
        lo = np.where(dense, a & 1, (a & 63) == 0)
        hi = np.where(dense, b & 1, (b & 63) == 0)
    else:
        lo = np.where(dense, a & 7, np.where((a & 15) == 0, (a >> np.uint32(4)) & 7, 0))
        hi = np.where(dense, b & 7, np.where((b & 15) == 0, (b >> np.uint32(4)) & 7, 0))
    return lo.astype(np.int64), hi.astype(np.int64)


def _packed_totals(name, blocks):
    """Per-element (low, high) totals of a packed form, the initial 1 and 2 included."""
    op = OPS.index(name)
    gid, step = _grid(blocks)
    e = _elem(op, gid, step)
    lo, hi = _packed_operands(name, (_hash(op, gid, step) & U64(0xFFFFFFFF)).astype(np.uint32),
                              (gid >> U64(6)) < U64(DENSE_WAVES))
    tl, th = np.full(ELEMS, 1, np.int64), np.full(ELEMS, 2, np.int64)
    np.add.at(tl, e, lo)
    np.add.at(th, e, hi)
    return tl, th


def model(name, blocks):
    op = OPS.index(name)
    waves = blocks * 4
    if name == "ticket":
        t = np.zeros(1 + MAX_WAVES, np.uint32)
        t[0] = waves
        t[1:1 + waves] = 1
        return t
    if name == "cas_inc":  # lane 0 of each wave
        wave, step = np.broadcast_arrays(np.arange(waves, dtype=U64)[:, None], np.arange(STEPS, dtype=U64)[None, :])
        word = (_row_hash(op, wave, step) & U64(63)).astype(np.int64)
        amount = (U64(1) + (_hash(op, wave * U64(64), step) & U64(7))).astype(np.uint32)
        t = np.zeros(64, np.uint32)
        np.add.at(t, word, amount)
        return t
    gid, step = _grid(blocks)
    e = _elem(op, gid, step)
    h = _hash(op, gid, step)
    h32 = (h & U64(0xFFFFFFFF)).astype(np.uint32)
    idx = np.arange(ELEMS)
    if name == "u32_add":
        t = idx.astype(np.uint32)
        np.add.at(t, e, h32)
    elif name == "u64_add":
        t = idx.astype(U64)
        np.add.at(t, e, h)
    elif name == "i32_min":
        t = (0x7FFFFFFF - idx).astype(np.int32)
        np.minimum.at(t, e, h32.view(np.int32))
    elif name == "u32_max":
        t = idx.astype(np.uint32)
        np.maximum.at(t, e, h32)
    elif name == "u64_max":
        t = idx.astype(U64)
        np.maximum.at(t, e, h)
    elif name == "and":
        t = np.full(ELEMS, 0xFFFFFFFF, np.uint32)
        np.bitwise_and.at(t, e, ~((np.uint32(1) << (h32 & np.uint32(31))) & _bit_sel(e)))
    elif name == "or":
        t = np.zeros(ELEMS, np.uint32)
        np.bitwise_or.at(t, e, (np.uint32(1) << (h32 & np.uint32(31))) & _bit_sel(e))
    elif name == "xor":
        t = (idx.astype(U64) * U64(0x9E3779B1) & U64(0xFFFFFFFF)).astype(np.uint32)
        np.bitwise_xor.at(t, e, h32)
    elif name in ("f32_add", "f64_add"):
        v = (h32 & 15).astype(np.int64) - 8 if name == "f32_add" else (h32 & 0xFFFFF).astype(np.int64) - (1 << 19)
        s = np.zeros(ELEMS, np.int64)
        np.add.at(s, e, v)
        t = s.astype(np.float32 if name == "f32_add" else np.float64)
        assert np.abs(s).max() < 2 ** 24  # exact
    else:  # packed: 16-bit patterns, low half first
        tl, th = _packed_totals(name, blocks)
        both = np.stack([tl, th], axis=1).reshape(-1)
        if name == "pk_add_bf16":
            t = (both.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        else:
            t = both.astype(np.float16).view(np.uint16)
    return t


def test_atomic_ops_are_exported_in_table_order():
    assert canary.ATOMIC_OPS == OPS


@pytest.mark.parametrize("blocks", (1, 3, 16))
@pytest.mark.parametrize("op", OPS)
def test_atomic_expected_matches_numpy_model(op, blocks):
    got = canary.atomic_expected(op, blocks)
    want = model(op, blocks)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))  # bit for bit, floats included


@pytest.mark.parametrize("op", [o for o in OPS if o not in ("cas_inc", "ticket")])
def test_one_workgroup_leaves_elements_untouched(op):
    """blocks=1: the 32 hashed row picks (4 waves x 8 steps) of every form repeat some of the
    32 rows, so part of each table stays untouched (asserted below); those elements hold
    their initial value in the reference too."""
    gid, step = _grid(1)
    touched = np.zeros(ELEMS, bool)
    touched[_elem(OPS.index(op), gid, step)] = True
    assert 0 < touched.sum() < ELEMS
    got = canary.atomic_expected(op, 1)
    init = model(op, 0) if op not in ("pk_add_bf16", "pk_add_f16") else None
    if init is not None:
        assert np.array_equal(got[~touched].view(np.uint8), init[~touched].view(np.uint8))
    else:
        one_two = [0x3F80, 0x4000] if op == "pk_add_bf16" else [0x3C00, 0x4000]
        assert np.array_equal(got.reshape(-1, 2)[~touched], np.tile(np.uint16(one_two), ((~touched).sum(), 1)))


def test_atomic_expected_rejects_bad_arguments():
    for blocks in (0, 4097):
        with pytest.raises(ValueError):
            canary.atomic_expected("u32_add", blocks)


def test_packed_totals_stay_representable_at_the_largest_grid():
    """Operands are non-negative, so the totals grow with the grid: 4096 workgroups is the
    worst case.  A running bf16 sum holds 8 significant bits, an f16 sum 11: with every
    element's total (initial value included) <= 256 / <= 2048, every partial sum in any order
    is an integer of at most that size, so it is representable and the result is exact."""
    for name, bound in (("pk_add_bf16", 256), ("pk_add_f16", 2048)):
        tl, th = _packed_totals(name, 4096)
        print("%s at 4096 workgroups: largest element total %d (bound %d)" % (name, max(tl.max(), th.max()), bound))
        assert tl.min() >= 1 and th.min() >= 2
        assert max(tl.max(), th.max()) <= bound
    for name in ("pk_add_bf16", "pk_add_f16"):  # and the operands themselves are non-negative
        op = OPS.index(name)
        gid, step = _grid(16)
        lo, hi = _packed_operands(name, (_hash(op, gid, step) & U64(0xFFFFFFFF)).astype(np.uint32),
                                  (gid >> U64(6)) < U64(DENSE_WAVES))
        assert lo.min() >= 0 and hi.min() >= 0 and lo.max() > 0 and hi.max() > 0


# ---- metrics, log line, CLI ------------------------------------------------------------
def _result(**extra):
    r = {"ok": True, "device": 0, "error": "", "hbm_errors": 0, "mfma_errors": 0, "gemm_errors": 0,
         "lowp_errors": 0, "lds_errors": 0, "write_gbps": 6100.0, "read_gbps": 5900.0, "mfma_tflops": 1800.0}
    r.update(extra)
    return r


def _error_samples(m):
    rows = [x for x in m._canary_lines() if x.startswith("amdgpu_canary_errors{")]
    return {x.split('check="')[1].split('"')[0]: int(x.rsplit(" ", 1)[1]) for x in rows}


def test_canary_lines_carry_fabric_checks_only_when_present(make_cfg):
    m = PluginManager(make_cfg())
    m.canary_results[(0, 0)] = (time.time(), _result(l2_errors=3, xcd_errors=2, atomic_errors=4,
                                                     xcd_pairs_unreached=1))
    got = _error_samples(m)
    assert (got["l2"], got["xcd"], got["atomic"], got["xcd_unreached"]) == (3, 2, 4, 1)
    assert set(got) == {"hbm", "mfma", "gemm", "lowp", "lds", "l2", "xcd", "atomic", "xcd_unreached"}
    m.canary_results[(0, 0)] = (time.time(), _result(xcd_errors=0))
    assert set(_error_samples(m)) == {"hbm", "mfma", "gemm", "lowp", "lds", "xcd"}
    # a result without the new keys renders exactly what the site probe's tests expect today
    m.canary_results[(0, 0)] = (time.time(), _result(site_errors=5, cus_unreached=2))
    assert set(_error_samples(m)) == {"hbm", "mfma", "gemm", "lowp", "lds", "site", "unreached"}
    m.canary_results[(0, 0)] = (time.time(), _result())
    assert set(_error_samples(m)) == {"hbm", "mfma", "gemm", "lowp", "lds"}


def test_canary_result_appends_the_fabric_fields_at_the_end():
    names = [f[0] for f in canary.CanaryResult._fields_]
    assert names[-8:] == ["l2_errors", "xcd_errors", "atomic_errors", "l2_gbps", "fabric_ms", "xccs_reached",
                          "xcd_pairs_reached", "xcd_pairs_unreached"]
    assert names[-9] == "bad_sites"


class _Records(logging.Handler):
    def __init__(self):
        super().__init__(logging.DEBUG)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def test_startup_canary_log_names_the_xcd_pair(make_cfg, plugin_dir, monkeypatch):
    from k8s_gpu_device_plugin_amd.plugin import manager as manager_mod
    why = "xcd check: 2 wrong words written on xcc1, read on xcc6 (+1 more pair)"

    def run_isolated(device, nbytes, timeout=120.0):
        if device != 9:
            return {"ok": True, "device": device, "error": ""}
        return {"ok": False, "device": device, "error": why, "l2_errors": 0, "xcd_errors": 2, "atomic_errors": 0,
                "xcd_pairs_unreached": 0}
    monkeypatch.setattr(canary, "run_isolated", run_isolated)
    rec = _Records()
    manager_mod.log.addHandler(rec)
    level = manager_mod.log.level
    manager_mod.log.setLevel(logging.INFO)
    m = t = None
    try:
        with KubeletStub(plugin_dir) as k:
            m = PluginManager(make_cfg(fixture="2gpu_cpx_nps2", migStrategy="single", health={"canaryOnStart": True}))
            t = m.start_background()
            k.wait_for_registrations(1)
            deadline = time.monotonic() + 10
            while time.monotonic() < deadline and (m._start_pending or not m.counters.get("canary_failures")):
                time.sleep(0.02)
            failed = [x for x in rec.lines if x.startswith("start-up canary failed")]
            assert len(failed) == 1, rec.lines
            assert "partition 1" in failed[0] and "written on xcc1, read on xcc6" in failed[0] and why in failed[0]
            assert 'check="xcd"} 2' in "\n".join(m._canary_lines())
    finally:
        manager_mod.log.removeHandler(rec)
        manager_mod.log.setLevel(level)
        if m is not None:
            m.stop()
            t.join(10)


@pytest.mark.parametrize("counts, rc", [((0, 0, 0), 0), ((3, 0, 0), 1), ((0, 2, 0), 1), ((0, 0, 4), 1)])
def test_fabric_cli_prints_json_and_fails_on_any_error(monkeypatch, capsys, counts, rc):
    calls = []

    def fabric_check(device=0, **kw):
        calls.append((device, kw))
        return {"l2_errors": counts[0], "xcd_errors": counts[1], "atomic_errors": counts[2], "xccs_reached": 8,
                "pairs": {"xcc1>xcc6": {"reads": 4, "bad": counts[1]}}}
    monkeypatch.setattr(canary, "fabric_check", fabric_check)
    assert canary.main(["--fabric", "--device", "2"]) == rc
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1
    assert json.loads(out[0])["pairs"]["xcc1>xcc6"] == {"reads": 4, "bad": counts[1]}
    assert calls == [(2, {})]
