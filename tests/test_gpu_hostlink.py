"""Host-link check of the gfx950 canary (``ops/hostlink/hostlink.hip``) on a real MI355X: a
payload crosses the link to the host in both directions by kernel and by copy engine, the
system-scope atomics are exact next to the host's own, and an injected fault is counted
exactly and reported at its place.

Rates measured on an MI355X (SPX, x16 Gen5, 64 MiB, median of 12 calls in one process):
kernel read 56.6, kernel write 51.8, copy h2d 54.3, copy d2h 56.1 GB/s, beside the link's
63 GB/s (``docs/CANARY.md``).  The only rate bound asserted here is that ceiling."""
import math

import pytest

pytestmark = pytest.mark.gpu

RATES = ("kernel_read_gbps", "kernel_write_gbps", "copy_h2d_gbps", "copy_d2h_gbps")
LINK_SPEC_GBPS = 63.0  # PCIe Gen5 x16 per direction
COUNTS = ("read_errors", "write_errors", "h2d_errors", "d2h_errors", "atomic_errors", "unlocated_errors")
FLIP_BYTE = 4  # the injected flip is bit 9 of 32-bit word 1 of a 16-byte word


def _check(**kw):
    from k8s_gpu_device_plugin_amd.ops import hostlink
    return hostlink.host_link_check(**kw)


@pytest.fixture(scope="module")
def healthy():
    return _check()


def _assert_clean(r, nbytes):
    assert {k: r[k] for k in COUNTS} == dict.fromkeys(COUNTS, 0), r["error"]
    assert r["ok"] is True and r["error"] == "" and r["moved"] == 0
    assert not any(r["atomic"].values()) and all(v is None for v in r["first_bad"].values())
    assert r["bytes"] == nbytes
    # every byte was read once per repetition, by workgroups that are accounted for
    assert sum(x["read_bytes"] for x in r["xccs"].values()) == nbytes * r["reps"]
    assert all(x["read_bad"] == 0 and x["write_bad"] == 0 for x in r["xccs"].values())
    assert len([x for x in r["xccs"].values() if x["read_blocks"]]) == r["xccs_reached"]


def test_healthy_defaults(healthy):
    from k8s_gpu_device_plugin_amd.ops import canary
    r = healthy
    print("host link: %d workgroups, 64 MiB: kernel read %.1f, kernel write %.1f, copy h2d %.1f, copy d2h %.1f GB/s; "
          "ms read %.3f write %.3f h2d %.3f d2h %.3f atomic %.3f (grid %d), host cpu %.1f; xccs %d, moved %d, overlap %d"
          % (r["blocks"], r["kernel_read_gbps"], r["kernel_write_gbps"], r["copy_h2d_gbps"], r["copy_d2h_gbps"],
             r["read_ms"], r["write_ms"], r["h2d_ms"], r["d2h_ms"], r["atomic_ms"], r["atomic_blocks"],
             r["host_cpu_ms"], r["xccs_reached"], r["moved"], r["atomic_overlap"]))
    _assert_clean(r, 64 << 20)
    assert r["reps"] == 1 and r["host_adds"] == 1024 and r["atomic_blocks"] == 64 and r["blocks"] >= 1
    assert r["xccs_reached"] == canary.fabric_check()["xccs_reached"]
    busy = [x for x in r["read_block_xcc"] if x >= 0]
    assert len(busy) == r["blocks"] == sum(x["read_blocks"] for x in r["xccs"].values())  # 4096 tiles: no idle workgroup
    assert r["write_block_xcc"] and all(x >= 0 for x in r["write_block_xcc"])
    assert r["atomic_overlap"] in (0, 1)  # reported, not required


def test_rates_are_finite_positive_and_below_the_links_ceiling(healthy):
    for k in RATES:
        assert math.isfinite(healthy[k]) and healthy[k] > 0, (k, healthy[k])
        # more than the link can carry means the bytes did not cross it
        assert healthy[k] <= 1.25 * LINK_SPEC_GBPS, (k, healthy[k])
    assert all(healthy[k] > 0 for k in ("read_ms", "write_ms", "h2d_ms", "d2h_ms", "atomic_ms", "host_cpu_ms"))


def test_one_word_one_active_lane():
    r = _check(nbytes=16)
    _assert_clean(r, 16)
    assert r["xccs_reached"] == 1 and [x for x in r["read_block_xcc"] if x >= 0] == r["read_block_xcc"][:1]
    (slot,) = r["xccs"].values()
    assert (slot["read_blocks"], slot["read_bytes"], slot["write_blocks"]) == (1, 16, 1)


def test_one_tile_and_one_word_exercises_the_tail():
    from k8s_gpu_device_plugin_amd.ops import hostlink
    tile = hostlink.tile_words()
    r = _check(nbytes=(tile + 1) * 16, blocks=4)
    _assert_clean(r, (tile + 1) * 16)
    assert r["read_block_xcc"][2:] == [-1, -1] and min(r["read_block_xcc"][:2]) >= 0  # a whole tile, then the tail
    assert sorted(x["read_bytes"] for x in r["xccs"].values() if x["read_bytes"])[0] in (16, (tile + 1) * 16)
    _assert_clean(_check(nbytes=(tile + 1) * 16, blocks=1), (tile + 1) * 16)  # both in one workgroup


def test_one_workgroup():
    r = _check(nbytes=1 << 20, blocks=1)
    _assert_clean(r, 1 << 20)
    assert r["blocks"] == 1 and r["xccs_reached"] == 1 and r["read_block_xcc"] == r["write_block_xcc"]


def test_idle_workgroups_add_nothing():
    from k8s_gpu_device_plugin_amd.ops import hostlink
    tile = hostlink.tile_words()
    r = _check(nbytes=4 * tile * 16, blocks=64)  # 4 tiles, 64 workgroups
    _assert_clean(r, 4 * tile * 16)
    assert r["blocks"] == 64
    assert [x >= 0 for x in r["read_block_xcc"]] == [True] * 4 + [False] * 60
    assert [x >= 0 for x in r["write_block_xcc"]] == [True] * 4 + [False] * 60
    assert sum(x["read_blocks"] for x in r["xccs"].values()) == 4 == sum(x["write_blocks"] for x in r["xccs"].values())


def test_two_repetitions():
    r = _check(nbytes=1 << 20, blocks=8, reps=2)
    _assert_clean(r, 1 << 20)  # read_bytes sums to twice the buffer
    assert r["reps"] == 2 and sum(x["read_blocks"] for x in r["xccs"].values()) == 16


@pytest.mark.parametrize("unroll", [2, 8])
def test_the_other_tile_sizes(unroll):
    from k8s_gpu_device_plugin_amd.ops import hostlink
    n = 3 * hostlink.tile_words(unroll) + 5
    _assert_clean(_check(nbytes=n * 16, blocks=2, unroll=unroll), n * 16)


# ---- fault injection: 3 faults at 1 MiB, 8 workgroups --------------------------------------
N_WORDS, BLOCKS, INJECT_N = (1 << 20) // 16, 8, 3
STAGE_COUNT = {"read": "read_errors", "write": "write_errors", "h2d": "h2d_errors", "d2h": "d2h_errors"}
TEXT = {"read": "host read check: 3 wrong words read on xcc", "write": "host write check: 3 wrong words written on xcc",
        "h2d": "host copy check: 3 wrong words after the host-to-device copy (first at offset 0x",
        "d2h": "host copy check: 3 wrong words after the device-to-host copy (first at offset 0x"}


def _planted_words(kind, tile):
    """The 16-byte words the injection corrupts: the host's are spread over the buffer, a
    workgroup's is the first word it stores (word b * tile of workgroup b)."""
    if kind in ("read", "h2d"):
        stride = N_WORDS // INJECT_N
        return [f * stride + stride // 2 for f in range(INJECT_N)]
    return [b * tile for b in range(INJECT_N)]


@pytest.mark.parametrize("kind", ["read", "write", "h2d", "d2h"])
def test_injected_bulk_fault_is_counted_and_located(kind):
    from k8s_gpu_device_plugin_amd.ops import hostlink
    tile = hostlink.tile_words()
    r = _check(nbytes=1 << 20, blocks=BLOCKS, inject=kind, inject_n=INJECT_N)
    want = dict.fromkeys(COUNTS, 0)
    want[STAGE_COUNT[kind]] = INJECT_N
    assert {k: r[k] for k in COUNTS} == want and r["ok"] is False
    words = _planted_words(kind, tile)
    first = {s: None for s in ("read", "write", "h2d", "d2h", "atomic")}
    first[kind] = {"offset": words[0] * 16 + FLIP_BYTE}
    owners = [(w // tile) % BLOCKS for w in words]  # the workgroup that read or wrote each planted word
    if kind in ("read", "write"):
        block_xcc = r[kind + "_block_xcc"]
        first[kind]["xcc"] = block_xcc[owners[0]]
        bad = {}
        for b in owners:
            bad["xcc%d" % block_xcc[b]] = bad.get("xcc%d" % block_xcc[b], 0) + 1
        assert {x: s[kind + "_bad"] for x, s in r["xccs"].items() if s[kind + "_bad"]} == bad
    else:
        assert all(s["read_bad"] == 0 and s["write_bad"] == 0 for s in r["xccs"].values())
    assert r["first_bad"] == first
    assert r["error"].startswith(TEXT[kind]), r["error"]
    assert "(first at offset 0x%x)" % (words[0] * 16 + FLIP_BYTE) in r["error"]
    if kind in ("read", "write"):
        assert r["error"].startswith(TEXT[kind] + "%d " % first[kind]["xcc"]), r["error"]


@pytest.mark.parametrize("op", ["u32_add", "u64_add", "ticket", "cas_inc", "swap"])
def test_injected_atomic_fault_shows_in_that_form_only(op):
    r = _check(nbytes=1 << 20, blocks=BLOCKS, inject="atomic", inject_op=op)
    assert {k: r[k] for k in COUNTS} == dict(dict.fromkeys(COUNTS, 0), atomic_errors=1)
    assert r["atomic"] == dict({name: 0 for name in r["atomic"]}, **{op: 1})
    assert r["first_bad"]["atomic"]["op"] == op and r["first_bad"]["atomic"]["element"] >= 0
    assert r["error"] == "host atomic check: 1 wrong element in %s (first at %d)" % (
        op.replace("_", " "), r["first_bad"]["atomic"]["element"])


def test_atomics_are_exact_without_the_hosts_adds_and_on_a_smaller_grid():
    r = _check(nbytes=1 << 20, blocks=BLOCKS, host_adds=0, atomic_blocks=13)
    _assert_clean(r, 1 << 20)
    assert r["atomic_blocks"] == 13 and r["host_adds"] == 0 and r["atomic_overlap"] == 0


# ---- merged into the full run --------------------------------------------------------------
def test_run_merges_the_check_only_when_asked():
    from k8s_gpu_device_plugin_amd.ops import canary
    merged = {"host_read_errors", "host_write_errors", "host_copy_errors", "host_atomic_errors", "host_ms"} | set(RATES)
    plain = canary.run(0, 64 << 20, 1, 256)
    assert plain["ok"], plain["error"]
    assert not merged & set(plain)
    r = canary.run(0, 64 << 20, 1, 256, host_link=True, host_link_bytes=1 << 20)
    assert r["ok"], r["error"]
    assert set(r) - set(plain) == merged
    assert (r["host_read_errors"], r["host_write_errors"], r["host_copy_errors"], r["host_atomic_errors"]) == (0, 0, 0, 0)
    assert all(0 < r[k] <= 1.25 * LINK_SPEC_GBPS for k in RATES) and r["host_ms"] > 0
