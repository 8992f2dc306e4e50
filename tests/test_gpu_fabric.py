"""Fabric check of the gfx950 canary (``ops/fabric.hip``) on a real MI355X: the march through
each XCD's L2, the cross-XCD exchange and the global atomics are exact on a healthy device,
cover what they report, and an injected fault is counted exactly and reported at its place."""
import pytest

pytestmark = pytest.mark.gpu

INJECT_WORD_OFFSET = 37 * 16 + 4  # the byte offset of the 32-bit word whose bit 9 is flipped


def _fabric(**kw):
    from k8s_gpu_device_plugin_amd.ops import canary
    return canary.fabric_check(**kw)


@pytest.fixture(scope="module")
def healthy():
    return _fabric()


def _lists(slice_xcc):
    """The slices of each writer xcc in slice order, as the host builds them."""
    out = {}
    for s, x in enumerate(slice_xcc):
        out.setdefault(x, []).append(s)
    return out


def _reads_per_slice(slice_xcc):
    """How often the exchange reads each slice: reader r takes list_w[r % len(list_w)] of every writer w."""
    reads = [0] * len(slice_xcc)
    for lst in _lists(slice_xcc).values():
        for r in range(len(slice_xcc)):
            reads[lst[r % len(lst)]] += 1
    return reads


def _assert_exact(r, blocks, slice_kb):
    assert (r["l2_errors"], r["xcd_errors"], r["atomic_errors"], r["unlocated_errors"]) == (0, 0, 0, 0), r["error"]
    assert r["moved"] == 0 and r["error"] == "" and r["first_bad"] == {"l2": None, "atomic": None}
    assert not any(r["atomic"].values())
    assert r["blocks"] == blocks == len(r["slice_xcc"])
    assert sum(x["blocks"] for x in r["xccs"].values()) == blocks
    assert all(x["bytes"] == x["blocks"] * slice_kb * 1024 and x["bad"] == 0 for x in r["xccs"].values())
    assert {"xcc%d" % x for x in r["slice_xcc"]} == set(r["xccs"]) and len(r["xccs"]) == r["xccs_reached"]
    assert r["pairs_reached"] == r["pairs_expected"] == r["xccs_reached"] ** 2 == len(r["pairs"])
    # every slice was read, and the matrix holds exactly the reads the r % len rule gives
    reads = _reads_per_slice(r["slice_xcc"])
    assert min(reads) >= 1
    for w in set(r["slice_xcc"]):
        got = sum(p["reads"] for k, p in r["pairs"].items() if k.startswith("xcc%d>" % w))
        assert got == blocks == sum(n for s, n in enumerate(reads) if r["slice_xcc"][s] == w)
    assert all(p["bad"] == 0 for p in r["pairs"].values())


def test_healthy_defaults(healthy):
    from k8s_gpu_device_plugin_amd.ops import canary
    r = healthy
    print("fabric check: %d workgroups x %d KiB, %.3f ms (march %.3f, exchange %.3f, atomics %.3f), l2 %.0f GB/s, "
          "xccs %d, pairs %d/%d, moved %d" % (r["blocks"], r["slice_kb"], r["ms"], r["march_ms"], r["exchange_ms"],
                                             r["atomic_ms"], r["l2_gbps"], r["xccs_reached"], r["pairs_reached"],
                                             r["pairs_expected"], r["moved"]))
    assert r["xccs_reached"] in (1, 2, 4, 8)  # CPX, QPX, DPX or SPX
    assert r["slice_kb"] == 64 and r["blocks"] >= 1
    _assert_exact(r, r["blocks"], 64)
    assert set(r["atomic"]) == set(canary.ATOMIC_OPS)
    assert r["ms"] > 0 and r["l2_gbps"] > 0


def test_one_workgroup_one_xcc_one_pair():
    r = _fabric(blocks=1)
    _assert_exact(r, 1, 64)
    assert r["xccs_reached"] == 1 and r["pairs_reached"] == 1
    (pair, cell), = r["pairs"].items()
    assert pair == "xcc%d>xcc%d" % (r["slice_xcc"][0], r["slice_xcc"][0]) and cell["reads"] == 1
    # 2048 lane-operations per form touch part of each 2048-element table: atomic_errors == 0
    # above says the untouched elements still hold their initial values


def test_grid_that_is_no_multiple_of_the_xcds(healthy):
    r = _fabric(blocks=13)
    _assert_exact(r, 13, 64)
    if healthy["xccs_reached"] == 8:  # 13 slices over 8 writers: lists of unequal length
        assert len({len(v) for v in _lists(r["slice_xcc"]).values()}) > 1


def test_smallest_slice_one_word_per_thread(healthy):
    r = _fabric(slice_kb=4, reps=1)
    _assert_exact(r, healthy["blocks"], 4)


def test_injected_l2_fault_is_counted_and_located():
    reps = 2
    r = _fabric(inject="l2", blocks=16, inject_blocks=3, reps=reps)
    print("inject l2:", r["error"], r["xccs"])
    assert r["l2_errors"] == 3 * reps  # seen once per reverse pass, then overwritten by the complement
    assert r["xcd_errors"] == 0 and r["atomic_errors"] == 0 and r["moved"] == 0
    bad = {x for x, v in r["xccs"].items() if v["bad"]}
    assert bad == {"xcc%d" % x for x in r["slice_xcc"][:3]}
    assert sum(v["bad"] for v in r["xccs"].values()) == 3 * reps
    assert r["first_bad"]["l2"] == {"xcc": r["slice_xcc"][0], "slice": 0, "offset": INJECT_WORD_OFFSET}
    assert r["error"].startswith("l2 check: %d wrong words on xcc%d (slice 0, offset 0x%x)"
                                 % (3 * reps, r["slice_xcc"][0], INJECT_WORD_OFFSET))


def test_injected_xcd_fault_is_seen_only_by_the_exchange():
    r = _fabric(inject="xcd", blocks=16, inject_blocks=3, reps=2)
    print("inject xcd:", r["error"], {k: v for k, v in r["pairs"].items() if v["bad"]})
    assert r["l2_errors"] == 0 and r["atomic_errors"] == 0 and r["moved"] == 0
    assert r["xcd_errors"] > 0
    writers = {k.split(">")[0] for k, v in r["pairs"].items() if v["bad"]}
    assert writers == {"xcc%d" % x for x in r["slice_xcc"][:3]}
    # one flipped bit per injected slice: each read of one contributes exactly one word
    reads = _reads_per_slice(r["slice_xcc"])
    assert r["xcd_errors"] == sum(reads[:3]) == sum(v["bad"] for v in r["pairs"].values())
    for w in {r["slice_xcc"][s] for s in range(3)}:
        want = sum(reads[s] for s in range(3) if r["slice_xcc"][s] == w)
        assert sum(v["bad"] for k, v in r["pairs"].items() if k.startswith("xcc%d>" % w)) == want
    assert all(v["bad"] <= v["reads"] for v in r["pairs"].values())
    assert r["error"].startswith("xcd check: %d wrong words written on xcc" % r["xcd_errors"])


def _atomic_ops():
    from k8s_gpu_device_plugin_amd.ops import canary
    return getattr(canary, "ATOMIC_OPS", ("missing",))


@pytest.mark.parametrize("op", _atomic_ops())
def test_injected_atomic_fault_is_reported_in_its_operation(op):
    r = _fabric(inject="atomic", inject_op=op, blocks=8, inject_blocks=2)
    print("inject atomic %s:" % op, r["error"])
    assert r["atomic"][op] > 0
    assert [n for o, n in r["atomic"].items() if o != op] == [0] * (len(r["atomic"]) - 1)
    assert r["atomic_errors"] == r["atomic"][op] and r["l2_errors"] == 0 and r["xcd_errors"] == 0
    assert r["first_bad"]["atomic"]["op"] == op
    name = op if op.startswith("pk_") else op.replace("_", " ")  # "u64 add", as the instruction: "pk_add_bf16"
    assert r["error"] == "atomic check: %d wrong elements in %s (first at %d)" % (
        r["atomic"][op], name, r["first_bad"]["atomic"]["element"])


@pytest.mark.parametrize("kw", [dict(slice_kb=6), dict(reps=0)])
def test_bad_arguments_raise_without_launching(kw):
    with pytest.raises(RuntimeError, match="bad arguments"):
        _fabric(**kw)


def test_canary_run_reports_the_fabric_check():
    from k8s_gpu_device_plugin_amd.ops import canary
    r = canary.run(0, 64 << 20, 1, 256)
    assert r["ok"], r
    assert (r["l2_errors"], r["xcd_errors"], r["atomic_errors"]) == (0, 0, 0)
    assert r["fabric_ms"] > 0 and r["xccs_reached"] >= 1 and r["xcd_pairs_unreached"] == 0
    assert r["xcd_pairs_reached"] == r["xccs_reached"] ** 2
