"""The LDS-path check's host side (``ops/ldspath/ldspath_host.h``, reached through
``ops/ldspath.py``) against the independent numpy model of ``tests/ldspath_model.py``, no GPU:
every lane map, the transposed read's addresses and gather, the image pattern, the atomics'
expected tables and operand rules, and the reduction with its texts on hand-built records.
``tests/native/ldspath_selftest.cpp`` runs the same header under AddressSanitizer and UBSan as a
program of its own."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ldspath_model as model
from k8s_gpu_device_plugin_amd import _build
from k8s_gpu_device_plugin_amd.ops import ldspath

A = ldspath.pack_site(3, 1, 0, 7, 2)
A3 = ldspath.pack_site(3, 1, 0, 7, 3)
B = ldspath.pack_site(4, 0, 1, 2, 1)
ROR3 = 20  # index of "dpp row_ror:3"
U64_ADD = 1


def rec(site, sub=0, bad=0, at=0, last=None):
    return (site, site if last is None else last, sub if bad else ldspath.UNWRITTEN, at, {sub: bad} if bad else {})


# ---- lane maps -----------------------------------------------------------------------------
def test_the_table_names_what_the_issue_lists():
    names = ldspath.LANE_OPS
    assert len(names) == len(set(names)) <= ldspath.SUBS and names[ROR3] == "dpp row_ror:3"
    for needle in ("ds_bpermute hash", "ds_bpermute rot:", "ds_permute", "ds_swizzle swap:", "ds_swizzle reverse:",
                   "ds_swizzle broadcast:", "ds_swizzle quad_perm:", "dpp quad_perm:", "dpp row_shl:1", "dpp row_shr:1",
                   "dpp row_ror:1", "dpp row_mirror", "dpp row_half_mirror", "dpp wave_shl:1", "dpp wave_rol:1",
                   "dpp wave_shr:1", "dpp wave_ror:1", "dpp row_bcast:15", "dpp row_bcast:31", "row_mask:0x6",
                   "bank_mask:0x9", "bound_ctrl", "v_permlane32_swap", "v_permlane16_swap", "v_readlane", "v_readfirstlane",
                   "v_writelane"):
        assert any(needle in n for n in names), needle
    assert sum(n.startswith("dpp quad_perm:") for n in names) >= 3
    assert ldspath.ATOMIC_FORMS == model.FORMS
    assert len(ldspath.WIDTH_PASSES) == len(ldspath.WIDTH_PASS_KINDS) == 6
    assert ldspath.WIDTH_PASS_KINDS == ("plain", "plain", "subword", "subword", "dma", "conflict")
    assert ldspath.WIDTH_PASSES[3] == "8-bit store" and ldspath.WIDTH_PASSES[4] == "dma fill"


def test_every_lane_map_equals_the_model():
    bijective = 0
    for k, name in enumerate(ldspath.LANE_OPS):
        want = [[int(c) for c in out] for out in model.lane_op(name)]
        got = ldspath.lane_map(k)
        assert got == want, name
        assert all(0 <= c <= ldspath.SRC_ZERO for out in got for c in out), name
        assert len(got) == (2 if "swap" in name and name.startswith("v_permlane") else 1), name
        if model.is_bijective(want):
            bijective += 1
            assert sorted(got[0]) == list(range(64)), name
        if name.startswith("ds_permute"):  # collisions are left out on purpose: bijections only
            assert model.is_bijective(want), name
    assert bijective >= 12
    # what the two swaps return together is all 128 values, each once
    for name in ("v_permlane32_swap", "v_permlane16_swap"):
        both = ldspath.lane_map(ldspath.LANE_OPS.index(name))
        assert sorted(both[0] + both[1]) == list(range(128))
    for bad in (-1, len(ldspath.LANE_OPS)):
        with pytest.raises(ValueError):
            ldspath.lane_map(bad)


def test_lanes_that_keep_old_and_lanes_that_read_zero_are_predicted():
    by_name = {n: ldspath.lane_map(k)[0] for k, n in enumerate(ldspath.LANE_OPS)}
    shr1 = by_name["dpp row_shr:1"]
    assert [shr1[l] for l in (0, 16, 32, 48)] == [64, 80, 96, 112] and shr1[1] == 0 and shr1[17] == 16
    zero = by_name["dpp row_shr:3 bound_ctrl"]
    assert zero[:4] == [ldspath.SRC_ZERO] * 3 + [0]
    masked = by_name["dpp row_mirror row_mask:0x6"]
    assert masked[:16] == list(range(64, 80)) and masked[16:32] == list(range(31, 15, -1)) and masked[48:] == list(range(112, 128))
    banked = by_name["dpp row_ror:5 bank_mask:0x9"]
    assert banked[4:12] == list(range(68, 76)) and banked[0] == 11 and banked[12] == 7


# ---- the transposed read -------------------------------------------------------------------
def test_tr_map_equals_the_model_and_stays_in_the_image():
    for r in range(ldspath.TR_FIXED_ROUNDS + 64):
        addr, src = ldspath.tr_map(r)
        want = model.tr_addresses(r)
        assert addr == want and src == model.tr_sources(want), r
        assert all(a % 8 == 0 and 0 <= a <= ldspath.TR_IMAGE_BYTES - 8 for a in addr), r
        assert all(0 <= e < ldspath.TR_IMAGE_BYTES // 2 for lane in src for e in lane), r
    strides = [ldspath.tr_map(r)[0][4] - ldspath.tr_map(r)[0][0] for r in range(4)]
    assert strides == [32, 64, 256, 264]
    # a hashed round: the rows of one group lie all over the image
    addr, _ = ldspath.tr_map(ldspath.TR_FIXED_ROUNDS)
    assert len(set(addr)) > 56 and max(addr) - min(addr) > ldspath.TR_IMAGE_BYTES // 2
    for bad in (-1, ldspath.TR_FIXED_ROUNDS + 64):
        with pytest.raises(ValueError):
            ldspath.tr_map(bad)


def test_the_image_pattern_is_a_bijection():
    for seed in (0, 1, 0x1D5A, 0x1D5D, 0xFFFF, 0x12345):
        assert len(np.unique(model.tr_pattern(seed))) == 65536


# ---- atomics -------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 8])
def test_atomic_expected_equals_the_model(steps):
    for form, name in enumerate(ldspath.ATOMIC_FORMS):
        assert ldspath.atomic_expected(form, steps) == [int(v) for v in model.atomic_table(form, steps)], name
    ticket = ldspath.atomic_expected(ldspath.ATOMIC_FORMS.index("ticket"), steps)
    assert ticket[:256] == [steps] * 256 and ticket[256] == 256 * steps and not any(ticket[257:])


def test_atomic_expected_refuses_bad_arguments():
    for form, steps in ((-1, 1), (10, 1), (0, 0), (0, 65)):
        with pytest.raises(ValueError):
            ldspath.atomic_expected(form, steps)


def test_operand_rules():
    """The injected bit is in no and / or mask, and no f32 partial sum can leave the exact range."""
    forms = model.FORMS
    for t in range(model.THREADS):
        for s in range(8):
            assert model.atomic_operand(forms.index("and"), t, s) & model.INJECT_BIT
            assert not model.atomic_operand(forms.index("or"), t, s) & model.INJECT_BIT
            assert -4 <= model.atomic_operand(forms.index("f32 add"), t, s) <= 4
    assert model.f32_partial_sum_bound(64) < 1 << 24  # 64: the most steps the check accepts
    # the and / or tables: bit 9 still set / still clear everywhere
    assert all(v & model.INJECT_BIT for v in ldspath.atomic_expected(forms.index("and"), 8))
    assert not any(v & model.INJECT_BIT for v in ldspath.atomic_expected(forms.index("or"), 8))


# ---- the reduction -------------------------------------------------------------------------
def test_reduce_a_clean_set_and_an_empty_set():
    r = ldspath.reduce(widths=[rec(A), rec(A3), rec(B)], atomic=[rec(A)], lane=[rec(A), rec(B)], tr=[rec(B)])
    assert r["ok"] is True and r["error"] == "" and r["ldspath_errors"] == 0 and r["bad_sites"] == []
    assert (r["waves"], r["moved"], r["cus_reached"], r["simds_reached"]) == (3, 0, 2, 3)
    assert r["stage_waves"] == {"widths": 3, "atomic": 1, "lane": 2, "tr": 1}
    assert all(t == "" for t in r["texts"].values())
    r = ldspath.reduce()
    assert r["ok"] is True and r["waves"] == 0 and r["cus_reached"] == 0 and r["error"] == ""


def test_reduce_one_bad_site_and_two():
    r = ldspath.reduce(widths=[rec(A, 3, 3, 0x1a40), rec(A3)])
    assert r["error"] == "lds check: 3 wrong words at xcc3/se1/sh0/cu7 (pass 4, 8-bit store; first at offset 0x1a40)"
    assert r["ok"] is False and (r["lds_errors"], r["subword_errors"], r["ldspath_errors"]) == (3, 3, 3)
    assert r["bad_sites"] == ["xcc3/se1/sh0/cu7/simd2"] and r["bad_by"]["widths"] == {"8-bit store": 3}
    r = ldspath.reduce(widths=[rec(B, 0, 1, 0x10), rec(A, 3, 3, 0x1a40), rec(A3, 5, 2, 0x20)])
    assert r["error"] == "lds check: 6 wrong words at xcc3/se1/sh0/cu7 (pass 4, 8-bit store; first at offset 0x1a40; +1 more CU)"
    assert (r["plain_errors"], r["subword_errors"], r["conflict_errors"], r["n_bad"]) == (1, 3, 2, 3)
    assert r["bad_sites"] == ["xcc3/se1/sh0/cu7/simd2", "xcc3/se1/sh0/cu7/simd3", "xcc4/se0/sh1/cu2/simd1"]


def test_the_four_texts_word_for_word():
    r = ldspath.reduce(widths=[rec(A, 3, 3, 0x1a40), rec(B, 0, 1)], atomic=[rec(ldspath.pack_site(1, 0, 0, 3), U64_ADD, 2, 41)],
                       lane=[rec(A, ROR3, 4), rec(B, ROR3, 1)], tr=[rec(A, 0, 2, 1), rec(A3, 0, 1), rec(B, 0, 1)])
    assert r["texts"] == {
        "widths": "lds check: 4 wrong words at xcc3/se1/sh0/cu7 (pass 4, 8-bit store; first at offset 0x1a40; +1 more CU)",
        "atomic": "lds atomic check: 2 wrong elements in u64 add at xcc1/se0/sh0/cu3 (first at 41)",
        "lane": "lane check: 5 wrong words in dpp row_ror:3 at xcc3/se1/sh0/cu7/simd2 (+1 more site)",
        "tr": "lds transpose check: 4 wrong elements at xcc3/se1/sh0/cu7/simd2 (+2 more sites)"}
    assert r["error"] == r["texts"]["widths"]
    assert r["bad_by"]["lane"] == {"dpp row_ror:3": 5} and r["bad_by"]["atomic"] == {"u64 add": 2}
    assert r["ldspath_errors"] == 4 + 2 + 5 + 4
    # the first failing stage supplies the error
    r = ldspath.reduce(widths=[rec(A)], lane=[rec(A, ROR3, 4)], tr=[rec(A, 0, 2)])
    assert r["error"] == "lane check: 4 wrong words in dpp row_ror:3 at xcc3/se1/sh0/cu7/simd2"


def test_reduce_a_moved_wave_is_unlocated_and_still_fails():
    r = ldspath.reduce(lane=[rec(A, ROR3, 4, last=B), rec(B)])
    assert (r["lane_errors"], r["unlocated_errors"], r["ldspath_errors"]) == (0, 4, 4) and r["ok"] is False
    assert r["stage_moved"]["lane"] == 1 and r["bad_sites"] == []
    assert r["error"] == "ldspath check: 4 wrong words at an unknown site"
    r = ldspath.reduce(widths=[rec(A, 0, 1, last=A3), rec(B)])
    assert (r["waves"], r["moved"], r["unlocated_errors"], r["cus_reached"]) == (1, 1, 1, 1)


def test_reduce_dma_alone_and_beside_a_plain_error():
    """Wrong words after the DMA fill may be L2's or HBM's: they fail the check while the plain-store
    passes are clean, and beside a plain-store error they are reported and not added."""
    r = ldspath.reduce(widths=[rec(A, 4, 1, 0x40)])
    assert (r["dma_errors"], r["lds_errors"], r["ldspath_errors"], r["ok"]) == (1, 0, 1, False)
    assert r["error"] == "lds dma check: 1 wrong word at xcc3/se1/sh0/cu7 (pass 5, dma fill; first at offset 0x40)"
    r = ldspath.reduce(widths=[rec(A, 4, 1, 0x40), rec(B, 0, 2, 8)])
    assert (r["dma_errors"], r["lds_errors"], r["ldspath_errors"]) == (1, 2, 2)
    assert r["error"].startswith("lds check: 2 wrong words at xcc3/se1/sh0/cu7 (pass 5, dma fill;")


def test_reduce_skips_unwritten_slots_and_refuses_a_site_out_of_range():
    r = ldspath.reduce(widths=[rec(A), (ldspath.UNWRITTEN, ldspath.UNWRITTEN, ldspath.UNWRITTEN, 0, {})])
    assert r["waves"] == 1 and r["moved"] == 0
    with pytest.raises(ValueError):
        ldspath.reduce(widths=[rec(ldspath.SITE_SLOTS)])
    with pytest.raises(ValueError):
        ldspath.reduce(tr=[rec(A, last=ldspath.SITE_SLOTS)])


def test_more_than_sixteen_bad_sites_are_counted():
    rows = [rec(ldspath.pack_site(x, 0, 0, cu, 0), ROR3, 1) for x in range(2) for cu in range(10)]
    r = ldspath.reduce(lane=rows)
    assert r["n_bad"] == 20 and len(r["bad_sites"]) == 16 and r["lane_errors"] == 20
    assert r["error"].endswith("(+19 more sites)")


# ---- the same header under sanitizers ------------------------------------------------------
def test_sanitized_selftest_program(tmp_path):
    """Host code under AddressSanitizer and UBSan as a program of its own: nothing sanitized
    is loaded into Python."""
    cxx = shutil.which(_build._cxx())
    assert cxx, "no C++ compiler"
    src = os.path.join(_build.HARNESS_DIR, "ldspath_selftest.cpp")
    exe = str(tmp_path / "ldspath_selftest")
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + _build.LDSPATH_DIR,
                        src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
           "PATH": "/usr/bin:/bin"}  # as tests/test_native_selftest.py runs its program
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", p.stdout[-3000:]
