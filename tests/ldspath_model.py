"""An independent numpy model of what the LDS-path check (``ops/ldspath/``) exercises, written
from the instruction descriptions and not from ``ldspath_host.h``: what every lane receives
from each lane-crossing op (``old`` retention included), the transposed read's gather, the
width passes' patterns and the atomics' tables.  The ops are named as ``ldspath.LANE_OPS``
names them, and their parameters are parsed from the names.

Source codes, as ``ldspath.lane_map`` uses them: 0..63 the ``x`` of that lane, ``64 + l`` the
second value of lane ``l`` (DPP's and writelane's ``old``, the swaps' other operand), 128 a zero."""
import re

import numpy as np

ZERO = 128
LANES = np.arange(64)
M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1


def mix32(x: int) -> int:
    """The 64-bit finaliser of MurmurHash3, low word."""
    x &= M64
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & M64
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & M64
    x ^= x >> 33
    return x & M32


# ---- lane-crossing ops ---------------------------------------------------------------------
def _gather(src):
    """A pull: lane l receives x of lane src[l]."""
    return [np.asarray(src, dtype=int) & 63]


def _quad_perm(sel):
    return (LANES & ~3) | np.array([sel[l & 3] for l in LANES])


def _dpp(ctrl, arg, row_mask=0xF, bank_mask=0xF, bound_ctrl=False):
    """v_*_dpp: the source lane per control, None where the control has none; a lane whose row
    or bank is masked off, or (without bound_ctrl) has no source, keeps ``old``."""
    out = []
    for l in range(64):
        row, i = l // 16, l % 16
        if ctrl == "quad_perm":
            s = (l & ~3) | arg[l & 3]
        elif ctrl == "row_shl":  # lane i of a row reads lane i + n of it
            s = l + arg if i + arg <= 15 else None
        elif ctrl == "row_shr":  # ... lane i - n
            s = l - arg if i - arg >= 0 else None
        elif ctrl == "row_ror":  # rotate right within the row: lane i reads lane (i - n) mod 16
            s = row * 16 + (i - arg) % 16
        elif ctrl == "wave_shl":
            s = l + 1 if l < 63 else None
        elif ctrl == "wave_rol":
            s = (l + 1) % 64
        elif ctrl == "wave_shr":
            s = l - 1 if l > 0 else None
        elif ctrl == "wave_ror":
            s = (l - 1) % 64
        elif ctrl == "row_mirror":
            s = row * 16 + 15 - i
        elif ctrl == "row_half_mirror":
            s = (l // 8) * 8 + 7 - l % 8
        elif ctrl == "row_bcast" and arg == 15:  # lane 15 of each row to the whole next row
            s = row * 16 - 1 if row > 0 else None
        elif ctrl == "row_bcast" and arg == 31:  # lane 31 to rows 2 and 3
            s = 31 if row >= 2 else None
        else:
            raise ValueError(ctrl)
        enabled = (row_mask >> row) & 1 and (bank_mask >> (i // 4)) & 1
        if not enabled:
            out.append(64 + l)
        elif s is None:
            out.append(ZERO if bound_ctrl else 64 + l)
        else:
            out.append(s)
    return [np.array(out)]


def lane_op(name: str):
    """One array of 64 source codes per output of the op called ``name``."""
    ints = [int(v, 0) for v in re.findall(r"0x[0-9a-fA-F]+|\d+", name.split(" ", 1)[1])] if " " in name else []
    if name == "ds_bpermute hash":  # a pull with a many-to-one address: every lane names its source
        return _gather([((l * 0x9E5 + 0x2B) >> 3) & 63 for l in range(64)])
    if name.startswith("ds_bpermute rot:"):
        return _gather(LANES + ints[0])
    if name.startswith("ds_permute"):  # a push: lane l sends x to lane dst(l); here dst is a bijection
        if name.endswith("reverse"):
            a, b = 63, 63  # 63 l + 63 = 63 - l (mod 64)
        else:
            a, b = (int(v) for v in re.match(r"ds_permute (\d+)l\+(\d+)", name).groups())
        got = np.full(64, -1)
        for l in range(64):
            got[(a * l + b) % 64] = l
        assert (got >= 0).all()
        return [got]
    if name.startswith("ds_swizzle quad_perm:"):
        return [_quad_perm(ints[:4])]
    if name.startswith("ds_swizzle"):  # bit-mask mode, within each half of 32: ((lane & and) | or) ^ xor
        if "swap:" in name:
            and_, or_, xor_ = 0x1F, 0, ints[0]
        elif "reverse:" in name:
            and_, or_, xor_ = 0x1F, 0, ints[0] - 1
        elif "broadcast:" in name:
            and_, or_, xor_ = 0, ints[0], 0
        else:
            and_, or_, xor_ = ints[:3]
        return [(LANES & 32) | ((((LANES & 31) & and_) | or_) ^ xor_)]
    if name.startswith("dpp "):
        m = re.match(r"dpp (\w+?)(?::(\[[\d,]+\]|\d+))?(?: |$)", name)
        ctrl, arg = m.group(1), m.group(2)
        arg = [int(v) for v in arg.strip("[]").split(",")] if arg and arg.startswith("[") else int(arg) if arg else None
        row_mask = int(re.search(r"row_mask:(0x[0-9a-f]+)", name).group(1), 16) if "row_mask:" in name else 0xF
        bank_mask = int(re.search(r"bank_mask:(0x[0-9a-f]+)", name).group(1), 16) if "bank_mask:" in name else 0xF
        return _dpp(ctrl, arg, row_mask, bank_mask, "bound_ctrl" in name)
    if name == "v_permlane32_swap":  # lanes 32..63 of the first operand change places with lanes 0..31 of the second
        first = np.where(LANES < 32, LANES, 64 + LANES - 32)
        second = np.where(LANES < 32, LANES + 32, 64 + LANES)
        return [first, second]
    if name == "v_permlane16_swap":  # rows 1 and 3 of the first operand change places with rows 0 and 2 of the second
        odd = (LANES // 16) % 2 == 1
        return [np.where(odd, 64 + LANES - 16, LANES), np.where(odd, 64 + LANES, LANES + 16)]
    if name.startswith("v_readlane "):
        return [np.full(64, ints[0])]
    if name == "v_readfirstlane":  # the first active lane; EXEC is full
        return [np.zeros(64, dtype=int)]
    if name.startswith("v_writelane "):  # x of lane a into lane b of the second value
        a, b = (int(v) for v in re.match(r"v_writelane (\d+)->(\d+)", name).groups())
        out = 64 + LANES
        out[b] = a
        return [out]
    raise ValueError("no model for %r" % name)


def is_bijective(codes) -> bool:
    return len(codes) == 1 and sorted(int(c) for c in codes[0]) == list(range(64))


# ---- the transposed read -------------------------------------------------------------------
def tr_off_a(row, ch):  # 8-row x 32-column subtiles of 512 B
    return 2048 * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3))


def tr_off_b(row, ch):  # plain 256-byte rows
    return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)))


def tr_addresses(r: int):
    """The byte address each lane supplies in round r: lane 4q + p of a group of 16 names row q,
    columns 4p .. 4p + 3 of the group's block."""
    out = []
    for l in range(64):
        g, q, p = l // 16, (l // 4) % 4, l % 4
        if r < 4:
            stride = (32, 64, 256, 264)[r]
            out.append(4096 * r + (4 * g + q) * stride + 8 * p)
        elif r == 4:
            out.append(32768 + tr_off_a(4 * g + q + 8, 2 * g + 4 + p // 2) + 8 * (p % 2))
        elif r == 5:
            out.append(65536 + tr_off_b(4 * g + q + 4, 2 * g + 6 + p // 2) + 8 * (p % 2))
        else:
            out.append(mix32((r << 8) ^ l ^ 0x7A0000) % (128 * 1024 // 8) * 8)
    return out


def tr_sources(addresses):
    """ds_read_b64_tr_b16: lane i of a group receives column i of the group's 4 x 16 block, row
    q in element q; column i lies in the 8 bytes lane 4q + i // 4 named, at element i % 4."""
    out = []
    for l in range(64):
        g, i = l // 16, l % 16
        out.append([addresses[16 * g + 4 * q + i // 4] // 2 + i % 4 for q in range(4)])
    return out


def tr_pattern(seed: int):
    return (np.arange(65536, dtype=np.uint64) * 0x9E37 + seed) & 0xFFFF


# ---- width passes --------------------------------------------------------------------------
def lds_pattern(words: int, s: int):
    return (np.arange(words, dtype=np.uint64) * 0x9E3779B1 & M32).astype(np.uint32) ^ np.uint32(s)


# ---- atomics -------------------------------------------------------------------------------
FORMS = ("u32 add", "u64 add", "i32 min", "u32 max", "and", "or", "xor", "f32 add", "ticket", "cas increment")
INJECT_BIT = 1 << 9
THREADS = 256


def _h(form, thread, step, what):
    return mix32((form << 48) ^ (what << 40) ^ (step << 16) ^ thread)


def atomic_index(form, thread, step):
    return _h(form, thread, step, 0) % (256 if FORMS[form] == "u64 add" else 512)


def atomic_operand(form, thread, step):
    h, h2 = _h(form, thread, step, 1), _h(form, thread, step, 2)
    name = FORMS[form]
    if name in ("u32 add", "xor"):
        return h
    if name == "u64 add":
        return h2 << 32 | h
    if name == "i32 min":
        return (h & 0x7FFFFFFF) - 0x40000000  # a signed value
    if name == "u32 max":
        return h >> 1
    if name == "and":
        return h | h2 | INJECT_BIT
    if name == "or":
        return h & h2 & ~INJECT_BIT & M32
    if name == "f32 add":
        return h % 9 - 4
    if name == "ticket":
        return 1
    return (h & 0xFF) + 1


def atomic_table(form: int, steps: int):
    """The 512 words of a form's region after 256 threads ran ``steps`` steps, as uint32."""
    name = FORMS[form]
    if name == "i32 min":
        table = [0x7FFFFFFF] * 512
    elif name == "and":
        table = [M32] * 512
    elif name in ("u32 max", "or", "f32 add", "ticket"):
        table = [0] * 512
    else:
        table = [mix32(0xA70B ^ (form << 32) ^ w) for w in range(512)]
    if name == "ticket":  # tickets 0 .. 256 * steps - 1 are each taken once; seen[ticket & 255] counts them
        return np.array([steps] * 256 + [THREADS * steps] + [0] * 255, dtype=np.uint32)
    if name == "u64 add":
        table = [table[2 * e] | table[2 * e + 1] << 32 for e in range(256)]
    if name == "i32 min":
        table = [v - (1 << 32) if v >> 31 else v for v in table]
    for s in range(steps):
        for t in range(THREADS):
            e, v = atomic_index(form, t, s), atomic_operand(form, t, s)
            if name in ("u32 add", "cas increment"):
                table[e] = (table[e] + v) & M32
            elif name == "u64 add":
                table[e] = (table[e] + v) & M64
            elif name == "i32 min":
                table[e] = min(table[e], v)
            elif name == "u32 max":
                table[e] = max(table[e], v)
            elif name == "and":
                table[e] &= v
            elif name == "or":
                table[e] |= v
            elif name == "xor":
                table[e] ^= v
            else:  # f32 add: small integers, every partial sum exact
                table[e] += v
    if name == "u64 add":
        return np.array([w for v in table for w in (v & M32, v >> 32)], dtype=np.uint32)
    if name == "f32 add":
        return np.array(table, dtype=np.float32).view(np.uint32)
    return np.array([v & M32 for v in table], dtype=np.uint32)


def f32_partial_sum_bound(steps: int) -> int:
    """No partial sum of the f32 form can exceed this in magnitude: every operand is within [-4, 4]."""
    return THREADS * steps * 4
