"""An independent numpy model of the matrix-forms check (``ops/matforms``): its own decoders of
every number format, its own statement of every operand map, and the product a wave must get
from the raw operand words it feeds its MFMAs.  Nothing here reads the library's table; the
tests compare the two."""
import numpy as np


# ---- decoders: code -> value ---------------------------------------------------------------
def minifloat(code, ebits, mbits, bias):
    """OCP-style small float without infinities in the range used: sign, ebits, mbits."""
    code = np.asarray(code, dtype=np.int64)
    sign = np.where(code >> (ebits + mbits) & 1, -1.0, 1.0)
    e = code >> mbits & ((1 << ebits) - 1)
    man = (code & ((1 << mbits) - 1)).astype(np.float64) / (1 << mbits)
    return sign * np.where(e == 0, man * 2.0 ** (1 - bias), (1.0 + man) * 2.0 ** (e.astype(np.float64) - bias))


DECODE = {
    "f16": lambda c: np.asarray(c, dtype=np.uint16).view(np.float16).astype(np.float64),
    "bf16": lambda c: (np.asarray(c, dtype=np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64),
    "i8": lambda c: np.asarray(c, dtype=np.uint8).view(np.int8).astype(np.float64),
    "f32": lambda c: np.asarray(c, dtype=np.uint32).view(np.float32).astype(np.float64),
    "f64": lambda c: np.asarray(c, dtype=np.uint64).view(np.float64),
    "e4m3": lambda c: minifloat(c, 4, 3, 7),
    "e5m2": lambda c: minifloat(c, 5, 2, 15),
    "e2m3": lambda c: minifloat(c, 2, 3, 1),
    "e3m2": lambda c: minifloat(c, 3, 2, 3),
    "e2m1": lambda c: minifloat(c, 2, 1, 1),
}
BITS = {"f16": 16, "bf16": 16, "i8": 8, "f32": 32, "f64": 64, "e4m3": 8, "e5m2": 8, "e2m3": 6, "e3m2": 6, "e2m1": 4}


def e8m0(byte):
    return 2.0 ** (np.asarray(byte, dtype=np.float64) - 127.0)


# ---- maps ------------------------------------------------------------------------------------
def linear(g, j, elems, K):
    return elems * g + j


def halves(g, j, elems, K):
    return (K // 2) * (j >> 4) + 16 * g + (j & 15)


def cd32(reg, g):
    return (reg & 3) + 8 * (reg >> 2) + 4 * g


def cd16(reg, g):
    return 4 * g + reg


def cd_f64(reg, g):
    return g + 4 * reg


def _form(instruction, m, elems, enc_a, enc_b, r, acc, map_a=linear, map_b=linear, cd=None, scaled=False):
    return {"instruction": instruction, "m": m, "elems": elems, "k": elems * 64 // m, "enc": (enc_a, enc_b), "r": r,
            "acc": acc, "map": (map_a, map_b), "cd": cd or (cd32 if m == 32 else cd16), "scaled": scaled}


FORMS = {
    "f16_32": _form("v_mfma_f32_32x32x16_f16", 32, 8, "f16", "f16", 128, "f32"),
    "f16_16": _form("v_mfma_f32_16x16x32_f16", 16, 8, "f16", "f16", 128, "f32"),
    "bf16_16": _form("v_mfma_f32_16x16x32_bf16", 16, 8, "bf16", "bf16", 128, "f32"),
    "i8_32": _form("v_mfma_i32_32x32x32_i8", 32, 16, "i8", "i8", 127, "i32"),
    "i8_16": _form("v_mfma_i32_16x16x64_i8", 16, 16, "i8", "i8", 127, "i32"),
    "f32_32": _form("v_mfma_f32_32x32x2_f32", 32, 1, "f32", "f32", 512, "f32"),
    "f32_16": _form("v_mfma_f32_16x16x4_f32", 16, 1, "f32", "f32", 512, "f32"),
    "f64_16": _form("v_mfma_f64_16x16x4_f64", 16, 1, "f64", "f64", 1 << 20, "f64", cd=cd_f64),
    "fp8_16": _form("v_mfma_f32_16x16x32_fp8_fp8", 16, 8, "e4m3", "e4m3", 4, "f32"),
    "bf8fp8_32": _form("v_mfma_f32_32x32x16_bf8_fp8", 32, 8, "e5m2", "e4m3", 4, "f32"),
    "mxfp6_32": _form("v_mfma_scale_f32_32x32x64_f8f6f4", 32, 32, "e2m3", "e2m3", 4, "f32", scaled=True),
    "mxbf6_32": _form("v_mfma_scale_f32_32x32x64_f8f6f4", 32, 32, "e3m2", "e3m2", 4, "f32", scaled=True),
    "mxfp8fp4_32": _form("v_mfma_scale_f32_32x32x64_f8f6f4", 32, 32, "e4m3", "e2m1", 4, "f32", map_a=halves, scaled=True),
    "mxfp8_16": _form("v_mfma_scale_f32_16x16x128_f8f6f4", 16, 32, "e4m3", "e4m3", 4, "f32", map_a=halves, map_b=halves,
                      scaled=True),
    "mxfp4_16": _form("v_mfma_scale_f32_16x16x128_f8f6f4", 16, 32, "e2m1", "e2m1", 4, "f32", scaled=True),
}
ACC_BITS = {"f32": 24, "i32": 31, "f64": 53}
MAX_KSTEPS = 8


def largest_sum(form):
    """The largest |partial sum| a check of the form can meet: K of one MFMA x 8 steps x R^2,
    times 4 where two E8M0 scales of 2^0 or 2^1 multiply a product (the scaled forms only)."""
    f = FORMS[form]
    return f["k"] * MAX_KSTEPS * f["r"] ** 2 * (4 if f["scaled"] else 1)


def unpack(words, bits, elems):
    """Element j (bits wide, at bit j * bits) of every lane's operand words (..., 8) -> codes (..., elems)."""
    words = np.asarray(words, dtype=np.uint64)
    codes = np.zeros(words.shape[:-1] + (elems,), dtype=np.uint64)
    mask = np.uint64((1 << bits) - 1)
    for j in range(elems):
        i, sh = (j * bits) >> 5, (j * bits) & 31
        v = words[..., i] >> np.uint64(sh)
        if sh + bits > 32:
            v = v | (words[..., i + 1] << np.uint64(32 - sh))
        codes[..., j] = v & mask
    return codes


def matrices(form, a_words, b_words, scale_a, scale_b):
    """A[m][K], B[K][m] (decoded values) and the E8M0 factors SA[m][K], SB[K][m] of one MFMA from
    the 64 lanes' raw words (64, 8) and scale bytes (64)."""
    f = FORMS[form]
    m, elems, K = f["m"], f["elems"], f["k"]
    va = DECODE[f["enc"][0]](unpack(a_words, BITS[f["enc"][0]], elems))
    vb = DECODE[f["enc"][1]](unpack(b_words, BITS[f["enc"][1]], elems))
    A, B = np.zeros((m, K)), np.zeros((K, m))
    SA, SB = np.ones((m, K)), np.ones((K, m))
    for lane in range(64):
        r, g = lane % m, lane // m
        for j in range(elems):
            A[r, f["map"][0](g, j, elems, K)] = va[lane, j]
            B[f["map"][1](g, j, elems, K), r] = vb[lane, j]
        if f["scaled"]:  # the lane's byte: k-block g (32 k) of its row of A and its column of B
            SA[r, 32 * g:32 * g + 32] = e8m0(scale_a[lane])
            SB[32 * g:32 * g + 32, r] = e8m0(scale_b[lane])
    return A, B, SA, SB


def product(form, a_words, b_words, scale_a, scale_b):
    """C[m][m] (float64, exact for the integer data of the check) summed over the steps:
    ``a_words`` / ``b_words`` (steps, 64, 8), ``scale_a`` / ``scale_b`` (steps, 64)."""
    m = FORMS[form]["m"]
    C = np.zeros((m, m))
    for s in range(len(a_words)):
        A, B, SA, SB = matrices(form, a_words[s], b_words[s], scale_a[s], scale_b[s])
        C += (A * SA) @ (B * SB)
    return C


def integer_codes(enc, r):
    """Every code of the format that decodes to an integer in [-r, r] (both zeros included),
    for the formats of at most 16 bits."""
    codes = np.arange(1 << BITS[enc], dtype=np.uint64)
    with np.errstate(invalid="ignore"):  # the NaN codes of f16 and bf16 are among them, and are dropped
        v = DECODE[enc](codes)
        keep = np.isfinite(v) & (v == np.round(v)) & (np.abs(v) <= r)
    return codes[keep]


def random_codes(rng, enc, r, shape):
    """Random raw codes of integers in [-r, r]."""
    if enc == "f32":
        return rng.integers(-r, r + 1, shape).astype(np.float32).view(np.uint32).astype(np.uint64)
    if enc == "f64":
        return rng.integers(-r, r + 1, shape).astype(np.float64).view(np.uint64)
    return rng.choice(integer_codes(enc, r), size=shape)


def pack(codes, bits):
    """The inverse of ``unpack``."""
    codes = np.asarray(codes, dtype=np.uint64)
    words = np.zeros(codes.shape[:-1] + (8,), dtype=np.uint64)
    for j in range(codes.shape[-1]):
        i, sh = (j * bits) >> 5, (j * bits) & 31
        words[..., i] |= (codes[..., j] << np.uint64(sh)) & np.uint64(0xFFFFFFFF)
        if sh + bits > 32:
            words[..., i + 1] |= codes[..., j] >> np.uint64(32 - sh)
    return words.astype(np.uint32)


def read_accumulators(form, out):
    """Raw accumulators (64, 16) of one wave as C[m][m] by the model's C/D map."""
    f = FORMS[form]
    m, n = f["m"], 16 if f["m"] == 32 else 4
    out = np.ascontiguousarray(out, dtype=np.uint32)
    vals = {"f32": lambda: out[:, :n].copy().view(np.float32), "i32": lambda: out[:, :n].copy().view(np.int32),
            "f64": lambda: out[:, :2 * n].copy().view(np.float64)}[f["acc"]]().astype(np.float64)
    C = np.full((m, m), np.nan)
    for lane in range(64):
        for reg in range(n):
            C[f["cd"](reg, lane // m), lane % m] = vals[lane, reg]
    return C
