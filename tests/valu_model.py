"""An independent model of the vector-ALU check's ops (``ops/valu/valu_ops.h``): ``EXACT[op](a, b,
c, lane)`` gives the result words of an exact op from its operand words, in Python integers,
``struct`` floats and exact ``Fraction`` arithmetic followed by one rounding; ``APPROX[op]`` is a
float64 function for a transcendental.  The low-precision formats share one pair: ``decode`` from
sign, exponent and mantissa, ``encode`` by enumerating every value of the format (nearest, ties
to the even code).  None of the library's bit manipulation is repeated here."""
import bisect
import functools
import math
import struct
from fractions import Fraction

M32 = 0xFFFFFFFF
FMT = {"fp8": (4, 3, 7), "bf8": (5, 2, 15), "fp4": (2, 1, 1), "fp6": (2, 3, 1), "bf6": (3, 2, 3), "f16": (5, 10, 15), "bf16": (8, 7, 127)}  # e, m, bias


def f32(u): return struct.unpack("<f", struct.pack("<I", u & M32))[0]
def b32(x): return struct.unpack("<I", struct.pack("<f", x))[0]   # one rounding to nearest even
def f64(u): return struct.unpack("<d", struct.pack("<Q", u))[0]
def b64(x): return list(struct.unpack("<II", struct.pack("<d", x)))
def s32(u): return (u & M32) - (1 << 32) if u & 0x80000000 else u & M32
def s8(u): return (u & 0xFF) - 256 if u & 0x80 else u & 0xFF
def u64(x): return [x & M32, (x >> 32) & M32]
def byts(u): return [(u >> (8 * j)) & 0xFF for j in range(4)]
def halves(u): return [u & 0xFFFF, (u >> 16) & 0xFFFF]
def sat8(v): return max(-128, min(127, v)) & 0xFF
def s16(u): return (u & 0xFFFF) - 65536 if u & 0x8000 else u & 0xFFFF
def s4(u): return (u & 0xF) - 16 if u & 8 else u & 0xF
def s64(u): return u - (1 << 64) if u >> 63 else u
def nibbles(u): return [(u >> (4 * j)) & 0xF for j in range(8)]


def finite(fmt, mag):
    e, m, _ = FMT[fmt]
    return mag != (1 << (e + m)) - 1 if fmt == "fp8" else fmt in ("fp4", "fp6", "bf6") or (mag >> m) != (1 << e) - 1


def decode(fmt, code):
    """The value of a code (sign, exponent, mantissa) as an exact Fraction."""
    e, m, bias = FMT[fmt]
    ef, mf = (code >> m) & ((1 << e) - 1), code & ((1 << m) - 1)
    v = Fraction(mf, 1 << m) * Fraction(2) ** (1 - bias) if ef == 0 else (1 + Fraction(mf, 1 << m)) * Fraction(2) ** (ef - bias)
    return -v if (code >> (e + m)) & 1 else v


@functools.lru_cache(None)
def _values(fmt):
    e, m, _ = FMT[fmt]
    return [decode(fmt, c) for c in range(1 << (e + m)) if finite(fmt, c)]  # ascending with the code


def encode(fmt, x, toward_zero=False):
    """The code of the format's value nearest to x (ties: the even code), or the nearest toward zero."""
    e, m, _ = FMT[fmt]
    vals, ax = _values(fmt), abs(Fraction(x))
    hi = bisect.bisect_left(vals, ax)
    if hi < len(vals) and vals[hi] == ax:
        mag = hi
    else:
        lo = hi - 1
        assert 0 <= lo and hi < len(vals), "outside the format's range"
        up, down = vals[hi] - ax, ax - vals[lo]
        mag = lo if toward_zero or down < up or (down == up and lo % 2 == 0) else hi
    return mag | ((1 << (e + m)) if math.copysign(1.0, x) < 0 else 0)


def rounded(x, p):
    """The Fraction x rounded once to p significant bits, ties to even."""
    if x == 0:
        return 0.0
    e = math.floor(math.log2(abs(x)))
    e += (Fraction(2) ** (e + 1) <= abs(x)) - (Fraction(2) ** e > abs(x))
    q = Fraction(2) ** (e - p + 1)
    return float(round(x / q) * q)


def fma32(a, b, c): return b32(rounded(Fraction(f32(a)) * Fraction(f32(b)) + Fraction(f32(c)), 24))
def half(u): return decode("f16", u & 0xFFFF)
def bf16(u): return decode("bf16", u & 0xFFFF)
def scaled(fmt, code, s=0x3F800000):  # the sign bit apart: a Fraction has no -0
    top = 1 << sum(FMT[fmt][:2])
    return b32(math.copysign(float(decode(fmt, code & (top - 1)) * Fraction(f32(s))), -1.0 if code & top else 1.0))
def enc(fmt, u, s=0x3F800000): return encode(fmt, math.copysign(1, f32(u)) * 0.0 if f32(u) == 0 else Fraction(f32(u)) / Fraction(f32(s)))


def bitop3(table):
    def run(a, b, c, lane):
        return [sum(((table >> (((a >> i) & 1) << 2 | ((b >> i) & 1) << 1 | ((c >> i) & 1))) & 1) << i for i in range(32))]
    return run


def perm(a, b, c, lane):
    src = byts(b) + byts(a)
    return [sum((src[s] if s < 8 else 0 if s == 12 else 0xFF) << (8 * j) for j, s in enumerate(byts(c)))]


def bfe(signed):
    def run(a, b, c, lane):
        off = b & 31
        width = 1 + c % min(32 - off, 31)
        v = (a >> off) & ((1 << width) - 1)
        return [(v - (1 << width)) & M32 if signed and v >> (width - 1) else v]
    return run


def mbcnt(a, b, c, lane):
    return [bin(a & ((1 << min(lane, 32)) - 1)).count("1") + bin(b & ((1 << max(lane - 32, 0)) - 1)).count("1")]


def fclass(a, b, c, lane):
    x = f32(a)
    bit = (5 if math.copysign(1, x) < 0 else 6) if x == 0 else (3 if x < 0 else 8)
    return [(b >> bit) & 1]


def pk16(fn): return lambda a, b, c, lane: [sum((fn(x, y, z) & 0xFFFF) << (16 * j) for j, (x, y, z) in enumerate(zip(halves(a), halves(b), halves(c))))]
def pkf16(fn): return pk16(lambda x, y, z: encode("f16", fn(half(x), half(y), half(z))))
def dot8(sx): return lambda a, b, c, lane: [(c + sum(sx(x) * sx(y) for x, y in zip(nibbles(a), nibbles(b)))) & M32]


def pack6(codes):
    v = sum(code << (6 * j) for j, code in enumerate(codes))
    return [(v >> (32 * i)) & M32 for i in range(6)]


def dot4(sx): return lambda a, b, c, lane: [(c + sum(sx(x) * sx(y) for x, y in zip(byts(a), byts(b)))) & M32]


EXACT = {
    "mul_lo_u32": lambda a, b, c, lane: [(a * b) & M32],
    "mul_hi_u32": lambda a, b, c, lane: [(a * b) >> 32],
    "mul_hi_i32": lambda a, b, c, lane: [((s32(a) * s32(b)) >> 32) & M32],
    "mad_u64_u32": lambda a, b, c, lane: u64(a * b + c),
    "mad_i64_i32": lambda a, b, c, lane: u64(s32(a) * s32(b) + c),
    "add3_u32": lambda a, b, c, lane: [(a + b + c) & M32],
    "lshl_b64": lambda a, b, c, lane: u64(a << (b & 63)),
    "pk_add_u16": pk16(lambda x, y, z: x + y),
    "pk_mul_lo_u16": pk16(lambda x, y, z: x * y),
    "sdot4": dot4(s8),
    "udot4": dot4(int),
    "sad_u8": lambda a, b, c, lane: [(c + sum(abs(x - y) for x, y in zip(byts(a), byts(b)))) & M32],
    "lerp_u8": lambda a, b, c, lane: [sum(((x + y + (z & 1)) >> 1) << (8 * j) for j, (x, y, z) in enumerate(zip(byts(a), byts(b), byts(c))))],
    "lshl_add_u32": lambda a, b, c, lane: [((a << (b & 3)) + c) & M32],
    "ashr_i64": lambda a, b, c, lane: u64(s64(a) >> (b & 63)),
    "min_i32": lambda a, b, c, lane: [min(s32(a), s32(b)) & M32],
    "max_u32": lambda a, b, c, lane: [max(a, b)],
    "med3_i32": lambda a, b, c, lane: [sorted([s32(a), s32(b), s32(c)])[1] & M32],
    "med3_u32": lambda a, b, c, lane: [sorted([a, b, c])[1]],
    "pk_mad_u16": pk16(lambda x, y, z: x * y + z),
    "pk_min_i16": pk16(lambda x, y, z: min(s16(x), s16(y))),
    "pk_max_u16": pk16(lambda x, y, z: max(x, y)),
    "pk_lshlrev_b16": pk16(lambda x, y, z: x << (y & 15)),
    "sdot8": dot8(s4),
    "udot8": dot8(int),
    "sdot2": lambda a, b, c, lane: [(c + sum(s16(x) * s16(y) for x, y in zip(halves(a), halves(b)))) & M32],
    "msad_u8": lambda a, b, c, lane: [(c + sum(abs(x - y) for x, y in zip(byts(a), byts(b)) if y)) & M32],
    "ffbl": lambda a, b, c, lane: [(((a << (b & 31)) & M32 | 0x80000000) & -(((a << (b & 31)) & M32 | 0x80000000))).bit_length() - 1],
    "perm_b32": perm,
    "alignbit": lambda a, b, c, lane: [((a << 32 | b) >> (c & 31)) & M32],
    "alignbyte": lambda a, b, c, lane: [((a << 32 | b) >> (8 * (c & 3))) & M32],
    "bfe_u32": bfe(False),
    "bfe_i32": bfe(True),
    "bfrev": lambda a, b, c, lane: [int(format(a, "032b")[::-1], 2)],
    "bcnt": lambda a, b, c, lane: [(bin(a).count("1") + b) & M32],
    "ffbh": lambda a, b, c, lane: [32 - ((a >> (b & 31)) | 1).bit_length()],
    "bitop3_96": bitop3(0x96), "bitop3_e8": bitop3(0xE8), "bitop3_ca": bitop3(0xCA), "bitop3_6b": bitop3(0x6B),
    "ashr_pk_i8_i32": lambda a, b, c, lane: [sat8(s32(a) >> (c & 31)) | sat8(s32(b) >> (c & 31)) << 8],
    "mbcnt": mbcnt,
    "add_f32": lambda a, b, c, lane: [b32(f32(a) + f32(b))],   # exact in float64, then one rounding
    "mul_f32": lambda a, b, c, lane: [b32(f32(a) * f32(b))],
    "fma_f32": lambda a, b, c, lane: [fma32(a, b, c)],
    "pk_fma_f32": lambda a, b, c, lane: [fma32(a, b, c), fma32(a >> 32, b >> 32, c >> 32)],
    "div_f32": lambda a, b, c, lane: [b32(rounded(Fraction(f32(a)) / Fraction(f32(b)), 24))],
    "sqrt_f32": lambda a, b, c, lane: [b32(math.sqrt(f32(a)))],  # float64's sqrt has 53 bits: no double rounding at 24
    "med3_f32": lambda a, b, c, lane: [b32(sorted([f32(a), f32(b), f32(c)])[1])],
    "ldexp_f32": lambda a, b, c, lane: [b32(math.ldexp(f32(a), s32(b)))],
    "frexp_mant_f32": lambda a, b, c, lane: [b32(math.frexp(f32(a))[0])],
    "frexp_exp_f32": lambda a, b, c, lane: [math.frexp(f32(a))[1] & M32],
    "fract_f32": lambda a, b, c, lane: [b32(f32(a) - math.floor(f32(a)))],
    "rndne_f32": lambda a, b, c, lane: [b32(float(round(Fraction(f32(a)))))],  # Python rounds a Fraction half to even
    "floor_f32": lambda a, b, c, lane: [b32(float(math.floor(f32(a))))],
    "cvt_i32_f32": lambda a, b, c, lane: [int(f32(a)) & M32],
    "cvt_f32_i32": lambda a, b, c, lane: [b32(rounded(Fraction(s32(a)), 24))],
    "cvt_f32_ubyte": lambda a, b, c, lane: [b32(float(x)) for x in byts(a)],
    "class_f32": fclass,
    "pk_mul_f32": lambda a, b, c, lane: [b32(f32(a) * f32(b)), b32(f32(a >> 32) * f32(b >> 32))],
    "pk_add_f32": lambda a, b, c, lane: [b32(f32(a) + f32(b)), b32(f32(a >> 32) + f32(b >> 32))],
    "min_f32": lambda a, b, c, lane: [b32(min(f32(a), f32(b)))],
    "max_f32": lambda a, b, c, lane: [b32(max(f32(a), f32(b)))],
    "ceil_f32": lambda a, b, c, lane: [b32(float(math.ceil(f32(a))))],
    "trunc_f32": lambda a, b, c, lane: [b32(float(math.trunc(f32(a))))],
    "cvt_u32_f32": lambda a, b, c, lane: [int(f32(a))],
    "cvt_f32_u32": lambda a, b, c, lane: [b32(rounded(Fraction(a & M32), 24))],
    "mul_f64": lambda a, b, c, lane: b64(f64(a) * f64(b)),
    "cvt_f64_f32": lambda a, b, c, lane: b64(f32(a)),
    "cvt_i32_f64": lambda a, b, c, lane: [int(f64(a)) & M32],
    "cvt_f64_i32": lambda a, b, c, lane: b64(float(s32(a))),
    "add_f64": lambda a, b, c, lane: b64(f64(a) + f64(b)),
    "fma_f64": lambda a, b, c, lane: b64(rounded(Fraction(f64(a)) * Fraction(f64(b)) + Fraction(f64(c)), 53)),
    "div_f64": lambda a, b, c, lane: b64(f64(a) / f64(b)),
    "sqrt_f64": lambda a, b, c, lane: b64(math.sqrt(f64(a))),
    "cvt_f32_f64": lambda a, b, c, lane: [b32(f64(a))],
    "pk_fma_f16": pkf16(lambda x, y, z: x * y + z),
    "pk_add_f16": pkf16(lambda x, y, z: x + y),
    "pk_mul_f16": pkf16(lambda x, y, z: x * y),
    "cvt_f16_f32": lambda a, b, c, lane: [encode("f16", f32(a))],
    "fdot2": lambda a, b, c, lane: [b32(float(half(a) * half(b) + half(a >> 16) * half(b >> 16) + Fraction(f32(c))))],
    "fdot2_f32_bf16": lambda a, b, c, lane: [b32(float(bf16(a) * bf16(b) + bf16(a >> 16) * bf16(b >> 16) + Fraction(f32(c))))],
    "cvt_pkrtz": lambda a, b, c, lane: [encode("f16", f32(a), True) | encode("f16", f32(b), True) << 16],
    "cvt_f32_f16": lambda a, b, c, lane: [b32(float(half(a)))],
    "cvt_pk_bf16_f32": lambda a, b, c, lane: [encode("bf16", f32(a)) | encode("bf16", f32(b)) << 16],
    "cvt_f32_fp8": lambda a, b, c, lane: [scaled("fp8", x) for x in byts(a)],
    "cvt_f32_bf8": lambda a, b, c, lane: [scaled("bf8", x) for x in byts(a)],
    "cvt_pk_f32_fp8": lambda a, b, c, lane: [scaled("fp8", x) for x in byts(a)],
    "cvt_scalef32_pk_f32_fp8": lambda a, b, c, lane: [scaled("fp8", x, c) for x in byts(a)],
    "cvt_scalef32_pk_f32_bf8": lambda a, b, c, lane: [scaled("bf8", x, c) for x in byts(a)],
    "cvt_scalef32_pk_f32_fp4": lambda a, b, c, lane: [scaled("fp4", (a >> (4 * j)) & 0xF, c) for j in range(8)],
    "cvt_pk_f32_bf8": lambda a, b, c, lane: [scaled("bf8", x) for x in byts(a)],
    "cvt_pk_fp8_f32": lambda a, b, c, lane: [enc("fp8", a) | enc("fp8", b) << 8],
    "cvt_pk_bf8_f32": lambda a, b, c, lane: [enc("bf8", a) | enc("bf8", b) << 8],
    "cvt_scalef32_pk_fp8_f32": lambda a, b, c, lane: [enc("fp8", a, c) | enc("fp8", b, c) << 8],
    "cvt_scalef32_pk_bf8_f32": lambda a, b, c, lane: [enc("bf8", a, c) | enc("bf8", b, c) << 8],
    "cvt_scalef32_pk_fp4_f32": lambda a, b, c, lane: [enc("fp4", a, c) | enc("fp4", b, c) << 4],
}

# The wide conversions: (elems, c) -> result words, from the 32 elements valu.expand gives
WIDE = {
    "cvt_scalef32_pk32_f32_fp6": lambda elems, c: [scaled("fp6", x, c) for x in elems],
    "cvt_scalef32_pk32_f32_bf6": lambda elems, c: [scaled("bf6", x, c) for x in elems],
    # the two 16-element sources interleave in the result (read from the hardware with valu.raw)
    "cvt_scalef32_2xpk16_fp6_f32": lambda elems, c: pack6([enc("fp6", elems[(j >> 1) + 16 * (j & 1)], c) for j in range(32)]),
    "cvt_scalef32_2xpk16_bf6_f32": lambda elems, c: pack6([enc("bf6", elems[(j >> 1) + 16 * (j & 1)], c) for j in range(32)]),
}

# op -> (float64 reference of the operand, the result is f64)
APPROX = {
    "exp2_f32": (lambda x: 2.0 ** x, False), "log2_f32": (math.log2, False), "rcp_f32": (lambda x: 1.0 / x, False),
    "rsq_f32": (lambda x: 1.0 / math.sqrt(x), False), "sqrt_raw_f32": (math.sqrt, False),
    "sin_f32": (lambda x: math.sin(2 * math.pi * x), False), "cos_f32": (lambda x: math.cos(2 * math.pi * x), False),
    "rcp_f64": (lambda x: 1.0 / x, True), "rsq_f64": (lambda x: 1.0 / math.sqrt(x), True),
    "exp2_f16": (lambda x: 2.0 ** x, "f16"), "log2_f16": (math.log2, "f16"), "rcp_f16": (lambda x: 1.0 / x, "f16"),
}


def approx_error_ulp(op, a_word, result_words):
    """The error of an approx op's result against float64, in ulps of the result type."""
    fn, kind = APPROX[op]
    if kind == "f16":
        ref = fn(float(half(int(a_word))))
        return abs(float(half(int(result_words[0]))) - ref) / 2.0 ** (math.frexp(ref)[1] - 11)
    if kind:
        ref = fn(f64(a_word))
        return abs(f64(int(result_words[0]) | int(result_words[1]) << 32) - ref) / math.ulp(ref)
    ref = fn(f32(a_word))
    return abs(f32(int(result_words[0])) - ref) / 2.0 ** (math.frexp(ref)[1] - 24)

def operand_floats_ok(kind, word):
    """Every floating value an operand word of that kind (a name of valu_ops.h) holds is a normal number or a zero."""
    if kind.startswith("f32") or kind == "scale" or kind.startswith("enc_f") or kind.startswith("enc_b"):
        return all(normal_or_zero(f32(w), 2.0 ** -126) for w in ([word & M32, word >> 32] if kind == "f32x2" else [word & M32]))
    if kind.startswith("f64"):
        return normal_or_zero(f64(word), 2.0 ** -1022)
    if kind.startswith("f16") or kind.startswith("bf16"):
        fmt, least = ("f16", 2.0 ** -14) if kind.startswith("f16") else ("bf16", 2.0 ** -126)
        return all(finite(fmt, h & 0x7FFF) and normal_or_zero(float(decode(fmt, h)), least) for h in halves(word)[:2 if "x2" in kind else 1])
    return True


def normal_or_zero(x, min_normal):
    return x == 0 or (min_normal <= abs(x) < math.inf)


def result_floats_ok(rkind, words):
    if rkind == 1:
        return all(normal_or_zero(f32(w), 2.0 ** -126) for w in words)
    if rkind == 2:
        return all(normal_or_zero(f64(words[i] | words[i + 1] << 32), 2.0 ** -1022) for i in range(0, len(words), 2))
    if rkind == 3:
        return all(finite("f16", h & 0x7FFF) and normal_or_zero(float(half(h)), 2.0 ** -14) for w in words for h in halves(w))
    return True


def results(op, a, b, c, expand=None):
    """The model's result words (rounds, 64, n) for operand arrays (rounds, 64); a wide conversion
    takes its 32 elements from ``expand(op, a, c)``."""
    if op in WIDE:
        return [[WIDE[op]([int(x) for x in expand(op, int(a[r][l]), int(c[r][l]))], int(c[r][l])) for l in range(64)] for r in range(len(a))]
    fn = EXACT[op]
    return [[fn(int(a[r][l]), int(b[r][l]), int(c[r][l]), l) for l in range(64)] for r in range(len(a))]
