"""Seeded inputs of the sample-format tests (TEST INFRASTRUCTURE): one int16 programme rendered in every sample
format a WAV carries, a writer for plain, EXTENSIBLE, RF64 and BW64 headers, float samples with every special value planted, and
the sample rule written out one sample at a time."""
import math
import struct

import numpy as np

FORMATS = ("u8", "s16", "s24", "s32", "f32", "f64")
WIDTH = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4, "f64": 8}
TAG = {"u8": 1, "s16": 1, "s24": 1, "s32": 1, "f32": 3, "f64": 3}
GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


def subformat(tag):
    return struct.pack("<H", tag) + GUID_TAIL


# ---------------------------------------------------------------------------------------------- one programme, six renditions
def programme(n, channels, seed, step=1):
    """int16 [n, channels], seeded, over the whole range, the extremes and zero planted; step=256: multiples of 256 (what an
    8-bit file can hold)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, (n, channels), dtype=np.int64)
    x.reshape(-1)[:5] = (-32768, 32767, 0, -1, 1)[:min(5, x.size)]
    if step > 1:
        x = (x // step) * step
    return x.astype(np.int16)


def rendition(x, fmt, seed=0):
    """The bytes of the int16 frames x as a `fmt` file's data whose samples decode to x again: 's24' / 's32' carry x in their top
    two bytes and seeded noise below; 'f32' / 'f64' hold x / 32768; 'u8' needs multiples of 256."""
    x = np.asarray(x, dtype=np.int64)
    rng = np.random.default_rng(seed)
    if fmt == "s16":
        return x.astype("<i2").tobytes()
    if fmt == "u8":
        assert (x % 256 == 0).all()
        return (x // 256 + 128).astype(np.uint8).tobytes()
    if fmt == "s24":
        v = (x * 256 + rng.integers(0, 256, x.shape)).astype("<i4").reshape(-1)
        return np.ascontiguousarray(v.view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()
    if fmt == "s32":
        return (x * 65536 + rng.integers(0, 65536, x.shape)).astype("<i4").tobytes()
    if fmt == "f32":
        return (x.astype(np.float32) / np.float32(32768.0)).astype("<f4").tobytes()      # exact: a power of two
    if fmt == "f64":
        return (x.astype(np.float64) / 32768.0).astype("<f8").tobytes()
    raise ValueError(fmt)


# ---------------------------------------------------------------------------------------------- headers
def fmt_chunk(tag, channels, rate, bits, extensible=None, mask=0, valid_bits=None, cb=22):
    """The body of a fmt chunk.  extensible: None -> the 16-byte form with `tag`; a 16-byte GUID -> WAVE_FORMAT_EXTENSIBLE with it
    as SubFormat (cb: how much of the extension is written; 22 is all of it)."""
    width = (bits + 7) // 8
    if extensible is None:
        return struct.pack("<HHLLHH", tag, channels, rate, rate * channels * width, channels * width, bits)
    ext = struct.pack("<HL", bits if valid_bits is None else valid_bits, mask) + extensible
    return struct.pack("<HHLLHHH", 0xFFFE, channels, rate, rate * channels * width, channels * width, bits, cb) + ext[:cb]


def write_file(path, fmt_body, data, container=b"RIFF", data_size32=None, ds64=None, junk=(), ds64_size=None):
    """container + WAVE, [ds64], fmt, junk chunks, data.  data_size32: the data chunk's 32-bit size field (default: the truth);
    ds64: None -> no ds64 chunk, else the dataSize it states (riffSize and sampleCount follow from it); ds64_size: the ds64 chunk's
    own size (default 28: the three u64 and an empty table's length); junk: (name, size field, body) chunks between fmt and data."""
    body = b""
    if ds64 is not None:
        full = struct.pack("<QQQL", 0, ds64, 0, 0)
        size = 28 if ds64_size is None else ds64_size
        chunk = full[:size]
        body += b"ds64" + struct.pack("<L", size) + chunk + (b"\0" if len(chunk) & 1 else b"")
    body += b"fmt " + struct.pack("<L", len(fmt_body)) + fmt_body
    for name, size, blob in junk:
        body += name + struct.pack("<L", size) + blob
    body += b"data" + struct.pack("<L", len(data) if data_size32 is None else data_size32) + data
    riff = 0xFFFFFFFF if container != b"RIFF" else 4 + len(body)
    with open(path, "wb") as f:
        f.write(container + struct.pack("<L", riff) + b"WAVE" + body)


def write_wav(path, x, rate, fmt, seed=0, extensible=False, mask=0, **kw):
    """The int16 frames x [n, C] as a `fmt` file (rendition); extensible: an EXTENSIBLE header with the format's own GUID."""
    x = np.asarray(x)
    guid = subformat(TAG[fmt]) if extensible else None
    write_file(path, fmt_chunk(TAG[fmt], x.shape[1], rate, 8 * WIDTH[fmt], guid, mask), rendition(x, fmt, seed), **kw)


# ---------------------------------------------------------------------------------------------- float samples, specials planted
F32_SPECIAL_BITS = (
    0x00000000, 0x80000000,              # +-0.0
    0x00000001, 0x80000001,              # the smallest denormals
    0x007FFFFF, 0x807FFFFF,              # the largest denormals
    0x00800000,                          # the smallest normal
    0x3F800000, 0xBF800000,              # +-1.0
    0x3F7FFFFF,                          # 1 - 2^-24
    0x3FC00000, 0xC2C80000, 0x7149F2CA,  # above full scale: 1.5, -100, 1e30
    0x7F7FC99E, 0xFF7FC99E,              # +-3.4e38: the multiply overflows
    0x7F000000,                          # 2^127: overflows too
    0x7FC00000, 0xFFC00000,              # quiet NaNs of both signs
    0x7FC12345, 0xFF812345, 0x7F800001,  # NaNs with payloads, signalling ones among them
    0x7F800000, 0xFF800000,              # +-inf
    0x38800000, 0x33800000,              # 2^-14, 2^-24
)
F64_SPECIAL_BITS = (
    0x0000000000000000, 0x8000000000000000,     # +-0.0
    0x0000000000000001, 0x8000000000000001,     # the smallest denormals
    0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF,     # the largest denormals
    0x3FF0000000000000, 0xBFF0000000000000,     # +-1.0
    0x3FEFFFFFE0000000,                         # 1 - 2^-24
    0x3FF8000000000000, 0xC059000000000000,     # 1.5, -100
    0x46293E5939A08CEA,                         # 1e30
    0x47EFF933C78CDFAD,                         # 3.4e38: finite as float64 after the multiply, the cast overflows
    0x7E37E43C8800759C, 0xFE37E43C8800759C,     # +-1e300: the cast overflows
    0x7FE0000000000000,                         # 2^1023: the multiply overflows
    0x7FF8000000000000, 0xFFF8000000000000,     # quiet NaNs of both signs
    0x7FF8000012345678, 0xFFF0000000000001,     # NaNs with payloads
    0x7FF0000000000000, 0xFFF0000000000000,     # +-inf
    0x3F00000010000000,                         # (1 + 2^-24) / 32768: between 1 and 1 + 2^-23 -> the even one, 1
    0x3F00000030000000,                         # (1 + 3 * 2^-24) / 32768: between 1 + 2^-23 and 1 + 2^-22 -> the even one, 1 + 2^-22
    0x3F00000010000001,                         # just above the first tie: rounds up
    0x3620000000000000,                         # 2^-157: 2^-142 after the multiply, a float32 denormal
    0x35F0000000000000,                         # 2^-160: 2^-145 after the multiply, a float32 denormal
    0x35A0000000000000,                         # 2^-165: 2^-150 after the multiply -- a tie between 0 and the smallest denormal -> 0
)
# what the rule makes of some of them, stated by hand: float32 bit patterns
F32_EXPECTED = {0x00000000: 0x00000000, 0x80000000: 0x80000000, 0x00000001: 0x00008000, 0x80000001: 0x80008000,
                0x3F800000: 0x47000000, 0xBF800000: 0xC7000000, 0x3F7FFFFF: 0x46FFFFFF, 0x7F7FC99E: 0x00000000,
                0xFF7FC99E: 0x00000000, 0x7FC00000: 0x00000000, 0xFFC00000: 0x00000000, 0xFF812345: 0x00000000,
                0x7F800000: 0x00000000, 0xFF800000: 0x00000000, 0x007FFFFF: 0x07FFFFFE}
F64_EXPECTED = {0x0000000000000000: 0x00000000, 0x8000000000000000: 0x80000000, 0x3FF0000000000000: 0x47000000,
                0x3FEFFFFFE0000000: 0x46FFFFFF, 0x47EFF933C78CDFAD: 0x00000000, 0x7E37E43C8800759C: 0x00000000,
                0xFE37E43C8800759C: 0x00000000, 0x7FE0000000000000: 0x00000000, 0xFFF8000000000000: 0x00000000,
                0x7FF0000000000000: 0x00000000, 0x3F00000010000000: 0x3F800000, 0x3F00000030000000: 0x3F800002,
                0x3F00000010000001: 0x3F800001, 0x3620000000000000: 0x00000080, 0x35F0000000000000: 0x00000010,
                0x35A0000000000000: 0x00000000, 0x0000000000000001: 0x00000000, 0x8000000000000001: 0x80000000}


def float_bytes(n, channels, fmt, seed):
    """The data of n frames of an 'f32' / 'f64' file: seeded samples around full scale with every special of the tables above
    planted, frame 0 all zeros (the signed-zero cases of the sums)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n * channels) * 0.4
    if fmt == "f32":
        out = v.astype("<f4")
        bits, special = out.view(np.uint32), np.array(F32_SPECIAL_BITS, np.uint32)
    else:
        out = v.astype("<f8")
        bits, special = out.view(np.uint64), np.array(F64_SPECIAL_BITS, np.uint64)
    bits[:channels] = 0
    where = rng.permutation(np.arange(channels, n * channels))[:special.shape[0]]
    bits[where] = special[:where.shape[0]]
    return out.tobytes()


def random_bytes(n, channels, fmt, seed):
    """n frames of a `fmt` file: any bytes for the integer formats (frame 0 zeros), float_bytes for the float ones."""
    if fmt in ("f32", "f64"):
        return float_bytes(n, channels, fmt, seed)
    raw = np.random.default_rng(seed).integers(0, 256, n * channels * WIDTH[fmt], dtype=np.uint8)
    raw[:channels * WIDTH[fmt]] = 128 if fmt == "u8" else 0
    return raw.tobytes()


# ---------------------------------------------------------------------------------------------- the rule, one sample at a time
def rule_sample(container, fmt):
    """The value of one sample from its container's bytes, as include/sushi_hip.h states the rule: a np.float32."""
    b = bytes(container)
    assert len(b) == WIDTH[fmt]
    if fmt == "u8":
        return np.float32((b[0] - 128) * 256)
    if fmt in ("s16", "s24", "s32"):
        return np.float32(struct.unpack("<h", b[-2:])[0])
    with np.errstate(all="ignore"):
        if fmt == "f32":
            s = np.float32(struct.unpack("<f", b)[0]) * np.float32(32768.0)
            assert s.dtype == np.float32
        else:
            s = np.float32(np.float64(struct.unpack("<d", b)[0]) * np.float64(32768.0))
    return s if math.isfinite(float(s)) else np.float32(0.0)


def exact_float_sample(bits, fmt):
    """The F32 / F64 rule on a sample's bit pattern in exact rational arithmetic, with no floating-point operation: the float32 bit
    pattern of v * 32768 rounded once to nearest-even (for 'f32' the product of two float32 values rounded once is the same
    thing), +0.0 for a NaN, an infinity or a result beyond float32's range."""
    from fractions import Fraction
    ebits, mbits = (8, 23) if fmt == "f32" else (11, 52)
    negative = bits >> (ebits + mbits)
    e, m = (bits >> mbits) & ((1 << ebits) - 1), bits & ((1 << mbits) - 1)
    if e == (1 << ebits) - 1:
        return 0
    bias = (1 << (ebits - 1)) - 1
    q = (Fraction(m + (1 << mbits if e else 0)) * Fraction(2) ** (max(e, 1) - bias - mbits)) * 32768
    if q == 0:
        return negative << 31
    e2 = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e2 > q:
        e2 -= 1
    e2 = max(e2, -126)
    steps = q / Fraction(2) ** (e2 - 23)                # in units of the last place; 2^23 .. 2^24 for a normal result
    k = steps.numerator // steps.denominator
    rest = steps - k
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and k & 1):
        k += 1
    if k == 1 << 24:
        k, e2 = 1 << 23, e2 + 1
    if e2 > 127:
        return 0
    field = e2 + 127 if k >= 1 << 23 else 0
    return (negative << 31) | (field << 23) | (k & ((1 << 23) - 1))


def rule_samples(data, channels, fmt):
    """rule_sample over the bytes of whole frames: float32 [n, channels]."""
    w = WIDTH[fmt]
    n = len(data) // (channels * w)
    out = np.empty(n * channels, np.float32)
    for k in range(n * channels):
        out[k] = rule_sample(data[k * w:(k + 1) * w], fmt)
    return out.reshape(n, channels)


# ---------------------------------------------------------------------------------------------- the entry points' refusals
def check_entry_point_refusals(L):
    """Every EINVAL (-1) / EALIGN (-2) of sushi_hip_load_decode_format / _decode_mix_format, and n_frames == 0: all answered
    before any HIP call, so the pointers need not be real and no device is touched."""
    import ctypes as C
    p, q = C.c_void_p(4096), C.c_void_p(8192)
    dec, mix = L.sushi_hip_load_decode_format, L.sushi_hip_load_decode_mix_format
    w = np.ones((8, 32), np.float32)
    wp = w.ctypes.data
    for fmt in range(1, 7):
        assert dec(p, 0, 2, fmt, q, None) == 0 and mix(p, 0, 2, fmt, wp, 1, q, 0, None) == 0       # nothing to do: no launch
        assert dec(None, 10, 2, fmt, q, None) == -1 and dec(p, 10, 2, fmt, None, None) == -1
        assert dec(p, -1, 2, fmt, q, None) == -1 and dec(p, 10, 0, fmt, q, None) == -1
        assert dec(p, 10, 2, fmt, C.c_void_p(8194), None) == -2 and dec(p, 10, 2, fmt, C.c_void_p(8193), None) == -2
        assert mix(None, 10, 2, fmt, wp, 1, q, 10, None) == -1 and mix(p, 10, 2, fmt, None, 1, q, 10, None) == -1
        assert mix(p, 10, 2, fmt, wp, 1, None, 10, None) == -1 and mix(p, -1, 2, fmt, wp, 1, q, 10, None) == -1
        assert mix(p, 10, 0, fmt, wp, 1, q, 10, None) == -1 and mix(p, 10, 33, fmt, wp, 1, q, 10, None) == -1
        assert mix(p, 10, 2, fmt, wp, 0, q, 10, None) == -1 and mix(p, 10, 2, fmt, wp, 9, q, 10, None) == -1
        assert mix(p, 10, 2, fmt, wp, 1, q, 9, None) == -1                                          # rows would overlap
        assert mix(p, 10, 2, fmt, wp, 2, C.c_void_p(8194), 10, None) == -2
        for bad in (np.nan, np.inf, -np.inf):
            wb = np.ones((2, 2), np.float32)
            wb[1, 1] = bad
            assert mix(p, 10, 2, fmt, wb.ctypes.data, 2, q, 10, None) == -1
    for fmt in (0, 7, -1, 16, 1 << 20):
        assert dec(p, 10, 2, fmt, q, None) == -1 and mix(p, 10, 2, fmt, wp, 1, q, 10, None) == -1
        assert dec(p, 0, 2, fmt, q, None) == -1 and mix(p, 0, 2, fmt, wp, 1, q, 0, None) == -1      # before the n_frames == 0 answer
    # the order: an unknown format (EINVAL) is reported before a misaligned output (EALIGN)
    assert dec(p, 10, 2, 0, C.c_void_p(8194), None) == -1 and mix(p, 10, 2, 0, wp, 1, C.c_void_p(8194), 10, None) == -1
