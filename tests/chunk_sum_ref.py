"""The exact chunk sum of csrc/srt_path.h (toFixed36 / commitFixed / fromFixed36, srt_sum_chunks_kernel and
srt_finalize_kernel), stated in Python integers.  No float arithmetic decides anything here.

Per slot value v (a float32) and the launch's limit (limit(chunks), csrc/srt_render.cpp chunkFixLimit):
  * v is not representable when it is not finite or |v| >= limit; it then raises a flag of its channel: NaN for a NaN,
    +inf for v > 0, -inf otherwise;
  * otherwise q = sign(v) * floor(|v| * 2^36), from fractions.Fraction(float(v)): exact for |v| >= 2^-13 (a float32 ulp of
    2^-36 or more), truncated towards zero below.
Per channel: NaN if any slot was NaN or both infinities were flagged, else the flagged infinity, else the integer sum of the
q, times 2^-36, rounded ONCE to float32 -- nearest, ties to even -- by bit length, shift and the remainder against the
half (round_once).  A sum of zero is +0.0: the kernels return +0.0 also where every partial sum was -0.0 (a float sum would
give -0.0), and so does this reference.
w: on the chunk-slot path (0) the float32 sum of the slots' counts in slot order, on the atomic path (1) float32(samples)."""
from fractions import Fraction
import math

import numpy as np

F = np.float32
UNITS = 1 << 36
NAN, PINF, NINF = "nan", "+inf", "-inf"


def limit(chunks):
    """A partial sum of this much or more counts as infinite: 2^26 / (chunks rounded up to a power of two)."""
    pow2 = 1
    while pow2 < chunks:
        pow2 *= 2
    return float(2 ** 26) / pow2


def to_fixed(v, lim):
    """One slot value: its integer in units of 2^-36, or the flag it raises."""
    v = float(v)
    if v != v:
        return NAN
    if math.isinf(v) or abs(v) >= lim:
        return PINF if v > 0 else NINF
    m = int(abs(Fraction(v)) * UNITS)  # floor of a non-negative fraction
    return -m if v < 0 else m


def round_once(q):
    """The integer q, in units of 2^-36, as the nearest float32 (ties to even); +0.0 for 0."""
    a = abs(q)
    if a == 0:
        return F(0.0)
    shift = a.bit_length() - 24
    if shift <= 0:
        m, shift = a, 0  # at most 24 bits: exact
    else:
        m, rem, half = a >> shift, a & ((1 << shift) - 1), 1 << (shift - 1)
        if rem > half or (rem == half and (m & 1)):
            m += 1
    # m <= 2^24 and the exponent is far from float32's ends: ldexp and the narrowing are both exact
    x = math.ldexp(m, shift - 36)
    return F(-x if q < 0 else x)


def channel_sum(values, lim):
    """One channel of one pixel: the float32 the kernels must return for these slot values, in any order."""
    total, flags = 0, set()
    for v in values:
        q = to_fixed(v, lim)
        if isinstance(q, str):
            flags.add(q)
        else:
            total += q
    if NAN in flags or (PINF in flags and NINF in flags):
        return F(np.nan)
    if PINF in flags:
        return F(np.inf)
    if NINF in flags:
        return F(-np.inf)
    return round_once(total)


def rows_sum(rows, chunks):
    """rows: (R, chunks) float32, one channel's slot values per row -> (R,) float32."""
    rows = np.asarray(rows, F)
    assert rows.ndim == 2 and rows.shape[1] == chunks
    lim = limit(chunks)
    return np.array([channel_sum(r, lim) for r in rows], F)


def chunk_sum(slots, path, samples=0):
    """slots: (chunks, n, 4) float32 as srtTestChunkSum takes them -> (n, 4) float32."""
    slots = np.asarray(slots, F)
    chunks, n, _ = slots.shape
    out = np.zeros((n, 4), F)
    for k in range(3):
        out[:, k] = rows_sum(slots[:, :, k].T, chunks)
    if path == 0:
        w = np.zeros(n, F)
        for c in range(chunks):
            w = (w + slots[c, :, 3]).astype(F)
        out[:, 3] = w
    else:
        out[:, 3] = F(samples)
    return out


def same_bits(a, b):
    """Bit equality of float32 arrays, any NaN equal to any NaN (the kernels return one quiet NaN; its payload is not
    part of the contract)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---------------------------------------------------------------- directed sets (three slots: a render of 3 chunks, limit 2^24)

def _orders(triple):
    a, b, c = triple
    return [(a, b, c), (a, c, b), (b, a, c), (b, c, a), (c, a, b), (c, b, a)]


def double_rounding_rows():
    """(rows (R, 3) float32, want (R,) float32): sums of 2^17 and more that a conversion through double rounds twice.
    For e in 17..24, with h = 2^(e-1) and u = ulp(h) = 2^(e-24) (half a float32 ulp at 2^e):
      up:    h + u, h, 2^-36         = 2^e + u + 2^-36      just above the tie: one ulp above 2^e
      down:  h + u, h + 2u, -2^-36   = 2^e + 3u - 2^-36     an odd mantissa plus half an ulp minus one unit: 2^e + 2u
    both signs, all six slot orders.  `want` is stated here from the construction, not computed by round_once."""
    rows, want = [], []
    for e in range(17, 25):
        h, u = 2.0 ** (e - 1), 2.0 ** (e - 24)
        for sign in (1.0, -1.0):
            for triple, w in (((h + u, h, 2.0 ** -36), 2.0 ** e + 2 * u), ((h + u, h + 2 * u, -(2.0 ** -36)), 2.0 ** e + 2 * u)):
                for o in _orders(triple):
                    rows.append([sign * x for x in o])
                    want.append(sign * w)
    return np.array(rows, F), np.array(want, F)


def tie_rows():
    """(rows, want): sums of the same magnitudes that ARE ties (the third slot, +-2^-37, converts to 0): to even.
      h + u, h, 2^-37        = 2^e + u    -> 2^e          (even mantissa below)
      h + u, h + 2u, -2^-37  = 2^e + 3u   -> 2^e + 4u     (odd mantissa below, even above)"""
    rows, want = [], []
    for e in range(17, 25):
        h, u = 2.0 ** (e - 1), 2.0 ** (e - 24)
        for sign in (1.0, -1.0):
            for triple, w in (((h + u, h, 2.0 ** -37), 2.0 ** e), ((h + u, h + 2 * u, -(2.0 ** -37)), 2.0 ** e + 4 * u)):
                for o in _orders(triple):
                    rows.append([sign * x for x in o])
                    want.append(sign * w)
    return np.array(rows, F), np.array(want, F)


def naive_sum(rows, chunks):
    """What fromFixed36 computed before it rounded once: the integer sum through double.  Finite rows only."""
    lim = limit(chunks)
    out = []
    for r in np.asarray(rows, F):
        q = sum(to_fixed(v, lim) for v in r)
        out.append(np.float32(np.float64(q) * 2.0 ** -36))
    return np.array(out, F)
