"""The 8-bit quantisation of a pixel sum (color.h:25-41 writeColorTarget; csrc/srt_device.h srtQuantise8 and its three
callers), as an exact statement, and the caller-made sums that sit where a level changes.

    s = fl32(1 / spp);  m = fl32(c * s);  g = the correctly rounded float32 square root of m;
    level = floor(256 * g), capped as the clamp to 0.999f caps it (255);  a NaN or negative m gives 0 (-0.0 too: its root
    is -0.0);  +inf gives 255;  alpha is 255.

The product of two float32 is exact in double, so its narrowing is the one rounding of m.  The root is taken with
math.isqrt on the float's integer mantissa scaled by an even power of two, and rounded to 24 bits by the remainder: no
float square root is trusted anywhere."""
from fractions import Fraction
import functools
import math

import numpy as np

F = np.float32
SPPS = (1, 3, 5, 7, 64, 1000, 5000, 8192)


def scale_of(spp):
    return F(1.0) / F(spp)


def mean_of(c, spp):
    """fl32(c * fl32(1 / spp)) for an array of float32 sums."""
    with np.errstate(all="ignore"):
        return (np.asarray(c, F).astype(np.float64) * np.float64(scale_of(spp))).astype(F)


def sqrt_rn(m):
    """The float32 nearest sqrt(m) for a finite float32 m > 0, as a Python float (exact)."""
    mant, exp = math.frexp(float(m))          # m = mant * 2^exp, mant in [0.5, 1)
    M, E = int(mant * (1 << 53)), exp - 53    # m = M * 2^E exactly
    k = 64 + ((E - 64) & 1)                   # scale by 2^k with E - k even; N has far more than 2 * 25 bits
    N = M << k
    r = math.isqrt(N)                         # floor(sqrt(N)), about 58 bits
    shift = r.bit_length() - 24
    top, rem, half = r >> shift, r & ((1 << shift) - 1), 1 << (shift - 1)
    exact = r * r == N
    if rem > half or (rem == half and (not exact or (top & 1))):
        top += 1
    return math.ldexp(top, shift + (E - k) // 2)


def level_of_mean(m):
    m = float(m)
    if m != m or m < 0.0 or m == 0.0:
        return 0
    if math.isinf(m):
        return 255
    g = sqrt_rn(m)
    return min(255, int(256.0 * g))  # g > 0.999f clamps to 0.999f: 255.744 -> 255, as every g >= 255/256 gives


def levels(c, spp):
    """uint8 levels of the float32 sums c (any shape) at `spp` samples."""
    m = mean_of(c, spp)
    uniq, inv = np.unique(m.view(np.uint32).ravel(), return_inverse=True)
    lv = np.array([level_of_mean(x) for x in uniq.view(F)], np.uint8)
    return lv[inv].reshape(m.shape)


def rgba(accum, spp):
    """(H, W, 4) sums -> (H, W, 4) uint8 as srtResolveTiles writes it."""
    out = np.empty(accum.shape[:2] + (4,), np.uint8)
    out[..., :3] = levels(accum[..., :3], spp)
    out[..., 3] = 255
    return out


def boundary(L):
    """The smallest mean whose exact root reaches level L: (L / 256)^2, exact in float32."""
    return F(L * L) / F(65536.0)


def one_below_holds(L):
    """Whether the float one ulp below boundary(L) still resolves to L.  With x = L / 256 = mx * 2^e, mx in [1, 2): the root
    of x^2 - ulp(x^2) is x less 1 / (2 mx) ulps of x where x^2 stays in the binade of 2^(2e) (mx < sqrt 2): under half an
    ulp, so the correctly rounded root is x itself and the level is L.  For mx > sqrt 2 it is x less 1 / mx ulps, and for
    mx = 1 the ulp below x is half as large: both round to a float below x, level L - 1.  The first kind is what catches a
    square root that is not correctly rounded."""
    mx = Fraction(L, 1 << (L.bit_length() - 1))
    return 1 < mx and mx * mx < 2


def step(x, n):
    """x moved by n float32 ulps."""
    x = F(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, F(np.inf) if n > 0 else F(-np.inf))
    return x


def sums_for_mean(target, spp):
    """Sums c around target / s: the five floats c0 - 2 .. c0 + 2 ulps.  Where some c has fl32(c * s) == target, it is
    among them (a float product moves by at most two ulps of the result per ulp of c)."""
    c0 = F(np.float64(target) / np.float64(scale_of(spp)))
    return [step(c0, d) for d in (-2, -1, 0, 1, 2)]


def boundary_sums(spp):
    """(sums, hits): for every level 1..255 its boundary mean at -2..+2 ulps, each through sums_for_mean; hits[(L, d)] =
    one sum whose mean IS boundary(L) moved by d ulps, where there is one."""
    out, hits = [], {}
    for L in range(1, 256):
        for d in (-2, -1, 0, 1, 2):
            t = step(boundary(L), d)
            cs = sums_for_mean(t, spp)
            out.extend(cs)
            for c in cs:
                if mean_of(c, spp) == t:
                    hits[(L, d)] = c
    return np.array(out, F), hits


def divide_differs(spp, reach=12):
    """Sums near the level boundaries where fl32(c / spp) and fl32(c * fl32(1 / spp)) fall on different levels."""
    cands = []
    for L in range(1, 256):
        c0 = F(np.float64(boundary(L)) * np.float64(spp))
        cands.extend(step(c0, d) for d in range(-reach, reach + 1))
    c = np.unique(np.array(cands, F))
    by_div = (c / F(spp)).astype(F)
    a = np.array([level_of_mean(x) for x in by_div], np.uint8)
    b = levels(c, spp)
    return c[a != b]


def special_sums(spp):
    """The clamp, the ends of the range and everything that is not a positive finite mean."""
    s = np.float64(scale_of(spp))
    top = F(0.999) * F(0.999)
    vals = []
    for t in [step(top, d) for d in range(-3, 4)] + [step(F(1.0), d) for d in (-2, -1, 0, 1, 2)] + [F(255.0 / 256.0) ** 2, F(4.0), F(1e10)]:
        vals.extend(sums_for_mean(t, spp))
    fmax = np.finfo(F).max
    tiny = np.finfo(F).tiny
    sub = np.nextafter(F(0), F(1))
    nan_pos = np.array([0x7fc00000], np.uint32).view(F)[0]
    nan_neg = np.array([0xffc00000], np.uint32).view(F)[0]
    # (the two NaNs apart: image_for puts three neighbours of this list into one pixel, and a NaN is to sit beside two good values)
    vals += [nan_pos, fmax, F(np.inf), F(-np.inf), F(0.0), F(-0.0), sub, -sub, step(tiny, -1), -step(tiny, -1), tiny, -tiny, F(1e-30),
             F(-1e-30), F(-1e-10), F(-1.0), -fmax, F(2.0 ** -16 / s), nan_neg, F(spp), F(0.5 * spp)]
    return np.array(vals, F)


def image_for(spp, width, height):
    """(accum (H, W, 4) float32, info): every sum of the sets above in each of the three channels -- pixel i holds value
    i, i - 1 and i - 2 of the list in r, g, b -- so a NaN channel sits beside two good ones; w = spp."""
    b, hits = boundary_sums(spp)
    dd = divide_differs(spp) if spp & (spp - 1) else np.zeros(0, F)
    sp = special_sums(spp)
    vals = np.concatenate([sp, dd, b])
    n = width * height
    assert len(vals) + 2 <= n, (len(vals), n)
    fill = np.random.default_rng(spp).uniform(0.0, 1.2 * spp, n - len(vals)).astype(F)
    vals = np.concatenate([vals, fill])
    acc = np.empty((n, 4), F)
    for k in range(3):
        acc[:, k] = np.roll(vals, k)
    acc[:, 3] = spp
    return acc.reshape(height, width, 4), {"hits": hits, "divide_differs": len(dd), "specials": len(sp)}


W, H = 127, 81  # no whole number of 8 x 8 tiles either way; 10 287 pixels


@functools.lru_cache(maxsize=None)
def case(spp):
    """(accum, the exact bytes, info) of image_for(spp, W, H): computed once, shared by the CPU and the GPU tests, read-only."""
    acc, info = image_for(spp, W, H)
    want = rgba(acc, spp)
    acc.setflags(write=False)
    want.setflags(write=False)
    return acc, want, info
