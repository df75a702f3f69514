"""Independent references for the two places where the shading step (csrc/srt_path.h shade()) is cleverer than the
reference it restates, plus the adversarial inputs the tests of both sides share:

  * the checker's choice (texture.h:42-48): the sign of sin(ax) * sin(ay) * sin(az) evaluated by mpmath (`checker_truth`),
    and a float32 replay of the kernel's float-float range reduction piPeriods (`pi_periods`, `checker_replay`);
  * imagePNG::value's index arithmetic (texture.h:129-148) in float32 (`texel_lookup`), with the 1- and 2-byte images'
    read of pixel[1], pixel[2] defined as 0 at and past the image's own width * height * bpp bytes.

Nothing here calls the oracle or the device library."""
import numpy as np

f32 = np.float32
INV_PI_HI = f32(float.fromhex("0x1.45f306p-2"))   # piPeriods: ih + il = 1 / pi to 2^-51
INV_PI_LO = f32(float.fromhex("0x1.b9391p-27"))
PERIODS_MARGIN = f32(1e-6)
PERIODS_LIMIT = f32(4194304.0)


def _fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays: the product of two float32 is exact in float64; the float64 sum is turned into
    its round-to-odd value with the error term of a two-sum, so that the one rounding to float32 is the fused one."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


def pi_periods(x):
    """csrc/srt_path.h piPeriods on a float32 array: (accepted, periods, r) -- floor(x / pi) and the fraction of x / pi as
    the kernel's float-float arithmetic has them, and whether the kernel trusts them."""
    x = np.asarray(x, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        qh = x * INV_PI_HI
        ql = _fma32(x, np.full_like(x, INV_PI_LO), _fma32(x, np.full_like(x, INV_PI_HI), -qh))
        f = np.floor(qh)
        r = (qh - f) + ql
        below, above = r < 0, r >= 1
        f = np.where(below, f - f32(1), np.where(above, f + f32(1), f))
        r = np.where(below, r + f32(1), np.where(above, r - f32(1), r)).astype(f32)
        ok = (r > PERIODS_MARGIN) & (r < f32(1) - PERIODS_MARGIN) & (np.abs(qh) < PERIODS_LIMIT)
    periods = np.where(ok, f, 0).astype(np.int64)
    return ok, periods, r


def sines(a, prec=128):
    """sin(a) for every float32 in `a` by mpmath at `prec` bits, rounded to float64 (no float32 is close enough to a
    multiple of pi for that to lose the sign); 0 for a == 0 and for non-finite a."""
    import mpmath
    a = np.asarray(a, f32)
    uniq, inverse = np.unique(np.ascontiguousarray(a).view(np.uint32), return_inverse=True)
    vals = uniq.view(f32)
    out = np.zeros(len(vals), np.float64)
    with mpmath.workprec(prec):
        for i, v in enumerate(vals):
            if np.isfinite(v) and v != 0:
                out[i] = float(mpmath.sin(mpmath.mpf(float(v))))
                assert out[i] != 0, float(v)
    return out[inverse.reshape(a.shape)]


def sin_signs(a):
    """-1, 0 (a == 0 or not finite) or +1: the sign of sin(a)."""
    return np.sign(sines(a)).astype(np.int8)


def checker_args(p):
    """The three arguments checker::value takes the sine of: 10.0f * p, in float32 as the kernel evaluates them."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (f32(10.0) * np.asarray(p, f32)).astype(f32)


def checker_truth(p):
    """True where checker::value picks the ODD texture at the points p (n, 3): sinf(ax) * sinf(ay) * sinf(az) < 0, the
    product taken in float32 from left to right over mpmath's sines rounded to float32 -- so a product that underflows is
    +-0 and a non-finite argument makes it NaN, neither of which is < 0.  (A libm's sinf may be an ulp off these sines; the
    tests' points keep every product either far above the smallest denormal or far below it.)"""
    a = checker_args(p)
    s = sines(a).astype(f32)
    with np.errstate(under="ignore", invalid="ignore"):
        s = np.where(np.isfinite(a), s, f32(np.nan))
        return ((s[..., 0] * s[..., 1]).astype(f32) * s[..., 2]).astype(f32) < 0


def checker_replay(p):
    """(odd, decided): checkerOdd's fast path on the points p (n, 3) -- decided where all three range reductions are
    accepted, odd = the parity it returns there."""
    a = checker_args(p)
    ok, k, _ = pi_periods(a)
    decided = ok.all(axis=-1)
    return ((k[..., 0] ^ k[..., 1] ^ k[..., 2]) & 1).astype(bool) & decided, decided


# ---------------------------------------------------------------- adversarial coordinates of the checker
CHECKER_K = (1, 2, 3, 7, 100, 31416, 10 ** 6, 4194303, 4194304, 4194305)  # the last three straddle |qh| < 2^22
ULP_SPAN = 40


def ulp_neighbours(x, span):
    """The float32 x and its +-1 .. +-span ulp neighbours (in the order of the reals, across zero)."""
    x = f32(x)
    bits = np.array([x]).view(np.int32)[0].astype(np.int64)
    key = bits if bits >= 0 else -(bits & 0x7fffffff)  # sign-magnitude -> a monotonic integer
    keys = key + np.arange(-span, span + 1, dtype=np.int64)
    out = np.where(keys >= 0, keys, (-keys) | 0x80000000).astype(np.uint32)
    return out.view(f32)


def near_pi_multiples(ks=CHECKER_K, span=ULP_SPAN):
    """The float32 nearest k * pi / 10 and its +-span ulp neighbours, for k = 0 and +-k of `ks`."""
    import mpmath
    out = []
    with mpmath.workprec(128):
        for k in (0,) + tuple(ks) + tuple(-k for k in ks):
            out.append(ulp_neighbours(f32(float(mpmath.pi * k / 10)), span))
    return np.concatenate(out)


def checker_coordinates(n_uniform=20000, seed=11):
    """Every adversarial value one coordinate takes (tests/test_shading.py group (a))."""
    rng = np.random.default_rng(seed)
    tiny = np.finfo(f32).tiny
    special = np.array([0.0, -0.0, 1e-20, tiny, 1e-40, np.inf, -np.inf, np.nan], f32)
    return np.concatenate([near_pi_multiples(), special,
                           rng.uniform(-10, 10, n_uniform).astype(f32), rng.uniform(-1.3e6, 1.3e6, n_uniform).astype(f32)])


def checker_points(xs):
    """One coordinate at a time takes the values xs; the other two sit at 0.05 and 0.4 (sin 0.5 > 0, sin 4 < 0) in both
    pairings: (6 * len(xs), 3) points."""
    xs = np.asarray(xs, f32)
    out = []
    for axis in range(3):
        others = [k for k in range(3) if k != axis]
        for a, b in ((0.05, 0.4), (0.4, 0.05)):
            p = np.empty((len(xs), 3), f32)
            p[:, axis] = xs
            p[:, others[0]], p[:, others[1]] = a, b
            out.append(p)
    return np.concatenate(out)


def underflow_points():
    """Two coordinates so small that the product of their sines underflows to zero whatever the third is -- the reference's
    expression is then +-0, not < 0 -- in every placement, with 0.05 and 0.4 as the third: what the margin piPeriods keeps
    from the integers is for."""
    small = np.array([1e-25, -1e-25, 1e-30, np.finfo(f32).tiny, 1e-40], f32)
    out = []
    for third in range(3):
        pair = [k for k in range(3) if k != third]
        for c in (0.05, 0.4):
            uu, vv = np.meshgrid(small, small, indexing="ij")
            p = np.empty((uu.size, 3), f32)
            p[:, pair[0]], p[:, pair[1]], p[:, third] = uu.reshape(-1), vv.reshape(-1), c
            out.append(p)
    return np.concatenate(out)


# ---------------------------------------------------------------- imagePNG::value
MAGENTA = (1.0, 0.0, 1.0)  # a failed load (texture.h:130-131)


def _clampf(x, lo, hi):  # globals.h:17-24: two compares, a NaN passes through
    return np.where(x < lo, f32(lo), np.where(x > hi, f32(hi), x)).astype(f32)


def texel_index(width, height, u, v):
    """(i, j) of texture.h:129-146 in float32; NaN coordinates index texel 0."""
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    with np.errstate(invalid="ignore"):
        u = _clampf(u, 0, 1)
        v = (f32(1) - _clampf(v, 0, 1)).astype(f32)
        fi, fj = (u * f32(width)).astype(f32), (v * f32(height)).astype(f32)
        i = np.where(np.isnan(u), 0, np.trunc(np.nan_to_num(fi))).astype(np.int64)
        j = np.where(np.isnan(v), 0, np.trunc(np.nan_to_num(fj))).astype(np.int64)
    return np.minimum(i, width - 1), np.minimum(j, height - 1)


def texel_lookup(pixels, u, v):
    """imagePNG::value on an image given as the uint8 array (height, width, bpp) it was loaded as, or None for a failed
    load: (n, 3) float32.  texture.h:147 reads pixel[0..2] whatever bpp is: for 1 and 2 bytes per pixel that runs into the
    following texels, and at and past the image's own last byte it reads 0."""
    u, v = np.broadcast_arrays(np.asarray(u, f32), np.asarray(v, f32))
    if pixels is None:
        return np.broadcast_to(np.array(MAGENTA, f32), u.shape + (3,)).copy()
    height, width, bpp = pixels.shape
    i, j = texel_index(width, height, u, v)
    flat = np.concatenate([pixels.reshape(-1), np.zeros(3, np.uint8)])
    at = (j * width + i) * bpp
    k = at[..., None] + np.arange(3)
    return np.where(k < width * height * bpp, flat[np.minimum(k, len(flat) - 1)], 0).astype(f32)


def uv_coordinates(size):
    """The values one texture coordinate takes against a side of `size` texels: the edges of [0, 1], i / size with its
    +-1 ulp neighbours for every i (where the float product u * size rounds), and what lies outside."""
    one = f32(1)
    edge = np.array([0.0, -0.0, 1.0, np.nextafter(one, f32(0)), np.nextafter(one, f32(2))], f32)
    grid = (np.arange(size + 1, dtype=f32) / f32(size)).astype(f32)
    grid = np.concatenate([np.nextafter(grid, f32(-1)), grid, np.nextafter(grid, f32(2))])
    outside = np.array([-1.0, 2.0, np.inf, -np.inf, np.nan, 1e-40], f32)
    return np.concatenate([edge, grid, outside])
