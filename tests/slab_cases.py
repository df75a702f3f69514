"""(box, ray) cases for the certified slab test (csrc/srt_slab.h), class by class, as NumPy arrays with fixed seeds, and the
reference's box test (aabb.h:14-22) stated in NumPy float32.  Shared by tests/test_slab_host.py (the host compile, through the
probe's replay mode) and tests/test_gpu_slab_cert.py (the device compile, through srtTestSlabVisit).  The classes are those of
examples/slab_probe.cpp's sweep, drawn again here; `edges` and `ulp2` of the sweep are about the host's reciprocal and have
no counterpart: the device makes its own.

A case is 13 float32: box min[3], box max[3], origin[3], direction[3], tMax.  tMin belongs to the launch."""
import numpy as np

F = np.float32
CLASSES = ("random", "zeros", "flat", "ground", "d_edges", "o_edges", "aimed", "uncertified", "far", "touch", "tmin_zero")
T_MINS = (0.001, 0.0, 64.0)

GROUND = np.array([0.0, -0.0, 1000.0, -1000.0, -2000.0], F)
ZEROS = np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -77, -2.0 ** -77, 2.0 ** 30, -2.0 ** 30, 0.5, -3.25], F)
ORIGINS = np.array([0.0, -0.0, 2.0 ** 30, -2.0 ** 30, 2.0 ** -77, -2.0 ** -77, 1.0, -13.0], F)
DIRS = np.array([2.0 ** -20, -2.0 ** -20, 2.0 ** 20, -2.0 ** 20, 1.0, -1.0], F)
BAD_D = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** -21, -2.0 ** 21, 2.0 ** -130, 2.0 ** -127], F)


def operand_ok(o, d):
    """srtSlabOperandOk per component: |d| in [2^-20, 2^20]; o zero or |o| in [2^-77, 2^30]."""
    with np.errstate(invalid="ignore"):
        ad, ao = np.abs(d), np.abs(o)
        return (ad >= F(2.0 ** -20)) & (ad <= F(2.0 ** 20)) & ((o == 0) | ((ao >= F(2.0 ** -77)) & (ao <= F(2.0 ** 30))))


def certified(cases):
    return operand_ok(cases[:, 6:9], cases[:, 9:12]).all(axis=1)


def reference(cases, t_min):
    """aabb.h:14-22 in float32: per axis the two quotients, fminf / fmaxf (np.fmin / np.fmax: a NaN operand is ignored), and
    !(tMax <= tMin) after the three axes.  Returns (entered, tMin, tMax)."""
    lo, hi, o, d = cases[:, 0:3], cases[:, 3:6], cases[:, 6:9], cases[:, 9:12]
    t0 = np.full(len(cases), t_min, F)
    t1 = cases[:, 12].copy()
    with np.errstate(all="ignore"):
        for k in range(3):
            a = (lo[:, k] - o[:, k]) / d[:, k]
            b = (hi[:, k] - o[:, k]) / d[:, k]
            assert a.dtype == F and b.dtype == F
            t0 = np.fmax(np.fmin(a, b), t0)
            t1 = np.fmin(np.fmax(a, b), t1)
        return ~(t1 <= t0), t0, t1


def gate(cases, t_min):
    """The gate form of the exact test, from DESIGN 6.1 (not from the kernel): the verdict on a box taken as an inner node of
    the regrouped tree.  On an axis with d == +-0 it passes iff min <= o <= max -- closed, and written so that a NaN origin
    passes as it does in the reference -- and puts no bound on t; on every other axis it is the reference's arithmetic."""
    lo, hi, o, d = cases[:, 0:3], cases[:, 3:6], cases[:, 6:9], cases[:, 9:12]
    t0 = np.full(len(cases), t_min, F)
    t1 = cases[:, 12].copy()
    inside = np.ones(len(cases), bool)
    with np.errstate(all="ignore"):
        for k in range(3):
            zero = d[:, k] == 0
            a = (lo[:, k] - o[:, k]) / d[:, k]
            b = (hi[:, k] - o[:, k]) / d[:, k]
            assert a.dtype == F and b.dtype == F
            t0 = np.where(zero, t0, np.fmax(np.fmin(a, b), t0))
            t1 = np.where(zero, t1, np.fmin(np.fmax(a, b), t1))
            inside &= ~zero | (~(o[:, k] < lo[:, k]) & ~(o[:, k] > hi[:, k]))
        return inside & ~(t1 <= t0)


GATE_T_MIN = 0.001


def gate_grid():
    """The nested pairs of tests/test_regroup_host.py (_gate_cases over _axis_cases: shared planes, flat and point boxes, d of
    +-0, +-2^-20, +-1, +-inf and NaN, origins on planes, off planes and NaN, tMax of +inf and 1.5) as cases of this module:
    (inner, outer), row i of both the same ray at tMin = GATE_T_MIN, the inner box inside the outer one."""
    from test_regroup_host import _gate_cases
    g = _gate_cases()
    assert (g[:, 18] == F(GATE_T_MIN)).all()
    assert (g[:, 6:9] <= g[:, 0:3]).all() and (g[:, 0:3] <= g[:, 3:6]).all() and (g[:, 3:6] <= g[:, 9:12]).all()
    inner = np.concatenate([g[:, 0:6], g[:, 12:18], g[:, 19:20]], axis=1).astype(F)
    outer = np.concatenate([g[:, 6:12], g[:, 12:18], g[:, 19:20]], axis=1).astype(F)
    return inner, outer


def ulps(x, k):
    """x moved by k float32 steps (k an int array, |k| <= 4)."""
    x = np.array(x, F)
    for j in range(4):
        x = np.where(k > j, np.nextafter(x, F(np.inf)), x)
        x = np.where(k < -j, np.nextafter(x, F(-np.inf)), x)
    return x.astype(F)


def _order(a, b):
    return np.minimum(a, b).astype(F), np.maximum(a, b).astype(F)


def _sym(rng, shape, a):
    return (2.0 * rng.random(shape) - 1.0) * a


def _sign(rng, shape):
    return np.where(rng.random(shape) < 0.5, -1.0, 1.0)


def _direction(rng, shape, span=20.0):
    return (_sign(rng, shape) * np.exp2(_sym(rng, shape, span))).astype(F)


def _aim_inside(rng, lo, hi, o, d, t, rows, bound=2.0 ** 40):
    """On `rows`: the origin moved so that the ray meets a point of the box (clipped to +-bound) at parameter t; a component
    that leaves the certified range becomes 0."""
    l, h = np.maximum(lo.astype(np.float64), -bound), np.minimum(hi.astype(np.float64), bound)
    p = np.where(l <= h, l + rng.random(lo.shape) * (h - l), lo)
    moved = (p - t[:, None] * d.astype(np.float64)).astype(F)
    moved = np.where(operand_ok(moved, d), moved, F(0))
    o[rows] = moved[rows]


def _aim_direction(rng, lo, hi, o, d, t, rows):
    """On `rows`: d = (p - o) / t for a point p of the box, kept where it is inside the certified range."""
    p = lo.astype(np.float64) + rng.random(lo.shape) * (hi.astype(np.float64) - lo)
    aimed = ((p - o) / t[:, None]).astype(F)
    keep = operand_ok(o, aimed) & rows[:, None]
    d[keep] = aimed[keep]


def _t_max(rng, n):
    return np.where(rng.random(n) < 0.75, np.inf, np.exp2(_sym(rng, n, 12.0))).astype(F)


def cases(name, n, t_min, seed=1):
    """n cases of one class for a launch at t_min: the rays that are aimed meet their box beyond t_min."""
    rng = np.random.default_rng([seed, CLASSES.index(name), int(t_min * 1000)])
    base = max(float(t_min), 1.0)
    t = base * (1.0 + np.exp2(_sym(rng, n, 4.0)))  # where an aimed ray meets its point
    half = np.arange(n) % 2 == 1
    s3 = (n, 3)
    t_max = _t_max(rng, n)
    if name == "random":
        scale = np.exp2(_sym(rng, n, 10.0))[:, None]
        lo, hi = _order(_sym(rng, s3, scale), _sym(rng, s3, scale))
        o = _sym(rng, s3, 4.0 * scale).astype(F)
        d = _direction(rng, s3)
        d[half] = (_sign(rng, s3) * np.exp2(_sym(rng, s3, 3.0))).astype(F)[half]
        _aim_inside(rng, lo, hi, o, d, t * scale[:, 0], half)
    elif name == "zeros":
        lo, hi = _order(rng.choice(ZEROS, s3), rng.choice(ZEROS, s3))
        swap = (lo == hi) & (rng.random(s3) < 0.5)  # both orders of the two zeros
        lo, hi = np.where(swap, hi, lo), np.where(swap, lo, hi)
        o = np.where(rng.random(s3) < 0.5, _sym(rng, s3, 8.0), rng.choice(ORIGINS, s3)).astype(F)
        d = _direction(rng, s3)
        d[half] = (_sign(rng, s3) * np.exp2(_sym(rng, s3, 3.0))).astype(F)[half]
        _aim_inside(rng, lo, hi, o, d, t, half, bound=8.0)
    elif name == "flat":
        lo, hi = _order(_sym(rng, s3, 50.0), _sym(rng, s3, 50.0))
        flat = rng.random(s3) < 0.5
        flat[:, 0] = True
        hi = np.where(flat, lo, hi)
        o = _sym(rng, s3, 100.0).astype(F)
        d = _direction(rng, s3)
        _aim_inside(rng, lo, hi, o, d, t, half)
    elif name == "ground":
        lo, hi = _order(rng.choice(GROUND, s3), rng.choice(GROUND, s3))
        o = _sym(rng, s3, 30.0).astype(F)
        d = (_sign(rng, s3) * np.exp2(_sym(rng, s3, 3.0))).astype(F)
        _aim_inside(rng, lo, hi, o, d, t, half)
    elif name == "d_edges":
        lo, hi = _order(_sym(rng, s3, 6.0), _sym(rng, s3, 6.0))
        o = _sym(rng, s3, 6.0).astype(F)
        d = np.where(rng.random(s3) < 0.75, rng.choice(DIRS, s3), _direction(rng, s3)).astype(F)
        _aim_inside(rng, lo, hi, o, d, t, half)
    elif name == "o_edges":
        lo, hi = _order(_sym(rng, s3, 2000.0), _sym(rng, s3, 2000.0))
        o = rng.choice(ORIGINS, s3).astype(F)
        d = _direction(rng, s3)
        _aim_direction(rng, lo, hi, o, d, max(float(t_min), 1.0) * 2.0 ** 11 * (1.0 + rng.random(n)), half)
    elif name == "aimed":  # through a corner of the box, the origin moved by -2 .. 2 ulps
        lo, hi = _order(_sym(rng, s3, 5.0), _sym(rng, s3, 5.0))
        p = np.where(rng.random(s3) < 0.5, lo, hi).astype(np.float64)
        d = (_sign(rng, s3) * np.exp2(_sym(rng, s3, 2.0))).astype(F)
        o = ulps((p - t[:, None] * d.astype(np.float64)).astype(F), rng.integers(-2, 3, s3))
    elif name == "uncertified":
        lo, hi = _order(_sym(rng, s3, 6.0), _sym(rng, s3, 6.0))
        o = _sym(rng, s3, 6.0).astype(F)
        d = _direction(rng, s3)
        _aim_inside(rng, lo, hi, o, d, t, half)
        rows, k, how = np.arange(n), rng.integers(0, 3, n), rng.integers(0, 3, n)
        bad_d = rng.choice(BAD_D, n)
        bad_o = np.where(how == 1, _sign(rng, n) * np.where(rng.random(n) < 0.5, 2.0 ** 31, 2.0 ** -80),
                         np.where(rng.random(n) < 0.5, np.nan, _sign(rng, n) * np.inf)).astype(F)
        d[rows, k] = np.where(how == 0, bad_d, d[rows, k])
        o[rows, k] = np.where(how == 0, o[rows, k], bad_o)
    elif name == "far":
        lo, hi = _order(_sym(rng, s3, 4.0), _sym(rng, s3, 4.0))
        o = (_sign(rng, s3) * np.exp2(10.0 + 20.0 * rng.random(s3))).astype(F)
        d = _direction(rng, s3)
        big = np.abs(o).max(axis=1).astype(np.float64)
        rows = np.arange(n) % 4 != 0
        _aim_direction(rng, lo, hi, o, d, np.maximum(big * np.exp2(-19.0 * rng.random(n)), 2.0 * float(t_min)), rows)
        t_max = np.where(rows, np.inf, t_max).astype(F)
    elif name == "touch":  # tMax within 4 ulps of one of the box's own quotients on one axis, the other two axes open
        axis = rng.integers(0, 3, n)
        on = np.arange(3)[None, :] == axis[:, None]
        half_side = np.where(on, 5.0, 100.0)
        lo, hi = _order(_sym(rng, s3, half_side), _sym(rng, s3, half_side))
        lo = np.where(on, lo, -half_side - rng.random(s3)).astype(F)
        hi = np.where(on, hi, half_side + rng.random(s3)).astype(F)
        d = (_sign(rng, s3) * np.exp2(np.where(on, 2.0 + 2.0 * rng.random(s3), -2.0 * rng.random(s3)))).astype(F)
        o = np.zeros(s3, F)
        _aim_inside(rng, lo, hi, o, d, t, np.ones(n, bool), bound=5.0)
        rows = np.arange(n)
        qa = (lo[rows, axis] - o[rows, axis]) / d[rows, axis]
        qb = (hi[rows, axis] - o[rows, axis]) / d[rows, axis]
        q = np.where(rng.random(n) < 0.5, np.fmin(qa, qb), np.fmax(qa, qb))
        t_max = ulps(q, rng.integers(-4, 5, n))
    elif name == "tmin_zero":
        lo, hi = _order(_sym(rng, s3, 5.0), _sym(rng, s3, 5.0))
        o = _sym(rng, s3, 20.0).astype(F)
        d = (_sign(rng, s3) * np.exp2(_sym(rng, s3, 4.0))).astype(F)
        _aim_inside(rng, lo, hi, o, d, base * np.exp2(_sym(rng, n, 2.0)), half)
        t_max = np.where(rng.random(n) < 0.5, np.inf, base * np.exp2(2.0 * rng.random(n))).astype(F)
    else:
        raise ValueError(name)
    out = np.concatenate([lo, hi, o, d, t_max[:, None]], axis=1).astype(F)
    assert out.shape == (n, 13) and (out[:, 0:3] <= out[:, 3:6]).all()
    return out
