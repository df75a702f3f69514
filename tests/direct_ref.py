"""Steps 1-4 of the direct-light term (include/srt_hip.h "Direct light sampling") replayed in NumPy float32: the term's own
generator, the choice of the light, the uniform cone about it and the weight -- every operation and association as the
header states them (csrc/srt_direct.h performs the same ones).  The generator is tests/pathstep_ref.Pcg.

cone() and basis() work on float32 scalars and on arrays alike, so that tests/test_direct_ref.py can hold them to
themselves over many draws; sample() is one hit's replay, which the GPU tests compare srtDirectLightDevice with."""
import numpy as np

import pathstep_ref as PR

F = np.float32
SALT = 0x5DEECE66D2545F49
ONE, TWO = F(1.0), F(2.0)


def len_sq(v):
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def dot3(a, b):
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])


def basis(w):
    """Duff et al. 2017 about the unit vector w = (x, y, z): (t1, t2), each a tuple of three."""
    sign = np.copysign(ONE, w[2])
    ka = -ONE / (sign + w[2])
    kb = (w[0] * w[1]) * ka
    sx = sign * w[0]
    t1 = (ONE + (sx * w[0]) * ka, sign * kb, -sx)
    t2 = (kb, sign + (w[1] * w[1]) * ka, -w[1])
    return t1, t2


def one_minus_cos_max(q):
    """1 - cos of the cone's half angle from q = r^2 / d^2, without cancellation."""
    return q / (ONE + np.sqrt(ONE - q))


def cone(a, b, q, w):
    """The direction for the disk point (a, b), q = r^2 / d^2 and the unit vector w towards the centre: (dir, oneMinus, sD)."""
    sD = a * a + b * b
    one_minus = one_minus_cos_max(q)
    m = sD * one_minus
    cos_t = ONE - m
    sin_t = np.sqrt(m * (TWO - m))
    root = np.sqrt(sD)
    zero = sD == 0
    safe = np.where(zero, ONE, root)
    c_phi = np.where(zero, ONE, a / safe).astype(F)
    s_phi = np.where(zero, F(0.0), b / safe).astype(F)
    t1, t2 = basis(w)
    k1, k2 = c_phi * sin_t, s_phi * sin_t
    d = tuple((k1 * t1[c] + k2 * t2[c]) + cos_t * w[c] for c in range(3))
    return d, one_minus, sD


def sample(state, x, normal, lights):
    """One hit.  state: the path's generator state before the hit's scatter draws (a Python int, 64 bits); x, normal: three
    float32 each; lights: the table, [(centre (3,), radius, moving)] in prims[] order, K > 0.  Returns {"light": the table
    row or -1, "dir": (3,) float32, "weight": float32, "state": the term's generator state afterwards}."""
    K = len(lights)
    g = PR.Pcg(PR.mix64((state & PR.M64) ^ SALT))
    u = g.uniform()
    k = min(int(F(u * F(K))), K - 1)
    centre, radius, moving = lights[k]
    x = [F(v) for v in x]
    to_c = [F(centre[c]) - x[c] for c in range(3)]
    d2 = len_sq(to_c)
    r2 = F(radius) * F(radius)
    none = {"light": -1, "dir": np.zeros(3, F), "weight": F(0.0), "state": g.state}
    if moving or d2 <= r2:
        return none
    a, b = g.in_unit_disk()
    with np.errstate(all="ignore"):
        root_d2 = np.sqrt(d2)
        w = tuple(to_c[c] / root_d2 for c in range(3))
        d, one_minus, _ = cone(a, b, r2 / d2, w)
        n = [F(v) for v in normal]
        weight = (F(K) * (TWO * one_minus)) * np.fmax(dot3(n, d), F(0.0))  # fmaxf: a NaN cosine gives 0
    return {"light": k, "dir": np.array(d, F), "weight": F(weight), "state": g.state}
