"""tests/direct_ref.py held to itself: the cone of the direct-light term (include/srt_hip.h "Direct light sampling", steps
2-4) over 10^5 draws with q = r^2 / d^2 from 1e-6 to 0.99 -- unit directions, inside the cone, an orthonormal basis, a
uniformly sampled cone -- and sample() on cases worked by hand.  Needs no GPU.

Bounds: an ulp is that of 1.0f, 2^-23.  Lengths, cosines and dot products are evaluated in float64 from the float32 values."""
import numpy as np

import direct_ref as DR
import pathstep_ref as PR

F = np.float32
ULP = 2.0 ** -23
N = 100_000


def _draws():
    """N disk points from the replay's own generator (one stream), N values of q spread evenly in log q over [1e-6, 0.99], N
    unit vectors made as the kernel makes w: toC / sqrt(lenSq(toC)) in float32."""
    g = PR.Pcg(PR.rng_key(2024, 7, 0))
    ab = np.array([g.in_unit_disk() for _ in range(N)], F)
    rng = np.random.default_rng(5)
    q = np.exp(rng.uniform(np.log(1e-6), np.log(0.99), N)).astype(F)
    q[:4] = F(1e-6), F(0.99), F(0.5), F(0.25)
    to_c = rng.normal(0, 1, (N, 3)).astype(F) * np.exp(rng.uniform(-3, 6, (N, 1))).astype(F)
    to_c[:6] = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0], [1e-4, 0, -1], [0, 1e-3, 1]], F) * F(3.0)  # the poles of the basis
    d2 = DR.len_sq(to_c.T)
    w = (to_c / np.sqrt(d2)[:, None]).astype(F)
    return ab[:, 0].copy(), ab[:, 1].copy(), q, w


A, B, Q, W = _draws()
with np.errstate(all="ignore"):
    DIR, ONE_MINUS, SD = DR.cone(A, B, Q, tuple(W.T))
DIR = np.stack(DIR, axis=1)


def test_everything_is_float32():
    assert DIR.dtype == F and ONE_MINUS.dtype == F and SD.dtype == F and np.isfinite(DIR).all()
    t1, t2 = DR.basis(tuple(W.T))
    assert all(c.dtype == F for c in t1 + t2)


def test_directions_have_unit_length_within_4_ulp():
    length = np.sqrt((DIR.astype(np.float64) ** 2).sum(axis=1))
    w_length = np.sqrt((W.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(w_length - 1).max() <= 1.5 * ULP  # what the kernel's own normalisation leaves
    assert np.abs(length - 1).max() <= 4 * ULP, np.abs(length - 1).max() / ULP


def test_directions_lie_inside_the_cone_within_4_ulp():
    q = Q.astype(np.float64)
    cos_max = np.sqrt(1 - q)
    cos = (DIR.astype(np.float64) * W.astype(np.float64)).sum(axis=1)
    assert (cos >= cos_max - 4 * ULP).all(), ((cos_max - cos).max() / ULP)
    # ... and 1 - cos_max is the cancellation-free form of it, to an ulp of its own size
    exact = q / (1 + cos_max)
    assert (np.abs(ONE_MINUS.astype(np.float64) - exact) <= 2 * ULP * exact).all()


def test_basis_is_orthonormal():
    t1, t2 = (np.stack(t, axis=1).astype(np.float64) for t in DR.basis(tuple(W.T)))
    w = W.astype(np.float64)
    for v in (t1, t2):
        assert np.abs(np.sqrt((v ** 2).sum(axis=1)) - 1).max() <= 4 * ULP
    for a, b in ((t1, t2), (t1, w), (t2, w)):
        assert np.abs((a * b).sum(axis=1)).max() <= 4 * ULP
    # right-handed: t1 x t2 = w
    assert np.abs(np.cross(t1, t2) - w).max() <= 4 * ULP


def test_cone_is_sampled_uniformly():
    """Uniform over the cap means the cap's height m = sD * oneMinus is uniform on [0, oneMinus]: sD uniform on [0, 1), mean
    1/2, variance 1/12.  cosT = 1 - m exactly that height."""
    sd = SD.astype(np.float64)
    assert (sd >= 0).all() and (sd < 1).all()
    assert abs(sd.mean() - 0.5) <= 4 * np.sqrt(1.0 / 12.0 / N), sd.mean()
    assert abs(sd.std() - np.sqrt(1.0 / 12.0)) <= 0.005
    cos = (DIR.astype(np.float64) * W.astype(np.float64)).sum(axis=1)
    height = (1 - cos) / ONE_MINUS.astype(np.float64)
    big = Q > 1e-3  # where 1 - cos is well above the rounding of cos
    assert np.abs(height[big] - sd[big]).max() <= 1e-3


def test_the_centre_of_the_disk_is_the_axis():
    w = (F(0.6), F(0.0), F(0.8))
    d, one_minus, sd = DR.cone(F(0.0), F(0.0), F(0.25), w)
    assert sd == 0 and [float(c) for c in d] == [float(c) for c in w]
    assert float(one_minus) == float(F(0.25) / (F(1.0) + np.sqrt(F(0.75))))


def test_sample_by_hand():
    lights = [((0.0, 10.0, 0.0), 1.0, False), ((5.0, 0.0, 0.0), 2.0, True), ((0.0, 0.0, 0.0), 3.0, False)]
    x, n = (0.0, 1.0, 0.0), (0.0, 1.0, 0.0)
    seen = set()
    for state in range(200):
        s = DR.sample(state, x, n, lights)
        g = PR.Pcg(PR.mix64(state ^ DR.SALT))
        k = min(int(F(g.uniform() * F(3))), 2)
        seen.add(k)
        if k == 0:
            assert s["light"] == 0 and s["weight"] > 0
            a, b = g.in_unit_disk()
            assert s["state"] == g.state  # u, then the disk: nothing else is drawn
            cos = float(s["dir"][1])  # w = +y
            assert cos >= np.sqrt(1 - 1.0 / 81.0) - 4 * ULP
            # weight = K * 2 * oneMinus * cos
            one_minus = DR.one_minus_cos_max(F(1.0) / F(81.0))
            assert float(s["weight"]) == float((F(3) * (F(2) * one_minus)) * s["dir"][1])
        else:  # the moving light, and the one that encloses x (d2 = 1 <= 9): nothing sampled, nothing more drawn
            assert s["light"] == -1 and s["weight"] == 0 and not s["dir"].any() and s["state"] == g.state
    assert seen == {0, 1, 2}
    # a light below the horizon of n: chosen, weight exactly 0
    s = DR.sample(3, x, (0.0, -1.0, 0.0), lights[:1])
    assert s["light"] == 0 and s["weight"] == 0 and s["dir"][1] > 0
    # the salt is the header's, and the term's stream is not the path's
    assert DR.SALT == 0x5DEECE66D2545F49 and PR.mix64(5 ^ DR.SALT) != 5
