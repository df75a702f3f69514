"""csrc/srt_tri_hit.h on the host: the certified triangle test never decides against the exact one (the stand-alone program
examples/tri_cert_probe.cpp over more than 10^7 seeded pairs), the exact test it takes as truth is the CPU oracle's
triangle::hit bit for bit, and the triFast record is the float64 statement of its fields.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import tri_cert_cases as TC
from conftest import ROOT

F = np.float32
PROBE = os.path.join(ROOT, "examples", "srt_tri_cert_probe")
PER_CLASS = 1_100_000  # x 10 classes


@pytest.fixture(scope="module")
def probe():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "sexy-raytracer_amd", "csrc"), "../../examples/srt_tri_cert_probe"])
    return PROBE


@pytest.fixture(scope="module")
def sweep(probe):
    """{class: {pairs, plane_ok, undecided, diff, t_diff, max_ratio}} of one seeded run."""
    out = {}
    for line in subprocess.check_output([probe, "sweep", "1", str(PER_CLASS)], text=True).splitlines():
        w = line.split()
        assert w[0] == "class" and len(w) == 14, line
        out[w[1]] = {w[k]: (float(w[k + 1]) if w[k] == "max_ratio" else int(w[k + 1])) for k in range(2, 14, 2)}
        print(line)
    return out


def test_no_decided_verdict_differs(sweep):
    want = {"random", "edge", "vertex", "plane_origin", "grazing", "scales", "degenerate", "denormal_zero", "axis_directions", "far_origin"}
    assert set(sweep) == want
    assert sum(c["pairs"] for c in sweep.values()) >= 10_000_000
    for name, c in sweep.items():
        assert c["diff"] == 0 and c["t_diff"] == 0, (name, c)
        assert c["plane_ok"] > 0, (name, c)  # the class does reach the edge tests


def test_random_rays_are_decided(sweep):
    c = sweep["random"]
    assert c["plane_ok"] > 100_000 and c["undecided"] <= 1e-3 * c["plane_ok"], c


@pytest.mark.parametrize("name", ["edge", "vertex"])
def test_edge_aimed_rays_reach_the_exact_test(sweep, name):
    assert sweep[name]["undecided"] > 0, sweep[name]


def test_observed_error_is_inside_the_proven_bound(sweep):
    """srt_tri_hit.h proves |cheap - exact| <= 64 u N E (W + E); the sweep's largest ratio is recorded there."""
    worst = max(c["max_ratio"] for c in sweep.values())
    print("largest |exact - cheap| / unit: %.3f" % worst)
    assert 0 < worst < 64


# ---------------------------------------------------------------- the exact test against the oracle
TRIANGLES = [((-1.0, 0.5, -2.0), (1.5, 0.25, -1.0), (0.25, 2.0, -1.5)),
             ((0.0, 0.0, 0.0), (1e-3, 0.0, 0.0), (0.0, 1e-3, 2e-4)),
             ((1.25, -3.0, 2.0), (1.25, 4.0, 2.5), (1.25, 0.5, -3.0))]  # axis-aligned plane


@pytest.mark.parametrize("k", range(len(TRIANGLES)))
def test_exact_test_is_the_oracles(probe, abi, oracle, tmp_path, k):
    sb = TC.one_triangle(abi, TRIANGLES[k])
    by_class = TC.rays(abi, TC.triangles_of(sb), np.random.default_rng(40 + k), 500)
    rays = np.concatenate([by_class[c] for c in TC.CLASSES])
    want = oracle.OracleScene(sb).trace(rays)
    packed = np.concatenate([rays["o"], rays["d"], rays["tMin"][:, None]], axis=1).astype(F)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array(TRIANGLES[k], F).tobytes() + np.array([len(rays)], np.int32).tobytes() + packed.tobytes())
    subprocess.check_call([probe, "exact", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = np.fromfile(tmp_path / "out.bin", np.int32).reshape(-1, 4)
    hit = want["prim"] >= 0
    assert 0.05 < hit.mean() < 0.95  # both outcomes occur
    assert np.array_equal(got[:, 0] != 0, hit)
    assert np.array_equal(got[hit, 1], want["t"][hit].view(np.int32))
    decided = got[:, 3] == 0
    assert np.array_equal(got[decided, 2] != 0, hit[decided])  # and the certified verdict, where it decides
    assert (~decided).any() and decided.mean() > 0.5


# ---------------------------------------------------------------- the record
def _record64(p):
    """The triFast record of triangle p (3, 3) float32, stated in NumPy: float32 where the library's operation order
    matters (n, d, the edges), float64 rounded once for m0, m1, k, kappa and the last word."""
    v0, v1, v2 = p
    a, b = v1 - v0, v2 - v0
    n = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)
    d = -(n[0] * v0[0] + (n[1] * v0[1] + n[2] * v0[2]))
    e = np.array([v1 - v0, v2 - v1, v0 - v2], F)
    n64, e64 = n.astype(np.float64), e.astype(np.float64)
    with np.errstate(all="ignore"):
        m = np.array([np.cross(n64, e64[0]), np.cross(n64, e64[1])])
        k = F((m[1] * e64[0]).sum())
        m32 = m.astype(F)
    N, E = np.abs(n64).max(), np.abs(e64).max()

    def in_range(x, lo, hi):
        x = np.abs(np.asarray(x, np.float64))
        return bool(((x == 0) | ((x >= lo) & (x <= hi))).all())

    ok = in_range(e, 2.0 ** -36, 2.0 ** 30) and in_range(n, 2.0 ** -72, 2.0 ** 60) and in_range(m32, 2.0 ** -120, 2.0 ** 124) and in_range(k, 2.0 ** -120, 2.0 ** 124)
    kappa = 2.0 ** -18 * N * E
    last = kappa * E + 2.0 ** -120 * (1 + N) * (1 + E)
    return np.concatenate([v0, [d], n, [k], m32[0], [F(kappa) if ok else np.inf], m32[1], [F(last) if ok else np.inf]]).astype(F), ok


def test_records_against_float64(dev, abi):
    rng = np.random.default_rng(3)
    tris = [rng.uniform(-6, 6, (3, 3)).astype(F) for _ in range(200)]
    tris += [(c + rng.uniform(-s, s, (3, 3))).astype(F) for s in (1e-3, 0.08, 2.0 ** -20, 2.0 ** 10) for c in rng.uniform(-50, 50, (20, 1, 3))]
    tris += [np.array(TC.UNCERTIFIED, F), np.array([(-2.0 ** 30, -5, -6), (2.0 ** 30, -5, -6), (0, 2.0 ** 20, -6)], F),
             np.array([(0, 0, 0), (1e-40, 0, 0), (0, 1, 0)], F), np.zeros((3, 3), F), np.array([(1, 2, 3), (1, 2, 3), (4, 5, 6)], F)]
    certified = 0
    for p in tris:
        want, ok = _record64(p)
        got = dev.tri_fast_record(p.reshape(9))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (p.tolist(), got.tolist(), want.tolist())
        certified += ok
    assert 200 < certified < len(tris)
    for p in (TC.UNCERTIFIED, tris[-4], tris[-3]):  # an edge component below 2^-36, an edge of 2^31, a denormal edge
        rec = dev.tri_fast_record(np.array(p, F).reshape(9))
        assert np.isposinf(rec[11]) and np.isposinf(rec[15])
    assert dev.tri_fast_record(np.zeros(9, F))[11] == 0  # no extent at all: certified, kappa 0 (its plane test never passes)
