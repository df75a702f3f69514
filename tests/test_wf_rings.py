"""The rings of the path-pool kernel (csrc/srt_wf_rings.h) on the host, no GPU: the stand-alone program
examples/wf_rings_probe.cpp runs the header's own functions.

  * srtWfRingPos against c % capacity for the five capacities: 10^6 seeded counters each, and the edges around EVERY
    multiple of the capacity up to the top of the range -- 2^32 - 1 for the 2^j rings, 2 * 10^9 for the 3 * 2^j ones (what
    the planner admits them for).  The capacities are the header's table kSrtWfRings, as examples/plan_probe.cpp prints it.
  * a host replay of enqueue's reservation: waves of 64 lanes, each lane with a seeded ring of the call site's set or none,
    their atomics in a seeded interleaving.  Every (ring, place) is handed out exactly once; a wave's places in a ring are
    consecutive, in lane order; the rings' totals match; the replay over the call site's set gives the places of the
    replay over all rings.
  * the same program under the address and undefined-behaviour sanitizers, as a second stand-alone binary.

What this pins is the ARITHMETIC of the reservation as the header states it for the host (base + the lanes below in the
ring's mask) and its independence of the set.  The device forms -- v_mbcnt, v_writelane, srtWfEnqueue and srtWfClaim
themselves -- do not compile for the host: tests/test_gpu_wf_handover.py covers them, frame by frame."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "sexy-raytracer_amd", "csrc")
RINGS = 6
READY, RESTART, HIT, NEWITEM = 0, 1, 2, 5
CAPS = (1024, 1536, 2048, 3072, 4096)  # the parametrised tests' names; _capacities() holds them to the header's table
# the call sites of srt_wavefront.hip
SETS = {
    "swap": (RESTART, HIT, HIT + 1, HIT + 2),
    "hit_step": (READY, RESTART),
    "restart_and_item_pull": (READY, NEWITEM),
    "every_ring": tuple(range(RINGS)),
}


def _build(target):
    subprocess.check_call(["make", "-C", CSRC, "../../examples/" + target])
    return os.path.join(ROOT, "examples", target)


@pytest.fixture(scope="module")
def probe():
    return _build("srt_wf_rings_probe")


@functools.lru_cache(maxsize=None)
def _capacities():
    """capacity -> (shift, mul3): csrc/srt_wf_rings.h kSrtWfRings, the planner's table, read from the plan probe's output."""
    lines = subprocess.check_output([_build("srt_plan_probe"), "limits"], text=True).splitlines()
    table = {int(c): (int(s), int(m)) for key, c, s, m in (l.split() for l in lines if l.startswith("ring "))}
    assert sorted(table) == list(CAPS), table
    return table


def _run(exe, mode, blob, d):
    with open(d / "in.bin", "wb") as f:
        f.write(blob)
    subprocess.check_call([exe, mode, str(d / "in.bin"), str(d / "out.bin")])
    return np.fromfile(d / "out.bin", np.uint32)


def _top(cap):
    """The largest counter value a ring of this capacity is admitted for: 2^32 - 1, or 2 * 10^9 for the 3 * 2^j ones."""
    return 2 ** 32 - 1 if not _capacities()[cap][1] else 2 * 10 ** 9


def _edges(cap, first, count):
    """The counters m * cap - 2 .. m * cap + 2 for the multiples m in [first, first + count), clipped to [0, top]."""
    c = (np.arange(first, first + count, dtype=np.int64)[:, None] * cap + np.arange(-2, 3, dtype=np.int64)[None, :]).reshape(-1)
    return c[(c >= 0) & (c <= _top(cap))]


def _check_pos(exe, d, cap, c):
    shift, mul3 = _capacities()[cap]
    blob = np.array([cap, shift, mul3, len(c)], np.int32).tobytes() + c.astype(np.uint32).tobytes()
    got = _run(exe, "pos", blob, d)
    assert len(got) == len(c)
    bad = np.flatnonzero(got.astype(np.int64) != c % cap)
    assert len(bad) == 0, (cap, c[bad[:4]], got[bad[:4]])


@pytest.mark.parametrize("cap", CAPS)
def test_ring_pos_is_the_remainder(probe, tmp_path, cap):
    """10^6 seeded counters, the last 8192 values of the range, and the five counters around EVERY multiple of the capacity
    in the range (at most 4.2 M multiples, in chunks of 2^20): every quotient the multiply-shift modulo can meet."""
    shift, mul3 = _capacities()[cap]
    assert cap == (3 if mul3 else 1) << shift
    top = _top(cap)
    rng = np.random.default_rng(cap)
    _check_pos(probe, tmp_path, cap, np.concatenate([rng.integers(0, top + 1, 10 ** 6, dtype=np.int64), np.arange(top - 8191, top + 1, dtype=np.int64),
                                                     np.array([0, 1, top - 1, top], np.int64)]))
    multiples, seen = top // cap + 1, 0  # 0, cap, ..., the last multiple <= top
    for first in range(0, multiples, 1 << 20):
        count = min(1 << 20, multiples - first)
        c = _edges(cap, first, count)
        assert c[0] == max(0, first * cap - 2) and c[-1] == min(top, (first + count - 1) * cap + 2)
        _check_pos(probe, tmp_path, cap, c)
        seen += count
    assert seen == multiples and (multiples - 1) * cap <= top < multiples * cap


def _reservation_case(rings, rng, waves, calls_per_wave, tail0):
    """(blob, ring per call and lane, event list): `waves` waves make calls_per_wave calls each; a wave's calls follow each
    other, the atomics of different waves interleave at random, those of one call go in ring order (the lanes of one
    instruction; any order gives a call the same places only when no other wave's atomic falls between, so it is fixed)."""
    calls = waves * calls_per_wave
    ring = np.full((calls, 64), -1, np.int32)
    for c in range(calls):
        kind = c % 5
        fill = (0.0, 0.3, 0.7, 1.0, 1.0)[kind]  # nothing to enqueue / sparse / dense / every lane / every lane, one ring
        pick = rng.choice(rings, 64) if kind != 4 else np.full(64, rng.choice(rings))
        ring[c] = np.where(rng.uniform(size=64) < fill, pick, -1)
    # call c belongs to wave c % waves; per wave a queue of its atomics in order
    queues = [[] for _ in range(waves)]
    for c in range(calls):
        for r in sorted(set(int(x) for x in ring[c] if x >= 0)):
            queues[c % waves].append((c, r))
    events = []
    live = [w for w in range(waves) if queues[w]]
    at = [0] * waves
    while live:
        w = live[int(rng.integers(0, len(live)))]
        events.append(queues[w][at[w]])
        at[w] += 1
        if at[w] == len(queues[w]):
            live.remove(w)
    ev = np.array(events, np.int32).reshape(-1, 2)
    mask = sum(1 << r for r in rings)
    blob = np.array([mask, calls, len(ev)], np.int32).tobytes() + np.asarray(tail0, np.uint32).tobytes() + ring.tobytes() + ev.tobytes()
    return blob, ring, ev


@pytest.mark.parametrize("site", sorted(SETS))
def test_reservation_replay(probe, tmp_path, site):
    rings = SETS[site]
    rng = np.random.default_rng(sorted(SETS).index(site) + 100)
    # tails that start just below a multiple of every capacity, and one just below the counter's wrap
    tail0 = np.array([0, 3 * 4096 - 7, 1536 * 5 - 1, 2 ** 32 - 100, 12345, 3072 * 9 - 33], np.int64)
    blob, ring, ev = _reservation_case(rings, rng, waves=16, calls_per_wave=12, tail0=tail0)
    out = _run(probe, "reserve", blob, tmp_path)
    calls = len(ring)
    assert len(out) == calls * 128 + RINGS
    place = out[:calls * 128].reshape(calls, 64, 2).astype(np.int64)
    tail1 = out[calls * 128:].astype(np.int64)
    none = ring < 0
    assert (place[none] == 0xffffffff).all() and none.any() and (~none).any()
    # the specialised form gives the generic form's places
    assert np.array_equal(place[..., 0], place[..., 1])
    p = place[..., 0]
    for r in range(RINGS):
        mine = ring == r
        total = int(mine.sum())
        # the ring's total, and every place of [tail0, tail0 + total) handed out exactly once (counters wrap at 2^32)
        assert tail1[r] == (tail0[r] + total) % 2 ** 32, (r, tail0[r], total, tail1[r])
        if r not in rings:
            assert total == 0
            continue
        assert total > 64
        got = np.sort((p[mine] - tail0[r]) % 2 ** 32)
        assert np.array_equal(got, np.arange(total)), r
        # a wave's places in the ring: consecutive from the base its atomic returned, in lane order
        for c in range(calls):
            lanes = np.flatnonzero(mine[c])
            if len(lanes):
                rel = (p[c, lanes] - p[c, lanes[0]]) % 2 ** 32
                assert np.array_equal(rel, np.arange(len(lanes))), (r, c)
    # the interleaving was one: the first 32 atomics come from more than four of the sixteen waves
    assert len({int(c) % 16 for c, _ in ev[:32]}) > 4


def test_probe_under_sanitizers(tmp_path):
    """The header's host code under -fsanitize=address,undefined: a second stand-alone binary, one run of each mode (the
    3 * 2^j arithmetic at the top of its range and the counters' wrap in the reservation included)."""
    exe = _build("srt_wf_rings_probe_san")
    # (a stand-alone binary with the sanitizers' runtime linked in: the environment is inherited, plus their options)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for cap in (1536, 4096):
        shift, mul3 = _capacities()[cap]
        c = _edges(cap, _top(cap) // cap - 3999, 4000)  # the last 4000 multiples of the range
        blob = np.array([cap, shift, mul3, len(c)], np.int32).tobytes() + c.astype(np.uint32).tobytes()
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(blob)
        r = subprocess.run([exe, "pos", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0 and "runtime error" not in r.stdout and "Sanitizer" not in r.stdout, r.stdout[-2000:]
        assert np.array_equal(np.fromfile(tmp_path / "out.bin", np.uint32).astype(np.int64), c % cap)
    blob, ring, _ = _reservation_case(SETS["swap"], np.random.default_rng(8), waves=4, calls_per_wave=5, tail0=[0, 2 ** 32 - 10, 5, 6, 7, 8])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, "reserve", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stdout and "Sanitizer" not in r.stdout, r.stdout[-2000:]
    assert len(np.fromfile(tmp_path / "out.bin", np.uint32)) == len(ring) * 128 + RINGS
