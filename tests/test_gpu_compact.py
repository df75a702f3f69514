"""srtCompactPathsDevice (include/srt_hip.h "Path steps on device buffers") through the raw entry, and the user-land loop
with compaction between its bounces (sexy-raytracer_amd/pathloop.py, compact=True).

ZERO tolerance everywhere: compaction moves bytes.  The reference is tests/compact_ref.py (the predicate, np.flatnonzero,
row gathers).  Payload rows are random bytes -- any 64 bits are a generator state, and ray rows are compared as uint32,
so NaN payloads take part.

Every buffer is PAD elements longer than n and filled with a sentinel behind element n; the payload outputs are filled
with it throughout, so that it must also survive behind element `count`; the scratch carries it behind the documented
size, the count behind its 8 bytes."""
import importlib
import itertools
import os
import re

import numpy as np
import pytest
import torch

import compact_ref as CR
import exact_scenes
import tree_build_scenes as S
from conftest import ROOT

pytestmark = pytest.mark.gpu

PAD = 64
SENTINEL = 0x5A
TILE = CR.TILE
ROW = {"rays": 36, "rng": 8, "slot": 4, "active_out": 1}
STATUSES = (-1, 0, 1, 2)  # INVALID, MISS, ENDED, SCATTERED
ALL = ("rays", "rng", "slot", "active_out")
PATTERNS = ("all", "none", "first", "last", "alternating", "tiles", "waves", "random_0.06", "random_0.5", "random_0.94")


def _scan_trip():
    """Tile counts the scan workgroup covers per trip (csrc/srt_launch.h)."""
    text = open(os.path.join(ROOT, "sexy-raytracer_amd", "csrc", "srt_launch.h")).read()
    return int(re.search(r"#define SRT_COMPACT_SCAN_BLOCK (\d+)", text).group(1))


@pytest.fixture(scope="module")
def pathloop(srt):
    return importlib.import_module("sexy-raytracer_amd.pathloop")


def _pattern(name, n, seed=0):
    i = np.arange(n)
    if name == "all":
        return np.ones(n, bool)
    if name == "none":
        return np.zeros(n, bool)
    if name == "first":
        return i == 0
    if name == "last":
        return i == n - 1
    if name == "alternating":
        return i % 2 == 1
    if name == "tiles":  # whole tiles empty, then full
        return (i // TILE) % 2 == 1
    if name == "waves":
        return (i // 64) % 3 == 1
    return np.random.default_rng(seed).random(n) < float(name.split("_")[1])


def _inputs(keep, seed, stale=True):
    """Random rows and a (status, mask) pair whose predicate is `keep`: the four status values are mixed, and (with stale)
    about half of the dropped entries are dropped by the mask alone, behind any status -- SCATTERED included."""
    n = len(keep)
    g = np.random.default_rng(seed)
    status = np.where(keep, 2, g.choice(STATUSES[:3], n)).astype(np.int32)
    active = np.where(keep, g.choice((1, 2, 255), n), 1).astype(np.uint8)
    if stale:
        masked = ~keep & (g.random(n) < 0.5)
        status[masked] = g.choice(STATUSES, int(masked.sum()))
        active[masked] = 0
    out = g.integers(0, 2 ** 32, (n, 8), dtype=np.uint32)
    out[:, 3] = status.view(np.uint32)
    return {"out": out, "status": status, "active": active,
            "rays": g.integers(0, 2 ** 32, (n, 9), dtype=np.uint32),  # NaNs among them
            "rng": g.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64),
            "slot": g.integers(-2 ** 31, 2 ** 31 - 1, n, dtype=np.int32)}


def _padded(rows, n, row_bytes, pad=PAD):
    """A device byte buffer of n + pad rows: `rows` (or the sentinel where None) in the first n, the sentinel behind."""
    buf = np.full((n + pad) * row_bytes, SENTINEL, np.uint8)
    if rows is not None and n:
        buf[:n * row_bytes] = np.ascontiguousarray(rows).view(np.uint8).ravel()
    return torch.from_numpy(buf).cuda()


def _run(dev, c, n, out=None, active=None, rays=None, rng=None, slot=None, want=ALL, in_place=False, stream=None):
    """One raw call on padded buffers.  Checks every sentinel and that no input changed; returns {count, rays, rng, slot
    (the first count rows as bytes), active_out (n bytes)} with None for what was not asked for."""
    handle = stream.cuda_stream if stream is not None else None
    given = {"out": (out, 32), "active": (active, 1), "rays": (rays, 36), "rng": (rng, 8), "slot": (slot, 4)}
    with torch.cuda.stream(stream):
        d_in = {k: _padded(v[:n], n, b) if v is not None else None for k, (v, b) in given.items()}
        before = {k: t.clone() for k, t in d_in.items() if t is not None}
        d_out = {k: _padded(None, n, ROW[k]) if k in want else None for k in ALL}
        if in_place and "active_out" in want:
            d_out["active_out"] = d_in["active"]
        d_count = _padded(None, 1, 8)
        need = dev.lib.srtCompactPathsScratchBytes(n)
        d_scratch = _padded(None, need // 8, 8)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        rc = dev.lib.srtCompactPathsDevice(c.h, n, ptr(d_in["out"]), ptr(d_in["active"]), ptr(d_in["rays"]), ptr(d_in["rng"]),
                                           ptr(d_in["slot"]), ptr(d_out["rays"]), ptr(d_out["rng"]), ptr(d_out["slot"]),
                                           ptr(d_out["active_out"]), ptr(d_count), ptr(d_scratch), handle)
        assert rc == 0, dev.lib.srtLastError(c.h)
    (stream or torch.cuda).synchronize()
    assert bool((d_scratch[need:] == SENTINEL).all()), "written beyond the documented scratch size"
    for k, t in d_in.items():
        if t is not None and not (in_place and k == "active"):
            assert torch.equal(t, before[k]), "input %s changed" % k
    count_bytes = d_count.cpu().numpy()
    assert (count_bytes[8:] == SENTINEL).all()
    if n == 0:
        assert (count_bytes == SENTINEL).all(), "n == 0 writes no count"
        count = 0
    else:
        count = int(count_bytes[:8].view(np.int64)[0])
        assert 0 <= count <= n
    got = {"count": count}
    for k in ALL:
        if d_out[k] is None:
            got[k] = None
            continue
        a = d_out[k].cpu().numpy()
        rows = n if k == "active_out" else count
        assert (a[rows * ROW[k]:] == SENTINEL).all(), "%s written beyond element %d" % (k, rows)
        got[k] = a[:rows * ROW[k]].copy()
    return got


def _assert_is_reference(got, ref, what=None):
    assert got["count"] == ref["count"], what
    for k, dtype in (("rays", np.uint32), ("rng", np.int64), ("slot", np.int32), ("active_out", np.uint8)):
        if got[k] is not None:
            assert ref[k] is not None and got[k].tobytes() == np.ascontiguousarray(ref[k], dtype).tobytes(), (what, k)


# ------------------------------------------------------------------------------------------------ 1. sizes and patterns
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_sizes_and_patterns(ctx, dev, n):
    seen = set()
    for k, name in enumerate(PATTERNS):
        keep = _pattern(name, n, seed=n + k)
        d = _inputs(keep, seed=1000 * k + n)
        assert np.array_equal(CR.keep(n, d["status"], d["active"]), keep)
        ref = CR.compact(n, d["status"], d["active"], d["rays"], d["rng"], d["slot"])
        got = _run(dev, ctx, n, d["out"], d["active"], d["rays"], d["rng"], d["slot"])
        _assert_is_reference(got, ref, (n, name))
        assert got["count"] == int(keep.sum())
        seen |= set(d["status"].tolist())
    if n >= 63:
        assert seen == set(STATUSES)  # the four status values are mixed


# ------------------------------------------------------------------------------------------------ 2. the stale status
def test_mask_decides_where_the_status_is_stale(ctx, dev):
    n = 2 * TILE + 77
    d = _inputs(np.zeros(n, bool), seed=3, stale=False)
    d["out"][:, 3] = 2  # SCATTERED everywhere: two thirds of it stale
    active = (np.arange(n) % 3 == 1).astype(np.uint8) * 9
    ref = CR.compact(n, d["out"][:, 3].view(np.int32), active, d["rays"], d["rng"])
    assert ref["count"] == int((active != 0).sum()) and n // 3 - 1 <= ref["count"] <= n // 3 + 1
    got = _run(dev, ctx, n, d["out"], active, d["rays"], d["rng"])
    _assert_is_reference(got, ref, "status and mask")
    # the mask alone: a caller's own predicate
    alone = _run(dev, ctx, n, None, active, d["rays"], d["rng"])
    _assert_is_reference(alone, CR.compact(n, None, active, d["rays"], d["rng"]), "mask alone")
    # and with another status under it the two differ
    status = _inputs(_pattern("random_0.5", n, 8), seed=4, stale=False)
    both = _run(dev, ctx, n, status["out"], active, d["rays"], d["rng"])
    _assert_is_reference(both, CR.compact(n, status["status"], active, d["rays"], d["rng"]), "both")
    assert 0 < both["count"] < alone["count"]
    # dActiveOut == dActive: the same bytes as out of place
    in_place = _run(dev, ctx, n, d["out"], active, d["rays"], d["rng"], in_place=True)
    for k in ("count",) + ALL:
        assert np.array_equal(in_place[k], got[k]), k
    in_place = _run(dev, ctx, n, None, active, None, None, want=("active_out",), in_place=True)
    assert in_place["active_out"].tobytes() == alone["active_out"].tobytes()


# ------------------------------------------------------------------------------------------------ 3. slots
def test_slots_carry_through_and_compose(ctx, dev):
    n = 3 * TILE + 5
    a = _inputs(_pattern("random_0.5", n, 1), seed=5)
    own = _run(dev, ctx, n, a["out"], a["active"], slot=a["slot"], want=("slot",))
    _assert_is_reference(own, CR.compact(n, a["status"], a["active"], slot=a["slot"]), "a caller's slots")
    identity = _run(dev, ctx, n, a["out"], a["active"], rng=a["rng"], want=("rng", "slot"))
    ref1 = CR.compact(n, a["status"], a["active"], rng=a["rng"])
    _assert_is_reference(identity, ref1, "identity")
    assert identity["slot"].view(np.int32).tolist() == np.flatnonzero(CR.keep(n, a["status"], a["active"])).tolist()
    # a second compaction of the survivors, the first one's slots carried: the slots name entries of the first buffer
    m = ref1["count"]
    b = _inputs(_pattern("random_0.5", m, 2), seed=6)
    second = _run(dev, ctx, m, b["out"], b["active"], rng=identity["rng"].view(np.int64), slot=identity["slot"].view(np.int32),
                  want=("rng", "slot"))
    ref2 = CR.compact(m, b["status"], b["active"], rng=ref1["rng"], slot=ref1["slot"])
    _assert_is_reference(second, ref2, "composition")
    composed = np.flatnonzero(CR.keep(n, a["status"], a["active"]))[np.flatnonzero(CR.keep(m, b["status"], b["active"]))]
    assert second["slot"].view(np.int32).tolist() == composed.tolist()
    assert second["rng"].tobytes() == a["rng"][composed].tobytes()


# ------------------------------------------------------------------------------------------------ 4. optional payloads
def test_every_subset_of_the_payloads(ctx, dev):
    n = TILE + 300
    d = _inputs(_pattern("random_0.5", n, 3), seed=7)
    ref = CR.compact(n, d["status"], d["active"], d["rays"], d["rng"], d["slot"])
    ref_identity = CR.compact(n, d["status"], d["active"])
    for size in range(len(ALL) + 1):
        for want in itertools.combinations(ALL, size):
            got = _run(dev, ctx, n, d["out"], d["active"], d["rays"], d["rng"], d["slot"], want=want)
            _assert_is_reference(got, ref, want)
            assert [k for k in ALL if got[k] is not None] == list(want)
    # inputs left out with their outputs; an input without an output is ignored; slots without an input are the identity
    got = _run(dev, ctx, n, d["out"], d["active"], None, d["rng"], None, want=("rng", "slot"))
    _assert_is_reference(got, dict(ref, slot=ref_identity["slot"]), "no rays, identity")
    got = _run(dev, ctx, n, d["out"], d["active"], None, None, None, want=())
    assert got["count"] == ref["count"]


# ------------------------------------------------------------------------------------------------ 5. one large n
def test_more_tiles_than_one_trip_of_the_scan(ctx, dev):
    trip = _scan_trip()
    n = (trip + 1) * TILE + 517  # one tile beyond a trip, and a ragged tail
    assert dev.lib.srtCompactPathsScratchBytes(n) == 8 * (trip + 2)
    g = np.random.default_rng(11)
    keep = g.random(n) < 0.5
    keep[(trip - 14) * TILE:(trip + 1) * TILE] = False  # a run of empty tiles across the trip boundary
    status = np.where(keep, 2, g.choice(STATUSES[:3], n)).astype(np.int32)
    active = np.ones(n, np.uint8)
    stale = ~keep & (g.random(n) < 0.5)
    status[stale], active[stale] = 2, 0
    out = np.zeros((n, 8), np.int32)
    out[:, 3] = status
    rng = g.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64)
    got = _run(dev, ctx, n, out, active, rng=rng, want=("rng", "slot", "active_out"))
    ref = CR.compact(n, status, active, rng=rng)
    assert ref["count"] == int(keep.sum()) and keep[:(trip - 14) * TILE].any() and keep[(trip + 1) * TILE:].any()
    _assert_is_reference(got, ref, "large")


# ------------------------------------------------------------------------------------------------ 6. a side stream
def test_call_runs_behind_the_op_that_made_the_rays(ctx, dev):
    n = 64 * TILE + 9
    d = _inputs(_pattern("random_0.5", n, 4), seed=9)
    rays = np.random.default_rng(10).random((n, 9), dtype=np.float32)
    moved = rays + np.float32(0.75)
    ref = CR.compact(n, d["status"], d["active"], moved.view(np.uint32), d["rng"])
    side = torch.cuda.Stream()
    d_rays, d_out, d_active, d_rng = (torch.from_numpy(a).cuda() for a in (rays, d["out"].view(np.int32), d["active"], d["rng"]))
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d_rays += 0.75
        rays_out, rng_out, slot_out, active_out, count = ctx.compact_paths_device(out=d_out, active=d_active, rays=d_rays, rng=d_rng,
                                                                                  active_out=True, stream=side)
    side.synchronize()
    assert count.dim() == 0 and count.dtype == torch.int64 and count.is_cuda
    m = int(count)
    assert m == ref["count"]
    assert rays_out[:m].cpu().numpy().view(np.uint32).tobytes() == ref["rays"].tobytes()
    assert rng_out[:m].cpu().numpy().tobytes() == ref["rng"].tobytes()
    assert slot_out[:m].cpu().numpy().tobytes() == ref["slot"].tobytes()
    assert active_out.cpu().numpy().tobytes() == ref["active_out"].tobytes()
    torch.cuda.synchronize()
    # the wrapper on nothing
    empty = ctx.compact_paths_device(out=torch.zeros((0, 8), dtype=torch.int32, device="cuda"))
    assert int(empty[4]) == 0 and empty[0] is None and tuple(empty[2].shape) == (0,)


# ------------------------------------------------------------------------------------------------ 7. the loop is the loop
def _same_image(a, b, what):
    a, b = a.cpu().numpy(), (b.cpu().numpy() if hasattr(b, "cpu") else b)
    assert a.shape == b.shape
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan), what
    assert np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]), what


def _assert_compacted_loop_is_the_loop_and_the_render(ctx, pathloop, p, what):
    want = ctx.render_image(p, want_rgba=False)[0]
    counts = {}
    for fused in (True, False):
        for compact in (False, True):
            counts[fused, compact] = []
            got = pathloop.render(ctx, p, fused=fused, compact=compact, active_counts=counts[fused, compact])
            torch.cuda.synchronize()
            _same_image(got, want, (what, fused, compact))
            if compact:
                _same_image(got, plain, (what, fused, "against the uncompacted loop"))
            else:
                plain = got
    numbers = {k: [int(c) for c in v] for k, v in counts.items()}
    assert numbers[True, True] == numbers[True, False] == numbers[False, True] == numbers[False, False], what
    assert len(numbers[True, True]) == p.maxBounce and numbers[True, True][0] == p.imageWidth * p.imageHeight * p.spp
    return numbers[True, True]


@pytest.mark.parametrize("tier", exact_scenes.TIERS)
def test_compacted_loop_on_exact_scenes(ctx, abi, camera, pathloop, tier):
    ctx.upload_scene(exact_scenes.random(abi, 0, tier))
    ctx.set_camera(camera)
    for bounces in (1, 4, 16):
        p = abi.default_render_params(32, 24, 4, bounces, seed=11)
        _assert_compacted_loop_is_the_loop_and_the_render(ctx, pathloop, p, (tier, bounces))
    p = abi.default_render_params(32, 24, 4, 4, seed=11)
    for fused in (True, False):
        whole = pathloop.render(ctx, p, fused=fused, compact=True)
        parts = pathloop.render(ctx, p, fused=fused, compact=True, samples_per_batch=3)
        assert torch.equal(whole.view(torch.int32), parts.view(torch.int32))


def test_compacted_loop_on_masterchief(ctx, srt, abi, camera, pathloop):
    ctx.upload_scene(srt.scenes.SCENES["masterchief"]())
    ctx.set_camera(camera)
    p = abi.default_render_params(64, 36, 2, 8, seed=5)
    live = _assert_compacted_loop_is_the_loop_and_the_render(ctx, pathloop, p, "masterchief")
    assert 0 < live[2] < live[0] // 2  # the set really shrinks: below half by the third bounce


# ------------------------------------------------------------------------------------------------ 8. side effects, errors
def test_side_effects_and_errors(ctx, dev, abi, camera):
    ctx.upload_scene(S.soup(abi, 3000, abi.SRT_BUILDER_PLOC))
    ctx.set_camera(camera)
    p = abi.default_render_params(64, 36, 2, 4, seed=5)
    first = ctx.render_image(p)[0]
    info, ms, stats = ctx.launch_info(), ctx.last_kernel_ms(), ctx.stats()
    n = 2 * TILE + 40
    d = _inputs(_pattern("random_0.5", n, 5), seed=12)
    ref = CR.compact(n, d["status"], d["active"], d["rays"], d["rng"], d["slot"])
    _assert_is_reference(_run(dev, ctx, n, d["out"], d["active"], d["rays"], d["rng"], d["slot"]), ref, "good call")
    assert (ctx.launch_info(), ctx.last_kernel_ms(), ctx.stats()) == (info, ms, stats)
    assert ctx.render_image(p)[0].tobytes() == first.tobytes()
    # no scene uploaded is not an error
    fresh = dev.Context(0)
    try:
        _assert_is_reference(_run(dev, fresh, n, d["out"], d["active"], d["rays"], d["rng"], d["slot"]), ref, "no scene")
    finally:
        fresh.close()

    # errors: refused on the host, nothing launched, the outputs keep their sentinel.  Every address below is either NULL
    # or inside a live buffer: a misaligned pointer is a live buffer's address plus a few bytes.
    ins = {k: _padded(d[k], n, b) for k, b in (("out", 32), ("active", 1), ("rays", 36), ("rng", 8), ("slot", 4))}
    outs = {k: _padded(None, n, ROW[k]) for k in ALL}
    outs["count"] = _padded(None, 1, 8)
    outs["scratch"] = _padded(None, dev.lib.srtCompactPathsScratchBytes(n) // 8, 8)
    O, A, R, G, SL = (ins[k].data_ptr() for k in ("out", "active", "rays", "rng", "slot"))
    RO, GO, SO, AO, CN, SC = (outs[k].data_ptr() for k in ("rays", "rng", "slot", "active_out", "count", "scratch"))
    assert all(a % 16 == 0 for a in (O, A, R, G, SL, RO, GO, SO, AO, CN, SC))
    call = dev.lib.srtCompactPathsDevice

    def refused(rc, text):
        assert rc != 0 and text in dev.lib.srtLastError(ctx.h), (rc, text, dev.lib.srtLastError(ctx.h))
        torch.cuda.synchronize()
        for buf in outs.values():
            assert bool((buf == SENTINEL).all())

    refused(call(ctx.h, -1, O, A, R, G, SL, RO, GO, SO, AO, CN, SC, None), b"negative")
    refused(call(ctx.h, n, None, None, R, G, SL, RO, GO, SO, AO, CN, SC, None), b"no predicate")
    refused(call(ctx.h, n, O, A, R, G, SL, RO, GO, SO, AO, None, SC, None), b"null count")
    refused(call(ctx.h, 0, O, A, R, G, SL, RO, GO, SO, AO, None, SC, None), b"null count")
    refused(call(ctx.h, n, O, A, R, G, SL, RO, GO, SO, AO, CN, None, None), b"null scratch")
    refused(call(ctx.h, n, O, A, None, G, SL, RO, GO, SO, AO, CN, SC, None), b"rays without rays")
    refused(call(ctx.h, n, O, A, R, None, SL, RO, GO, SO, AO, CN, SC, None), b"rng states without rng states")
    refused(call(ctx.h, n, O + 8, A, R, G, SL, RO, GO, SO, AO, CN, SC, None), b"outputs are not aligned to 16")
    refused(call(ctx.h, n, O, A, R + 2, G, SL, RO, GO, SO, AO, CN, SC, None), b"rays are not aligned to 4")
    refused(call(ctx.h, n, O, A, R, G, SL, RO + 2, GO, SO, AO, CN, SC, None), b"rays are not aligned to 4")
    refused(call(ctx.h, n, O, A, R, G + 4, SL, RO, GO, SO, AO, CN, SC, None), b"rng states are not aligned to 8")
    refused(call(ctx.h, n, O, A, R, G, SL, RO, GO + 4, SO, AO, CN, SC, None), b"rng states are not aligned to 8")
    refused(call(ctx.h, n, O, A, R, G, SL + 2, RO, GO, SO, AO, CN, SC, None), b"slots are not aligned to 4")
    refused(call(ctx.h, n, O, A, R, G, SL, RO, GO, SO + 2, AO, CN, SC, None), b"slots are not aligned to 4")
    refused(call(ctx.h, n, O, A, R, G, SL, RO, GO, SO, AO, CN + 4, SC, None), b"count are not aligned to 8")
    refused(call(ctx.h, n, O, A, R, G, SL, RO, GO, SO, AO, CN, SC + 4, None), b"scratch are not aligned to 8")
    refused(call(ctx.h, 2 ** 31, O, A, None, None, None, None, None, SO, None, CN, SC, None), b"32-bit slot")
    # overlap: in place, shifted, an output on another output, on the count, on the scratch, on a predicate
    refused(call(ctx.h, n, O, A, R, G, SL, R, GO, SO, AO, CN, SC, None), b"compacted rays overlap the rays")
    refused(call(ctx.h, n, O, A, R, G, SL, RO, G, SO, AO, CN, SC, None), b"compacted rng states overlap the rng states")
    refused(call(ctx.h, n, O, A, R, G, SL, RO, GO, SL, AO, CN, SC, None), b"compacted slots overlap the slots")
    refused(call(ctx.h, n, O, A, R, G, SL, R + 36 * (n - 1), GO, SO, AO, CN, SC, None), b"compacted rays overlap the rays")
    refused(call(ctx.h, n // 2, O, A, R, G, SL, RO, RO + 8 * (n // 2 - 1), SO, AO, CN, SC, None), b"compacted rays overlap the compacted rng states")
    refused(call(ctx.h, n // 8, O, A, R, G, SL, RO, GO, SO, AO, GO + 8, SC, None), b"compacted rng states overlap the count")
    refused(call(ctx.h, n // 8, O, A, R, G, SL, RO, GO, SO, AO, CN, SO + 8, None), b"compacted slots overlap the scratch")
    refused(call(ctx.h, n // 8, O, A, R, G, SL, RO, GO, SO, AO, SC, SC, None), b"count overlap the scratch")
    refused(call(ctx.h, n, O, A, R, G, SL, RO, GO, SO, O, CN, SC, None), b"compacted mask overlap the outputs")
    refused(call(ctx.h, n, O, A, R, G, SL, RO, GO, A, AO, CN, SC, None), b"compacted slots overlap the mask")
    refused(call(ctx.h, n - 1, O, A, R, G, SL, RO, GO, SO, A + 1, CN, SC, None), b"compacted mask overlap the mask")  # a shifted mask is not in place
    refused(call(ctx.h, n, O, A, R, G, SL, RO, GO, SO, AO, CN, O, None), b"scratch overlap the outputs")
    assert call(None, n, O, A, R, G, SL, RO, GO, SO, AO, CN, SC, None) != 0
    # an input whose output is NULL is ignored, overlaps and misalignment included
    assert call(ctx.h, n, O, A, RO + 2, GO + 4, SO + 2, None, None, None, None, CN, SC, None) == 0, dev.lib.srtLastError(ctx.h)
    torch.cuda.synchronize()
    assert int(outs["count"].cpu().numpy()[:8].view(np.int64)[0]) == ref["count"]
    for k in ALL:
        assert bool((outs[k] == SENTINEL).all())
    for k, t in ins.items():
        assert t.cpu().numpy()[:n * (32 if k == "out" else ROW.get(k, 1))].tobytes() == np.ascontiguousarray(d[k]).tobytes()
    with pytest.raises(dev.SrtError, match="compacted rays overlap the rays"):
        both = torch.zeros((n, 9), dtype=torch.float32, device="cuda")
        ctx.compact_paths_device(active=ins["active"][:n], rays=both, rays_out=both)
