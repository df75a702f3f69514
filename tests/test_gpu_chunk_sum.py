"""The exact chunk sum (csrc/srt_path.h toFixed36 / commitFixed / fromFixed36; srt_sum_chunks_kernel, srt_finalize_kernel)
on caller-made partial sums, through srtTestChunkSum, against the integer reference tests/chunk_sum_ref.py.  Every
comparison is on bits (any NaN equals any NaN); both paths on every case, path 0 and path 1 bit-identical throughout.

A case is a ROW: one channel's slot values, `chunks` of them.  A launch lays R rows out as R pixels whose channel k holds row
(i - k) mod R, so every row is summed in each of the three channels, beside two other rows: a channel mix-up, or a
non-finite channel leaking into its neighbours, shows.  The slot counts in w differ from slot to slot."""
import functools
import itertools

import numpy as np
import pytest

import chunk_sum_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
SAMPLES = 77  # path 1's w


def lay_out(rows):
    """(R, chunks) rows -> slots (chunks, R, 4): channel k of pixel i = row (i - k) mod R, w = 1 + (c + i) % 3."""
    rows = np.asarray(rows, F)
    n, chunks = rows.shape
    slots = np.zeros((chunks, n, 4), F)
    for k in range(3):
        slots[:, :, k] = np.roll(rows, k, axis=0).T
    slots[:, :, 3] = 1 + (np.arange(chunks)[:, None] + np.arange(n)[None, :]) % 3
    return slots


def check_rows(ctx, rows, want=None, ref=None):
    """Both paths on the rows laid out over the channels against the reference's per-row sums (ref: those, where the
    caller has them already); want: (R,) answers stated by the test, which the reference must agree with first.
    Returns path 0's (R, 4)."""
    rows = np.asarray(rows, F)
    n, chunks = rows.shape
    ref = R.rows_sum(rows, chunks) if ref is None else ref
    if want is not None:
        assert R.same_bits(ref, want).all(), "the reference disagrees with the stated answers"
    slots = lay_out(rows)
    got = [ctx.chunk_sum_test(slots, path, SAMPLES) for path in (0, 1)]
    for path, g in enumerate(got):
        for k in range(3):
            ok = R.same_bits(g[:, k], np.roll(ref, k))
            bad = np.flatnonzero(~ok)
            assert ok.all(), "path %d channel %d: %d of %d rows differ; first: slots %r -> %r, want %r" % (
                path, k, len(bad), n, np.roll(rows, k, axis=0)[bad[0]][:8], g[bad[0], k], np.roll(ref, k)[bad[0]])
    assert R.same_bits(got[0][:, :3], got[1][:, :3]).all()
    counts = np.zeros(n, F)
    for c in range(chunks):
        counts = (counts + slots[c, :, 3]).astype(F)
    assert np.array_equal(got[0][:, 3], counts) and (got[1][:, 3] == F(SAMPLES)).all()
    return got[0]


def test_the_sum_is_rounded_once(ctx):
    """Sums of 2^17 .. 2^25 that sit half a float ulp, plus or minus one unit of 2^-36, from a float: one ulp above 2^e
    where the exact sum is just above the tie, down to the odd mantissa where it is just below; both signs, all six slot
    orders; and the exact ties beside them, to even.  A conversion of the integer sum through double rounds twice and
    misses every row of the first set by one ulp (tests/test_chunk_sum_ref.py shows that on the CPU)."""
    rows, want = R.double_rounding_rows()
    check_rows(ctx, rows, want)
    rows, want = R.tie_rows()
    check_rows(ctx, rows, want)


def all_bits_set(lim):
    """Floats with all 24 mantissa bits set, at every exponent from 2^-13 up to the limit."""
    out, e = [], -13
    while float(2 ** 24 - 1) * 2.0 ** (e - 23) < lim:
        out.append(float(2 ** 24 - 1) * 2.0 ** (e - 23))
        e += 1
    assert out[-1] == float(np.nextafter(F(lim), F(0)))
    return out


def test_conversion_to_fixed_point(ctx):
    """toFixed36 at its edges, three slots (limit 2^24): the unit, what truncates to zero (and comes out +0.0), the
    truncation below 2^-13, cancellation that leaves a small term exactly, full mantissas at every exponent."""
    u = 2.0 ** -36
    tiny = [2.0 ** -37, -(2.0 ** -37), 0.0, -0.0, 1e-40, -1e-40, float(np.nextafter(F(0), F(1))), 2.0 ** -126, 0.99 * u]
    rows, want = [], []

    def add(row, w):
        rows.append(row)
        want.append(w)
    add([u, 0.0, 0.0], u)
    add([-u, 0.0, -0.0], -u)
    for t in tiny:
        add([t, 0.0, 0.0], 0.0)   # q = 0: +0.0, also for -0.0 and -2^-37
        add([t, t, t], 0.0)
        add([t, 1024.0, -1024.0], 0.0)
        add([1.0, t, u], 1.0)     # 1 + 2^-36 rounds to 1
    add([-0.0, -0.0, -0.0], 0.0)
    add([1.5 * u, 1.5 * u, 1.5 * u], 3 * u)  # each truncates to one unit: 3, not 4.5
    add([-1.5 * u, -1.5 * u, 0.0], -2 * u)    # towards zero
    for v in (float(np.nextafter(F(2.0 ** -12), F(0))), 2.0 ** -12, float(np.nextafter(F(2.0 ** -12), F(1))), 2.0 ** -13):
        add([v, 0.0, 0.0], v)                 # an ulp of 2^-36 or more: exact
        add([-v, 0.0, 0.0], -v)
    below = float(np.nextafter(F(2.0 ** -13), F(0)))  # (2^24 - 1) 2^-37: the last bit is half a unit and is dropped
    add([below, 0.0, 0.0], below - 2.0 ** -37)
    add([-below, 0.0, 0.0], -(below - 2.0 ** -37))
    add([below, below, 0.0], 2 * (below - 2.0 ** -37))
    for o in itertools.permutations([2.0 ** 20, -(2.0 ** 20), 2.0 ** -30]):
        add(list(o), 2.0 ** -30)
    for v in all_bits_set(R.limit(3)):
        add([v, 0.0, 0.0], v)
        add([-v, 0.0, -0.0], -v)
        add([v, v, -v], v)
        add([v, -v, u], u)
    got = check_rows(ctx, rows, np.array(want, F))
    # +0.0, not -0.0, wherever the sum is zero (same_bits has compared the sign bit already; said once more in the open)
    zero = np.array(want, F) == 0
    assert zero.sum() > 20 and not np.signbit(got[zero, 0]).any()


def test_640_slots_truncate_one_by_one(ctx):
    """640 slots (the default plan's cap, limit 2^16) of 1.5 * 2^-36 sum to 640 units, not 960; full mantissas up to that
    limit; and slots just below the limit everywhere."""
    u = 2.0 ** -36
    lim = R.limit(640)
    assert lim == 2.0 ** 16
    rows = [[1.5 * u] * 640, [-1.5 * u] * 640, [1.5 * u] * 639 + [-0.0]]
    want = [640 * u, -640 * u, 639 * u]
    for v in all_bits_set(lim):
        rows.append([v] + [0.0] * 639)
        want.append(v)
        rows.append([0.0] * 320 + [-v] + [u] * 319)
        want.append(None)  # -v + 319 units, rounded: the reference's
    ref = R.rows_sum(np.array(rows, F), 640)
    check_rows(ctx, rows, np.array([r if w is None else w for r, w in zip(ref, want)], F), ref)


RANGE_CHUNKS = (1, 2, 3, 4, 5, 64, 65, 640)


@functools.lru_cache(maxsize=None)
def range_rows(chunks):
    """Rows at the range rule of `chunks` chunks, finite rows between the non-finite ones (so that every non-finite row
    has finite rows in the other two channels of its pixels)."""
    rng = np.random.default_rng(100 + chunks)
    lim = R.limit(chunks)
    b = float(np.nextafter(F(lim), F(0)))

    def finite():
        return list((np.exp2(rng.uniform(-20.0, np.log2(lim), chunks)) * rng.choice([-1.0, 1.0], chunks)).astype(F).clip(-b, b))

    def with_at(base, **at):
        r = list(base)
        for pos, v in at.items():
            r[{"first": 0, "last": chunks - 1, "mid": chunks // 2}[pos]] = v
        return r
    rows, kinds = [], []

    def add(row, kind):
        rows.extend([row, finite(), finite()])
        kinds.extend([kind, "finite", "finite"])
    add([b] * chunks, "finite")    # chunks * (limit - ulp): the largest sum there is; no wrap
    add([-b] * chunks, "finite")
    for pos in ("first", "mid", "last"):
        add(with_at([b] * chunks, **{pos: lim}), "+inf")
        add(with_at([-b] * chunks, **{pos: -lim}), "-inf")
        add(with_at(finite(), **{pos: lim}), "+inf")
        add(with_at(finite(), **{pos: -lim}), "-inf")
        for v, kind in ((np.nan, "nan"), (-np.nan, "nan"), (np.inf, "+inf"), (-np.inf, "-inf"), (3e38, "+inf"), (-3e38, "-inf")):
            add(with_at(finite(), **{pos: v}), kind)
    if chunks >= 2:  # (one slot cannot hold both)
        add(with_at([b] * chunks, first=lim, last=-lim), "nan")
        add(with_at(finite(), first=-lim, last=lim), "nan")
        add(with_at(finite(), first=np.inf, last=-3e38), "nan")
        add(with_at(finite(), first=np.nan, last=lim), "nan")
    return np.array(rows, F), tuple(kinds)


@pytest.mark.parametrize("chunks", RANGE_CHUNKS)
def test_range_rule_and_flags(ctx, chunks):
    """limit = 2^26 / pow2(chunks): every slot one ulp below it gives the finite, correctly rounded sum (no wrap); a slot
    exactly at it +inf, at minus it -inf, one of each NaN; NaN, +-inf and +-3e38 slots; and the two finite channels beside
    a non-finite one keep their sums."""
    rows, kinds = range_rows(chunks)
    lim = R.limit(chunks)
    b = float(np.nextafter(F(lim), F(0)))
    want = R.rows_sum(rows, chunks)
    # the stated answers, independent of the reference's flag logic
    for kind, w in zip(kinds, want):
        assert {"finite": np.isfinite(w), "+inf": w == np.inf, "-inf": w == -np.inf, "nan": np.isnan(w)}[kind], (kind, w)
    # chunks * (limit - ulp) has at most 34 bits: exact in double, so the narrowing is the one rounding
    assert want[0] == F(np.float64(chunks) * np.float64(b)) and want[3] == -want[0] and want[0] > F(0.99 * chunks * lim)
    got = check_rows(ctx, rows, ref=want)
    # a pixel with exactly one non-finite channel exists for every non-finite row, and its other channels are finite
    fin = np.isfinite(got[:, :3])
    assert ((~fin).sum(axis=1) == 1).sum() == 3 * sum(k != "finite" for k in kinds) and ((~fin).sum(axis=1) <= 1).all()


@functools.lru_cache(maxsize=None)
def random_rows(chunks):
    rng = np.random.default_rng(200 + chunks)
    n = {2: 2048, 3: 2048, 7: 1024, 64: 256, 640: 48}[chunks]
    lim = R.limit(chunks)
    b = np.nextafter(F(lim), F(0))
    rows = (np.exp2(rng.uniform(-40.0, np.log2(lim), (n, chunks))) * rng.choice([-1.0, 1.0], (n, chunks))).astype(F).clip(-b, b)
    rows[rng.random(rows.shape) < 0.02] = 0.0
    for i in rng.choice(n, n // 10, replace=False):  # a few non-finite values, sprinkled
        for _ in range(int(rng.integers(1, 3))):
            rows[i, rng.integers(chunks)] = rng.choice(np.array([np.nan, np.inf, -np.inf, lim, -lim, 3e38], F))
    return rows


@pytest.mark.parametrize("chunks", (2, 3, 7, 64, 640))
def test_random_slots_and_their_permutations(ctx, chunks):
    """Seeded random slots, log-uniform magnitudes in [2^-40, limit), mixed signs, a few non-finite ones: the reference's
    bits, and the same bits for a permutation of every pixel's slots."""
    rows = random_rows(chunks)
    ref = R.rows_sum(rows, chunks)
    a = check_rows(ctx, rows, ref=ref)
    perm = np.random.default_rng(300 + chunks).permuted(rows, axis=1)
    assert not np.array_equal(perm.view(np.uint32), rows.view(np.uint32))
    b = check_rows(ctx, perm, ref=ref)  # integer addition commutes: the reference's sums are the rows'
    assert R.same_bits(a[:, :3], b[:, :3]).all()
    assert np.isfinite(a[:, :3]).mean() > 0.7 and (~np.isfinite(a[:, :3])).any()


def test_argument_errors(ctx, dev):
    import ctypes as C
    lib = dev.lib
    slots = np.zeros((2, 4, 4), F)
    out = np.zeros((4, 4), F)

    def call(h=None, n=4, chunks=2, path=0, src=slots.ctypes.data, dst=out.ctypes.data):
        return lib.srtTestChunkSum(ctx.h if h is None else h, src, n, chunks, path, 1, dst)
    assert call() == 0
    for kw, text in ((dict(n=0), "n = 0"), (dict(n=-3), "n = -3"), (dict(chunks=0), "chunks = 0"), (dict(chunks=-1), "chunks = -1"),
                     (dict(chunks=30813), "30813 chunks"), (dict(path=2), "path 2"), (dict(path=-1), "path -1"),
                     (dict(src=None), "null slots"), (dict(dst=None), "null output")):
        assert call(**kw) != 0, kw
        assert text in lib.srtLastError(ctx.h).decode(), (kw, lib.srtLastError(ctx.h))
    assert lib.srtTestChunkSum(None, slots.ctypes.data, 4, 2, 0, 1, out.ctypes.data) != 0
    assert dev.plan_spp_chunks(1, 1, 30812, 30812) == 30812 and dev.plan_spp_chunks(1, 1, 30813, 30813) == -1
    with pytest.raises(dev.SrtError):
        ctx.chunk_sum_test(np.zeros((2, 4, 4), F), 5)
    assert call() == 0  # the context is still good
