"""srtSortPathsDevice (include/srt_hip.h) stated in NumPy: compact_ref's predicate (here with neither part required), the
key in float32 step by step, np.argsort(kind="stable") and row gathers."""
import numpy as np

import compact_ref as CR

MAX_CELL_BITS = 9  # SRT_SORT_MAX_CELL_BITS


def keep(n, status=None, active=None):
    """compact_ref.keep, and everything where there is neither a status nor a mask."""
    return np.ones(n, bool) if status is None and active is None else CR.keep(n, status, active)


def cells(origin, lo, hi, cell_bits):
    """q of one axis: s = 2^bits / (hi - lo), c = (o - lo) * s, each a float32 operation of its own; q = 0 unless c >= 0,
    otherwise min(trunc(c), 2^bits - 1).  origin: float32 (n,); lo, hi: float32 scalars."""
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(all="ignore"):
        s = np.float32(1 << cell_bits) / np.float32(hi - lo)
        c = (np.asarray(origin, np.float32) - lo).astype(np.float32) * s
    assert c.dtype == np.float32
    last = (1 << cell_bits) - 1
    q = np.zeros(c.shape, np.uint32)
    inside = c >= 0  # False for a NaN
    big = inside & (c >= np.float32(last))  # +inf among them
    small = inside & ~big
    q[big] = last
    q[small] = np.trunc(c[small]).astype(np.uint32)
    return q


def spread3(q):
    """Bit k of q to bit 3k, for the low 10 bits (the usual shift-and-mask ladder; tests/test_sort_abi.py checks it bit by bit)."""
    q = np.asarray(q, np.uint32)
    for shift, mask in ((16, 0x030000ff), (8, 0x0300f00f), (4, 0x030c30c3), (2, 0x09249249)):
        q = (q | (q << np.uint32(shift))) & np.uint32(mask)
    return q


def dead_key(cell_bits):
    return 1 << (3 * cell_bits + 3)


def keys(rays, box, cell_bits, kept=None):
    """The 32-bit key of every entry.  rays: (n, 9), float32 or its bits as uint32; box: 6 float32 (lo.xyz, hi.xyz)."""
    assert 1 <= cell_bits <= MAX_CELL_BITS
    bits = np.ascontiguousarray(rays).view(np.uint32).reshape(-1, 9)
    rows = bits.view(np.float32)
    box = np.asarray(box, np.float32)
    cell = np.zeros(len(bits), np.uint32)
    octant = np.zeros(len(bits), np.uint32)
    for a in range(3):
        cell |= spread3(cells(rows[:, a], box[a], box[3 + a], cell_bits)) << np.uint32(a)
        octant |= (bits[:, 3 + a] >> np.uint32(31)) << np.uint32(a)
    key = cell << np.uint32(3) | octant
    if kept is not None:
        key = np.where(kept, key, np.uint32(dead_key(cell_bits)))
    return key.astype(np.uint32)


def origin_box(rays, kept=None):
    """What Context.sort_paths_device(box=None) makes: min and max over the kept origins (+inf, -inf without any)."""
    o = np.ascontiguousarray(rays).view(np.float32).reshape(-1, 9)[:, 0:3]
    if kept is not None:
        o = o[kept]
    if len(o) == 0:
        return np.array([np.inf] * 3 + [-np.inf] * 3, np.float32)
    return np.concatenate((o.min(0), o.max(0))).astype(np.float32)  # NumPy's min and max pass a NaN on, as torch's do


def sort(n, cell_bits, box, rays, status=None, active=None, rng=None, slot=None):
    """{count, index (the kept i in their stable order by key), key (every entry's), rays, rng, slot (the kept rows in
    that order; slot without one: the identity), active_out}.  Rows behind count are not written and not returned."""
    kept = keep(n, status, active)
    key = keys(np.asarray(rays)[:n], box, cell_bits, kept)
    order = np.argsort(key, kind="stable")
    count = int(kept.sum())
    index = order[:count]
    assert kept[index].all()
    return {"count": count, "index": index, "key": key,
            "rays": np.asarray(rays)[index],
            "rng": None if rng is None else np.asarray(rng)[index],
            "slot": index.astype(np.int32) if slot is None else np.asarray(slot, np.int32)[index],
            "active_out": (np.arange(n) < count).astype(np.uint8)}
