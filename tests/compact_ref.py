"""srtCompactPathsDevice (include/srt_hip.h) stated in NumPy: the predicate, np.flatnonzero and row gathers."""
import numpy as np

SCATTERED = 2  # SRT_PATH_SCATTERED
TILE = 1024    # SRT_COMPACT_TILE


def scratch_bytes(n, tile=TILE):
    """The documented formula: one 64-bit word per tile of `tile` entries."""
    return 0 if n <= 0 else 8 * -(-n // tile)


def keep(n, status=None, active=None):
    """keep[i] = (active is None or active[i] != 0) and (status is None or status[i] == SCATTERED)."""
    assert status is not None or active is not None
    k = np.ones(n, bool)
    if active is not None:
        k &= np.asarray(active)[:n] != 0
    if status is not None:
        k &= np.asarray(status)[:n] == SCATTERED
    return k


def compact(n, status=None, active=None, rays=None, rng=None, slot=None):
    """{count, index (the kept i, increasing), rays, rng, slot (the kept rows; slot without one: the identity), active_out}."""
    index = np.flatnonzero(keep(n, status, active))
    count = len(index)
    return {"count": count, "index": index,
            "rays": None if rays is None else np.asarray(rays)[index],
            "rng": None if rng is None else np.asarray(rng)[index],
            "slot": index.astype(np.int32) if slot is None else np.asarray(slot, np.int32)[index],
            "active_out": (np.arange(n) < count).astype(np.uint8)}
