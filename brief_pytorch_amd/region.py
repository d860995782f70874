"""Boxes of a decode grid: what a region of interest, a strided preview or a resampled view asks the forward kernel for.

A region is a numpy basic slice of the spatial axes (start:stop:step per axis, steps >= 1, bounds inside the grid).  It becomes the
(start, step, extent) triple of brief_grid_box (include/brief_hip.h); everything here is host arithmetic, no device work."""
import numpy as np


def parse_region(text):
    """'z0:z1,y0:y1,x0:x1' (or 'y0:y1,x0:x1' for 2-D data; a part may be ':', 'a:', ':b' or 'a:b:s') -> tuple of slices"""
    out = []
    for part in text.split(","):
        f = part.strip().split(":")
        if len(f) not in (2, 3):
            raise ValueError("region part %r is not start:stop or start:stop:step" % part)
        try:
            v = [int(x) if x.strip() else None for x in f]
        except ValueError:
            raise ValueError("region part %r holds a non-integer bound" % part) from None
        out.append(slice(*v))
    return tuple(out)


def parse_shape(text):
    """'D,H,W' -> list of ints >= 1"""
    try:
        dims = [int(x) for x in text.split(",")]
    except ValueError:
        raise ValueError("shape %r is not a comma-separated list of integers" % text) from None
    if any(d < 1 for d in dims):
        raise ValueError("shape %r has an axis below 1" % text)
    return dims


def _per_axis(v, nd, what):
    if v is None or np.isscalar(v):
        return [v] * nd
    v = list(v)
    if len(v) != nd:
        raise ValueError("%s has %d entries for %d spatial axes" % (what, len(v), nd))
    return v


def normalize_region(dims, region, step=1):
    """(dims, region as a tuple of slices, default step) -> (start, stop, step) lists, one entry per spatial axis.

    numpy slice semantics with nothing clipped: a missing start / stop is 0 / the axis length, an explicit one must lie in
    [0, dims] and give a non-empty range; steps are integers >= 1 (a slice's own step overrides `step`).  Anything else raises
    ValueError."""
    dims = [int(d) for d in dims]
    nd = len(dims)
    if isinstance(region, str):
        region = parse_region(region)
    if isinstance(region, slice):
        region = (region,)
    region = tuple(region)
    if len(region) != nd:
        raise ValueError("region has %d axes, the grid %d" % (len(region), nd))
    steps = _per_axis(step, nd, "step")
    start, stop, stp = [], [], []
    for a, (s, n) in enumerate(zip(region, dims)):
        if not isinstance(s, slice):
            raise ValueError("region axis %d is not a slice" % a)
        st = steps[a] if s.step is None else s.step
        b = 0 if s.start is None else s.start
        e = n if s.stop is None else s.stop
        for v, what in ((st, "step"), (b, "start"), (e, "stop")):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError("region axis %d: %s %r is not an integer" % (a, what, v))
        if st < 1:
            raise ValueError("region axis %d: step %d (steps must be >= 1)" % (a, st))
        if not (0 <= b <= n and 0 <= e <= n):
            raise ValueError("region axis %d: %d:%d lies outside 0:%d" % (a, b, e, n))
        if e <= b:
            raise ValueError("region axis %d: %d:%d is empty" % (a, b, e))
        start.append(int(b)); stop.append(int(e)); stp.append(int(st))
    return start, stop, stp


def extents(start, stop, step):
    """voxels per axis of a normalised region: len(range(start, stop, step))"""
    return [(e - b + s - 1) // s for b, e, s in zip(start, stop, step)]


def block_intersection(start, step, extent, lo, hi):
    """the part of a strided region that falls inside one block of a partition (inclusive grid range [lo, hi] per axis).

    Returns None when they do not meet, else (out_lo, out_hi, local_start, local_stop): the region's box indices
    [out_lo, out_hi) the block supplies, and the block-local slice start:stop (with the region's step) that yields them.
    The samples stay on the region's lattice start + step * i, so the stride is continuous across block faces."""
    out_lo, out_hi, l_start, l_stop = [], [], [], []
    for b, s, n, bl, bh in zip(start, step, extent, lo, hi):
        i0 = max(0, -((b - bl) // s))               # first i with b + s i >= bl  (ceil division)
        i1 = min(n - 1, (bh - b) // s) if bh >= b else -1
        if i0 > i1:
            return None
        out_lo.append(i0); out_hi.append(i1 + 1)
        l_start.append(b + s * i0 - bl); l_stop.append(b + s * i1 - bl + 1)
    return out_lo, out_hi, l_start, l_stop
