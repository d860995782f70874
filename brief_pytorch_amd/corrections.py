"""Stored corrections of the error-bounded mode (Compress.error_bound): after the fit the stored artefact is decoded, every element
off by more than the bound gets a small correction, and every decode adds the corrections back, so max |x - x^| <= bound holds
exactly.  (DESIGN.md "Error-bounded mode"; kernels: csrc/brief_correct.inc.)

    m = 2 bound + 1,  d = x - y^ (integers),  q = floor((d + bound) / m)      q != 0 <=> |d| > bound,  |d - q m| <= bound
    decoder: clamp(y^ + q m, 0, type max)

quantise / write / read / select are host code (numpy); find / apply run on the device through libbrief_hip.so."""
import lzma
import os
import struct
import zlib

import numpy as np

MAGIC = b"BRIEFCOR"
VERSION = 1
FILE_NAME = "corrections.bin"
MAX_ELEMS = 1 << 40
CODECS = {"zlib": 0, "lzma": 1}
# header: magic, format version, bytes per element of the volume (1 uint8 | 2 uint16), codec, bytes per index gap (4 | 8), pad,
# bound, element count n of the volume the indices refer to, number of corrections K, packed length of the gap / the q stream
_HEADER = struct.Struct("<8sHBBBxxxIQQQQ")
_DTYPES = {1: np.dtype(np.uint8), 2: np.dtype(np.uint16)}
DEFAULT_CODEC = "lzma"


class CorrectionsError(RuntimeError):
    pass


def parse_bound(value):
    """Compress.error_bound -> None (off: absent, null, 'none') or a non-negative int (grey levels of the source dtype)"""
    if value is None or (isinstance(value, str) and value.strip().lower() in ("none", "null", "")):
        return None
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError("Compress.error_bound must be a non-negative integer (grey levels), null or none; got %r" % (value,))
    if value < 0 or value > 65535:
        raise ValueError("Compress.error_bound must lie in 0 .. 65535; got %d" % value)
    return int(value)


def path_for(module_path):
    """the corrections file of the artefact whose weights are at `module_path`: beside the `module` entry"""
    return os.path.join(os.path.dirname(module_path), FILE_NAME)


# ---- the definition (host restatement) ------------------------------------------------------------------------------------------
def quantise(d, bound):
    """q = floor((d + bound) / (2 bound + 1)) for integer differences d = x - y^ (numpy's // floors)"""
    bound = int(bound)
    if bound < 0:
        raise ValueError("bound must be >= 0")
    return (np.asarray(d).astype(np.int64) + bound) // (2 * bound + 1)


def find_host(dec, src, bound, base=0):
    """numpy restatement of find(): (ascending flat indices + base as int64, q as int32) of the elements off by more than bound"""
    q = quantise(np.asarray(src).reshape(-1).astype(np.int64) - np.asarray(dec).reshape(-1).astype(np.int64), bound)
    idx = np.flatnonzero(q)
    return idx.astype(np.int64) + int(base), q[idx].astype(np.int32)


def apply_host(out, idx, q, bound, base=0):
    """numpy restatement of apply(): a corrected copy of `out` (flat indices idx - base)"""
    res = np.array(out, copy=True)
    flat = res.reshape(-1)
    i = np.asarray(idx, np.int64) - int(base)
    v = flat[i].astype(np.int64) + np.asarray(q, np.int64) * (2 * int(bound) + 1)
    flat[i] = np.clip(v, 0, np.iinfo(res.dtype).max).astype(res.dtype)
    return res


# ---- device side ----------------------------------------------------------------------------------------------------------------
def _elem_bytes(t):
    import torch
    if t.dtype == torch.uint8:
        return 1
    if t.dtype == torch.uint16:
        return 2
    raise CorrectionsError("corrections exist for uint8 / uint16 volumes only (got %s)" % t.dtype)


def _flat_aligned(t):
    t = t.reshape(-1)
    if not t.is_contiguous() or t.data_ptr() % 16:
        t = t.clone(memory_format=__import__("torch").contiguous_format)
    return t


def find(dec_t, src_t, bound, base=0):
    """(idx int64, q int32) device tensors: the elements of the decoded tensor off by more than `bound` from the source, ascending,
    idx = base + flat index.  dec_t / src_t: device tensors of one dtype (uint8 | uint16) and size.  Two passes without atomics
    (brief_correct_count, a device cumsum, brief_correct_emit); the one host synchronisation reads K to size the output."""
    import torch
    from . import _lib
    eb = _elem_bytes(dec_t)
    if src_t.dtype != dec_t.dtype or src_t.numel() != dec_t.numel():
        raise CorrectionsError("corrections: decoded and source tensors differ in dtype or size (%s %d, %s %d)" % (
            dec_t.dtype, dec_t.numel(), src_t.dtype, src_t.numel()))
    if not dec_t.is_cuda or not src_t.is_cuda:
        raise _lib.BriefError("corrections.find runs on a ROCm GPU only; there is no CPU fallback (find_host restates it for tests)")
    bound, base, n = int(bound), int(base), dec_t.numel()
    dev = dec_t.device
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    a, b = _flat_aligned(dec_t), _flat_aligned(src_t)
    L = _lib.lib()
    per = int(L.brief_correct_chunk_elems(eb))
    counts = torch.empty((n + per - 1) // per, dtype=torch.int32, device=dev)
    _lib.check(L.brief_correct_count(_lib.ptr(a), _lib.ptr(b), eb, n, bound, base, _lib.ptr(counts), _lib.stream_ptr()))
    incl = torch.cumsum(counts, 0, dtype=torch.int64)
    offsets = incl - counts
    total = int(incl[-1].item())
    idx = torch.empty(total, dtype=torch.int64, device=dev)
    q = torch.empty(total, dtype=torch.int32, device=dev)
    _lib.check(L.brief_correct_emit(_lib.ptr(a), _lib.ptr(b), eb, n, bound, base, _lib.ptr(offsets), total, _lib.ptr(idx), _lib.ptr(q),
                                    _lib.stream_ptr()))
    return idx, q


def apply(out_t, idx, q, bound, base=0):
    """in place: out_t.flat[idx - base] = clamp(out_t.flat[idx - base] + q (2 bound + 1), 0, type max).  out_t: a contiguous device
    tensor (uint8 | uint16); idx / q: device tensors or numpy arrays (int64 / int32) of distinct indices in [base, base + numel)."""
    import torch
    from . import _lib
    eb = _elem_bytes(out_t)
    if not out_t.is_cuda:
        raise _lib.BriefError("corrections.apply runs on a ROCm GPU only; there is no CPU fallback (apply_host restates it for tests)")
    if not out_t.is_contiguous():
        raise CorrectionsError("corrections.apply needs a contiguous tensor")
    idx = torch.as_tensor(idx, dtype=torch.int64).to(out_t.device).contiguous()
    q = torch.as_tensor(q, dtype=torch.int32).to(out_t.device).contiguous()
    if idx.numel() != q.numel():
        raise CorrectionsError("corrections: %d indices, %d values" % (idx.numel(), q.numel()))
    if idx.numel() == 0 or out_t.numel() == 0:
        return out_t
    _lib.check(_lib.lib().brief_correct_apply(_lib.ptr(out_t), eb, out_t.numel(), _lib.ptr(idx), _lib.ptr(q), idx.numel(), int(bound), int(base),
                                              _lib.stream_ptr()))
    return out_t


def max_abs_diff(a_t, b_t):
    """max |a - b| of two integer device tensors as a Python int (slab by slab: the int32 temporaries stay small)"""
    import torch
    a, b = a_t.reshape(-1), b_t.reshape(-1)
    worst = 0
    for o in range(0, a.numel(), 1 << 26):
        d = a[o:o + (1 << 26)].to(torch.int32) - b[o:o + (1 << 26)].to(torch.int32)
        worst = max(worst, int(d.abs().max().item()))
    return worst


# ---- the file -------------------------------------------------------------------------------------------------------------------
def _shuffle(a):
    """byte planes of a little-endian integer array: all lowest bytes, then all second bytes, ... (the high planes of small
    numbers are runs of zeros)"""
    a = np.ascontiguousarray(a)
    return np.ascontiguousarray(a.view(np.uint8).reshape(a.size, a.dtype.itemsize).T).tobytes()


def _unshuffle(buf, dtype, count):
    dtype = np.dtype(dtype)
    if len(buf) != count * dtype.itemsize:
        raise CorrectionsError("corrections file: a stream of %d bytes where %d x %d were expected" % (len(buf), count, dtype.itemsize))
    planes = np.frombuffer(buf, np.uint8).reshape(dtype.itemsize, count)
    return np.ascontiguousarray(planes.T).view(dtype).reshape(count)


def _pack(raw, codec):
    if codec == "zlib":
        return zlib.compress(raw, 9)
    # a raw LZMA2 stream with fixed filters: no container header, the same bytes for the same input
    return lzma.compress(raw, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "preset": 6}])


def _unpack(buf, codec):
    if codec == "zlib":
        return zlib.decompress(buf)
    return lzma.decompress(buf, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "preset": 6}])


def encode(idx, q, bound, n, dtype, codec=DEFAULT_CODEC):
    """the bytes of a corrections file (see write)"""
    dtype = np.dtype(dtype)
    if dtype not in _DTYPES.values():
        raise CorrectionsError("corrections exist for uint8 / uint16 volumes only (got %s)" % dtype)
    if codec not in CODECS:
        raise ValueError("codec must be one of %s" % sorted(CODECS))
    bound, n = int(bound), int(n)
    if not 0 <= bound <= 65535 or not 0 <= n <= MAX_ELEMS:
        raise CorrectionsError("corrections: bound must be 0 .. 65535 and n 0 .. 2^40 (got %d, %d)" % (bound, n))
    idx = np.asarray(_to_numpy(idx), np.int64).reshape(-1)
    q = np.asarray(_to_numpy(q), np.int64).reshape(-1)
    if idx.size != q.size:
        raise CorrectionsError("corrections: %d indices, %d values" % (idx.size, q.size))
    gaps = np.diff(idx, prepend=np.int64(0))               # gap 0 is the first index itself
    if idx.size and (idx[0] < 0 or idx[-1] >= n or (gaps[1:] <= 0).any()):
        raise CorrectionsError("corrections: indices must be strictly ascending within 0 .. n - 1")
    if (q == 0).any() or (np.abs(q) > 65535).any():
        raise CorrectionsError("corrections: stored values are non-zero and at most 65535 in magnitude")
    gap_dt = np.dtype("<u4") if n < (1 << 32) else np.dtype("<u8")
    zz = ((q << 1) ^ (q >> 63)).astype("<u4")              # zigzag: small magnitudes of either sign -> small unsigned numbers
    s_gap, s_q = _pack(_shuffle(gaps.astype(gap_dt)), codec), _pack(_shuffle(zz), codec)
    return _HEADER.pack(MAGIC, VERSION, dtype.itemsize, CODECS[codec], gap_dt.itemsize, bound, n, idx.size, len(s_gap), len(s_q)) + s_gap + s_q


def write(path, idx, q, bound, n, dtype, codec=DEFAULT_CODEC):
    """corrections file: a self-describing header (magic, format version, dtype, bound, element count n, K), then the index gaps
    (32-bit when n < 2^32, else 64-bit) and the zigzag-coded q values as two byte-plane shuffled streams, each packed with a
    standard-library codec.  The bytes are a function of the arguments alone.  Returns the file's size."""
    blob = encode(idx, q, bound, n, dtype, codec)
    with open(path, "wb") as f:
        f.write(blob)
    return len(blob)


def read(path):
    """-> (idx int64, q int32, header dict) of a file written by write(); header: version, dtype, bound, n, count, codec, bytes"""
    with open(path, "rb") as f:
        blob = f.read()
    if len(blob) < _HEADER.size or blob[:8] != MAGIC:
        raise CorrectionsError("%s is not a corrections file" % path)
    _, version, eb, codec_id, gap_bytes, bound, n, count, len_gap, len_q = _HEADER.unpack_from(blob)
    codec = {v: k for k, v in CODECS.items()}.get(codec_id)
    if version != VERSION or eb not in _DTYPES or codec is None or gap_bytes not in (4, 8) or len(blob) != _HEADER.size + len_gap + len_q:
        raise CorrectionsError("%s: unsupported or damaged corrections file (version %d)" % (path, version))
    o = _HEADER.size
    gaps = _unshuffle(_unpack(blob[o:o + len_gap], codec), "<u4" if gap_bytes == 4 else "<u8", count)
    zz = _unshuffle(_unpack(blob[o + len_gap:], codec), "<u4", count).astype(np.int64)
    idx = np.cumsum(gaps.astype(np.int64), dtype=np.int64)
    q = ((zz >> 1) ^ -(zz & 1)).astype(np.int32)
    if count and idx[-1] >= n:
        raise CorrectionsError("%s: an index beyond the element count" % path)
    return idx, q, {"version": version, "dtype": _DTYPES[eb].name, "bound": int(bound), "n": int(n), "count": int(count), "codec": codec,
                    "bytes": len(blob)}


def _to_numpy(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else a


# ---- regions --------------------------------------------------------------------------------------------------------------------
def select(idx, q, dims, start, stop, step):
    """the corrections that fall on the box start:stop:step (one entry per axis of `dims`, numpy slice semantics, as
    region.normalize_region returns them) of an array of shape `dims` whose flat indices `idx` (ascending) refer to; returns
    (flat indices INTO THE BOX, q), still ascending.  The first axis is a range of the ascending indices (one searchsorted);
    the strided rest is a mask and an index remap."""
    idx, q = np.asarray(idx, np.int64), np.asarray(q)
    dims = [int(v) for v in dims]
    nd = len(dims)
    start, stop, step = ([int(v) for v in a] for a in (start, stop, step))
    if not (len(start) == len(stop) == len(step) == nd):
        raise ValueError("start / stop / step need one entry per axis of dims")
    ext = [(e - b + s - 1) // s for b, e, s in zip(start, stop, step)]
    plane = int(np.prod(dims[1:], dtype=np.int64)) if nd > 1 else 1
    last0 = start[0] + (ext[0] - 1) * step[0]              # the last index of axis 0 the box touches
    lo, hi = np.searchsorted(idx, [start[0] * plane, (last0 + 1) * plane])
    idx, q = idx[lo:hi], q[lo:hi]
    keep = np.ones(idx.size, bool)
    out = np.zeros(idx.size, np.int64)
    rem = idx
    coords = []
    for a in reversed(range(nd)):
        coords.append(rem % dims[a])
        rem = rem // dims[a]
    coords.reverse()
    for a in range(nd):
        rel = coords[a] - start[a]
        keep &= (rel >= 0) & (coords[a] < stop[a]) & (rel % step[a] == 0)
        out = out * ext[a] + rel // step[a]
    return out[keep], q[keep]


def select_range(idx, q, lo, hi):
    """the corrections with lo <= index < hi (a contiguous part of the flattened volume, e.g. a z-range): one searchsorted"""
    a, b = np.searchsorted(idx, [int(lo), int(hi)])
    return idx[a:b], q[a:b]
