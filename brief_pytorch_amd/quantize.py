"""Quantised artefacts: module/quantized.bin holds every weight matrix and bias of a SIREN-shaped net (.net[l][0].weight / .bias)
as 2..16-bit codes instead of the raw float32 weight-l-out-in / bias-l-n files.

The quantiser (csrc/brief_quant.h is the same arithmetic for the kernels) is uniform, affine and per tensor, and every float32
operation rounds on its own, so that numpy restates it exactly:

    lo = min(w); hi = max(w); top = 2^bits - 1
    step = (hi - lo) / top
    code = clamp(rint((w - lo) / step), 0, top)        (step == 0: code = 0)
    deq  = code * step + lo

File layout (little-endian):
    header   16 bytes: magic b"BRQW", format version (uint32), bits (uint32), tensor count (uint32)
    table    per tensor 24 bytes: kind (uint32: 0 weight | 1 bias), layer, rows, cols (uint32; a bias has cols = 1), lo, step (float32)
    codes    all codes, tensor after tensor in table order, row-major, `bits` bits each, packed into one bit stream: bit k of the
             stream is bit k % 8 of byte k // 8, a code's least significant bit comes first; zero-padded to a whole byte at the end
"""
import os
import struct

import numpy as np

FILE_NAME = "quantized.bin"
MAGIC = b"BRQW"
VERSION = 1
MIN_BITS, MAX_BITS = 2, 16
KIND_WEIGHT, KIND_BIAS = 0, 1
_HEADER = struct.Struct("<4sIII")
_ENTRY = struct.Struct("<IIIIff")

#: the nets whose artefact is the weight-file directory with SIREN's .net[l][0] shape
NETS = ("SIREN", "SIREN_Pyramid", "SIRENFT", "SIRENPS")


class QuantizedFileError(ValueError):
    """a quantized.bin that cannot be read, or does not belong to the net it is loaded into"""


class BadMagic(QuantizedFileError):
    pass


class UnknownVersion(QuantizedFileError):
    pass


class TruncatedFile(QuantizedFileError):
    pass


class TensorTableMismatch(QuantizedFileError):
    pass


class NonFiniteTensor(ValueError):
    """a tensor with a NaN or an infinity has no range to quantise"""


def check_bits(bits):
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not MIN_BITS <= int(bits) <= MAX_BITS:
        raise ValueError("quantize: bits must be an integer in %d..%d (got %r)" % (MIN_BITS, MAX_BITS, bits))
    return int(bits)


def overhead_bytes(layers):
    """bytes of quantized.bin that are not codes: the header and one table entry per weight matrix and per bias"""
    return _HEADER.size + _ENTRY.size * 2 * int(layers)


def code_bytes(count, bits):
    return (int(count) * int(bits) + 7) // 8


def ranges(w, bits):
    """(lo, step) of a float32 tensor, as float32 scalars"""
    w = np.asarray(w, dtype=np.float32)
    lo, hi = np.float32(w.min()), np.float32(w.max())
    top = np.float32((1 << int(bits)) - 1)
    with np.errstate(over="ignore"):
        return lo, np.float32(np.float32(hi - lo) / top)


def quantise(w, lo, step, bits):
    """the integer codes (uint16, the shape of w) of a float32 tensor under (lo, step)"""
    w = np.asarray(w, dtype=np.float32)
    lo, step = np.float32(lo), np.float32(step)
    if step == 0:
        return np.zeros(w.shape, dtype=np.uint16)
    top = np.float32((1 << int(bits)) - 1)
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.rint((w - lo) / step)
    return np.clip(q, np.float32(0), top).astype(np.uint16)


def dequantise(codes, lo, step):
    """float32 values of integer codes: one rounding for the product, one for the sum"""
    p = np.asarray(codes).astype(np.float32) * np.float32(step)
    return (p + np.float32(lo)).astype(np.float32)


def fake_quantise(w, bits):
    """deq(code(w)) with the tensor's own range: what a quantised artefact of w decodes to"""
    lo, step = ranges(w, bits)
    return dequantise(quantise(w, lo, step, bits), lo, step)


# ---- bit packing
_PACK_BLOCK = 1 << 20      # codes per round (a multiple of 8: every round ends on a byte boundary)


def pack_bits(codes, bits):
    """codes (any integer array, values < 2^bits) -> bytes: `bits` bits each, least significant bit first"""
    c = np.ascontiguousarray(np.asarray(codes).reshape(-1), dtype="<u2")
    out = []
    for i in range(0, c.size, _PACK_BLOCK):
        b = np.unpackbits(c[i:i + _PACK_BLOCK].view(np.uint8).reshape(-1, 2), axis=1, bitorder="little")[:, :bits]
        out.append(np.packbits(b.reshape(-1), bitorder="little"))
    return b"".join(o.tobytes() for o in out)


def unpack_bits(buf, count, bits):
    """the inverse of pack_bits: `count` codes (uint16) from a bytes-like object"""
    raw = np.frombuffer(buf, dtype=np.uint8, count=code_bytes(count, bits))
    out = np.empty(count, dtype=np.uint16)
    per = _PACK_BLOCK * bits // 8
    for k, i in enumerate(range(0, count, _PACK_BLOCK)):
        n = min(_PACK_BLOCK, count - i)
        b = np.unpackbits(raw[k * per:k * per + code_bytes(n, bits)], bitorder="little")[:n * bits].reshape(n, bits)
        full = np.zeros((n, 16), dtype=np.uint8)
        full[:, :bits] = b
        out[i:i + n] = np.packbits(full, axis=1, bitorder="little").view("<u2").reshape(-1)
    return out


# ---- the file
def model_tensors(model):
    """[(kind, layer, float32 array)] of a net with SIREN's .net[l][0] shape, in file order (= the canonical parameter order)"""
    if not hasattr(model, "net"):
        raise TypeError("quantize: %s has no .net[l][0].weight / .bias (quantised artefacts exist for %s)" % (type(model).__name__, ", ".join(NETS)))
    out = []
    for l in range(len(model.net)):
        lin = model.net[l][0]
        out.append((KIND_WEIGHT, l, np.ascontiguousarray(lin.weight.data.detach().to("cpu").numpy(), dtype=np.float32)))
        out.append((KIND_BIAS, l, np.ascontiguousarray(lin.bias.data.detach().to("cpu").numpy(), dtype=np.float32)))
    return out


def write(path, model, bits):
    """quantise every tensor of `model` with its own range and write quantized.bin at `path`.  Returns the file's size in bytes."""
    bits = check_bits(bits)
    tensors = model_tensors(model)
    table, codes = [], []
    for kind, l, w in tensors:
        if not np.all(np.isfinite(w)):
            raise NonFiniteTensor("quantize: %s of layer %d holds a non-finite value" % ("weight" if kind == KIND_WEIGHT else "bias", l))
        lo, step = ranges(w, bits)
        rows, cols = (w.shape[0], w.shape[1]) if kind == KIND_WEIGHT else (w.shape[0], 1)
        table.append(_ENTRY.pack(kind, l, rows, cols, lo, step))
        codes.append(quantise(w, lo, step, bits).reshape(-1))
    with open(path, "wb") as f:
        f.write(_HEADER.pack(MAGIC, VERSION, bits, len(tensors)))
        f.write(b"".join(table))
        f.write(pack_bits(np.concatenate(codes), bits))
    return os.path.getsize(path)


def read(path):
    """{"bits", "tensors": [{"kind", "layer", "rows", "cols", "lo", "step", "codes" (uint16 [rows, cols] | [rows])}]}"""
    with open(path, "rb") as f:
        buf = f.read()
    if len(buf) < _HEADER.size:
        raise TruncatedFile("%s: truncated file (%d bytes, the header alone has %d)" % (path, len(buf), _HEADER.size))
    magic, version, bits, n = _HEADER.unpack_from(buf, 0)
    if magic != MAGIC:
        raise BadMagic("%s: bad magic %r (a quantised artefact starts with %r)" % (path, magic, MAGIC))
    if version != VERSION:
        raise UnknownVersion("%s: unknown format version %d (this reader knows %d)" % (path, version, VERSION))
    if not MIN_BITS <= bits <= MAX_BITS:
        raise QuantizedFileError("%s: bits = %d outside %d..%d" % (path, bits, MIN_BITS, MAX_BITS))
    off = _HEADER.size
    if len(buf) < off + n * _ENTRY.size:
        raise TruncatedFile("%s: truncated file (the tensor table of %d entries ends at byte %d, the file has %d)" % (path, n, off + n * _ENTRY.size, len(buf)))
    tensors = []
    for i in range(n):
        kind, l, rows, cols, lo, step = _ENTRY.unpack_from(buf, off + i * _ENTRY.size)
        if kind not in (KIND_WEIGHT, KIND_BIAS) or (kind == KIND_BIAS and cols != 1):
            raise QuantizedFileError("%s: tensor %d: bad kind / shape (%d, %d x %d)" % (path, i, kind, rows, cols))
        tensors.append({"kind": kind, "layer": l, "rows": rows, "cols": cols, "lo": np.float32(lo), "step": np.float32(step)})
    off += n * _ENTRY.size
    count = sum(t["rows"] * t["cols"] for t in tensors)
    if len(buf) < off + code_bytes(count, bits):
        raise TruncatedFile("%s: truncated file (%d codes of %d bits need %d bytes behind the table, the file has %d)"
                            % (path, count, bits, code_bytes(count, bits), len(buf) - off))
    codes = unpack_bits(memoryview(buf)[off:], count, bits)
    pos = 0
    for t in tensors:
        k = t["rows"] * t["cols"]
        t["codes"] = codes[pos:pos + k].reshape((t["rows"], t["cols"]) if t["kind"] == KIND_WEIGHT else (t["rows"],))
        pos += k
    return {"bits": bits, "tensors": tensors}


def load_into(model, path, device="cpu"):
    """fill model.net[l][0].weight / .bias with the dequantised tensors of quantized.bin; the file's tensor table must be the net's"""
    import torch
    art = read(path)
    want = []
    for l in range(len(model.net)):
        rows, cols = (int(v) for v in model.net[l][0].weight.shape)
        want += [(KIND_WEIGHT, l, rows, cols), (KIND_BIAS, l, rows, 1)]
    have = [(t["kind"], t["layer"], t["rows"], t["cols"]) for t in art["tensors"]]
    if have != want:
        raise TensorTableMismatch("%s: tensor table mismatch: the file holds %s, the net it is loaded into has %s (kind, layer, rows, cols)" % (path, have, want))
    for t in art["tensors"]:
        lin = model.net[t["layer"]][0]
        deq = torch.from_numpy(dequantise(t["codes"], t["lo"], t["step"])).to(device)
        if t["kind"] == KIND_WEIGHT:
            lin.weight.data = deq
        else:
            lin.bias.data = deq
    return model
