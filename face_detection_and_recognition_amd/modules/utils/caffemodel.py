"""A reader for Caffe ``.caffemodel`` files (binary ``NetParameter`` protobuf messages) without a protobuf dependency.

Only what a weight loader needs is decoded: each layer's name and its blobs, from either form Caffe has written:
  NetParameter.layer  = 100 (LayerParameter:   name = 1, blobs = 7)   -- the current ("V2") form
  NetParameter.layers = 2   (V1LayerParameter: name = 4, blobs = 6)   -- the legacy ("V1") form
  BlobProto: num = 1, channels = 2, height = 3, width = 4 (legacy shape), data = 5 (float, packed or not),
             shape = 7 (BlobShape: dim = 1, int64, packed or not), double_data = 8.
Everything else is skipped by wire type.  Malformed input raises CaffeModelError.
"""
import struct

import numpy as np


class CaffeModelError(ValueError):
    pass


def _varint(buf, i):
    shift = result = 0
    while True:
        if i >= len(buf):
            raise CaffeModelError("truncated varint")
        b = buf[i]
        i += 1
        result |= (b & 0x7F) << shift
        if not b & 0x80:
            return result, i
        shift += 7
        if shift > 63:
            raise CaffeModelError("varint longer than 10 bytes")


def _fields(buf):
    """Yield (field number, wire type, value) of a message: value = int (varint / fixed) or a memoryview (length-delimited)."""
    i, n = 0, len(buf)
    while i < n:
        key, i = _varint(buf, i)
        field, wt = key >> 3, key & 7
        if field == 0:
            raise CaffeModelError("field number 0")
        if wt == 0:
            v, i = _varint(buf, i)
        elif wt == 1:
            if i + 8 > n:
                raise CaffeModelError("truncated 64-bit field")
            v, i = buf[i:i + 8], i + 8
        elif wt == 2:
            ln, i = _varint(buf, i)
            if i + ln > n:
                raise CaffeModelError("truncated length-delimited field")
            v, i = buf[i:i + ln], i + ln
        elif wt == 5:
            if i + 4 > n:
                raise CaffeModelError("truncated 32-bit field")
            v, i = buf[i:i + 4], i + 4
        else:
            raise CaffeModelError(f"unsupported wire type {wt}")
        yield field, wt, v


def _packed_varints(v):
    out, i = [], 0
    while i < len(v):
        x, i = _varint(v, i)
        out.append(x)
    return out


def _blob(buf):
    """BlobProto -> float32 array in its shape."""
    data, ddata, dims, legacy = [], [], None, {}
    for field, wt, v in _fields(buf):
        if field == 5:
            if wt == 2:
                if len(v) % 4:
                    raise CaffeModelError("packed float data not a multiple of 4 bytes")
                data.append(np.frombuffer(bytes(v), dtype="<f4"))
            elif wt == 5:
                data.append(np.frombuffer(bytes(v), dtype="<f4"))
            else:
                raise CaffeModelError("BlobProto.data with a wrong wire type")
        elif field == 8:
            if wt == 2:
                if len(v) % 8:
                    raise CaffeModelError("packed double data not a multiple of 8 bytes")
                ddata.append(np.frombuffer(bytes(v), dtype="<f8"))
            elif wt == 1:
                ddata.append(np.frombuffer(bytes(v), dtype="<f8"))
        elif field == 7 and wt == 2:
            dims = []
            for f2, wt2, v2 in _fields(v):
                if f2 == 1:
                    dims.extend(_packed_varints(v2) if wt2 == 2 else [v2])
        elif field in (1, 2, 3, 4) and wt == 0:
            legacy[field] = v
    arr = np.concatenate(data).astype(np.float32) if data else (
        np.concatenate(ddata).astype(np.float32) if ddata else np.zeros(0, np.float32))
    if dims is None:
        dims = [legacy.get(f, 1) for f in (1, 2, 3, 4)] if legacy else [arr.size]
    if int(np.prod(dims, dtype=np.int64)) != arr.size:
        raise CaffeModelError(f"blob shape {tuple(dims)} does not match its {arr.size} values")
    return arr.reshape([int(d) for d in dims])


def read_caffemodel(path_or_bytes):
    """{layer name: [blob arrays]} of every layer that has blobs, V2 (``layer``) and V1 (``layers``) forms alike."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        buf = memoryview(bytes(path_or_bytes))
    else:
        with open(path_or_bytes, "rb") as f:
            buf = memoryview(f.read())
    out = {}
    for field, wt, v in _fields(buf):
        if wt != 2 or field not in (2, 100):
            continue
        name_f, blob_f = (1, 7) if field == 100 else (4, 6)
        name, blobs = None, []
        for f2, wt2, v2 in _fields(v):
            if f2 == name_f and wt2 == 2:
                name = bytes(v2).decode("utf-8", "replace")
            elif f2 == blob_f and wt2 == 2:
                blobs.append(_blob(v2))
        if name is not None and blobs:
            out[name] = blobs
    return out


def _squeeze_lead(shape):
    s = list(shape)
    while len(s) > 1 and s[0] == 1:
        s.pop(0)
    return tuple(s)


def read_caffemodel_blobs(path_or_bytes, expected):
    """expected: {layer name: (weight shape, bias shape)} -> {layer name: (weight, bias)} float32 arrays in those shapes.
    Legacy 4-d blob shapes with leading 1s ((1, 1, 512, 18816) for a (512, 18816) weight) are accepted; a missing layer,
    a missing blob or any other shape raises CaffeModelError."""
    layers = read_caffemodel(path_or_bytes)
    out = {}
    for name, shapes in expected.items():
        if name not in layers:
            raise CaffeModelError(f"layer {name!r} not found in the caffemodel (layers with blobs: {sorted(layers)})")
        blobs = layers[name]
        if len(blobs) < 2:
            raise CaffeModelError(f"layer {name!r} has {len(blobs)} blob(s); weight and bias expected")
        pair = []
        for blob, want, what in zip(blobs, shapes, ("weight", "bias")):
            if _squeeze_lead(blob.shape) != _squeeze_lead(want):
                raise CaffeModelError(f"layer {name!r} {what}: shape {blob.shape}, expected {tuple(want)}")
            pair.append(np.ascontiguousarray(blob.reshape(want), dtype=np.float32))
        out[name] = tuple(pair)
    return out


# ---- writer (tests and fixtures: the same wire format, both forms) ----
def _enc_varint(x):
    out = bytearray()
    while True:
        b = x & 0x7F
        x >>= 7
        if x:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _enc_field(field, wt, payload):
    key = _enc_varint((field << 3) | wt)
    if wt == 2:
        return key + _enc_varint(len(payload)) + payload
    return key + payload


def encode_blob(arr, legacy_shape=False, packed=True):
    arr = np.asarray(arr, np.float32)
    msg = b""
    if legacy_shape:
        dims = [1] * (4 - arr.ndim) + list(arr.shape)
        for f, d in zip((1, 2, 3, 4), dims):
            msg += _enc_field(f, 0, _enc_varint(int(d)))
    else:
        msg += _enc_field(7, 2, _enc_field(1, 2, b"".join(_enc_varint(int(d)) for d in arr.shape)))
    flat = arr.reshape(-1).astype("<f4")
    if packed:
        msg += _enc_field(5, 2, flat.tobytes())
    else:
        msg += b"".join(_enc_field(5, 5, struct.pack("<f", float(v))) for v in flat)
    return msg


def encode_net(layers, v1=False, legacy_shape=False, packed=True):
    """layers: [(name, [arrays])] -> NetParameter bytes, V2 (``layer``) or V1 (``layers``) form."""
    out = _enc_field(1, 2, b"levi_hassner")
    for name, blobs in layers:
        if v1:
            msg = _enc_field(4, 2, name.encode()) + _enc_field(5, 0, _enc_varint(4))   # type = CONVOLUTION (any enum)
            msg += b"".join(_enc_field(6, 2, encode_blob(b, legacy_shape, packed)) for b in blobs)
            out += _enc_field(2, 2, msg)
        else:
            msg = _enc_field(1, 2, name.encode()) + _enc_field(2, 2, b"Convolution")
            msg += b"".join(_enc_field(7, 2, encode_blob(b, legacy_shape, packed)) for b in blobs)
            out += _enc_field(100, 2, msg)
    return out
