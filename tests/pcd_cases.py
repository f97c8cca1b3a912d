"""An independent PCD v0.7 reader and writer (numpy) and a plain-Python LZF decoder, written from the format descriptions:
the yardstick of tests/test_pcd_codec.py and tests/test_gpu_map_io.py, not the library under test.

PCD: text header (VERSION FIELDS SIZE TYPE COUNT WIDTH HEIGHT VIEWPOINT POINTS DATA, `#` comments), then the data:
ascii rows; binary records; or binary_compressed = uint32 compressed size, uint32 raw size, LZF stream of the columns.
LZF: control byte c < 32: c + 1 literal bytes; otherwise a back reference of length (c >> 5) + 2 (c >> 5 == 7: + the next
byte), at distance ((c & 31) << 8 | next byte) + 1.
"""
from fractions import Fraction

import numpy as np

POINT_FIELDS = [("x", "F", 4), ("y", "F", 4), ("z", "F", 4), ("time", "F", 8), ("intensity", "F", 4), ("laser_id", "U", 2), ("device_id", "U", 1), ("label", "U", 1)]
FORMATS = ["ascii", "binary", "binary_compressed"]


def np_type(t, size):
    return np.dtype({"F": "<f", "I": "<i", "U": "<u"}[t] + str(size))


def lzf_decode(data, raw_size=None):
    data = bytes(data)
    out = bytearray()
    i = 0
    while i < len(data):
        c = data[i]
        i += 1
        if c < 32:
            assert i + c + 1 <= len(data), "literal run past the end"
            out += data[i : i + c + 1]
            i += c + 1
        else:
            length = c >> 5
            if length == 7:
                length += data[i]
                i += 1
            length += 2
            dist = ((c & 31) << 8 | data[i]) + 1
            i += 1
            assert dist <= len(out), "reference before the start"
            for _ in range(length):
                out.append(out[-dist])
    if raw_size is not None:
        assert len(out) == raw_size, (len(out), raw_size)
    return bytes(out)


def lzf_literals(data):
    """A valid stream of literal runs only (the writer below needs no compressor)."""
    data = bytes(data)
    out = bytearray()
    for i in range(0, len(data), 32):
        run = data[i : i + 32]
        out.append(len(run) - 1)
        out += run
    return bytes(out)


def write(path, columns, fields, fmt, comment=True, points=None, width=None, height=1):
    """columns: name -> array [n] (or [n, count]); fields: [(name, type, size, count)] in file order."""
    n = len(next(iter(columns.values())))
    head = ("# .PCD v0.7 - Point Cloud Data file format\n" if comment else "") + "VERSION 0.7\n"
    head += "FIELDS " + " ".join(f[0] for f in fields) + "\n"
    head += "SIZE " + " ".join(str(f[2]) for f in fields) + "\n"
    head += "TYPE " + " ".join(f[1] for f in fields) + "\n"
    head += "COUNT " + " ".join(str(f[3]) for f in fields) + "\n"
    head += f"WIDTH {n if width is None else width}\nHEIGHT {height}\n# a comment in the middle\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n if points is None else points}\nDATA {fmt}\n"
    cols = [np.ascontiguousarray(np.asarray(columns[f[0]]).reshape(n, f[3]).astype(np_type(f[1], f[2]))) for f in fields]
    with open(path, "wb") as fh:
        fh.write(head.encode())
        if fmt == "ascii":
            # nine and seventeen significant digits read back to the same float and double
            spec = " ".join(" ".join([("%.17g" if c.dtype.itemsize == 8 else "%.9g") if c.dtype.kind == "f" else "%d"] * c.shape[1]) for c in cols)
            flat = [c.reshape(n, -1).tolist() for c in cols]
            rows = [spec % tuple(v for c in flat for v in c[i]) for i in range(n)]
            fh.write(("\n".join(rows) + "\n").encode())
        elif fmt == "binary":
            rec = np.dtype([(f"f{j}", c.dtype, (c.shape[1],)) for j, c in enumerate(cols)])
            a = np.zeros(n, rec)
            for j, c in enumerate(cols):
                a[f"f{j}"] = c
            fh.write(a.tobytes())
        else:
            raw = b"".join(c.tobytes() for c in cols)
            z = lzf_literals(raw)
            fh.write(np.array([len(z), len(raw)], "<u4").tobytes() + z)
    return head


def write_points(path, pts, fmt):
    """LidarPoints (POINT_DTYPE) with the LidarPoint field list."""
    return write(path, {f[0]: pts[f[0]] for f in POINT_FIELDS}, [(f[0], f[1], f[2], 1) for f in POINT_FIELDS], fmt)


def f32_from_decimal(tok):
    """The float32 nearest to a decimal token, without rounding twice (decimal -> double -> float): the candidates around
    the double's float are compared exactly."""
    d = float(tok)
    c = np.float32(d)
    if not np.isfinite(c) or float(c) == d:
        return c
    exact = Fraction(tok)
    with np.errstate(over="ignore"):
        near = [c, np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))]
    near = [v for v in near if np.isfinite(v)]
    return min(near, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))


def read(path):
    """-> (fields [(name, type, size, count)], columns name -> array [n, count], format)"""
    blob = open(path, "rb").read()
    pos = 0
    meta = {}
    while True:
        end = blob.index(b"\n", pos)
        line = blob[pos:end].decode().strip()
        pos = end + 1
        if not line or line.startswith("#"):
            continue
        key, *tok = line.split()
        meta[key] = tok
        if key == "DATA":
            break
    names = meta["FIELDS"]
    sizes = [int(v) for v in meta["SIZE"]]
    counts = [int(v) for v in meta.get("COUNT", ["1"] * len(names))]
    fields = list(zip(names, meta["TYPE"], sizes, counts))
    n = int(meta["POINTS"][0])
    assert n == int(meta["WIDTH"][0]) * int(meta["HEIGHT"][0])
    fmt = meta["DATA"][0]
    types = [np_type(t, s) for _, t, s, _ in fields]
    cols = {}
    if fmt == "ascii":
        rows = [r.split() for r in blob[pos:].decode().splitlines() if r.strip()]
        assert len(rows) == n
        j = 0
        for (name, _, _, c), t in zip(fields, types):
            # through Python's own number parsing: float(str) is correctly rounded for doubles, numpy rounds the decimal to float32
            cols[name] = np.array([[f32_from_decimal(v) if t == np.float32 else (float(v) if t.kind == "f" else int(v)) for v in r[j : j + c]] for r in rows], t).reshape(n, c)
            j += c
    elif fmt == "binary":
        rec = np.dtype([(f"f{j}", t, (c,)) for j, ((_, _, _, c), t) in enumerate(zip(fields, types))])
        assert len(blob) - pos >= n * rec.itemsize
        a = np.frombuffer(blob, rec, n, pos)
        for j, f in enumerate(fields):
            cols[f[0]] = a[f"f{j}"].reshape(n, f[3])
    else:
        csize, usize = np.frombuffer(blob, "<u4", 2, pos)
        raw = lzf_decode(blob[pos + 8 : pos + 8 + int(csize)], int(usize))
        at = 0
        for f, t in zip(fields, types):
            cols[f[0]] = np.frombuffer(raw, t, n * f[3], at).reshape(n, f[3])
            at += n * f[3] * t.itemsize
        assert at == usize
    return fields, cols, fmt


def to_points(cols, point_dtype):
    """The helper's own decoding into LidarPoints: C conversions (numpy astype), missing fields 0, w = 1, COUNT 1 only."""
    n = len(next(iter(cols.values())))
    out = np.zeros(n, point_dtype)
    out["w"] = 1.0
    for name, _, _ in POINT_FIELDS:
        if name in cols and cols[name].shape[1] == 1:
            out[name] = cols[name][:, 0].astype(point_dtype[name])
    return out


def read_points(path, point_dtype):
    return to_points(read(path)[1], point_dtype)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
