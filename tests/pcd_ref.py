"""An independent reading of the two on-disk formats, for tests/test_io_formats.py and tests/test_io_formats_malformed.py.
Written from the published formats -- the PCD v0.7 file format of the Point Cloud Library's documentation, Marc Lehmann's LZF
stream layout as liblzf's lzf.h describes it, and MathWorks' "MAT-File Format" (Level 5) -- not from io_formats.hip:

  parse_header / read_pcd    header and payload of a .pcd file with struct / numpy dtypes, all three DATA kinds
  make_pcd                   the bytes of a .pcd file from columns (the test's own writer: any TYPE / SIZE / COUNT, line end, ...)
  lzf_decompress             the LZF stream format, strictly: every reference inside the output, the length exact
  lzf_compress               a small greedy compressor (hash chains of 3-byte keys, the longest of a few candidates)
  lzf_stats                  what kinds of items a stream holds
  mat_tag / mat_matrix / mat_opaque / mat_file   MAT Level-5 elements by hand (what scipy.io does not write)
  mat_walk                   a tolerant walk over a MAT file's top-level variables (None where it cannot follow)
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

# ------------------------------------------------------------------------------------------------ PCD
KIND = {"I": "i", "U": "u", "F": "f"}
LEGAL = {("I", 1), ("I", 2), ("I", 4), ("I", 8), ("U", 1), ("U", 2), ("U", 4), ("U", 8), ("F", 4), ("F", 8)}


class PcdError(ValueError):
    pass


def parse_header(data: bytes) -> dict:
    """The header up to and including the DATA line.  -> fields [(name, size, type, count)], width, height, points, data, offset"""
    h = {"width": 0, "height": 1, "points": None, "data": None}
    names = sizes = types = counts = None
    pos = 0
    while h["data"] is None:
        end = data.find(b"\n", pos)
        if end < 0:
            end = len(data)
        line, nxt = data[pos:end], min(end + 1, len(data))
        if nxt == pos:
            raise PcdError("no DATA line")
        pos = nxt
        tok = line.decode("latin-1").split()
        if not tok or tok[0].startswith("#"):
            continue
        key, val = tok[0], tok[1:]
        if key in ("FIELDS", "COLUMNS"):
            names = val
        elif key == "SIZE":
            sizes = [int(v) for v in val]
        elif key == "TYPE":
            types = val
        elif key == "COUNT":
            counts = [int(v) for v in val]
        elif key in ("WIDTH", "HEIGHT", "POINTS"):
            h[key.lower()] = int(val[0])
        elif key == "DATA":
            if val[0] not in ("ascii", "binary", "binary_compressed"):
                raise PcdError("DATA " + val[0])
            h["data"] = val[0]
    if not names or sizes is None or types is None:
        raise PcdError("no FIELDS / SIZE / TYPE")
    if counts is None:
        counts = [1] * len(names)
    if not len(names) == len(sizes) == len(types) == len(counts):
        raise PcdError("lists of different lengths")
    if any(names.count(k) > 1 for k in "xyz"):
        raise PcdError("a coordinate declared twice")
    for s, t, c in zip(sizes, types, counts):
        if (t, s) not in LEGAL or c < 1:
            raise PcdError(f"field {t}{s} x {c}")
    if h["points"] is None:
        h["points"] = h["width"] * h["height"]
    if min(h["width"], h["height"], h["points"]) < 0 or h["points"] > 2**31 - 1:
        raise PcdError("counts")
    h["fields"] = list(zip(names, sizes, types, counts))
    h["offset"] = pos
    return h


def _dtype(size, typ):
    return np.dtype("<" + KIND[typ] + str(size))


def read_pcd(data: bytes):
    """-> (header, {field name: array [n][count] of the field's own type}); a name that occurs twice keeps its last column"""
    h = parse_header(data)
    n, fields = h["points"], h["fields"]
    body = data[h["offset"]:]
    cols = {}
    if h["data"] == "binary":
        rec = np.dtype({"names": [f"f{i}" for i in range(len(fields))],
                        "formats": [(_dtype(s, t), (c,)) for _, s, t, c in fields]})
        if len(body) < n * rec.itemsize:
            raise PcdError("short payload")
        arr = np.frombuffer(body, dtype=rec, count=n)
        for i, (name, _s, _t, c) in enumerate(fields):
            cols[name] = arr[f"f{i}"].reshape(n, c).copy()
    elif h["data"] == "binary_compressed":
        if len(body) < 8:
            raise PcdError("no sizes")
        comp, raw = struct.unpack_from("<II", body)
        if raw != n * sum(s * c for _, s, _, c in fields) or len(body) < 8 + comp:
            raise PcdError("sizes")
        soa = lzf_decompress(body[8:8 + comp], raw)
        at = 0
        for name, s, t, c in fields:                     # field by field: all x, then all y, ...
            cols[name] = np.frombuffer(soa, dtype=_dtype(s, t), count=n * c, offset=at).reshape(n, c).copy()
            at += n * c * s
    else:
        tok = body.split()
        per = sum(c for *_x, c in fields)
        if len(tok) < n * per:
            raise PcdError("short payload")
        at = 0
        for name, s, t, c in fields:
            cols[name] = np.zeros((n, c), dtype=_dtype(s, t))
        for i in range(n):
            for name, s, t, c in fields:
                for k in range(c):
                    w = tok[at].decode("latin-1"); at += 1
                    if t == "F":
                        cols[name][i, k] = float(w)                       # a ValueError for what is no number
                    else:
                        val = int(w, 10)
                        lo, hi = (0, 2**(8 * s) - 1) if t == "U" else (-2**(8 * s - 1), 2**(8 * s - 1) - 1)
                        if not lo <= val <= hi:
                            raise PcdError(f"{w} does not fit {t}{s}")
                        cols[name][i, k] = val
    return h, cols


def location_word(data: bytes):
    """-> Location [n][3] float32 by numpy's conversion of the x / y / z columns, the colour field's 4 bytes as one word [n] or None"""
    h, cols = read_pcd(data)
    with np.errstate(over="ignore"):                     # a double past FLT_MAX becomes inf, as in C
        xyz = np.stack([cols[k][:, 0].astype(np.float32) for k in "xyz"], axis=1).reshape(h["points"], 3)
    word = None
    for name in ("rgb", "rgba"):
        if name in cols:
            if cols[name].dtype.itemsize != 4 or cols[name].shape[1] != 1:
                raise PcdError("a colour field is one 4-byte word")
            word = cols[name][:, 0].copy().view("<u4")
    return xyz, word


def location_color(data: bytes):
    """-> what pcread returns: Location [n][3] float32, Color [n][3] uint8 (the word's 0x00RRGGBB) or None"""
    xyz, w = location_word(data)
    return xyz, None if w is None else np.stack([(w >> 16) & 255, (w >> 8) & 255, w & 255], axis=1).astype(np.uint8)


def fnv1a(*parts: bytes) -> str:
    """the 64-bit FNV-1a hash that tests/iofuzz/io_formats_main.cpp prints of what it was handed back"""
    h = 14695981039346656037
    for p in parts:
        for b in p:
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def make_pcd(fields, cols, kind, points=True, eol="\n", key="FIELDS", width=None, height=1, count_line=True, comments=(), lzf=None) -> bytes:
    """fields [(name, size, type, count)], cols [array [n][count]] in the same order.  lzf: the compressor (binary_compressed)"""
    n = len(cols[0]) if cols else 0
    width = n if width is None else width
    cols = [np.asarray(c).reshape(n, f[3]).astype(_dtype(f[1], f[2])) for f, c in zip(fields, cols)]
    lines = list(comments) + ["VERSION .7", key + " " + " ".join(f[0] for f in fields), "SIZE " + " ".join(str(f[1]) for f in fields),
                              "TYPE " + " ".join(f[2] for f in fields)]
    if count_line:
        lines.append("COUNT " + " ".join(str(f[3]) for f in fields))
    lines += [f"WIDTH {width}", f"HEIGHT {height}", "VIEWPOINT 0 0 0 1 0 0 0"]
    if points:
        lines.append(f"POINTS {n}")
    lines.append("DATA " + kind)
    head = (eol.join(lines) + eol).encode()
    if kind == "binary":
        rec = np.dtype({"names": [f"f{i}" for i in range(len(fields))], "formats": [(c.dtype, (c.shape[1],)) for c in cols]})
        arr = np.zeros(n, dtype=rec)
        for i, c in enumerate(cols):
            arr[f"f{i}"] = c
        return head + arr.tobytes()
    if kind == "binary_compressed":
        soa = b"".join(c.tobytes() for c in cols)
        stream = (lzf or lzf_compress)(soa)
        return head + struct.pack("<II", len(stream), len(soa)) + stream
    rows = []
    for i in range(n):
        rows.append(" ".join(_ascii(v) for c in cols for v in c[i]))
    return head + (eol.join(rows) + eol if rows else "").encode()


def _ascii(v) -> str:
    if isinstance(v, np.floating):
        return "%.9g" % v if v.dtype == np.float32 else "%.17g" % v       # both round-trip their type exactly
    return str(int(v))


# ------------------------------------------------------------------------------------------------ LZF
# A stream is a sequence of items.  Control byte c < 32: c + 1 literal bytes follow.  Otherwise a back reference: length
# (c >> 5) + 2, where c >> 5 == 7 means one more byte follows that is added to the length; then one byte that forms, with the
# low five bits of c as its high part, the distance - 1.  Lengths 3 .. 264, distances 1 .. 8192; a copy may overlap its output.
MAX_LIT, MAX_REF, MAX_DIST = 32, 264, 8192


def lzf_decompress(stream: bytes, out_len: int) -> bytes:
    out = bytearray()
    i = 0
    while i < len(stream):
        c = stream[i]; i += 1
        if c < 32:
            run = c + 1
            if i + run > len(stream) or len(out) + run > out_len:
                raise PcdError("literal run past the end")
            out += stream[i:i + run]; i += run
        else:
            ln = c >> 5
            if ln == 7:
                if i >= len(stream):
                    raise PcdError("truncated item")
                ln += stream[i]; i += 1
            if i >= len(stream):
                raise PcdError("truncated item")
            dist = ((c & 31) << 8 | stream[i]) + 1; i += 1
            ln += 2
            if dist > len(out):
                raise PcdError("reference before the start")
            if len(out) + ln > out_len:
                raise PcdError("copy past the end")
            for _ in range(ln):
                out.append(out[-dist])
    if len(out) != out_len:
        raise PcdError("short output")
    return bytes(out)


def lzf_compress(data: bytes, chain: int = 8) -> bytes:
    """greedy: at every position the longest match among the last `chain` places that began with the same three bytes"""
    out, lit = bytearray(), bytearray()
    seen: dict[bytes, list[int]] = {}

    def flush():
        for k in range(0, len(lit), MAX_LIT):
            part = lit[k:k + MAX_LIT]
            out.append(len(part) - 1); out.extend(part)
        lit.clear()

    def remember(p):
        if p + 3 <= len(data):
            lst = seen.setdefault(data[p:p + 3], [])
            lst.append(p)
            if len(lst) > chain:
                del lst[0]

    pos, n = 0, len(data)
    while pos < n:
        best_len, best_dist = 0, 0
        for cand in reversed(seen.get(data[pos:pos + 3], ())):
            if pos - cand > MAX_DIST:
                break
            ln, cap = 0, min(MAX_REF, n - pos)
            while ln < cap and data[cand + ln] == data[pos + ln]:      # cand + ln may run past pos: an overlapping copy
                ln += 1
            if ln > best_len:
                best_len, best_dist = ln, pos - cand
        if best_len >= 3:
            flush()
            ln, d = best_len - 2, best_dist - 1
            if ln < 7:
                out.append(ln << 5 | d >> 8)
            else:
                out.append(7 << 5 | d >> 8); out.append(ln - 7)
            out.append(d & 255)
            for p in range(pos, pos + best_len):
                remember(p)
            pos += best_len
        else:
            lit.append(data[pos]); remember(pos); pos += 1
    flush()
    return bytes(out)


def lzf_stats(stream: bytes) -> dict:
    """-> items by kind: literal runs, references, those with the length-extension byte, with a distance above 255, overlapping"""
    s = {"literals": 0, "refs": 0, "extended": 0, "far": 0, "overlapping": 0}
    i = 0
    while i < len(stream):
        c = stream[i]; i += 1
        if c < 32:
            s["literals"] += 1; i += c + 1
            continue
        ln = c >> 5
        if ln == 7:
            ln += stream[i]; i += 1; s["extended"] += 1
        dist = ((c & 31) << 8 | stream[i]) + 1; i += 1
        s["refs"] += 1; s["far"] += dist > 255; s["overlapping"] += dist < ln + 2
    return s


# ------------------------------------------------------------------------------------------------ MAT Level 5
MI = {"int8": 1, "uint8": 2, "int16": 3, "uint16": 4, "int32": 5, "uint32": 6, "single": 7, "double": 9, "int64": 12, "uint64": 13,
      "matrix": 14, "compressed": 15, "utf8": 16}
MI_SIZE = {1: 1, 2: 1, 3: 2, 4: 2, 5: 4, 6: 4, 7: 4, 9: 8, 12: 8, 13: 8}
MX = {"cell": 1, "struct": 2, "object": 3, "char": 4, "sparse": 5, "double": 6, "single": 7, "int8": 8, "uint8": 9, "int16": 10,
      "uint16": 11, "int32": 12, "uint32": 13, "int64": 14, "uint64": 15}


def mat_header(endian: bytes = b"IM", text: bytes = b"MATLAB 5.0 MAT-file, written by hand") -> bytes:
    """128 bytes: 116 of text, 8 of subsystem offset, the version 0x0100 and the endian indicator as a little-endian writer puts them"""
    return text.ljust(116, b" ") + b"\0" * 8 + (b"\x00\x01" if endian == b"IM" else b"\x01\x00") + endian


def mat_tag(mi: int, payload: bytes, small: bool = True, nbytes: int | None = None) -> bytes:
    """one data element; 1 .. 4 bytes go into the small format (type and count in one word) unless small is False.  nbytes: a lie"""
    n = len(payload) if nbytes is None else nbytes
    if small and 1 <= len(payload) <= 4 and nbytes is None:
        return struct.pack("<I", n << 16 | mi) + payload.ljust(4, b"\0")
    return struct.pack("<II", mi, n) + payload + b"\0" * (-len(payload) % 8)


def mat_matrix(name: str, cls: int, dims, mi: int, data: bytes, flags: int = 0, small: bool = True) -> bytes:
    """one miMATRIX element of a real numeric array: array flags, dimensions, name, real part (of data type mi, whatever cls is)"""
    body = (mat_tag(MI["uint32"], struct.pack("<II", flags << 8 | cls, 0)) + mat_tag(MI["int32"], struct.pack(f"<{len(dims)}i", *dims), small)
            + mat_tag(MI["int8"], name.encode(), small) + mat_tag(mi, data, small))
    return mat_tag(MI["matrix"], body, small=False)


def mat_opaque(name: str, class_name: str = "string") -> bytes:
    """one miMATRIX element of class mxOPAQUE (17), how MATLAB stores string, table, datetime, categorical and containers.Map
    objects: array flags, name, type-system name, class name, metadata (a uint32 matrix) -- and NO dimensions element"""
    meta = mat_matrix("", MX["uint32"], [6, 1], MI["uint32"], struct.pack("<6I", 0xDD000000, 2, 1, 1, 1, 1))
    body = (mat_tag(MI["uint32"], struct.pack("<II", 17, 0)) + mat_tag(MI["int8"], name.encode()) + mat_tag(MI["int8"], b"MCOS")
            + mat_tag(MI["int8"], class_name.encode()) + meta)
    return mat_tag(MI["matrix"], body, small=False)


def mat_file(elements, compress: bool = False, endian: bytes = b"IM") -> bytes:
    out = mat_header(endian)
    for e in elements:
        if compress:
            z = zlib.compress(e)
            out += struct.pack("<II", MI["compressed"], len(z)) + z          # compressed elements are not padded
        else:
            out += e
    return out


def _tag(b: bytes, at: int):
    """-> (type, count, payload offset, offset of the next element)"""
    w0, = struct.unpack_from("<I", b, at)
    if w0 >> 16:
        return w0 & 0xFFFF, w0 >> 16, at + 4, at + 8
    n, = struct.unpack_from("<I", b, at + 4)
    return w0, n, at + 8, at + 8 + n + (-n % 8)


def mat_walk(data: bytes):
    """-> (variables [{name, dims, mi, nbytes}] the walk could follow, the bytes it had after inflating: file + every inflated element)"""
    out, total = [], len(data)
    at = 128
    try:
        while at + 8 <= len(data):
            t, n, pay, nxt = _tag(data, at)
            body = data[pay:pay + n]
            if t == MI["compressed"]:
                nxt = pay + n
                try:
                    body = zlib.decompressobj().decompress(body)
                except zlib.error:
                    body = b""
                total += len(body)
                if len(body) >= 8:
                    t, n, pay2, _ = _tag(body, 0)
                    body = body[pay2:pay2 + n]
            if t == MI["matrix"] and len(body) >= 16:
                try:
                    _t, _n, p, q = _tag(body, 0)
                    cls = body[p]
                    _t, n2, p, q = _tag(body, q)
                    dims = list(struct.unpack_from(f"<{n2 // 4}i", body, p))
                    _t, n3, p, q = _tag(body, q)
                    name = body[p:p + n3].decode("latin-1")
                    var = {"name": name, "dims": dims, "cls": cls, "mi": None, "nbytes": 0}
                    if 6 <= cls <= 15:
                        t4, n4, p, q = _tag(body, q)
                        var["mi"], var["nbytes"] = t4, min(n4, len(body) - p)
                    out.append(var)
                except (struct.error, IndexError):
                    pass
            at = nxt
    except struct.error:
        pass
    return out, total
