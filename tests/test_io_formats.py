"""PCD and MAT-v5 readers of the C ABI.  Host code: runs without a GPU."""
import struct

import numpy as np
import pytest
import scipy.io

from pcreg_amd import io as pio
from pcreg_amd._lib import PcregError


def test_pcd_ascii_binary_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    xyz = rng.normal(0, 30, (1000, 3)).astype(np.float32)
    col = rng.integers(0, 256, (1000, 3)).astype(np.uint8)
    for enc in ("ascii", "binary"):
        p = str(tmp_path / f"c_{enc}.pcd")
        pio.pcwrite(p, xyz, col, encoding=enc)
        got, gc = pio.pcread(p)
        np.testing.assert_array_equal(got, xyz)          # %.9g round-trips float32 exactly
        np.testing.assert_array_equal(gc, col)
        p2 = str(tmp_path / f"n_{enc}.pcd")
        pio.pcwrite(p2, xyz, None, encoding=enc)
        got2, none = pio.pcread(p2)
        assert none is None
        np.testing.assert_array_equal(got2, xyz)


def test_pcd_foreign_headers(tmp_path):
    # a PCL-style file: double coordinates, an extra field before x, float-typed rgb, comment lines
    p = tmp_path / "pcl.pcd"
    rgb = struct.unpack("f", struct.pack("I", (10 << 16) | (20 << 8) | 30))[0]
    p.write_text("# .PCD v.7\nVERSION .7\nFIELDS intensity x y z rgb\nSIZE 4 8 8 8 4\nTYPE F F F F F\nCOUNT 1 1 1 1 1\n"
                 "WIDTH 2\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS 2\nDATA ascii\n"
                 f"0.5 1.25 -2.5 3 {rgb:.9g}\n0.25 1e2 0 -1 {rgb:.9g}\n")
    xyz, col = pio.pcread(str(p))
    np.testing.assert_array_equal(xyz, np.array([[1.25, -2.5, 3], [100, 0, -1]], dtype=np.float32))
    np.testing.assert_array_equal(col, [[10, 20, 30], [10, 20, 30]])
    # binary_compressed: field-major payload behind an LZF stream of literal runs and one back reference
    pts = np.arange(12, dtype=np.float32).reshape(4, 3)
    soa = b"".join(pts[:, k].tobytes() for k in range(3))            # 48 bytes
    lzf = bytes([31]) + soa[:32] + bytes([15]) + soa[32:48]           # two literal runs
    hdr = ("VERSION .7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\nWIDTH 4\nHEIGHT 1\nPOINTS 4\nDATA binary_compressed\n").encode()
    q = tmp_path / "bc.pcd"
    q.write_bytes(hdr + struct.pack("II", len(lzf), 48) + lzf)
    got, _ = pio.pcread(str(q))
    np.testing.assert_array_equal(got, pts)
    # a back reference: 16 zero bytes = literal [0] then copy 15 bytes from distance 1, three times over
    z = np.zeros((4, 3), dtype=np.float32)
    stream = bytes([0, 0]) + bytes([(7 << 5) | 0, 47 - 2 - 7, 0])     # literal 1 byte, then 47 more from dist 1
    q2 = tmp_path / "bz.pcd"
    q2.write_bytes(hdr + struct.pack("II", len(stream), 48) + stream)
    got2, _ = pio.pcread(str(q2))
    np.testing.assert_array_equal(got2, z)


def test_pcd_errors(tmp_path):
    with pytest.raises(PcregError):
        pio.pcread(str(tmp_path / "missing.pcd"))
    bad = tmp_path / "bad.pcd"
    bad.write_text("hello\n")
    with pytest.raises(PcregError):
        pio.pcread(str(bad))
    trunc = tmp_path / "t.pcd"
    trunc.write_text("FIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\nWIDTH 3\nHEIGHT 1\nPOINTS 3\nDATA ascii\n1 2 3\n4 5\n")
    with pytest.raises(PcregError):
        pio.pcread(str(trunc))


@pytest.mark.parametrize("compress", [False, True])
def test_mat_v5_against_scipy(tmp_path, compress):
    rng = np.random.default_rng(1)
    desc = rng.poisson(3.0, (300, 980)).astype(np.float64)
    feat = rng.normal(0, 10, (300, 3))
    small = np.array([[1, 2, 3]], dtype=np.uint8)                     # small-element tags, integer class
    single = rng.normal(0, 1, (7, 5)).astype(np.float32)
    p = str(tmp_path / "d.mat")
    scipy.io.savemat(p, {"featModel": feat, "descModel": desc, "tiny": small, "s": single, "txt": "hello"}, do_compression=compress)
    ref = scipy.io.loadmat(p)
    np.testing.assert_array_equal(pio.load_mat(p, "descModel"), ref["descModel"])
    np.testing.assert_array_equal(pio.load_mat(p, "featModel"), feat)
    np.testing.assert_array_equal(pio.load_mat(p, "tiny"), [[1.0, 2.0, 3.0]])
    np.testing.assert_array_equal(pio.load_mat(p, "s"), single.astype(np.float64))
    np.testing.assert_array_equal(pio.load_mat(p), feat)              # first numeric variable
    with pytest.raises(PcregError):
        pio.load_mat(p, "nope")
    with pytest.raises(PcregError):
        pio.load_mat(p, "txt")                                        # char array: listed, not numeric


def test_mat_rejects_other_containers(tmp_path):
    p = tmp_path / "x.mat"
    p.write_bytes(b"\x89HDF\r\n\x1a\n" + b"\0" * 200)                 # a v7.3 (HDF5) signature
    with pytest.raises(PcregError):
        pio.load_mat(str(p))


# ------------------------------------------------------------------------------------------------------------------------------
# Valid files against an independent reading: tests/pcd_ref.py (a parser with struct / numpy dtypes, an LZF decompressor and a
# greedy LZF compressor, written from the formats) and scipy.io.  Everything is compared bit for bit.
import pcd_ref                                                                 # noqa: E402
import scipy.sparse                                                            # noqa: E402
from pcd_ref import MI, MX                                                     # noqa: E402

KINDS = ("ascii", "binary", "binary_compressed")
XYZ = [("x", 4, "F", 1), ("y", 4, "F", 1), ("z", 4, "F", 1)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def same_as_reference(tmp_path, name, data):
    """pcread of the bytes == the independent reading of the same bytes, bit for bit -> (Location, Color)"""
    p = tmp_path / name
    p.write_bytes(data)
    got, color = pio.pcread(str(p))
    want, wcolor = pcd_ref.location_color(data)
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_array_equal(bits(got), bits(want))
    assert (color is None) == (wcolor is None)
    if color is not None:
        np.testing.assert_array_equal(color, wcolor)
    return got, color


def edge_values(typ, size):
    """values of one field type at which a conversion to float32 can go wrong"""
    if typ == "F":
        v = [0.0, -0.0, 1.5, -2.25, np.inf, -np.inf, np.nan, 3.4028234663852886e38, 1e-45, 1.17549435e-38, 16777217.0]
        if size == 8:
            v += [1e39, -1e39, 1e-50, 16777217.000000002, 1.0000000596046448, 3.4028235677973366e38, 0.1]     # inf, 0, and halfway cases
        return np.array(v, dtype=f"<f{size}")
    info = np.iinfo(f"{'i' if typ == 'I' else 'u'}{size}")
    v = [0, 1, info.max, info.min, info.max - 1, 77]
    for e in (2**24 + 1, 2**24 + 3, 2**31 - 65, 2**53 + 1, 2**60 + 2**36 + 1, 2**60 + 2**36, 2**60 + 2**36 - 1, 2**63 + 2**39 + 1):
        v += [x for x in (e, -e) if info.min <= x <= info.max]       # 2^60 + 2^36 + 1 rounds up only if it is rounded ONCE
    return np.array(v, dtype=f"<{'i' if typ == 'I' else 'u'}{size}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("typ,size", sorted(pcd_ref.LEGAL))
def test_pcd_every_type_and_size(tmp_path, typ, size, kind):
    v = edge_values(typ, size)
    cols = [v, v[::-1], np.roll(v, 3)]
    fields = [(k, size, typ, 1) for k in "xyz"]
    got, _ = same_as_reference(tmp_path, "t.pcd", pcd_ref.make_pcd(fields, cols, kind))
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(bits(got[:, 0]), bits(v.astype(np.float32)))        # numpy's conversion, stated here as well


@pytest.mark.parametrize("kind", KINDS)
def test_pcd_layouts(tmp_path, kind):
    rng = np.random.default_rng(3)
    n = 37
    xyz = rng.normal(0, 50, (n, 3)).astype(np.float32)
    word = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    cols = [xyz[:, 0], xyz[:, 1], xyz[:, 2]]
    # a COUNT 3 field and an 8-byte field in front of x, a 1-byte field behind z, then the colour
    fields = [("normal", 4, "F", 3), ("stamp", 8, "U", 1)] + XYZ + [("ring", 1, "U", 1), ("rgb", 4, "U", 1)]
    many = [rng.normal(size=(n, 3)), rng.integers(0, 2**63, n, dtype=np.uint64)] + cols + [rng.integers(0, 256, n), word]
    got, color = same_as_reference(tmp_path, "wide.pcd", pcd_ref.make_pcd(fields, many, kind))
    np.testing.assert_array_equal(bits(got), bits(xyz))
    np.testing.assert_array_equal(color, np.stack([(word >> 16) & 255, (word >> 8) & 255, word & 255], axis=1))
    # rgba, and a float-typed rgb as PCL writes it
    for cname, ctype in (("rgba", "U"), ("rgb", "F")):
        f = XYZ + [(cname, 4, ctype, 1)]
        c4 = word.view(np.float32) if ctype == "F" else word
        if kind == "ascii" and ctype == "F":
            c4 = (word & 0x00FFFFFF).view(np.float32)                  # as text only what %.9g carries: no NaN payloads
        _, color = same_as_reference(tmp_path, cname + ".pcd", pcd_ref.make_pcd(f, cols + [c4], kind))
        assert color is not None
    # COLUMNS for FIELDS; CRLF line ends; no COUNT line; no POINTS line
    same_as_reference(tmp_path, "columns.pcd", pcd_ref.make_pcd(XYZ, cols, kind, key="COLUMNS"))
    got, _ = same_as_reference(tmp_path, "crlf.pcd", pcd_ref.make_pcd(XYZ, cols, kind, eol="\r\n", comments=["# made by a test"]))
    np.testing.assert_array_equal(bits(got), bits(xyz))
    same_as_reference(tmp_path, "nocount.pcd", pcd_ref.make_pcd(XYZ, cols, kind, count_line=False))
    got, _ = same_as_reference(tmp_path, "nopoints.pcd", pcd_ref.make_pcd(XYZ, cols, kind, points=False))
    assert len(got) == n
    # an organised 4 x 5 cloud with NaN points
    org = rng.normal(0, 5, (20, 3)).astype(np.float32)
    org[[0, 7, 19]] = np.nan
    got, _ = same_as_reference(tmp_path, "organised.pcd", pcd_ref.make_pcd(XYZ, list(org.T), kind, width=5, height=4, points=False))
    assert got.shape == (20, 3) and np.isnan(got[[0, 7, 19]]).all() and np.isfinite(np.delete(got, [0, 7, 19], axis=0)).all()
    # zero points, with and without colour
    for f in (XYZ, XYZ + [("rgb", 4, "U", 1)]):
        got, color = same_as_reference(tmp_path, "empty.pcd", pcd_ref.make_pcd(f, [np.zeros(0)] * len(f), kind))
        assert got.shape == (0, 3) and (color is None or color.shape == (0, 3))


def test_pcd_compressed_5000_points(tmp_path):
    """a stream of the reference compressor that holds every kind of LZF item: references with the length-extension byte,
    distances above 255, overlapping copies (distance < length)"""
    rng = np.random.default_rng(9)
    n = 5000
    x = np.repeat(rng.normal(0, 3, n // 250).astype(np.float32), 250)          # long constant runs: distance 4, length up to 264
    y = np.tile(rng.normal(0, 3, 100).astype(np.float32), n // 100)            # period 400 bytes: distances above 255
    z = rng.normal(0, 3, n).astype(np.float32)                                 # incompressible: literal runs
    word = np.tile(np.arange(7, dtype=np.uint32) * 0x010203, n // 7 + 1)[:n]
    fields = XYZ + [("rgb", 4, "U", 1)]
    data = pcd_ref.make_pcd(fields, [x, y, z, word], "binary_compressed")
    h = pcd_ref.parse_header(data)
    comp, raw = struct.unpack_from("<II", data, h["offset"])
    stream = data[h["offset"] + 8:]
    assert raw == n * 16 and comp == len(stream) < raw
    s = pcd_ref.lzf_stats(stream)
    print(s)
    assert s["extended"] > 100 and s["far"] > 100 and s["overlapping"] > 100 and s["literals"] > 100
    got, color = same_as_reference(tmp_path, "big.pcd", data)
    np.testing.assert_array_equal(bits(got), bits(np.stack([x, y, z], axis=1)))
    np.testing.assert_array_equal(color[:, 2], word & 255)


@pytest.mark.parametrize("enc", ["ascii", "binary"])
def test_pcd_write_read_special_values(tmp_path, enc):
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, 3.4028235e38, -3.4028235e38, 1.17549435e-38,
                        0.1, 16777216.0, 1 / 3], dtype=np.float32)
    assert np.signbit(special[3]) and special[5] > 0 and special[7] < np.finfo(np.float32).tiny                    # denormals really
    xyz = np.stack([special, np.roll(special, 5), special[::-1]], axis=1)
    col = np.arange(3 * len(special)).reshape(-1, 3).astype(np.uint8)
    p = tmp_path / f"special_{enc}.pcd"
    pio.pcwrite(str(p), xyz, col, encoding=enc)
    got, gc = pio.pcread(str(p))
    np.testing.assert_array_equal(bits(got), bits(xyz))
    np.testing.assert_array_equal(gc, col)
    want, wc = pcd_ref.location_color(p.read_bytes())                          # and the file itself reads the same independently
    np.testing.assert_array_equal(bits(want), bits(xyz))
    np.testing.assert_array_equal(wc, col)


def test_lzf_reference_round_trip():
    """the reference compressor and decompressor agree with each other on awkward inputs"""
    rng = np.random.default_rng(2)
    for data in (b"", b"a", b"ab" * 3, bytes(1000), bytes(rng.integers(0, 256, 3000, dtype=np.uint8)), (bytes(range(256)) * 40)[:9001],
                 b"abc" + bytes(300) + b"abc" * 100):
        stream = pcd_ref.lzf_compress(data)
        assert pcd_ref.lzf_decompress(stream, len(data)) == data


# ---- MAT
CLASSES = ["int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "float32", "float64", "bool"]


def load_same_as_scipy(path, name, want=None):
    got = pio.load_mat(path, name)
    ref = scipy.io.loadmat(path)[name]
    ref2 = np.asarray(ref).astype(np.float64)
    ref2 = ref2.reshape(ref2.shape[0], -1, order="F") if ref2.ndim > 2 else ref2
    assert got.dtype == np.float64 and got.shape == ref2.shape, (got.shape, ref2.shape)
    np.testing.assert_array_equal(bits(got), bits(ref2))
    if want is not None:
        np.testing.assert_array_equal(bits(got), bits(np.asarray(want, dtype=np.float64)))
    return got


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("cls", CLASSES)
def test_mat_every_class(tmp_path, cls, compress):
    rng = np.random.default_rng(4)
    if cls == "bool":
        a = rng.random((5, 7)) < 0.5
    elif cls.startswith("float"):
        a = rng.normal(0, 1e3, (5, 7)).astype(cls)
        a[0, :4] = [np.nan, np.inf, -0.0, np.finfo(cls).tiny / 4]
    else:
        info = np.iinfo(cls)
        a = rng.integers(info.min, info.max, (5, 7), dtype=cls, endpoint=True)
        a[0, :2] = [info.min, info.max]
        if info.bits == 64:                              # beyond 2^53: numpy's astype(float64), rounded once
            a[1, :3] = [2**53 + 1, info.max - 1, 2**62 + 2**9 + 1]
    p = str(tmp_path / "c.mat")
    scipy.io.savemat(p, {"a": a}, do_compression=compress)
    load_same_as_scipy(p, "a", a.astype(np.float64))


@pytest.mark.parametrize("compress", [False, True])
def test_mat_shapes_and_names(tmp_path, compress):
    rng = np.random.default_rng(6)
    cube = rng.normal(size=(2, 3, 4))
    names = ["q", "four", "fives", "n" * 31]             # 1 and 4 characters: small-element name tags; 5 and 31: full ones
    v = {n: rng.normal(size=(k + 1, 2)) for k, n in enumerate(names)}
    p = str(tmp_path / "s.mat")
    scipy.io.savemat(p, {"cube": cube, "e00": np.zeros((0, 0)), "e05": np.zeros((0, 5)), "e30": np.zeros((3, 0)), "one": np.array([[2.5]]), **v},
                     do_compression=compress)
    got = load_same_as_scipy(p, "cube", cube.reshape(2, 12, order="F"))      # trailing dimensions folded into columns
    assert got.shape == (2, 12)
    assert pio.load_mat(p, "e00").shape == (0, 0) and pio.load_mat(p, "e05").shape == (0, 5) and pio.load_mat(p, "e30").shape == (3, 0)
    load_same_as_scipy(p, "one", [[2.5]])
    for n in names:
        load_same_as_scipy(p, n, v[n])
    with pytest.raises(PcregError):
        pio.load_mat(p, "n" * 30)


@pytest.mark.parametrize("compress", [False, True])
def test_mat_variable_behind_other_classes(tmp_path, compress):
    want = np.arange(15, dtype=np.float64).reshape(3, 5) / 7
    cell = np.empty((1, 2), dtype=object)
    cell[0, 0], cell[0, 1] = np.eye(2), "text"
    p = str(tmp_path / "o.mat")
    scipy.io.savemat(p, {"txt": "some characters", "st": {"a": np.eye(3), "b": "x"}, "ce": cell, "sp": scipy.sparse.csc_matrix(np.eye(4)),
                         "zz": np.array([[1 + 2j, 3 - 1j]]), "want": want, "after": np.ones((2, 2))}, do_compression=compress)
    load_same_as_scipy(p, "want", want)
    np.testing.assert_array_equal(pio.load_mat(p), want)                       # the first REAL NUMERIC variable
    load_same_as_scipy(p, "after")
    for other in ("txt", "st", "ce", "sp", "zz"):
        with pytest.raises(PcregError):
            pio.load_mat(p, other)


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("stored", ["uint8", "uint16", "int32", "int16", "single"])
def test_mat_double_class_stored_as_smaller_type(tmp_path, stored, compress):
    """how MATLAB itself stores a double matrix of whole numbers -- this project's descriptor counts: class mxDOUBLE, the real part
    an element of the smallest integer type that holds the values.  scipy never writes this; the element is made by hand."""
    dt = {"uint8": "<u1", "uint16": "<u2", "int32": "<i4", "int16": "<i2", "single": "<f4"}[stored]
    rng = np.random.default_rng(8)
    lo, hi = {"uint8": (0, 255), "uint16": (0, 65535), "int32": (-2**31, 2**31 - 1), "int16": (-32768, 32767), "single": (-999, 999)}[stored]
    for shape in ((300, 98), (1, 3), (5, 1)):                                # 1 x 3 of uint8: a small-element data tag
        a = rng.integers(lo, hi, shape, endpoint=True).astype(dt)
        a.flat[:2] = [lo, hi]
        el = pcd_ref.mat_matrix("descModel", MX["double"], list(shape), MI[stored], a.tobytes(order="F"))
        other = pcd_ref.mat_matrix("featModel", MX["double"], [2, 3], MI["double"], np.arange(6, dtype="<f8").tobytes())
        p = tmp_path / "m.mat"
        p.write_bytes(pcd_ref.mat_file([other, el], compress))
        got = load_same_as_scipy(str(p), "descModel", a.astype(np.float64))
        assert got.shape == shape
        load_same_as_scipy(str(p), "featModel", np.arange(6.0).reshape(2, 3, order="F"))


@pytest.mark.parametrize("compress", [False, True])
def test_mat_many_variables(tmp_path, compress):
    """more variables than the reader's first reservation for inflated elements, the wanted ones spread among them"""
    rng = np.random.default_rng(12)
    v = {f"v{k:03d}": rng.normal(size=(2, 3)) for k in range(200)}
    p = str(tmp_path / "many.mat")
    scipy.io.savemat(p, v, do_compression=compress)
    for name in ("v000", "v063", "v064", "v065", "v199"):
        load_same_as_scipy(p, name, v[name])
    np.testing.assert_array_equal(pio.load_mat(p), v["v000"])


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("order", ["in_front", "behind", "both"])
@pytest.mark.filterwarnings("ignore:Duplicate variable name")          # scipy gives every opaque object the same name
def test_mat_opaque_object_beside_the_variable(tmp_path, order, compress):
    """a string / table / datetime object is an mxOPAQUE element, which has no dimensions tag (made by hand: scipy does not write
    one): the reader passes it and reads the numeric variable next to it, as scipy does"""
    want = np.arange(12, dtype=np.float64).reshape(3, 4) / 3
    v = pcd_ref.mat_matrix("v", MX["double"], [3, 4], MI["double"], want.tobytes(order="F"))
    els = {"in_front": [pcd_ref.mat_opaque("s"), v], "behind": [v, pcd_ref.mat_opaque("s", "table")],
           "both": [pcd_ref.mat_opaque("s"), v, pcd_ref.mat_opaque("t", "datetime")]}[order]
    p = tmp_path / "opaque.mat"
    p.write_bytes(pcd_ref.mat_file(els, compress))
    load_same_as_scipy(str(p), "v", want)
    np.testing.assert_array_equal(bits(pio.load_mat(str(p))), bits(want))     # the first numeric variable
    with pytest.raises(PcregError, match="not a real numeric array"):
        pio.load_mat(str(p), "s")


@pytest.mark.parametrize("compress", [False, True])
def test_mat_unreadable_variable_is_refused_only_when_asked_for(tmp_path, compress):
    """a numeric variable this reader cannot return (more than INT_MAX elements; no dimensions) does not cost its neighbours"""
    want = np.arange(6, dtype=np.float64).reshape(2, 3)
    v = pcd_ref.mat_matrix("v", MX["double"], [2, 3], MI["double"], want.tobytes(order="F"))
    huge = pcd_ref.mat_matrix("h", MX["uint8"], [65536, 32768], MI["uint8"], bytes(8))
    neg = pcd_ref.mat_matrix("n", MX["double"], [-1, -1], MI["double"], bytes(8))
    p = tmp_path / "beside.mat"
    p.write_bytes(pcd_ref.mat_file([huge, v, neg], compress))
    np.testing.assert_array_equal(bits(pio.load_mat(str(p), "v")), bits(want))
    for name, why in (("h", "INT_MAX"), ("n", "negative"), (None, "INT_MAX")):   # unnamed: the first numeric variable is `h`
        with pytest.raises(PcregError, match=why):
            pio.load_mat(str(p), name)
