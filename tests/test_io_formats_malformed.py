"""Malformed .pcd and .mat files against the readers of pcreg_amd/csrc/io_formats.hip (host code: no GPU).

a. a named corpus through tests/iofuzz/io_formats_main.cpp -- io_formats.hip and a main of its own, built with the address and
   undefined-behaviour sanitizers where the toolchain links them statically (a plain build otherwise; the fixture prints which):
   every file is refused with PCREG_E_ARG and a message that names it, by pcreg_pcd_info already where the header shows the
   fault, or -- where it is legal after all -- read to the values that tests/pcd_ref.py gives;
b. a deterministic mutation sweep over six small valid files: no crash, no sanitizer report, OK or PCREG_E_ARG, and no count
   or shape that the file could not back;
c. the corpus through pcreg_amd.io of the shipped library, in a child python: PcregError, never an abort.
Every file is made here, in tmp_path."""
import json
import os
import random
import re
import struct
import subprocess
import sys
import time
import zlib
from typing import NamedTuple

import numpy as np
import pytest

import pcd_ref
from pcd_ref import MI, MX, mat_file, mat_header, mat_matrix, mat_tag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRCS = [os.path.join(ROOT, "tests", "iofuzz", "io_formats_main.cpp"), os.path.join(ROOT, "pcreg_amd", "csrc", "io_formats.hip")]
# -x hip: io_formats.hip includes the library's common header; --offload-host-only: there is no device code in either file;
# -no-hip-rt: nor a call into the HIP runtime, which is not linked
FLAGS = ["-x", "hip", "--offload-arch=gfx950", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-Wall", "-Wextra"]
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"]
OK, E_ARG = 0, 1
REPORT = re.compile(r"ERROR: \w+Sanitizer|runtime error:|SUMMARY: \w+Sanitizer")


def f32(*v):
    return struct.pack(f"<{len(v)}f", *v)


def hdr(fields="x y z", size="4 4 4", typ="F F F", count="1 1 1", width=1, height=1, points=1, data="binary", extra=()):
    lines = ["# .PCD v0.7 - Point Cloud Data file format", "VERSION 0.7", f"FIELDS {fields}", f"SIZE {size}", f"TYPE {typ}"]
    if count is not None:
        lines.append(f"COUNT {count}")
    lines += [f"WIDTH {width}", f"HEIGHT {height}", "VIEWPOINT 0 0 0 1 0 0 0"]
    if points is not None:
        lines.append(f"POINTS {points}")
    lines += list(extra) + [f"DATA {data}"]
    return ("\n".join(lines) + "\n").encode()


XYZ2 = f32(1, 2, 3, 4, 5, 6)                             # two points, binary
FLAGS_TAG = mat_tag(MI["uint32"], struct.pack("<II", MX["double"], 0))
DIMS11 = mat_tag(MI["int32"], struct.pack("<ii", 1, 1))
NAME_V = mat_tag(MI["int8"], b"v")
ONE = struct.pack("<d", 1.0)


def matrix_of(body: bytes) -> bytes:
    return mat_header() + struct.pack("<II", MI["matrix"], len(body)) + body


# ---------------------------------------------------------------------------------------------- the six valid seeds
def _seed_cloud():
    rng = np.random.default_rng(5)
    xyz = rng.normal(0, 10, (6, 3)).astype(np.float32)
    xyz[3] = xyz[1]                                       # something for the compressor to refer back to
    word = rng.integers(0, 1 << 24, 6).astype(np.uint32)
    fields = [("x", 4, "F", 1), ("y", 4, "F", 1), ("z", 4, "F", 1), ("rgb", 4, "U", 1)]
    return fields, [xyz[:, 0], xyz[:, 1], xyz[:, 2], word]


SEED_V = np.arange(12, dtype=np.float64).reshape(3, 4) * 1.5 - 4
SEED_A = np.array([[7, -8]], dtype=np.int32)
SEED_U8 = (np.arange(12).reshape(3, 4) * 21 % 256).astype(np.uint8)


def _seed_mat(compress):
    els = [mat_matrix("a", MX["int32"], [1, 2], MI["int32"], SEED_A.tobytes(order="F")),
           mat_matrix("v", MX["double"], [3, 4], MI["double"], SEED_V.tobytes(order="F"))]
    return mat_file(els, compress)


SEEDS = {
    "seed_pcd_ascii": ("pcd", pcd_ref.make_pcd(*_seed_cloud(), "ascii")),
    "seed_pcd_binary": ("pcd", pcd_ref.make_pcd(*_seed_cloud(), "binary")),
    "seed_pcd_compressed": ("pcd", pcd_ref.make_pcd(*_seed_cloud(), "binary_compressed")),
    "seed_mat_plain": ("mat", _seed_mat(False)),
    "seed_mat_compressed": ("mat", _seed_mat(True)),
    # a double-class variable whose numbers are whole and small: MATLAB stores its real part as miUINT8
    "seed_mat_double_as_uint8": ("mat", mat_file([mat_matrix("v", MX["double"], [3, 4], MI["uint8"], SEED_U8.tobytes(order="F"))])),
}
SEED_MAT_VALUES = {"seed_mat_plain": {"": SEED_A.astype(np.float64), "v": SEED_V},
                   "seed_mat_compressed": {"": SEED_A.astype(np.float64), "v": SEED_V},
                   "seed_mat_double_as_uint8": {"": SEED_U8.astype(np.float64), "v": SEED_U8.astype(np.float64)}}


# ---------------------------------------------------------------------------------------------- the named corpus
class Case(NamedTuple):
    ext: str
    data: bytes
    legal: bool = False          # refused unless legal
    where: str = "info"          # a refused .pcd: "info" = pcreg_pcd_info refuses it (the header or the file's size shows the fault),
    #                              "read" = the payload's content shows it, so pcreg_pcd_read may be the one that refuses
    values: dict = None          # a legal .mat: name -> the matrix


def _corpus():
    c = {}
    # -- the twelve files that first showed the readers' faults (overruns, an escaping exception, wrapped counts and shapes)
    c["t01_f_size_2"] = Case("pcd", hdr(size="2 2 2") + b"\0" * 6)
    c["t02_rgb_size_1"] = Case("pcd", hdr("x y z rgb", "4 4 4 1", "F F F U", "1 1 1 1") + f32(1, 2, 3) + b"\x07")
    c["t03_size_negative"] = Case("pcd", hdr(size="-4 4 4", width=2, points=2) + XYZ2)
    c["t04_count_negative"] = Case("pcd", hdr(count="1 1 -5", width=2, points=2) + XYZ2)
    c["t05_points_4e12"] = Case("pcd", hdr(points=4000000000000) + f32(1, 2, 3))
    c["t06_points_minus_1"] = Case("pcd", hdr(points=-1) + f32(1, 2, 3))
    c["t07_size_16_ascii"] = Case("pcd", hdr(size="16 16 16", data="ascii") + b"1 2 3\n")
    c["t08_flags_tag_only"] = Case("mat", matrix_of(struct.pack("<II", MI["uint32"], 8)))
    c["t09_dims_count_huge"] = Case("mat", matrix_of(FLAGS_TAG + struct.pack("<II", MI["int32"], 0x7FFFFFF0) + struct.pack("<ii", 1, 1)))
    assert len(c["t09_dims_count_huge"].data) == 168
    c["t10_name_count_huge"] = Case("mat", matrix_of(FLAGS_TAG + DIMS11 + struct.pack("<II", MI["int8"], 0x00FFFFF0) + b"v" * 8))
    c["t11_dims_negative"] = Case("mat", mat_file([mat_matrix("v", MX["double"], [-1, -1], MI["double"], ONE)]))
    c["t12_dims_product_wraps"] = Case("mat", mat_file([mat_matrix("v", MX["double"], [65536] * 4, MI["double"], ONE)]))
    # -- PCD headers
    c["size_zero"] = Case("pcd", hdr(size="0 4 4", width=2, points=2) + XYZ2)
    c["count_zero"] = Case("pcd", hdr(count="1 1 0", width=2, points=2) + XYZ2)
    c["size_list_short"] = Case("pcd", hdr(size="4 4", width=2, points=2) + XYZ2)
    c["size_list_long"] = Case("pcd", hdr(size="4 4 4 4", width=2, points=2) + XYZ2)
    c["type_list_short"] = Case("pcd", hdr(typ="F F", width=2, points=2) + XYZ2)
    c["count_list_short"] = Case("pcd", hdr(count="1 1", width=2, points=2) + XYZ2)
    c["count_list_long"] = Case("pcd", hdr(count="1 1 1 1", width=2, points=2) + XYZ2)
    c["type_other"] = Case("pcd", hdr(typ="F F D", width=2, points=2) + XYZ2)
    c["type_word"] = Case("pcd", hdr(typ="F F Float", width=2, points=2) + XYZ2)
    c["f_size_1"] = Case("pcd", hdr(size="1 1 1") + b"\1\2\3")
    c["f_size_16"] = Case("pcd", hdr(size="4 4 16") + b"\0" * 24)
    c["i_size_3"] = Case("pcd", hdr(size="3 3 3", typ="I I I") + b"\0" * 9)
    c["u_size_16"] = Case("pcd", hdr(size="16 16 16", typ="U U U") + b"\0" * 48)
    c["size_not_a_number"] = Case("pcd", hdr(size="4 4 4x", width=2, points=2) + XYZ2)
    i8 = np.array([[2**60 + 2**36 + 1, -(2**40) - 3, 2**24 + 1], [-(2**63), 2**63 - 1, 5]], dtype="<i8")     # 2^60 + 2^36 + 1 rounds up
    c["i8_is_64_bits"] = Case("pcd", hdr(size="8 8 8", typ="I I I", width=2, points=2) + i8.tobytes(), legal=True)          # to float32 only
    u8 = np.array([[2**63 + 2**40, 2**32 + 7, 1], [2**64 - 1, 2**60 + 2**36 + 1, 0]], dtype="<u8")                      # if rounded once
    c["u8_is_64_bits"] = Case("pcd", hdr(size="8 8 8", typ="U U U", width=2, points=2) + u8.tobytes(), legal=True)
    c["i8_ascii"] = Case("pcd", hdr(size="8 8 8", typ="I I I", data="ascii") + b"1152921573326323713 -1099511627779 16777217\n", legal=True)
    c["x_twice"] = Case("pcd", hdr("x x y z", "4 4 4 4", "F F F F", "1 1 1 1") + f32(1, 2, 3, 4))
    c["no_z"] = Case("pcd", hdr("x y w") + f32(1, 2, 3))
    c["width_height_2p32"] = Case("pcd", hdr(width=65536, height=65536, points=None) + f32(1, 2, 3))
    c["width_height_2p64"] = Case("pcd", hdr(width=4294967296, height=4294967296, points=None) + f32(1, 2, 3))
    c["width_negative"] = Case("pcd", hdr(width=-3, height=-1, points=None) + f32(1, 2, 3) * 3)
    # -- POINTS the payload cannot back
    c["points_gt_payload_binary"] = Case("pcd", hdr(width=5, points=5) + XYZ2)
    c["points_gt_payload_ascii"] = Case("pcd", hdr(width=5, points=5, data="ascii") + b"1.5 2.5 3.5\n4.5 5.5 6.5\n", where="read")
    c["points_2e9_ascii"] = Case("pcd", hdr(width=2000000000, points=2000000000, data="ascii") + b"1 2 3\n")
    c["points_2e9_binary"] = Case("pcd", hdr(width=2000000000, points=2000000000) + XYZ2)
    lit24 = bytes([23]) + XYZ2                            # one literal run: the 24 bytes of two points
    bc = dict(width=2, points=2, data="binary_compressed")
    c["points_gt_payload_compressed"] = Case("pcd", hdr(width=5, points=5, data="binary_compressed") + struct.pack("<II", 25, 60) + lit24, where="read")
    c["points_2e8_compressed"] = Case("pcd", hdr(width=200000000, points=200000000, data="binary_compressed") + struct.pack("<II", 25, 2400000000) + lit24)
    c["compressed_size_exceeds_file"] = Case("pcd", hdr(**bc) + struct.pack("<II", 1000, 24) + lit24)
    c["compressed_raw_size_differs"] = Case("pcd", hdr(**bc) + struct.pack("<II", 25, 36) + lit24)
    c["compressed_no_sizes"] = Case("pcd", hdr(**bc) + b"\x19\0\0")
    ref_before = bytes([0, 9]) + bytes([(1 << 5) | 0, 4]) + bytes([19]) + XYZ2[:20]          # 1 literal, then 3 bytes from distance 5
    c["lzf_reference_before_start"] = Case("pcd", hdr(**bc) + struct.pack("<II", len(ref_before), 24) + ref_before, where="read")
    run_past = bytes([23]) + XYZ2 + bytes([3, 1, 2, 3, 4])
    c["lzf_literal_run_past_end"] = Case("pcd", hdr(**bc) + struct.pack("<II", len(run_past), 24) + run_past, where="read")
    copy_past = bytes([0, 9]) + bytes([(7 << 5) | 0, 255, 0])                                   # 1 literal, then 264 bytes from distance 1
    c["lzf_copy_past_end"] = Case("pcd", hdr(**bc) + struct.pack("<II", len(copy_past), 24) + copy_past, where="read")
    # -- header lines
    c["header_ends_without_newline"] = Case("pcd", hdr()[:hdr().index(b"COUNT")].rstrip(b"\n"))
    c["data_line_without_newline"] = Case("pcd", hdr(width=0, points=0, data="ascii").rstrip(b"\n"), legal=True)
    long_comment = "# " + "c" * 4093 + "POINTS 99 " + "d" * 900          # a reader with a 4096-byte line buffer sees POINTS 99 here
    c["header_line_5000"] = Case("pcd", hdr(width=2, points=2, extra=[long_comment]) + XYZ2, legal=True)
    c["header_nul_bytes"] = Case("pcd", hdr().replace(b"SIZE 4 4 4", b"SIZE 4 \0 4") + f32(1, 2, 3))
    # -- ASCII tokens
    asc = dict(width=2, points=2, data="ascii")
    c["ascii_not_a_number"] = Case("pcd", hdr(**asc) + b"1 2 3\n4 abc 6\n", where="read")
    c["ascii_trailing_garbage"] = Case("pcd", hdr(**asc) + b"1 2 3\n4 5.5.5 6\n", where="read")
    c["ascii_int_not_a_number"] = Case("pcd", hdr("x y z rgb", "4 4 4 4", "F F F U", "1 1 1 1", **asc) + b"1 2 3 4\n4 5 6 zz\n", where="read")
    au = dict(fields="x y z rgb", size="4 4 4 4", typ="F F F U", count="1 1 1 1", width=1, points=1, data="ascii")
    c["ascii_u_minus"] = Case("pcd", hdr(**au) + b"1 2 3 -1\n", where="read")
    c["ascii_u4_2p32"] = Case("pcd", hdr(**au) + b"1 2 3 4294967296\n", where="read")
    c["ascii_u4_max"] = Case("pcd", hdr(**au) + b"1 2 3 4294967295\n", legal=True)
    for typ, size, bad, good in (("U", 1, "256 0 0", "255 0 0"), ("U", 2, "0 65536 0", "0 65535 0"), ("U", 8, "0 0 18446744073709551616", "0 0 18446744073709551615"),
                                 ("I", 1, "128 0 -129", "127 0 -128"), ("I", 2, "0 -32769 0", "32767 -32768 0"), ("I", 4, "2147483648 0 0", "2147483647 -2147483648 0"),
                                 ("I", 8, "0 0 9223372036854775808", "9223372036854775807 -9223372036854775808 0")):
        kw = dict(size=" ".join([str(size)] * 3), typ=" ".join([typ] * 3), data="ascii")
        c[f"ascii_{typ.lower()}{size}_out_of_range"] = Case("pcd", hdr(**kw) + bad.encode() + b"\n", where="read")
        c[f"ascii_{typ.lower()}{size}_limits"] = Case("pcd", hdr(**kw) + good.encode() + b"\n", legal=True)
    c["ascii_nan_inf"] = Case("pcd", hdr(**asc) + b"nan -nan inf\n-inf NaN 1e-42\n", legal=True)
    # -- MAT
    c["mat_element_exceeds_file"] = Case("mat", mat_header() + struct.pack("<II", MI["matrix"], 5000) + FLAGS_TAG + DIMS11 + NAME_V)
    z = zlib.compress(mat_tag(MI["double"], ONE * 2))
    c["mat_compressed_not_a_matrix"] = Case("mat", mat_header() + struct.pack("<II", MI["compressed"], len(z)) + z)
    good = mat_matrix("v", MX["double"], [3, 4], MI["double"], SEED_V.tobytes(order="F"))
    z = zlib.compress(good + good)
    c["mat_compressed_two_matrices"] = Case("mat", mat_header() + struct.pack("<II", MI["compressed"], len(z)) + z, legal=True,
                                            values={"": SEED_V, "v": SEED_V})                  # the first is read, the rest passed over
    z = zlib.compress(good)[: len(zlib.compress(good)) // 2]
    c["mat_zlib_truncated"] = Case("mat", mat_header() + struct.pack("<II", MI["compressed"], len(z)) + z)
    c["mat_data_type_utf8"] = Case("mat", mat_file([mat_matrix("v", MX["double"], [1, 1], MI["utf8"], ONE)]))
    c["mat_data_type_matrix"] = Case("mat", mat_file([mat_matrix("v", MX["double"], [1, 1], MI["matrix"], ONE)]))
    c["mat_data_type_0"] = Case("mat", mat_file([mat_matrix("v", MX["double"], [1, 1], 0, ONE)]))
    c["mat_dims_0_entries"] = Case("mat", matrix_of(FLAGS_TAG + struct.pack("<II", MI["int32"], 0) + NAME_V + mat_tag(MI["double"], ONE)))
    c["mat_dims_1_entry"] = Case("mat", mat_file([mat_matrix("v", MX["double"], [1], MI["double"], ONE)]))
    c["mat_dims_count_7"] = Case("mat", matrix_of(FLAGS_TAG + struct.pack("<II", MI["int32"], 7) + struct.pack("<ii", 1, 1) + NAME_V + mat_tag(MI["double"], ONE)))
    c["mat_shape_gt_int_max"] = Case("mat", mat_file([mat_matrix("v", MX["uint8"], [65536, 32768], MI["uint8"], ONE)]))
    c["mat_cols_gt_int_max"] = Case("mat", mat_file([mat_matrix("v", MX["uint8"], [0, 65536, 65536], MI["uint8"], ONE)]))
    c["mat_data_shorter_than_shape"] = Case("mat", mat_file([mat_matrix("v", MX["double"], [3, 4], MI["double"], ONE * 11)]))
    c["mat_data_count_exceeds_element"] = Case("mat", matrix_of(FLAGS_TAG + DIMS11 + NAME_V + struct.pack("<II", MI["double"], 800) + ONE))
    c["mat_header_only_127"] = Case("mat", mat_header()[:127])
    v4 = struct.pack("<5i", 0, 1, 1, 0, 2) + b"v\0" + ONE                                       # MAT v4: type, rows, cols, imagf, namlen
    c["mat_v4"] = Case("mat", v4)
    be = (struct.pack(">II", MI["uint32"], 8) + struct.pack(">II", MX["double"], 0) + struct.pack(">II", MI["int32"], 8) + struct.pack(">ii", 1, 1)
          + struct.pack(">I", 1 << 16 | MI["int8"]) + b"v\0\0\0" + struct.pack(">II", MI["double"], 8) + struct.pack(">d", 1.0))
    c["mat_v5_big_endian"] = Case("mat", mat_header(b"MI") + struct.pack(">II", MI["matrix"], len(be)) + be)
    # -- more compressed variables than the reader first makes room for, the wanted one last
    many = [mat_matrix(f"w{k}", MX["double"], [1, 1], MI["double"], struct.pack("<d", k)) for k in range(150)] + [good]
    c["mat_151_compressed_variables"] = Case("mat", mat_file(many, compress=True), legal=True, values={"": np.array([[0.0]]), "v": SEED_V})
    # -- variables this reader does not read, and one it cannot, beside the wanted one: the file is not refused for them
    opaque = pcd_ref.mat_opaque("s")
    huge = mat_matrix("h", MX["uint8"], [65536, 32768], MI["uint8"], ONE)
    nodims = matrix_of(FLAGS_TAG + struct.pack("<II", MI["int32"], 0) + mat_tag(MI["int8"], b"n") + mat_tag(MI["double"], ONE))[128:]
    for compress in (False, True):
        tail = "_compressed" if compress else ""
        c["mat_opaque_in_front" + tail] = Case("mat", mat_file([opaque, good], compress), legal=True, values={"": SEED_V, "v": SEED_V})
        c["mat_opaque_behind" + tail] = Case("mat", mat_file([good, opaque], compress), legal=True, values={"": SEED_V, "v": SEED_V})
        c["mat_unreadable_behind" + tail] = Case("mat", mat_file([good, huge, nodims], compress), legal=True, values={"": SEED_V, "v": SEED_V})
    # -- the seeds themselves: the program's OK path
    for name, (ext, data) in SEEDS.items():
        c[name] = Case(ext, data, legal=True, values=SEED_MAT_VALUES.get(name))
    return c


CORPUS = _corpus()
TABLE = sorted(k for k in CORPUS if re.match(r"t\d\d_", k))
assert len(TABLE) == 12


# ---------------------------------------------------------------------------------------------- the program
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("iofuzz")
    exe, probe = str(d / "io_formats_main"), str(d / "probe.pcd")
    with open(probe, "wb") as f:
        f.write(SEEDS["seed_pcd_binary"][1])
    build = "-fsanitize=address,undefined"
    san = subprocess.run([HIPCC] + FLAGS + SAN + SRCS + ["-o", exe, "-lz"], stderr=subprocess.PIPE, text=True)
    why = "it does not build:\n" + san.stderr[-2000:]
    if san.returncode == 0:
        # the program prints the file's name before its first call: no output at all = it could not start (no room for the shadow
        # memory, say); the leak checker unable to stop the world at exit is the machine's doing too.  Anything else that goes
        # wrong on this valid file is a fault of the code under test, and is not hidden behind a plain build
        r = subprocess.run([exe, probe], capture_output=True, text=True, errors="replace")
        cannot_run = not r.stdout or "LeakSanitizer has encountered a fatal error" in r.stderr
        if r.returncode == 0 and not REPORT.search(r.stderr):
            why = None
        elif cannot_run:
            why = f"it does not run here (exit status {r.returncode}):\n" + r.stderr[-2000:]
        else:
            pytest.fail(f"the sanitized program fails on a valid file (exit status {r.returncode}):\n" + r.stderr[-3000:])
    if why:
        print("io_formats_main: no sanitized build here, a plain build instead -- " + why)
        build = "plain"
        subprocess.check_call([HIPCC] + FLAGS + SRCS + ["-o", exe, "-lz"])
        subprocess.check_call([exe, probe], stdout=subprocess.DEVNULL)
    print(f"io_formats_main: {build} build")
    return exe, build


def parse(stdout: str):
    """-> {path: [call, ...]}, a call being the dict of its fields"""
    res = {}
    for line in stdout.splitlines():
        part = line.split("\t")
        calls = []
        for p in part[1:]:
            k, _, v = p.partition("=")
            if k == "call":
                calls.append({"call": v})
            else:
                calls[-1][k] = v
        res[part[0]] = calls
    return res


def run(program, args, timeout=300):
    """the program's parsed output; fails on a crash, a sanitizer report, a non-zero exit"""
    r = subprocess.run([program[0]] + args, capture_output=True, text=True, errors="replace", timeout=timeout)
    report = [ln for ln in r.stderr.splitlines() if REPORT.search(ln)]
    report = [ln for ln in report if "SUMMARY" in ln] or report
    last = r.stdout.splitlines()[-1].split("\t")[0] if r.stdout.strip() else "<no output>"
    assert r.returncode == 0 and not report, f"exit status {r.returncode} at {os.path.basename(last)}: " + (" | ".join(report) or r.stderr[-400:])
    return parse(r.stdout)


def refused(call, fname):
    assert int(call["rc"]) == E_ARG, call
    assert call.get("msg") and fname in call["msg"], call


# ---------------------------------------------------------------------------------------------- a. the named corpus
@pytest.mark.parametrize("name", list(CORPUS))
def test_named_file(program, tmp_path, name):
    case = CORPUS[name]
    fname = f"{name}.{case.ext}"
    path = str(tmp_path / fname)
    with open(path, "wb") as f:
        f.write(case.data)
    calls = run(program, ["--name", "v", path])[path]
    print(name, calls)
    if case.ext == "pcd":
        info = calls[0]
        assert info["call"] == "info"
        if not case.legal:
            with pytest.raises(Exception):                 # the independent reading refuses it too
                pcd_ref.location_word(case.data)
            if case.where == "info" or int(info["rc"]) != OK:
                refused(info, fname)
                assert len(calls) == 1
            else:                                        # the payload's content is at fault: a count the file's size backs, then a refusal
                assert 0 <= int(info["n"]) <= len(case.data)
                refused(calls[1], fname)
            return
        xyz, word = pcd_ref.location_word(case.data)
        assert int(info["rc"]) == OK and int(info["n"]) == len(xyz) and int(info["rgb"]) == (word is not None), info
        read = calls[1]
        assert int(read["rc"]) == OK, read
        want = pcd_ref.fnv1a(np.asfortranarray(xyz).tobytes(order="F"), b"" if word is None else word.tobytes())
        assert int(read["bytes"]) == xyz.nbytes + (0 if word is None else word.nbytes) and read["sum"] == want, (read, want)
        return
    assert [(c["call"], c["name"]) for c in calls] in ([("shape", ""), ("shape", "v")], [("shape", ""), ("data", ""), ("shape", "v"), ("data", "v")])
    if not case.legal:
        for c in calls:
            assert c["call"] == "shape" and int(c["rc"]) != OK, c          # no shape, negative or wrapped ones least of all
            refused(c, fname)
        return
    for shape, data in (calls[0:2], calls[2:4]):
        want = case.values[shape["name"]]
        assert int(shape["rc"]) == OK and (int(shape["rows"]), int(shape["cols"])) == want.shape, shape
        assert int(data["rc"]) == OK and (int(data["rows"]), int(data["cols"])) == want.shape, data
        assert data["sum"] == pcd_ref.fnv1a(want.astype("<f8").tobytes(order="F")), data


# ---------------------------------------------------------------------------------------------- b. the mutation sweep
WORDS = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
TOKENS = (b"-1", b"0", b"3", b"2147483648", b"99999999999999")


def tag_region(ext: str, data: bytes) -> int:
    """the bytes in front of the payload: a PCD's header (and the two sizes of a compressed block), a MAT file's header and tags --
    these seeds are small enough to take the whole MAT file"""
    if ext == "mat":
        return len(data)
    end = data.index(b"\n", data.index(b"\nDATA ") + 1) + 1
    return min(len(data), end + (8 if b"DATA binary_compressed" in data else 0))


COMPOUND = 2000                                          # per seed


def mutants(ext: str, data: bytes):
    """(description, bytes) of every mutant, in a fixed order: the four single-edit classes, then COMPOUND mutants of two to four
    edits each -- bytes set, words set, runs deleted, inserted or copied from elsewhere -- drawn with a fixed seed"""
    for n in range(len(data)):
        yield f"prefix {n}", data[:n]
    for i in range(tag_region(ext, data)):
        for v in (0x00, 0x7F, 0x80, 0xFF):
            if data[i] != v:
                yield f"byte {i} = {v:#04x}", data[:i] + bytes([v]) + data[i + 1:]
    for i in range(0, len(data) - 3, 4):
        w, = struct.unpack_from("<I", data, i)
        for v in dict.fromkeys(WORDS + ((w + 1) & 0xFFFFFFFF, (w - 1) & 0xFFFFFFFF)):
            if v != w:
                yield f"word {i} = {v:#010x}", data[:i] + struct.pack("<I", v) + data[i + 4:]
    if ext == "pcd":
        head = tag_region(ext, data) - (8 if b"DATA binary_compressed" in data else 0)
        for m in re.finditer(rb"(?<=[ \n])-?[0-9.]+(?=[ \r\n])", data[:head]):
            for t in TOKENS:
                if m.group() != t:
                    yield f"token at {m.start()} ({m.group().decode()}) = {t.decode()}", data[:m.start()] + t + data[m.end():]
    rnd = random.Random(len(data))
    for k in range(COMPOUND):
        b = bytearray(data)
        for _ in range(rnd.randrange(2, 5)):
            i, op = rnd.randrange(len(b)), rnd.randrange(5)
            if op == 0:
                b[i] = rnd.choice((0x00, 0x7F, 0x80, 0xFF, rnd.randrange(256)))
            elif op == 1:
                b[i:i + 4] = struct.pack("<I", rnd.choice(WORDS + (8, len(b), rnd.randrange(1 << 32))))
            elif op == 2:
                del b[i:i + rnd.randrange(1, 9)]
            elif op == 3:
                b[i:i] = bytes(rnd.randrange(256) for _ in range(rnd.randrange(1, 9)))
            else:
                j = rnd.randrange(len(b))
                b[i:i + 8] = b[j:j + 8]
            if not b:
                break
        yield f"compound {k}", bytes(b)


def check_mutant(ext, data, calls):
    """-> what is wrong with the program's answer for this mutant, or None"""
    for c in calls:
        if "skipped" in c:
            return f"a count above the program's cap: {calls}"
        if int(c["rc"]) not in (OK, E_ARG):
            return f"return code {c['rc']}"
        if int(c["rc"]) == E_ARG and not c.get("msg"):
            return "no message"
    if ext == "pcd":
        if int(calls[0]["rc"]) == OK and not 0 <= int(calls[0]["n"]) <= len(data):
            return f"{calls[0]['n']} points from {len(data)} bytes"
        return None
    variables, inflated = pcd_ref.mat_walk(data)
    for c in calls:
        if int(c["rc"]) != OK:
            continue
        rows, cols = int(c["rows"]), int(c["cols"])
        hit = [v for v in variables if v["mi"] is not None and (c["name"] == "" or v["name"] == c["name"])]
        size = pcd_ref.MI_SIZE.get(hit[0]["mi"], 1) if hit else 1          # 1: the smallest element there is
        if rows < 0 or cols < 0 or rows * cols * size > inflated:
            return f"{rows} x {cols} elements of {size} bytes from {inflated} bytes"
    return None


def test_mutation_sweep(program, tmp_path):
    t0 = time.perf_counter()
    total, wrong = 0, []
    for seed, (ext, data) in SEEDS.items():
        d = tmp_path / seed
        d.mkdir()
        batch = {}
        for k, (what, mutant) in enumerate(mutants(ext, data)):
            path = str(d / f"m{k:05d}.{ext}")
            with open(path, "wb") as f:
                f.write(mutant)
            batch[path] = (what, mutant)
        lst = str(d / "list.txt")
        with open(lst, "w") as f:
            f.write("".join(p + ("\tv\n" if ext == "mat" else "\n") for p in batch))
        res = run(program, ["--list", lst])
        assert list(res) == list(batch), f"{seed}: {len(res)} answers for {len(batch)} mutants"
        for path, (what, mutant) in batch.items():
            bad = check_mutant(ext, mutant, res[path])
            if bad:
                wrong.append(f"{seed}, {what}: {bad}")
        print(f"{seed}: {len(data)} bytes, {len(batch)} mutants, {sum(int(c['rc']) == OK for r in res.values() for c in r)} calls OK")
        total += len(batch)
    print(f"{total} mutants ({program[1]} build) in {time.perf_counter() - t0:.1f} s, {len(wrong)} wrong")
    assert not wrong, "\n".join(wrong[:20])


# ---------------------------------------------------------------------------------------------- c. through pcreg_amd.io
CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from pcreg_amd import io
from pcreg_amd._lib import PcregError
out = {}
for line in open(sys.argv[2]):
    path = line.rstrip("\n")
    print(path, flush=True)
    res = []
    for name in ([None] if path.endswith(".pcd") else [None, "v"]):
        try:
            if path.endswith(".pcd"):
                xyz, color = io.pcread(path)
                res.append(["ok", list(xyz.shape), xyz.tobytes().hex(), None if color is None else color.tobytes().hex()])
            else:
                m = io.load_mat(path, name)
                res.append(["ok", list(m.shape), m.tobytes(order="F").hex(), None])
        except PcregError as e:
            res.append(["PcregError", str(e)])
        except Exception as e:
            res.append([type(e).__name__, str(e)])
    out[path] = res
with open(sys.argv[3], "w") as f:
    json.dump(out, f)
"""


@pytest.fixture(scope="module")
def through_python(tmp_path_factory):
    """the whole corpus through pcread / load_mat of the shipped library in ONE fresh child python -> (exit status, results, last file)"""
    d = tmp_path_factory.mktemp("iopy")
    paths = {}
    for name, case in CORPUS.items():
        paths[name] = str(d / f"{name}.{case.ext}")
        with open(paths[name], "wb") as f:
            f.write(case.data)
    script, lst, out = str(d / "child.py"), str(d / "list.txt"), str(d / "out.json")
    with open(script, "w") as f:
        f.write(CHILD)
    with open(lst, "w") as f:
        f.write("".join(p + "\n" for p in paths.values()))
    r = subprocess.run([sys.executable, script, ROOT, lst, out], capture_output=True, text=True, errors="replace", timeout=600)
    res = json.load(open(out)) if os.path.exists(out) else {}
    last = r.stdout.splitlines()[-1] if r.stdout.strip() else "<none>"
    return r.returncode, {n: res.get(p) for n, p in paths.items()}, os.path.basename(last), r.stderr[-600:]


def test_child_python_exits_0(through_python):
    status, res, last, err = through_python
    assert status == 0 and all(res.values()), f"the child ended with status {status} at {last}: {err}"


@pytest.mark.parametrize("name", list(CORPUS))
def test_named_file_through_python(through_python, name):
    status, res, last, _ = through_python
    case, got = CORPUS[name], res[name]
    assert got is not None, f"no answer: the child ended with status {status} at {last}"
    if not case.legal:
        assert [g[0] for g in got] == ["PcregError"] * len(got), got
        assert all(f"{name}.{case.ext}" in g[1] for g in got), got
        return
    if case.ext == "pcd":
        xyz, color = pcd_ref.location_color(case.data)
        assert got[0] == ["ok", list(xyz.shape), xyz.tobytes().hex(), None if color is None else color.tobytes().hex()]
        return
    for g, key in zip(got, ("", "v")):
        want = case.values[key]
        assert g == ["ok", list(want.shape), want.astype("<f8").tobytes(order="F").hex(), None]
