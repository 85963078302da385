"""GPU: the shim's bulk reader and writer of point vectors, libff::lsa_load_points / lsa_dump_points (one lsa_gN_decompress /
lsa_gN_validate / lsa_gN_compress call per vector), against the reference's per-element loops -- tests/cpp/test_shim_points_io.cc,
built against the shim as tests/test_shim_io.py builds its program, for [], -DNO_PT_COMPRESSION and -DBINARY_OUTPUT.

With 300 G1 and 300 G2 points, infinity among them: lsa_dump_points writes exactly the bytes of the dumpIntoFile loop;
lsa_load_points returns exactly what loadFromFile returns (text modes; under BINARY_OUTPUT the reference's read loop takes the
"\\n" separators for data and cannot read its own output, so there the result is compared with the normalised points only);
external_point_seen() is false after a checked load and true after one operator>>.  Then this script replaces one line of a
dumped G2 file by a point of the twist outside G2 (from the big-int model): the checked load refuses it naming the index, the
unchecked load takes it."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "pymodel"))
import bn254_model as m  # noqa: E402
import test_point_load_gpu as pl  # noqa: E402  (f2_sqrt, g2_rhs, twist_ladder: plain helpers)

FLAG_SETS = [[], ["-DNO_PT_COMPRESSION"], ["-DBINARY_OUTPUT"]]
INDEX = 123


def build(tmp_path, flags):
    import legosnark_amd
    if not os.path.exists(legosnark_amd.LIB_PATH):
        legosnark_amd.build()
    exe = str(tmp_path / ("shim_points_io" + "".join(f.replace("-D", "_") for f in flags)))
    libdir = os.path.join(ROOT, "legosnark_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", *flags, "-I", os.path.join(ROOT, "legosnark_amd", "shim"),
                           os.path.join(ROOT, "tests", "cpp", "test_shim_points_io.cc"), "-o", exe,
                           "-L" + libdir, "-llegosnark_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def run(exe, *args):
    r = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:]
    return r.stdout


def outside_point():
    i = 1
    while True:
        y = pl.f2_sqrt(pl.g2_rhs((i, 1)))
        if y is not None:
            t = ((i, 1), y)
            assert m.g2_is_on_curve(t) and pl.twist_ladder(t, m.R) is not None
            return t
        i += 1


def replace_entry(data, flags, t):
    (x0, x1), (y0, y1) = t
    if "-DBINARY_OUTPUT" in flags:
        entry = b"0" + x0.to_bytes(32, "little") + x1.to_bytes(32, "little") + str(y0 & 1).encode() + b"\n"
        head = data.index(b"\n") + 1
        assert (len(data) - head) % len(entry) == 0 and (len(data) - head) // len(entry) == 300
        at = head + INDEX * len(entry)
        assert data[at:at + 1] == b"0"                             # the point it replaces is not infinity
        return data[:at] + entry + data[at + len(entry):]
    lines = data.split(b"\n")
    assert lines[0] == b"300" and len(lines) == 302 and lines[1 + INDEX].startswith(b"0 ")
    tail = "%d %d" % (y0, y1) if "-DNO_PT_COMPRESSION" in flags else "%d" % (y0 & 1)
    lines[1 + INDEX] = ("0 %d %d %s" % (x0, x1, tail)).encode()
    return b"\n".join(lines)


@pytest.mark.parametrize("flags", FLAG_SETS, ids=["default", "no_pt_compression", "binary_output"])
def test_bulk_reader_and_writer_against_the_per_element_loops(tmp_path, flags):
    exe = build(tmp_path, flags)
    out = run(exe)
    assert "G1: 300 points" in out and "G2: 300 points" in out
    path = str(tmp_path / "g2.key")
    run(exe, "dump", path)
    with open(path, "rb") as f:
        data = f.read()
    with open(path, "wb") as f:
        f.write(replace_entry(data, flags, outside_point()))
    out = run(exe, "load", path, "1")
    assert "REJECTED" in out and "point %d " % INDEX in out and "NOT_IN_SUBGROUP" in out and "external_point_seen 0" in out, out
    out = run(exe, "load", path, "0")
    assert "LOADED 300" in out and "external_point_seen 1" in out, out
    with open(path, "wb") as f:                                        # untouched, the checked load takes the file
        f.write(data)
    out = run(exe, "load", path, "1")
    assert "LOADED 300" in out and "external_point_seen 0" in out, out
