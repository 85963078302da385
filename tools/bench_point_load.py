#!/usr/bin/env python3
"""Times key loading and writing (csrc/point_load.hip) at n = 2^16 and 2^20 points:

  the six calls    lsa_g1/g2_decompress, _validate, _compress -- G2 with and without the subgroup test -- on host arrays (numpy in
                   and out: upload, kernels, download) and on device-resident tensors (kernels only)
  the yardstick    what the library offered before: the shim's per-element operator>> / operator<< loop over the same kind of
                   points on ONE host core (tools/native/point_io_loop.cc, built here with g++), which performs no subgroup test;
                   beside it the shim's bulk lsa_load_points / lsa_dump_points, text parsing included

Every shape is warmed first (code objects, staging buffers); each figure is the median, minimum and maximum of --reps blocking
repetitions (host clock around the call and a device synchronise).  One JSON line per figure, also written to --out.
The merge condition of the feature is checked and printed: at n = 2^16, host arrays, g2 decompress WITH the subgroup test must
take less time than the host loop takes to read the same number of points without it.  Not part of bench.py."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import legosnark_amd as lsa  # noqa: E402

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
MONT = (1 << 256) % P
G2_GEN = ((10857046999023057135944570762232829481370756359578518086990519993285655852781, 11559732032986387107991004021392285783925812861821192530917403151452391805634),
          (8495653923123431417604973247489272438418190587263600148770280649306958101930, 4082367875863433681332203403145435568316851327593401208105741076214120093531))


def words(ints):
    return np.frombuffer(b"".join((v * MONT % P).to_bytes(32, "little") for v in ints), dtype=np.uint64).copy()


def points(group, n, seed):
    rng = np.random.default_rng(seed)
    sc = rng.integers(0, 1 << 64, (n, 4), dtype=np.uint64, endpoint=False)
    sc[:, 3] &= np.uint64((1 << 60) - 1)
    base = words([1, 2, 1]) if group == "g1" else words([G2_GEN[0][0], G2_GEN[0][1], G2_GEN[1][0], G2_GEN[1][1], 1, 0])
    return lsa.batch_exp(group, base, sc)


def measure(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    lsa.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        lsa.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def yardstick(log, reps):
    libdir = os.path.join(ROOT, "legosnark_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "point_io_loop")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-I", os.path.join(ROOT, "legosnark_amd", "shim"),
                               os.path.join(ROOT, "tools", "native", "point_io_loop.cc"), "-o", exe,
                               "-L" + libdir, "-llegosnark_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
        r = subprocess.run([exe, str(log), str(reps)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    if r.returncode != 0:
        raise SystemExit("point_io_loop failed:\n" + r.stdout[-2000:])
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,20")
    ap.add_argument("--yardstick-logs", default="16", help="sizes at which the one-core host loop runs too (2^20: about a minute)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if lsa.device_count() < 1:
        raise SystemExit("bench_point_load: no GPU (there is no CPU path to time)")
    lsa.init(0)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    host_g2_checked = {}
    for log in [int(x) for x in a.logs.split(",")]:
        n = 1 << log
        for group in ("g1", "g2"):
            pts = points(group, n, log)
            x, flags = lsa.compress(group, pts)
            d_pts = torch.from_numpy(pts.view(np.int64)).to("cuda:0")
            d_x = torch.from_numpy(x.view(np.int64)).to("cuda:0")
            d_f = torch.from_numpy(flags).to("cuda:0")
            d_out = torch.empty_like(d_pts)
            checks = [False] if group == "g1" else [True, False]
            calls = []
            for chk in checks:
                tag = "" if group == "g1" else ("+subgroup" if chk else "")
                calls.append(("decompress" + tag, "host", lambda chk=chk: lsa.decompress(group, x, flags, check_subgroup=chk)))
                calls.append(("decompress" + tag, "device", lambda chk=chk: lsa.decompress(group, d_x, d_f, check_subgroup=chk, out=d_out)))
                calls.append(("validate" + tag, "host", lambda chk=chk: lsa.validate_points(group, pts, check_subgroup=chk)))
                calls.append(("validate" + tag, "device", lambda chk=chk: lsa.validate_points(group, d_pts, check_subgroup=chk)))
            calls.append(("compress", "host", lambda: lsa.compress(group, pts)))
            calls.append(("compress", "device", lambda: lsa.compress(group, d_pts)))
            # results must be what went in before anything is timed
            back, st = lsa.decompress(group, x, flags)
            assert not st.any() and np.array_equal(back, lsa.normalize(group, pts))
            for name, where, fn in calls:
                med, lo, hi = measure(fn, a.warmup, a.reps)
                emit({"call": "%s_%s" % (group, name), "operands": where, "n": n, "median_ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
                      "ns_per_point": round(med * 1e6 / n, 1), "reps": a.reps})
                if group == "g2" and name == "decompress+subgroup" and where == "host":
                    host_g2_checked[n] = med
    for log in [int(x) for x in a.yardstick_logs.split(",") if x]:
        for rec in yardstick(log, 3 if log <= 16 else 1):
            emit(rec)
            if rec["yardstick"] == "g2" and rec["n"] in host_g2_checked:
                ours, theirs = host_g2_checked[rec["n"]], rec["loop_read_ms"]
                emit({"merge_condition": "g2 decompress with the subgroup test on host arrays < the host loop's read without it", "n": rec["n"],
                      "lsa_g2_decompress_ms": round(ours, 3), "host_loop_read_ms": theirs, "holds": ours < theirs})
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
