#!/usr/bin/env python3
"""Times the sparse Fr products and the QAP witness map on device-resident vectors (FrSparse.matvec, fr_qap_witness):

  r1cs-units    the constraint system of the n x n matrix product out of inner-product gadgets (legogrothmatrix.cc:79-117),
                n = 64: n^3 + 1 rows, 1 + 2 n^2 + n^3 variables, every coefficient +1 or -1
  r1cs-random   the same structure with uniformly random coefficients: what the +-1 path saves is the difference
  skewed        2^18 rows of one to three random coefficients and one row of 2^16
  mid           2^16 rows of 1 .. 96 entries, uniformly: the lengths around the one-lane / one-wavefront threshold (for
                comparing builds with other thresholds, -DLSA_SP_SHORT_MAX / -DLSA_SP_CHUNK, loaded through LSA_LIB_VARIANT)

Per matrix: ms per matvec on either side, entries per second, and the fraction of the HBM peak (8.0 TB/s, the data-sheet
figure) that the ALGORITHMIC bytes make -- 68 B per entry (32 B coefficient, 4 B index, 32 B gathered operand) plus 40 B per
result (8 B row pointer, 32 B result); the +-1 path reads fewer (no coefficient), which the figure does not credit.
Per system: ms for fr_qap_witness beside the standalone fr_hadamard_quotient on the same domain (their difference is the
three products), and the YARDSTICK: a one-core host loop over the same CSR arrays (tools/fr_sparse_host_loop.cc, csrc/fp.h's
host form, built and timed in the same run) -- the library had no device path for these products before.  The device result is
compared with the host loop's, byte for byte, before anything is timed.

Every shape is warmed first; each figure is the median of --reps repetitions, a repetition being --inner calls queued back to
back and one device synchronise (host clock; per call).  One JSON line per matrix and per system.  Not part of bench.py."""
import argparse
import ctypes as C
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

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MONT = (1 << 256) % R
TWO_ADICITY, GENERATOR = 28, 5
HBM_PEAK = 8.0e12
ENTRY_BYTES, ROW_BYTES = 68, 40


def words(xs):
    """raw integers -> (n, 4) uint64"""
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy()


def fr_mont(x):
    return words([x % R * MONT % R])[0]


def root_of_unity(log_n):
    w = pow(GENERATOR, (R - 1) >> TWO_ADICITY, R)
    for _ in range(TWO_ADICITY - log_n):
        w = w * w % R
    return w


def rand_vals(n, rng):
    a = rng.integers(0, 1 << 64, (n, 4), dtype=np.uint64, endpoint=False)
    a[:, 3] &= np.uint64((1 << 60) - 1)              # any value < r is a valid Montgomery residue
    return a


def unit_vals(signs):
    """signs: array of +1 / -1 -> their canonical words"""
    pm = np.stack([words([MONT])[0], words([R - MONT])[0]])
    return pm[(np.asarray(signs) < 0).astype(np.int64)]


def matrix_product_r1cs(n, rng):
    """CSR arrays (cols, row_ptr, signs) of A, B, C and the assignment z (words) of the n x n matrix product, laid out as
    libsnark's protoboard does: variable 0 = 1, rows of M and columns of N alternating, then per output U[r][c] followed by
    its gadget's n - 1 running sums; constraint (r, c, i): M[r][i] N[i][c] = S_i - S_(i-1); last the row A = z[0]."""
    k = np.arange(n * n * n, dtype=np.int64)
    out, i = k // n, k % n
    r, c = out // n, out % n
    base = 1 + 2 * n * n + out * n
    s_i = np.where(i == n - 1, base, base + 1 + i)
    s_prev = base + i                                  # S_(i-1) = base + 1 + (i - 1)
    a_cols = np.append(1 + 2 * n * r + i, 0).astype(np.uint32)
    b_cols = (1 + 2 * n * c + n + i).astype(np.uint32)
    two = i > 0
    c_len = 1 + two.astype(np.int64)
    c_ptr = np.zeros(len(k) + 2, dtype=np.uint64)
    c_ptr[1:-1] = np.cumsum(c_len)
    c_ptr[-1] = c_ptr[-2]
    c_cols = np.zeros(int(c_ptr[-1]), dtype=np.uint32)
    c_sign = np.ones(int(c_ptr[-1]), dtype=np.int64)
    first = c_ptr[:-2].astype(np.int64)
    c_cols[first] = s_i
    c_cols[first[two] + 1] = s_prev[two]
    c_sign[first[two] + 1] = -1
    rows = len(k) + 1
    a_ptr = np.arange(rows + 1, dtype=np.uint64)
    b_ptr = np.minimum(np.arange(rows + 1, dtype=np.uint64), np.uint64(len(k)))
    nvars = 1 + 2 * n * n + n * n * n
    # the assignment: 32-bit entries, the running sums as integers (they stay far below r)
    z = [0] * nvars
    z[0] = 1
    for v in range(1, 1 + 2 * n * n):
        z[v] = int(rng.integers(0, 1 << 32))
    for o in range(n * n):
        rr, cc, acc, b0 = o // n, o % n, 0, 1 + 2 * n * n + o * n
        for j in range(n):
            acc += z[1 + 2 * n * rr + j] * z[1 + 2 * n * cc + n + j]
            z[b0 if j == n - 1 else b0 + 1 + j] = acc
    zw = words([v * MONT % R for v in z])
    return {"A": (a_cols, a_ptr, np.ones(len(a_cols), dtype=np.int64)), "B": (b_cols, b_ptr, np.ones(len(b_cols), dtype=np.int64)),
            "C": (c_cols, c_ptr, c_sign)}, nvars, zw


def skewed(rng, rows_log=18, long_log=16):
    rows = 1 << rows_log
    lens = rng.integers(1, 4, rows).astype(np.uint64)
    lens[rows // 3] = 1 << long_log
    ptr = np.zeros(rows + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(lens)
    cols = rng.integers(0, rows, int(ptr[-1])).astype(np.uint32)
    return cols, ptr


def mid_rows(rng, rows_log=16, longest=96):
    rows = 1 << rows_log
    ptr = np.zeros(rows + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(rng.integers(1, longest + 1, rows).astype(np.uint64))
    return rng.integers(0, rows, int(ptr[-1])).astype(np.uint32), ptr


def host_loop_library(tmp):
    so = os.path.join(tmp, "fr_sparse_host_loop.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "legosnark_amd", "csrc"),
                           os.path.join(ROOT, "tools", "fr_sparse_host_loop.cc"), "-o", so])
    L = C.CDLL(so)
    L.fr_sparse_host_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.fr_sparse_host_loop.restype = None
    return L


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def median_ms(fn, reps, inner, warmup):
    for _ in range(warmup):
        fn()
    lsa.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        lsa.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / inner)
    return statistics.median(ts), min(ts), max(ts)


def bench_matrix(name, vals, cols, ptr, ncols, x, host, args):
    nrows, nnz = len(ptr) - 1, len(cols)
    h = lsa.FrSparse(vals, cols, ptr, ncols, keep_transpose=True)
    want = np.zeros((nrows, 4), dtype=np.uint64)
    ptr_ = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    th = []
    for _ in range(3):
        t0 = time.perf_counter()
        host.fr_sparse_host_loop(ptr_(vals), ptr_(cols), ptr_(ptr), nrows, ptr_(x), ptr_(want))
        th.append((time.perf_counter() - t0) * 1e3)
    dx = to_dev(x)
    got = h.matvec(dx, 1)
    lsa.synchronize()
    same = bool(np.array_equal(got.cpu().numpy().view(np.uint64), want))
    dx0 = to_dev(rand_vals(nrows, np.random.default_rng(nnz)))
    out1 = torch.empty((nrows, 4), dtype=torch.int64, device="cuda:0")
    out0 = torch.empty((ncols, 4), dtype=torch.int64, device="cuda:0")
    res = {"op": "fr_sparse matvec, device-resident", "matrix": name, "rows": nrows, "cols": ncols, "nnz": nnz,
           "longest_row": int(np.max(np.diff(ptr.astype(np.int64)))), "equals_host_loop": same, "host_loop_one_core_ms": round(statistics.median(th), 3)}
    for side, xin, out, nout in ((1, dx, out1, nrows), (0, dx0, out0, ncols)):
        med, lo, hi = median_ms(lambda: h.matvec(xin, side, out=out), args.reps, args.inner, args.warmup)
        byts = ENTRY_BYTES * nnz + ROW_BYTES * nout
        res["side%d" % side] = {"ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4), "entries_per_s": round(nnz / (med * 1e-3), 0),
                                "algorithmic_bytes": byts, "fraction_of_hbm_peak": round(byts / (med * 1e-3) / HBM_PEAK, 4)}
    res["speedup_vs_host_loop_side1"] = round(statistics.median(th) / res["side1"]["ms"], 1)
    res.update(reps=args.reps, inner=args.inner)
    print(json.dumps(res), flush=True)
    return h, statistics.median(th)


def bench_system(name, hs, host_ms, z, big_log, args):
    m = 1 << big_log
    w, g = fr_mont(root_of_unity(big_log)), fr_mont(GENERATOR)
    d123 = np.stack([fr_mont(11111), fr_mont(22222), fr_mont(33333)])
    dz = to_dev(z)
    n = hs[0].rows
    abc = [torch.empty((n, 4), dtype=torch.int64, device="cuda:0") for _ in hs]
    hq, hw = (torch.empty((m + 1, 4), dtype=torch.int64, device="cuda:0") for _ in range(2))
    for mat, v in zip(hs, abc):
        mat.matvec(dz, 1, out=v)
    witness = lambda: lsa.fr_qap_witness(*hs, dz, big_log, None, omega=w, coset=g, d123=d123, out=hw)                   # noqa: E731
    quotient = lambda: lsa.fr_hadamard_quotient(*abc, d123, big_log, None, omega=w, coset=g, out=hq)                     # noqa: E731
    witness(), quotient()
    lsa.synchronize()
    same = bool(torch.equal(hq, hw))
    tw = median_ms(witness, args.reps, 1, args.warmup)
    tq = median_ms(quotient, args.reps, 1, args.warmup)
    print(json.dumps({"op": "fr_qap_witness, device-resident", "system": name, "constraints": n, "variables": hs[0].cols, "domain": "2^%d" % big_log,
                      "equals_quotient_of_the_three_products": same, "qap_witness_ms": round(tw[0], 4), "qap_witness_min_ms": round(tw[1], 4),
                      "standalone_hadamard_quotient_ms": round(tq[0], 4), "three_products_by_difference_ms": round(tw[0] - tq[0], 4),
                      "three_products_host_loop_one_core_ms": round(sum(host_ms), 3), "reps": args.reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=10, help="matvec calls queued per repetition")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("-n", type=int, default=64, help="edge of the matrix product")
    ap.add_argument("--rows-log", type=int, default=18)
    ap.add_argument("--long-log", type=int, default=16)
    ap.add_argument("--shapes", default="r1cs,skewed,mid")
    args = ap.parse_args()
    lsa.init(0)
    shapes = args.shapes.split(",")
    print(json.dumps({"lib": os.path.basename(lsa.LIB_PATH), "fr_sparse_params": lsa.fr_sparse_params(), "hbm_peak_bytes_per_s": HBM_PEAK}), flush=True)
    rng = np.random.default_rng(64)
    with tempfile.TemporaryDirectory() as tmp:
        host = host_loop_library(tmp)
        mats, nvars, z = matrix_product_r1cs(args.n, rng)
        rows = args.n ** 3 + 1
        big_log = max(1, (rows - 1).bit_length())
        for system in ("r1cs-units", "r1cs-random") if "r1cs" in shapes else ():
            hs, host_ms = [], []
            for key in "ABC":
                cols, ptr, sign = mats[key]
                vals = unit_vals(sign) if system == "r1cs-units" else rand_vals(len(cols), rng)
                h, t = bench_matrix("%s %s n=%d" % (system, key, args.n), vals, cols, ptr, nvars, z, host, args)
                hs.append(h)
                host_ms.append(t)
            bench_system("%s n=%d" % (system, args.n), hs, host_ms, z, big_log, args)
            for h in hs:
                h.close()
        if "skewed" in shapes:
            cols, ptr = skewed(rng, args.rows_log, args.long_log)
            ncols = 1 << args.rows_log
            x = rand_vals(ncols, rng)
            name = "skewed 2^%d rows, one of 2^%d" % (args.rows_log, args.long_log)
            hs, host_ms = [], []
            for tag, vals in (("random", rand_vals(len(cols), rng)), ("units", unit_vals(rng.choice([-1, 1], len(cols))))):
                h, t = bench_matrix("%s, %s coefficients" % (name, tag), vals, cols, ptr, ncols, x, host, args)
                hs.append(h)
                host_ms.append(t)
            bench_system(name + " (A = B = random, C = units)", [hs[0], hs[0], hs[1]], [host_ms[0], host_ms[0], host_ms[1]], x, args.rows_log, args)
            for h in hs:
                h.close()
        if "mid" in shapes:
            cols, ptr = mid_rows(rng)
            x = rand_vals(len(ptr) - 1, rng)
            for tag, vals in (("random", rand_vals(len(cols), rng)), ("units", unit_vals(rng.choice([-1, 1], len(cols))))):
                bench_matrix("mid 2^16 rows of 1..96, %s coefficients" % tag, vals, cols, ptr, len(ptr) - 1, x, host, args)[0].close()


if __name__ == "__main__":
    main()
