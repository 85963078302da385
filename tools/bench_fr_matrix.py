#!/usr/bin/env python3
"""Times the matrix kernels of the matrix-product gadget on device-resident operands (csrc/fr_matrix.hip):

  fr_matmul   C = A B at n x n x n, n = 256, 1024, 2048: n^3 field products per call, reported as products per second and as a
              fraction of the 175 G products/s a lane-per-product loop of fr29.h's mul reaches (profiles/r04_ubench_field_mul.txt)
  fr_matvec   both sides at 4096 x 4096: one product per streamed element, reported as bytes of M per second beside the
              4.75 TB/s of k_mle_dot, which is the same shape of work
  cpu         the schoolbook triple loop of matrixsc.cc:83-91 at n = --cpu-n in Python integers on one host core (no NumPy in
              the loop): the host side of the comparison, in the same run

Every shape is warmed first (code objects, staging); each figure is the median, minimum and maximum of --reps blocking
repetitions (host clock around the call and a device synchronise).  One JSON line per shape, also written to --out.
Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import legosnark_amd as lsa  # noqa: E402

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
FIELD_MUL_CEILING = 175e9        # profiles/r04_ubench_field_mul.txt
MLE_DOT_BYTES_PER_S = 4.75e12    # k_mle_dot


def timed(fn):
    t0 = time.perf_counter()
    fn()
    lsa.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    lsa.synchronize()
    t = [timed(fn) for _ in range(reps)]
    return statistics.median(t), min(t), max(t)


def cpu_triple_loop(n):
    """C[i][j] += A[i][k] * B[k][j] over Python integers mod r, as the reference's example states it."""
    import random
    rnd = random.Random(n)
    A = [[rnd.randrange(R) for _ in range(n)] for _ in range(n)]
    B = [[rnd.randrange(R) for _ in range(n)] for _ in range(n)]
    t0 = time.perf_counter()
    C = [[0] * n for _ in range(n)]
    for i in range(n):
        Ai, Ci = A[i], C[i]
        for j in range(n):
            acc = 0
            for k in range(n):
                acc = (acc + Ai[k] * B[k][j]) % R
            Ci[j] = acc
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--matmul", default="256,1024,2048")
    ap.add_argument("--matvec", default="4096")
    ap.add_argument("--cpu-n", type=int, default=256, help="0: skip the host loop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_matrix.txt"))
    args = ap.parse_args()
    lsa.init(0)
    gen = torch.Generator(device="cuda:0").manual_seed(1)

    def vec(n):
        v = torch.randint(0, 1 << 62, (n, 4), dtype=torch.int64, device="cuda:0", generator=gen)
        v[:, 3] &= (1 << 60) - 1              # any value < r is a valid Montgomery residue
        return v

    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    shape = lsa.fr_matrix_params()
    for n in [int(x) for x in args.matmul.split(",") if x]:
        a, b = vec(n * n), vec(n * n)
        c = torch.empty((n * n, 4), dtype=torch.int64, device="cuda:0")
        med, lo, hi = measure(lambda: lsa.fr_matmul(a, b, n, n, n, out=c), args.warmup, args.reps)
        rate = n ** 3 / (med * 1e-3)
        emit({"op": "fr_matmul, device-resident", "n": n, "tile": shape["matmul_tile"], "kstep": shape["matmul_kstep"], "ms": round(med, 4),
              "min_ms": round(lo, 4), "max_ms": round(hi, 4), "products_per_s": round(rate / 1e9, 2), "unit": "G products/s",
              "range_G_products_per_s": [round(n ** 3 / (hi * 1e-3) / 1e9, 2), round(n ** 3 / (lo * 1e-3) / 1e9, 2)],
              "fraction_of_175G_ceiling": round(rate / FIELD_MUL_CEILING, 3), "reps": args.reps})
        del a, b, c
    for n in [int(x) for x in args.matvec.split(",") if x]:
        m, w = vec(n * n), vec(n)
        out = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
        for side in (0, 1):
            med, lo, hi = measure(lambda: lsa.fr_matvec(m, w, n, n, side, out=out), args.warmup, args.reps)
            rate = 32 * n * n / (med * 1e-3)
            emit({"op": "fr_matvec, device-resident", "rows": n, "cols": n, "side": side, "slices": lsa.fr_matvec_slices(n, n, side), "ms": round(med, 4),
                  "min_ms": round(lo, 4), "max_ms": round(hi, 4), "TB_per_s": round(rate / 1e12, 3),
                  "range_TB_per_s": [round(32 * n * n / (hi * 1e-3) / 1e12, 3), round(32 * n * n / (lo * 1e-3) / 1e12, 3)],
                  "fraction_of_k_mle_dot_4.75TB_per_s": round(rate / MLE_DOT_BYTES_PER_S, 3), "reps": args.reps})
        del m, w, out
    if args.cpu_n:
        n = args.cpu_n
        s = cpu_triple_loop(n)
        emit({"op": "host triple loop, Python integers, one core", "n": n, "s": round(s, 3), "products_per_s": round(n ** 3 / s / 1e6, 2), "unit": "M products/s"})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/bench_fr_matrix.py on one MI355X: device-resident operands, every shape warmed %d times, median / min / max of %d blocking\n"
                "# repetitions (host clock around the call and a device synchronise).  fr_matmul: n^3 products per call against the 175 G products/s of\n"
                "# profiles/r04_ubench_field_mul.txt; fr_matvec: 32 n^2 bytes of M per call beside k_mle_dot's 4.75 TB/s.\n" % (args.warmup, args.reps))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
