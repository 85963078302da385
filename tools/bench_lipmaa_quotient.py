#!/usr/bin/env python3
"""Times the resident Lipmaa prover's polynomial step on device-resident vectors at m = 2^20 (basic radix-2 domain) and
m = 2^20 + 2^19 (step domain):

  quotient    median time of lsa_fr_hadamard_quotient (three iFFTs, three coset FFTs, the pointwise kernel, one inverse
              coset FFT, the corrections; the copies of a, b, c into the working vectors included)
  transforms  the same seven transforms issued one by one through lsa_fr_ntt / lsa_fr_ntt_step in device mode, each timed
              as the median of its own blocking calls, summed: the yardstick (those entry points predate the quotient)
  ratio       quotient / transforms
  lagrange    median time of lsa_fr_lagrange (device mode) at a random point

Every shape is warmed first (tables, staging, code objects); each figure is the median of --reps blocking repetitions (host
clock around the call and a device synchronise), the two sides alternating within one repetition.  One JSON line per size.
Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import legosnark_amd as lsa  # noqa: E402

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
TWO_ADICITY, GENERATOR = 28, 5


def fr_mont(x):
    x = x % R * (1 << 256) % R
    return np.array([(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def root_of_unity(log_n):
    w = pow(GENERATOR, (R - 1) >> TWO_ADICITY, R)
    for _ in range(TWO_ADICITY - log_n):
        w = w * w % R
    return w


def timed(fn):
    t0 = time.perf_counter()
    fn()
    lsa.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="20,20+19", help="comma-separated: B (basic, 2^B) or B+S (step, 2^B + 2^S)")
    ap.add_argument("--lagrange-only", action="store_true",
                    help="time lsa_fr_lagrange alone (comparing builds of csrc/fr_batch_inv.h with another FR_BATCH_INV_RUN, "
                         "loaded through LSA_LIB_VARIANT)")
    args = ap.parse_args()
    lsa.init(0)
    g = fr_mont(GENERATOR)
    d123 = np.stack([fr_mont(11111), fr_mont(22222), fr_mont(33333)])
    t_pt = fr_mont(0x1234567890ABCDEF1234567890ABCDEF)
    for size in args.sizes.split(","):
        big_log, _, s = size.partition("+")
        big_log, small_log = int(big_log), (int(s) if s else None)
        m = (1 << big_log) + ((1 << small_log) if small_log is not None else 0)
        w = fr_mont(root_of_unity(big_log if small_log is None else big_log + 1))
        if args.lagrange_only:
            row = torch.empty((m, 4), dtype=torch.int64, device="cuda:0")
            for _ in range(args.warmup):
                lsa.fr_lagrange(big_log, small_log, w, t_pt, out=row)
            lsa.synchronize()
            tl = [timed(lambda: lsa.fr_lagrange(big_log, small_log, w, t_pt, out=row)) for _ in range(args.reps)]
            print(json.dumps({"op": "fr_lagrange, device-resident", "lib": os.path.basename(lsa.LIB_PATH), "m": size,
                              "lagrange_ms": round(statistics.median(tl), 4), "min_ms": round(min(tl), 4), "reps": args.reps}), flush=True)
            continue
        gen = torch.Generator(device="cuda:0").manual_seed(m)

        def vec(n):
            v = torch.randint(0, 1 << 62, (n, 4), dtype=torch.int64, device="cuda:0", generator=gen)
            v[:, 3] &= (1 << 60) - 1              # any value < r is a valid Montgomery residue
            return v

        a, b, c, work = vec(m), vec(m), vec(m), vec(m)
        h = torch.empty((m + 1, 4), dtype=torch.int64, device="cuda:0")
        row = torch.empty((m, 4), dtype=torch.int64, device="cuda:0")

        def ntt(inverse, coset):
            if small_log is None:
                lsa.fr_ntt(work, w, inverse=inverse, coset=coset)
            else:
                lsa.fr_ntt_step(work, big_log, small_log, w, inverse=inverse, coset=coset)

        # the seven transforms of one proof: (inverse, coset) and how often
        kinds = (("iFFT", True, None, 3), ("cosetFFT", False, g, 3), ("icosetFFT", True, g, 1))
        quotient = lambda: lsa.fr_hadamard_quotient(a, b, c, d123, big_log, small_log, omega=w, coset=g, out=h)     # noqa: E731
        lagrange = lambda: lsa.fr_lagrange(big_log, small_log, w, t_pt, out=row)                                     # noqa: E731
        for _ in range(args.warmup):
            quotient()
            lagrange()
            for _, inv, cs, _ in kinds:
                ntt(inv, cs)
        lsa.synchronize()
        tq, tl, tk = [], [], {k[0]: [] for k in kinds}
        for _ in range(args.reps):
            tq.append(timed(quotient))
            for name, inv, cs, _ in kinds:
                tk[name].append(timed(lambda: ntt(inv, cs)))
            tl.append(timed(lagrange))
        med = statistics.median
        per = {name: med(tk[name]) for name, _, _, _ in kinds}
        transforms = sum(per[name] * cnt for name, _, _, cnt in kinds)
        print(json.dumps({"op": "lipmaa quotient, device-resident", "m": "2^%d" % big_log + ("" if small_log is None else " + 2^%d" % small_log),
                          "quotient_ms": round(med(tq), 4), "quotient_min_ms": round(min(tq), 4), "quotient_max_ms": round(max(tq), 4),
                          "transform_ms": {k: round(v, 4) for k, v in per.items()}, "seven_transforms_ms": round(transforms, 4),
                          "ratio": round(med(tq) / transforms, 3), "lagrange_ms": round(med(tl), 4), "reps": args.reps}), flush=True)
        del a, b, c, work, h, row


if __name__ == "__main__":
    main()
