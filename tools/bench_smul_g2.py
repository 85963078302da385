#!/usr/bin/env python3
"""Times lsa_g2_scalar_mul_batch on one MI355X for resident inputs at n = 64, 124, 1 024, 2^14, 2^16, 2^18: the median of 21
blocking calls after warm-up, a device synchronise inside the timed region.  In the same run and at the same n it times
lsa_g1_scalar_mul_batch and lsa_g2_batch_exp on a base seen before, and prints items/s and the ratio G1 rate / G2 rate.
Nothing here gates a test.  The lines are also written to legosnark_amd/csrc/profiles/smul_g2.txt (or the path given as
the first argument).

With a second argument, the per-product time of the host ladder in microseconds (tests/cpp/test_shim_smul_g2.cc prints
it), the break-even batch size against a loop of host products is reported as well."""
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
SIZES = [64, 124, 1024, 1 << 14, 1 << 16, 1 << 18]
CALLS = 21
G1_GEN = [1, 2, 1]
# libff's G2 generator (alt_bn128_init.cpp), canonical integers: x.c0, x.c1, y.c0, y.c1
G2_GEN = [10857046999023057135944570762232829481370756359578518086990519993285655852781,
          11559732032986387107991004021392285783925812861821192530917403151452391805634,
          8495653923123431417604973247489272438418190587263600148770280649306958101930,
          4082367875863433681332203403145435568316851327593401208105741076214120093531, 1, 0]
P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47


def mont_words(ints, mod):
    buf = b"".join((x % mod * (1 << 256) % mod).to_bytes(32, "little") for x in ints)
    return np.frombuffer(buf, dtype=np.uint64).copy()


def scalars(rng, n):
    raw = rng.bytes(32 * n)
    return torch.from_numpy(mont_words([int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(n)], R).reshape(n, 4).view(np.int64)).to("cuda:0")


def median_ms(fn):
    for _ in range(3):
        fn()
    lsa.synchronize()
    t = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn()
        lsa.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "legosnark_amd", "csrc", "profiles", "smul_g2.txt")
    host_us = float(sys.argv[2]) if len(sys.argv) > 2 else None
    lsa.init(0)
    rng = np.random.default_rng(1)
    gens = {"g1": mont_words(G1_GEN, P), "g2": mont_words(G2_GEN, P)}
    lines = ["# tools/bench_smul_g2.py: median (min) of %d blocking calls, resident inputs, one MI355X" % CALLS,
             "# lanes per G2 item %d, window %d bits, %d items resident per pass" % (
                 lsa.smul_param("g2_lanes_per_item"), lsa.smul_param("g2_window_bits"), lsa.smul_param("g2_resident_items"))]
    g2_ms = {}
    for n in SIZES:
        d_sc, d_sc2 = scalars(rng, n), scalars(rng, n)
        row = {"n": n}
        for group in ("g1", "g2"):
            d_pts = lsa.batch_exp(group, gens[group], d_sc)
            d_out = torch.empty((n, 12 if group == "g1" else 24), dtype=torch.int64, device="cuda:0")
            med, lo = median_ms(lambda: lsa.scalar_mul_batch(d_pts, d_sc2, out=d_out, group=group))
            row[group + "_smul_ms"], row[group + "_smul_min_ms"], row[group + "_items_per_s"] = round(med, 4), round(lo, 4), round(n / med * 1e3)
            if group == "g2":
                g2_ms[n] = med
                med, lo = median_ms(lambda: lsa.batch_exp("g2", gens["g2"], d_sc2, out=d_out))
                row["g2_batch_exp_ms"], row["g2_batch_exp_items_per_s"] = round(med, 4), round(n / med * 1e3)
        row["g1_rate_over_g2_rate"] = round(row["g1_items_per_s"] / row["g2_items_per_s"], 2)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if host_us is not None:
        # smallest measured n at which one call beats n host products; the call's time is nearly flat below a few thousand items
        even = next((n for n in SIZES if g2_ms[n] * 1e3 < n * host_us), None)
        lines.append(json.dumps({"host_ladder_us_per_product": host_us, "g2_call_ms_at_64": round(g2_ms[64], 4),
                                 "host_loop_ms_at_124": round(124 * host_us / 1e3, 3), "g2_call_ms_at_124": round(g2_ms[124], 4),
                                 "break_even_n_estimate": round(g2_ms[64] * 1e3 / host_us, 1), "first_measured_n_ahead": even}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
