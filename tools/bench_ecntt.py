#!/usr/bin/env python3
"""Times lsa_g1_ecntt / lsa_g2_ecntt on one MI355X for device-resident vectors: G1 at 2^16 and 2^20, G2 at 2^16 and 2^18,
forward and inverse, the median of 21 calls after warm-up with a device synchronise inside the timed region, one process.

Beside every transform, in the same run, its yardstick on code the transform does not touch: the ladders of its stages as
independent products through lsa_g*_scalar_mul_batch on n/2 resident items -- (log_n - 1) calls for the forward transform,
(log_n + 1) for the inverse (n more ladders) -- timed as one sequence with one synchronise at its end.  The transform adds
two complete additions per butterfly, a batch normalisation per stage and the traffic of its two stage buffers to that,
and drops the per-call allocation and synchronise; the ratio transform / yardstick is reported, nothing here gates a test.

The lines are also written to legosnark_amd/csrc/profiles/ecntt.txt (or the path given as the first argument)."""
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
P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
SHAPES = [("g1", 16), ("g1", 20), ("g2", 16), ("g2", 18)]
CALLS = 21
G1_GEN = [1, 2, 1]
# libff's G2 generator (alt_bn128_init.cpp), canonical integers: x.c0, x.c1, y.c0, y.c1
G2_GEN = [10857046999023057135944570762232829481370756359578518086990519993285655852781,
          11559732032986387107991004021392285783925812861821192530917403151452391805634,
          8495653923123431417604973247489272438418190587263600148770280649306958101930,
          4082367875863433681332203403145435568316851327593401208105741076214120093531, 1, 0]
# what the compiler reports for the two stage kernels next to the ladder kernels they are built from (hipcc
# -Rpass-analysis=kernel-resource-usage, gfx950): VGPRs / scratch bytes per lane / waves per SIMD
RESOURCES = ("# k_ecntt_stage_g1 219 VGPRs, 0 B scratch, 2 waves/SIMD (k_smul_g1 204, 0, 2); "
             "k_ecntt_stage_g2 230, 0, 2 (k_smul_g2 220, 0, 2)")


def mont_words(ints, mod):
    buf = b"".join((x % mod * (1 << 256) % mod).to_bytes(32, "little") for x in ints)
    return np.frombuffer(buf, dtype=np.uint64).copy()


def root_of_unity(log_n):
    w = pow(5, (R - 1) >> 28, R)
    for _ in range(28 - log_n):
        w = w * w % R
    return w


def device_scalars(rng, n):
    a = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(n, 4).copy()
    a[:, 3] &= np.uint64((1 << 60) - 1)                    # below 2^252 < r: the Montgomery words of some scalar
    return torch.from_numpy(a.view(np.int64)).to("cuda:0")


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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "legosnark_amd", "csrc", "profiles", "ecntt.txt")
    lsa.init(0)
    rng = np.random.default_rng(1)
    gens = {"g1": mont_words(G1_GEN, P), "g2": mont_words(G2_GEN, P)}
    params = lsa.ecntt_params()
    lines = ["# tools/bench_ecntt.py: median (min) of %d calls, resident vectors, one MI355X, one process" % CALLS,
             "# butterflies in flight per pass: G1 %d, G2 %d (%d lanes each); yardstick: (log_n - 1) forward / (log_n + 1) inverse calls of"
             " lsa_g*_scalar_mul_batch on n/2 resident items" % (params["g1_resident_butterflies"], params["g2_resident_butterflies"],
                                                                 params["g2_lanes_per_butterfly"]),
             RESOURCES]
    for group, log_n in SHAPES:
        n, width = 1 << log_n, 12 if group == "g1" else 24
        w = mont_words([root_of_unity(log_n)], R)
        d_pts = lsa.batch_exp(group, gens[group], device_scalars(rng, n))
        d_out = torch.empty((n, width), dtype=torch.int64, device="cuda:0")
        d_half_sc, d_half_out = device_scalars(rng, n // 2), torch.empty((n // 2, width), dtype=torch.int64, device="cuda:0")
        d_half_pts = d_pts[:n // 2]

        def yardstick(calls):
            for _ in range(calls):
                lsa.scalar_mul_batch(d_half_pts, d_half_sc, out=d_half_out, group=group)

        for inverse in (False, True):
            calls = log_n + 1 if inverse else log_n - 1
            med, lo = median_ms(lambda: lsa.ecntt(group, d_pts, w, inverse=inverse, out=d_out))
            y_med, y_lo = median_ms(lambda: yardstick(calls))
            ladders = (n // 2) * (log_n - 2) + 1 + (n if inverse else 0)
            lines.append(json.dumps({"group": group, "log_n": log_n, "inverse": inverse, "ecntt_ms": round(med, 3), "ecntt_min_ms": round(lo, 3),
                                     "yardstick_calls": calls, "yardstick_ms": round(y_med, 3), "yardstick_min_ms": round(y_lo, 3),
                                     "ratio": round(med / y_med, 3), "ladders": ladders, "ladders_per_s": round(ladders / med * 1e3)}))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
