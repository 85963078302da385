#!/usr/bin/env python3
"""Times the element-wise Fr vector calls on device-resident vectors (fr_vec_mul, fr_vec_lincomb, fr_powers, fr_batch_inverse,
fr_poly_eval) beside a yardstick from the same library, timed in the same process, and writes csrc/profiles/fr_elem.txt.

  call                       algorithmic bytes / element    yardstick
  fr_vec_mul                 96                             lsa_fr_scale_upper (64 B / element, one product per element)
  fr_vec_lincomb k = 1, 2, 3 32 (k + 1)                     lsa_fr_scale_upper
  fr_powers                  32                             lsa_fr_lagrange on the basic domain of the same length
  fr_batch_inverse           64                             lsa_fr_lagrange
  fr_poly_eval               32                             lsa_fr_eval_mle of the same length

Expectations: the streaming calls reach the yardstick's bytes per second less its spread; fr_powers and fr_batch_inverse take no
longer than the yardstick plus its spread; fr_poly_eval stays within twice the yardstick plus its spread.  A miss is reported as
a miss, next to the kernel's resource-usage line.

Every shape is warmed first.  A figure is the median of --reps repetitions, a repetition being --inner calls queued back to
back and one device synchronise (host clock, per call).  The yardstick and the call alternate over --rounds rounds; reported are
the median of the rounds' medians and, for the yardstick, the spread of its rounds' medians (max - min).

The resource usage of the kernels (VGPRs, scratch, occupancy) comes from compiling csrc/fr_elem.hip with
-Rpass-analysis=kernel-resource-usage: --resources-only prints that table without a GPU, --resources FILE embeds a table made
that way instead of compiling again.  Not part of bench.py."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "legosnark_amd", "csrc")
DEFAULT_OUT = os.path.join(CSRC, "profiles", "fr_elem.txt")

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MONT = (1 << 256) % R
TWO_ADICITY, GENERATOR = 28, 5


def resource_table():
    """One line per kernel of fr_elem.hip from the compiler's resource-usage remarks."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(CSRC, "fr_elem.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark: .*?\s*Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], stdout=subprocess.PIPE, text=True).stdout.strip() or m.group(1)
            cur = {"kernel": re.sub(r"\(.*", "", name).replace("lsa::", "").replace("void ", "")}
            rows.append(cur)
            continue
        for key, pat in (("sgprs", r"TotalSGPRs: (\d+)"), ("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    out = ["%-28s %6s %6s %8s %10s %6s" % ("kernel", "VGPRs", "SGPRs", "scratch", "waves/SIMD", "LDS")]
    for r in rows:
        out.append("%-28s %6d %6d %6d B %10d %6d" % (r["kernel"], r.get("vgprs", -1), r.get("sgprs", -1), r.get("scratch", -1), r.get("occupancy", -1), r.get("lds", -1)))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--logs", default="20,24", help="vector lengths, as exponents of two")
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--calls", default="", help="time only the calls whose name contains this")
    ap.add_argument("--resources", default=None, help="a file holding the table of --resources-only")
    ap.add_argument("--resources-only", action="store_true")
    args = ap.parse_args()
    if args.resources_only:
        print(resource_table())
        return
    resources = open(args.resources).read().rstrip() if args.resources else resource_table()

    import numpy as np
    import torch
    import legosnark_amd as lsa
    lsa.init(0)
    L = lsa.lib()

    def words(xs):
        return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy()

    def rand_vals(n, seed):
        a = np.random.default_rng(seed).integers(0, 1 << 64, (n, 4), dtype=np.uint64, endpoint=False)
        a[:, 3] &= np.uint64((1 << 60) - 1)
        return a

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")

    def root_of_unity(log_n):
        w = pow(GENERATOR, (R - 1) >> TWO_ADICITY, R)
        for _ in range(TWO_ADICITY - log_n):
            w = w * w % R
        return w

    def median_ms(fn):
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for _ in range(args.inner):
                fn()
            lsa.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / args.inner)
        return statistics.median(ts)

    def versus(yard, call):
        """(yardstick ms, its spread over the rounds, call ms), the two alternating"""
        for fn in (yard, call):
            for _ in range(3):
                fn()
        lsa.synchronize()
        ty, tc = [], []
        for _ in range(args.rounds):
            ty.append(median_ms(yard))
            tc.append(median_ms(call))
        return statistics.median(ty), max(ty) - min(ty), statistics.median(tc)

    lines, results = [], []
    for log_n in [int(x) for x in args.logs.split(",")]:
        n = 1 << log_n
        a, b, c = (to_dev(rand_vals(n, 10 * log_n + j)) for j in range(3))
        out = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
        one = torch.empty((1, 4), dtype=torch.int64, device="cuda:0")
        k = rand_vals(4, 7)
        up_old = torch.cat([a, b])                          # lsa_fr_scale_upper reads the upper half of 2n elements
        kp = k[0].ctypes.data_as(C.c_void_p)
        omega, t = words([root_of_unity(log_n) * MONT % R])[0], rand_vals(1, 8)[0]
        rr = to_dev(rand_vals(log_n, 9))
        yard_scale = lambda: lsa._check(L.lsa_fr_scale_upper(C.c_void_p(up_old.data_ptr()), n, kp, C.c_void_p(out.data_ptr()), 1))   # noqa: E731
        yard_lagrange = lambda: lsa.fr_lagrange(log_n, None, omega, t, out=out)                                                       # noqa: E731
        yard_mle = lambda: lsa.eval_mle_device(a, rr, one)                                                                            # noqa: E731
        shapes = [
            ("fr_vec_mul", 96, "fr_scale_upper", 64, yard_scale, lambda: lsa.fr_vec_mul(a, b, out=out), "stream"),
            ("fr_vec_lincomb k=1", 64, "fr_scale_upper", 64, yard_scale, lambda: lsa.fr_vec_lincomb([a], k[:1], out=out), "stream"),
            ("fr_vec_lincomb k=2", 96, "fr_scale_upper", 64, yard_scale, lambda: lsa.fr_vec_lincomb([a, b], k[:2], out=out), "stream"),
            ("fr_vec_lincomb k=3", 128, "fr_scale_upper", 64, yard_scale, lambda: lsa.fr_vec_lincomb([a, b, c], k[:3], out=out), "stream"),
            ("fr_powers", 32, "fr_lagrange", 32, yard_lagrange, lambda: lsa.fr_powers(k[0], n, out=out), "time"),
            ("fr_batch_inverse", 64, "fr_lagrange", 32, yard_lagrange, lambda: lsa.fr_batch_inverse(a, out=out), "time"),
            ("fr_poly_eval", 32, "fr_eval_mle", 32, yard_mle, lambda: lsa.fr_poly_eval(a, k[1], out=one), "twice"),
        ]
        for name, bpe, yname, ybpe, yard, call, rule in shapes:
            if args.calls not in name:
                continue
            ty, spread, tc = versus(yard, call)
            bps, ybps, ybps_low = bpe * n / (tc * 1e-3), ybpe * n / (ty * 1e-3), ybpe * n / ((ty + spread) * 1e-3)
            if rule == "stream":
                ok, what = bps >= ybps_low, "bytes/s >= the yardstick's less its spread (%.3f TB/s)" % (ybps_low / 1e12)
            elif rule == "time":
                ok, what = tc <= ty + spread, "time <= the yardstick's plus its spread (%.4f ms)" % (ty + spread)
            else:
                ok, what = tc <= 2 * ty + spread, "time <= twice the yardstick's plus its spread (%.4f ms)" % (2 * ty + spread)
            res = {"call": name, "n": "2^%d" % log_n, "ms": round(tc, 4), "algorithmic_bytes_per_s": round(bps, 0), "yardstick": yname,
                   "yardstick_ms": round(ty, 4), "yardstick_spread_ms": round(spread, 4), "yardstick_bytes_per_s": round(ybps, 0),
                   "ratio_to_yardstick": round((bps / ybps) if rule == "stream" else (tc / ty), 3), "expectation": what, "met": bool(ok)}
            results.append(res)
            print(json.dumps(res), flush=True)
            lines.append("%-20s 2^%-3d %9.4f ms %7.3f TB/s   %-15s %9.4f ms (spread %.4f) %7.3f TB/s   ratio %6.3f (%s)   %s" % (
                name, log_n, tc, bps / 1e12, yname, ty, spread, ybps / 1e12, res["ratio_to_yardstick"], "bytes/s" if rule == "stream" else "time",
                "met" if ok else "MISSED: " + what))
        del a, b, c, out, up_old
        torch.cuda.empty_cache()

    p = lsa.fr_vec_params()
    head = [
        "Element-wise Fr vector calls on device-resident vectors (tools/bench_fr_elem.py), one MI355X.",
        "Median of %d repetitions of %d queued calls and one synchronise, per call; the yardstick and the call alternate over %d rounds;" % (args.reps, args.inner, args.rounds),
        "the figures are the medians of the rounds' medians, the yardstick's spread is max - min of its rounds' medians.",
        "Algorithmic bytes per element: vec_mul 96, lincomb 32 (k + 1), powers 32, batch_inverse 64, poly_eval 32; fr_scale_upper 64, fr_lagrange 32,",
        "fr_eval_mle 32.  ratio: bytes/s over the yardstick's for the streaming calls, time over the yardstick's for the others.",
        "fr_vec_params: %s" % json.dumps(p),
        "",
        "call                 n      time        bytes/s      yardstick       time                          bytes/s      ratio                 expectation",
    ]
    tail = ["", "Kernel resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, csrc/fr_elem.hip):", resources, ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(head + lines + tail))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
