"""GPU: the paths only an LSA_* switch or a huge input reaches, each against the oracle at the smallest shape that takes it.

The suite's pinned and random shapes run the default plan of their sizes.  What they leave out is selected by a size no test
that has seconds can have -- the two-level look-ups of pass 1's twiddles from 2^25 elements on and of the coset powers from
2^23 on (csrc/ntt_core.h: ntt_two_level), an eviction of the NTT's tables by bytes under queued transforms (ntt.hip:
ntt_make_room), the 64-bit sort records of MSMs beyond 2^25 pairs (k_scatter_wide<1> / k_fine_sort<u64>) -- or by a documented
switch no test set: the reduction variants of msm_reduce.h, the narrow / wide digit threshold, the older G2 base conversion,
evalMLE by fold passes at d >= 16, batch_exp without and with eight kept tables.  INTEGRATION.md documents a switch for each
of them, so every one runs here, at a size of seconds.

One test per variant.  The switches are read once per process, so a test starts ONE child interpreter with the variant's
environment (tests/test_sort_paths_gpu.py, tests/test_g1_bucket_addition_gpu.py); the child arms a watchdog
(faulthandler.dump_traceback_later(..., exit=True)) anew for every case, ends at the first case that fails, and reports every
case it ran: the parent requires the planned number, none skipped.  Every comparison is exact -- bytes for Fr, canonical affine
coordinates for points.  MSM results are checked by the known-discrete-log identity AND against the affine point a child without
the switch returns for the same input; the NTT tests prove through lsa.fr_ntt_params() that the switch took effect (without that
they could pass on the default path).  tests/cpp/test_msm_plan.cc asserts on the host that every (shape, switches) pair of M1 to
M6 sets the flag of the plan the variant is here for.

Wall times on an MI355X box: 54 s for the 13 tests, SECONDS_ON_MI355X below per test, children included.  A child spends about
2.3 s on import and lsa.init before its first case; the MSM children 0.3 s more on the oracle's 2^16 base points.  Inside the
cases the oracle dominates: N1's 127 cases take 3.3 s, 2.1 s of that (on a development CPU) the oracle's four transforms of 2^19
points; N2's 119 cases 3.2 s in either process, nearly all of it the oracle's transforms and the Python integers of the two
quotients; the MSM, evalMLE and batch_exp cases 0.1 to 0.6 s per child.  The children without a switch that a family's variants
are compared with (one each for the probe, the N2 sequence, the G1 shapes and the G2 shapes) run inside the first test that needs
them: N1 2.3 s, N2 5.4 s, M1 3.1 s, M5 2.7 s of the figures below.  Nothing asserts these times.
"""
import faulthandler
import functools
import json
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle_lib as o

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, P = o.R, o.P
LIMIT_S = 120                          # per case, in the child
CHILD_TIMEOUT_S = 900                  # subprocess.run's: the child's own watchdog ends a hung case long before
FUZZ_CASES = 20
NTT_KINDS = ["ntt", "ntt_step", "hadamard_quotient", "lagrange", "qap_witness"]
G1_GROUPS = {"five": 5, "plus1": 1, "queued": 3, "n4099": 1}
SWITCHES = ["LSA_NTT_T1_MB", "LSA_NTT_CACHE_MB", "LSA_NO_PART", "LSA_NO_REC32", "LSA_NO_REDUCE_BITS", "LSA_NO_LANE_L1", "LSA_G2_LANE_L1", "LSA_WIDE_BIG_MIN",
            "LSA_G2_PREPARE_OLD", "LSA_MLE_DOT", "LSA_FR_GRAPHS", "LSA_BEXP_TABLES", "LSA_NO_COMPACT", "LSA_NO_COMPACT_G2", "LSA_COMPACT_MAX", "LSA_COMPACT_MAX_G2",
            "LSA_WIDE_SPLIT", "LSA_G2_PAIR", "LSA_PRECOMPUTE", "LSA_PRECOMPUTE_MIN"]

# measured, for the record (nothing asserts them): seconds per test on an MI355X box, children included
SECONDS_ON_MI355X = {"n1": 8.0, "n2": 11.1, "m1": 6.0, "m3": 2.7, "m4": 2.6, "m5": 5.3, "m6a": 2.9, "m6b": 2.5, "m7": 2.4, "f1": 2.7, "f1_without_graphs": 2.3,
                     "f2_no_tables": 2.8, "f2_eight_tables": 2.5}


# ------------------------------------------------------------------------------------------------ the child's side
class Cases:
    """What a child ran: every case under a watchdog of its own, its outcome under its name.  A case that fails (or raises)
    is the child's last: nothing more is started on a device that may have faulted."""

    def __init__(self):
        self.out, self.extra = {}, {}

    def run(self, name, fn):
        assert name not in self.out, name
        faulthandler.dump_traceback_later(LIMIT_S, exit=True)
        t0 = time.time()
        v = fn()
        faulthandler.cancel_dump_traceback_later()
        if isinstance(v, tuple):                               # (ok, what) of a fuzz_parity generator
            v = {"ok": bool(v[0]), "what": v[1]}
        elif not isinstance(v, dict):
            v = {"ok": bool(v)}
        v["seconds"] = round(time.time() - t0, 2)
        self.out[name] = v
        print("CASE", name, v["ok"], flush=True)
        if not v["ok"]:
            self.finish(1)

    def finish(self, status=0):
        print("RESULT " + json.dumps({"cases": self.out, "extra": self.extra}), flush=True)
        if status:
            sys.exit(status)


def rand_fr(n, seed):
    """n canonical residues as limbs (any canonical residue is some value's Montgomery form); numpy, not a Python loop."""
    a = np.random.default_rng(seed).integers(0, 1 << 64, (n, 4), dtype=np.uint64, endpoint=False)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a


def to_dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


MODES = [(False, False), (True, False), (False, True), (True, True)]      # (inverse, coset)
G_MONT = o.fr_mont(o.FR_GENERATOR)


def ntt_probe(lsa):
    """One forward coset transform of 2^16 points in a cache that holds nothing yet -> fr_ntt_params() after it."""
    before = lsa.fr_ntt_params()
    a, w = rand_fr(1 << 16, 16), o.fr_mont(o.fr_root_of_unity(16))
    got = lsa.fr_ntt(a, w, coset=G_MONT)
    after = lsa.fr_ntt_params()
    fresh = before["resident_bytes"] == 0 and before["domain_tables"] == 0 and before["coset_tables"] == 0
    return dict(after, ok=fresh and np.array_equal(got, o.fr_domain_transform(a, w, coset=G_MONT)))


def ntt_case(lsa, log_n, inverse, coset):
    a, w = rand_fr(1 << log_n, 3000 + log_n), o.fr_mont(o.fr_root_of_unity(log_n))
    g = G_MONT if coset else None
    return np.array_equal(lsa.fr_ntt(a, w, inverse=inverse, coset=g), o.fr_domain_transform(a, w, inverse=inverse, coset=g))


def step_case(lsa, big_log, small_log, inverse, coset, device=False):
    m = (1 << big_log) + (1 << small_log)
    a, w = rand_fr(m, 5000 + 32 * big_log + small_log), o.fr_mont(o.fr_root_of_unity(big_log + 1))
    g = G_MONT if coset else None
    want = o.fr_step_domain_transform(a, big_log, small_log, w, inverse=inverse, coset=g)
    if not device:
        return np.array_equal(lsa.fr_ntt_step(a, big_log, small_log, w, inverse=inverse, coset=g), want)
    d_a = to_dev(a)
    lsa.fr_ntt_step(d_a, big_log, small_log, w, inverse=inverse, coset=g)
    lsa.synchronize()
    return np.array_equal(to_host(d_a), want)


def extreme_case(lsa, log_n):
    from test_fr_vec_gpu import ntt_extreme_patterns
    w = o.fr_mont(o.fr_root_of_unity(log_n))
    for a, modes in ntt_extreme_patterns(log_n):
        for inverse, coset in modes:
            if not np.array_equal(lsa.fr_ntt(a, w, inverse=inverse, coset=coset), o.fr_domain_transform(a, w, inverse=inverse, coset=coset)):
                return False
    return True


def fuzz_cases(lsa, c, plan):
    import fuzz_parity as fz
    for kind, seed in plan:
        c.run("fuzz/%s/%d" % (kind, seed), lambda: fz.run_case(lsa, fz.KINDS[kind], seed))


def fuzz_seed():
    from test_fuzz_gpu import SEEDS
    return SEEDS[0]


def child_ntt_probe(lsa, c):
    c.run("probe", lambda: ntt_probe(lsa))


def child_ntt_two_level(lsa, c):
    """N1.  The probe first (the cache is empty), then the transforms: 11 is the smallest size with a pass 1, 16 the largest
    of two passes, 17 the smallest of three, 19 has passes of 7 + 6 + 6 stages."""
    import fuzz_parity as fz
    c.run("probe", lambda: ntt_probe(lsa))
    for log_n in (11, 16, 17, 19):
        for inverse, coset in MODES:
            c.run("ntt/%d/inverse%d/coset%d" % (log_n, inverse, coset), lambda: ntt_case(lsa, log_n, inverse, coset))
    for log_n in (13, 17):
        c.run("extreme/%d" % log_n, lambda: extreme_case(lsa, log_n))
    for big_log, small_log in ((12, 10), (17, 11)):
        for inverse, coset in MODES:
            c.run("step/%d+%d/inverse%d/coset%d" % (big_log, small_log, inverse, coset), lambda: step_case(lsa, big_log, small_log, inverse, coset))
    fuzz_cases(lsa, c, [(kind, s) for kind in NTT_KINDS for s in fz.case_seeds(kind, fuzz_seed(), FUZZ_CASES)])
    c.extra["params"] = lsa.fr_ntt_params()


N1_PLANNED = 1 + 4 * 4 + 2 + 2 * 4 + len(NTT_KINDS) * FUZZ_CASES


def child_ntt_cache(lsa, c):
    """N2.  Transforms whose tables exceed a budget of 1 MB each: every table built evicts, by bytes, whatever an earlier
    transform left -- between the two sub-transforms of a step domain and between the seven transforms of a quotient, while
    the earlier one's kernels are still queued.  The sequence ends on 2^17 + 2^16 points, whose tables are 4 and 2 MB."""
    import fuzz_parity as fz
    import test_fr_vec_gpu as V
    import test_lipmaa_gpu as lip
    c.run("domains_alternate", lambda: (V.test_ntt_domains_alternate_and_tables_are_reused(lsa), True)[1])
    plan = [(kind, s) for kind in NTT_KINDS for s in fz.case_seeds(kind, fuzz_seed(), FUZZ_CASES)]
    random.Random("switch_paths/%d" % fuzz_seed()).shuffle(plan)
    fuzz_cases(lsa, c, plan)
    for key in ((14, None), (14, 12)):
        def quotient(key=key):
            a, b, cc, d, want = lip.case(key)
            return np.array_equal(lip.quotient(lsa, key, a, b, cc, d, device=True), want)
        c.run("quotient/%s" % (key,), quotient)
    for big_log, small_log in ((14, 13), (17, 16)):
        for inverse, coset in MODES:
            for device in (False, True):
                c.run("step/%d+%d/inverse%d/coset%d/device%d" % (big_log, small_log, inverse, coset, device),
                      lambda: step_case(lsa, big_log, small_log, inverse, coset, device))
    c.extra["params"] = lsa.fr_ntt_params()


N2_PLANNED = 1 + len(NTT_KINDS) * FUZZ_CASES + 2 + 2 * 4 * 2


def g1_affine(pt):
    return None if pt is None else [str(pt[0]), str(pt[1])]


def g2_affine(pt):
    return None if pt is None else [[str(pt[0][0]), str(pt[0][1])], [str(pt[1][0]), str(pt[1][1])]]


ONE_VALUE = 0x0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F % R


def child_msm_g1(lsa, c, groups):
    """The G1 variants: handles with the pre-shifted copies, calls on the general pipeline (the parent sets LSA_NO_COMPACT).
    five: the cases of tests/test_g1_bucket_addition_gpu.py at 2^16 pairs, blocking; plus1: 2^16 + 1 pairs; queued: three
    msm_async calls on one handle without a join between them; n4099: 4099 pairs."""
    import torch
    import fuzz_parity as fz
    import test_g1_bucket_addition_gpu as T
    N = T.N
    prog = T.progression()

    def blocking(bases, sc, dlogs, threshold=0):
        lsa.set_table_threshold(threshold)
        try:
            B = lsa.Bases("g1", bases)
            try:
                assert B.has_table()
                d_s = to_dev(fz.mont_array(sc))
                torch.cuda.synchronize()
                got = T.canon(B.msm(d_s))
            finally:
                B.close()
        finally:
            lsa.set_table_threshold(0)
        return {"ok": got == T.expected(sc, dlogs), "affine": g1_affine(got)}

    if "five" in groups:
        for name in T.CASES:
            c.run("five/" + name, lambda: blocking(*T.build_case(name, prog)))
    if "plus1" in groups:
        # (a handle of more than 2^16 points carries the copies only under an explicit threshold)
        c.run("plus1/uniform", lambda: blocking(o.arith_bases("g1", T.A0, T.B0, N + 1), o.random_scalars(N + 1, seed=65537)[1],
                                                [(T.A0 + i * T.B0) % R for i in range(N + 1)], threshold=1))
    if "queued" in groups:
        lsa.set_table_threshold(0)
        B = lsa.Bases("g1", prog[0])
        assert B.has_table()
        vectors = [("uniform_a", o.random_scalars(N, seed=41)[1]), ("one_value", [ONE_VALUE] * N), ("uniform_b", o.random_scalars(N, seed=43)[1])]
        d_s = [to_dev(fz.mont_array(sc)) for _, sc in vectors]
        outs = torch.zeros((3, 12), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        faulthandler.dump_traceback_later(LIMIT_S, exit=True)
        for i in range(3):
            B.msm_async(d_s[i], outs[i])
        lsa.synchronize()
        faulthandler.cancel_dump_traceback_later()
        host = to_host(outs)
        for i, (name, sc) in enumerate(vectors):
            got = T.canon(host[i])
            c.run("queued/%d_%s" % (i, name), lambda: {"ok": got == T.expected(sc, prog[1]), "affine": g1_affine(got)})
        B.close()
    if "n4099" in groups:
        n = 4099
        c.run("n4099/uniform", lambda: blocking(prog[0][:n].copy(), o.random_scalars(n, seed=4099)[1], prog[1][:n]))


def child_msm_g2_lane(lsa, c):
    """M5.  Three queued G2 calls of 2^16 pairs on the general pipeline (the parent sets LSA_NO_COMPACT_G2): uniform scalars
    and one scalar value over a progression, then copies of the generator under scalars that cancel pairwise but for the
    last sixteen -- every bucket addition a doubling or a cancellation."""
    import torch
    import fuzz_parity as fz
    N = 1 << 16
    a0, b0 = 0x1F2E3D4C5B6A7988 << 60 | 0x11, 0x9E3779B97F4A7C15 << 20 | 0x3
    lsa.set_table_threshold(0)
    B1 = lsa.Bases("g2", o.arith_bases("g2", a0, b0, N))
    B2 = lsa.Bases("g2", np.ascontiguousarray(np.repeat(o.generator("g2").reshape(1, 24), N, axis=0)))
    assert B1.has_table() and B2.has_table()
    logs = [(a0 + i * b0) % R for i in range(N)]
    half = o.random_scalars(N // 2, seed=77)[1]
    cancel = [v for s in half for v in (s, (R - s) % R)]
    cancel[N - 16:] = o.random_scalars(16, seed=78)[1]
    calls = [("uniform", B1, o.random_scalars(N, seed=76)[1], logs), ("one_value", B1, [ONE_VALUE] * N, logs), ("generator_copies_cancelling", B2, cancel, [1] * N)]
    d_s = [to_dev(fz.mont_array(sc)) for _, _, sc, _ in calls]
    outs = torch.zeros((3, 24), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    for i, (_, B, _, _) in enumerate(calls):
        B.msm_async(d_s[i], outs[i])
    lsa.synchronize()
    faulthandler.cancel_dump_traceback_later()
    host = to_host(outs)
    for i, (name, _, sc, dl) in enumerate(calls):
        got = o.g2_canonical_affine(host[i])
        k = sum(s * d for s, d in zip(sc, dl)) % R
        want = o.g2_canonical_affine(o.g2_mul(o.generator("g2"), o.fr_mont(k)))
        c.run("queued/%d_%s" % (i, name), lambda: {"ok": got == want, "affine": g2_affine(got)})
    B1.close()
    B2.close()


def child_g2_prepare(lsa, c):
    """M7.  700 G2 bases with random Z and both encodings of infinity (all words zero; Z = 0 under X and Y) through the base
    conversion: a handle without and with the copies, and lsa_g2_msm twice (the second call meets the CRS cache's entry)."""
    n = 700
    rng = random.Random(700)
    pts = o.arith_bases("g2", 0x51ED270B9F2F3A1 << 64 | 7, 0x2545F4914F6CDD1D, n)
    for i in range(n):
        pts[i] = o.g2_from_affine(o.g2_canonical_affine(pts[i]), (rng.randrange(1, P), rng.randrange(P)))
    for i in (3, 350, n - 1):
        pts[i] = 0
    for i in (0, 10, 351):
        pts[i, 16:] = 0
    mont, _ = o.random_scalars(n, seed=701)
    want = o.g2_canonical_affine(o.multi_exp("g2", pts, mont, chunks=1, mode="mixed"))

    def handle(threshold, table):
        lsa.set_table_threshold(threshold)
        try:
            B = lsa.Bases("g2", pts)
            try:
                ok = B.has_table() == table
                return ok and o.g2_canonical_affine(B.msm(to_dev(mont))) == want
            finally:
                B.close()
        finally:
            lsa.set_table_threshold(0)

    c.run("handle/plain", lambda: handle(1 << 30, False))
    c.run("handle/copies", lambda: handle(0, True))
    for rep in range(2):
        c.run("lsa_msm/%d" % rep, lambda: o.g2_canonical_affine(lsa.msm("g2", pts, mont)) == want)


def child_mle_fold(lsa, c, ds):
    """F1.  evalMLE by fold passes (k_eval_mle_fused, tiles of 4096 inputs) where the default is the dot product: host and
    device buffers, each called twice -- the first call captures the launch sequence as a graph, the second replays it."""
    for d in ds:
        v, r = rand_fr(1 << d, 500 + d), rand_fr(d, 600 + d)
        want = o.fr_eval_mle(v, r)

        def host():
            return all(np.array_equal(lsa.eval_mle(v, r), want) for _ in range(2))

        def device():
            import torch
            d_v, d_r = to_dev(v), to_dev(r)
            d_out = torch.empty((1, 4), dtype=torch.int64, device="cuda:0")      # (the same buffers both times: the graph's key)
            ok = True
            for _ in range(2):
                d_out.fill_(-1)
                torch.cuda.synchronize()
                lsa.eval_mle_device(d_v, d_r, d_out)
                lsa.synchronize()
                ok = ok and np.array_equal(to_host(d_out).reshape(4), want) and np.array_equal(to_host(d_v), v)
            return ok

        c.run("eval_mle/%d/host" % d, host)
        c.run("eval_mle/%d/device" % d, device)


def bexp_bases(group, k):
    """k distinct un-normalised Jacobian points."""
    return o.arith_bases(group, 9001, 13, k)


def bexp_check(lsa, group, base, sc, idx=None):
    canon = o.g1_canonical_affine if group == "g1" else o.g2_canonical_affine
    got = lsa.batch_exp(group, base, sc)
    idx = range(len(sc)) if idx is None else idx
    want = o.batch_exp(group, base, np.ascontiguousarray(sc[list(idx)]))
    return len(got) == len(sc) and all(canon(got[i]) == canon(want[j]) for j, i in enumerate(idx))


def child_bexp_no_tables(lsa, c):
    """F2.  LSA_BEXP_TABLES=0: every call builds its table; both kernels' sides of n = 512, each size twice."""
    sc = rand_fr(513, 31)
    sc[0], sc[1], sc[2] = o.fr_mont(0), o.fr_mont(1), o.fr_mont(R - 1)
    big = rand_fr(1 << 16, 3)
    for group in ("g1", "g2"):
        base = bexp_bases(group, 1)[0]
        for n in (1, 3, 512, 513):
            for rep in range(2):
                c.run("%s/%d/%d" % (group, n, rep), lambda: bexp_check(lsa, group, base, sc[:n]))
        c.run("%s/65536" % group, lambda: bexp_check(lsa, group, base, big, idx=[0, 1, 777, 65535]))


def child_bexp_eight_tables(lsa, c):
    """F2, second run.  LSA_BEXP_TABLES=8: nine distinct bases fill the eight slots and evict the first base's table; then the
    first base again (rebuilt), and once more (a hit)."""
    sc = rand_fr(600, 32)
    sc[0], sc[1], sc[2] = o.fr_mont(0), o.fr_mont(1), o.fr_mont(R - 1)
    for group in ("g1", "g2"):
        bases = bexp_bases(group, 9)
        for k in range(9):
            c.run("%s/base%d" % (group, k), lambda: bexp_check(lsa, group, bases[k], sc[:600 if k == 0 else 3]))
        c.run("%s/base0_again" % group, lambda: bexp_check(lsa, group, bases[0], sc[:600]))
        c.run("%s/base0_hit" % group, lambda: bexp_check(lsa, group, bases[0], sc[:5]))


CHILDREN = {f.__name__[len("child_"):]: f for f in (child_ntt_probe, child_ntt_two_level, child_ntt_cache, child_msm_g1, child_msm_g2_lane, child_g2_prepare,
                                                   child_mle_fold, child_bexp_no_tables, child_bexp_eight_tables)}


def child_main(lsa, name, args):
    c = Cases()
    CHILDREN[name](lsa, c, *args)
    c.finish()


SNIPPET = r"""
import faulthandler, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import test_switch_paths_gpu as T
faulthandler.dump_traceback_later(T.LIMIT_S, exit=True)       # set-up under a limit too
import legosnark_amd as lsa
lsa.init(0)
faulthandler.cancel_dump_traceback_later()
T.child_main(lsa, %(name)r, %(args)r)
"""


# ------------------------------------------------------------------------------------------------ the parent's side
def run_child(name, switches, planned, args=()):
    """One child interpreter with exactly `switches` of this module's switches set -> {case: outcome}, extra.  The child
    ended cleanly, ran the planned number of cases and every one of them passed."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches)
    t0 = time.time()
    r = subprocess.run([sys.executable, "-c", SNIPPET % {"root": ROOT, "name": name, "args": tuple(args)}], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    cases = res["cases"]
    print("%s %s: %d cases, %.1f s (in cases: %.1f s)" % (name, switches, len(cases), time.time() - t0, sum(v["seconds"] for v in cases.values())))
    assert len(cases) == planned, "%s: %d of %d cases ran" % (name, len(cases), planned)
    assert all(v["ok"] for v in cases.values()), [k for k, v in cases.items() if not v["ok"]]
    return cases, res["extra"]


@functools.lru_cache(maxsize=None)
def default_ntt_probe():
    return run_child("ntt_probe", {}, 1)[0]["probe"]


@functools.lru_cache(maxsize=None)
def default_ntt_cache():
    return run_child("ntt_cache", {}, N2_PLANNED)[1]["params"]


@functools.lru_cache(maxsize=None)
def default_msm_g1():
    """Every G1 group once on the general pipeline's default plan."""
    return run_child("msm_g1", {"LSA_NO_COMPACT": "1"}, sum(G1_GROUPS.values()), args=(sorted(G1_GROUPS),))[0]


def g1_variant(switches, groups):
    cases, _ = run_child("msm_g1", dict(switches, LSA_NO_COMPACT="1"), sum(G1_GROUPS[g] for g in groups), args=(sorted(groups),))
    ref = default_msm_g1()
    for name, v in cases.items():
        assert v["affine"] == ref[name]["affine"], name
    return cases


def test_n1_two_level_twiddle_and_coset_lookups():
    """LSA_NTT_T1_MB=0: ntt_two_level(Tlo, Thi) for pass 1's twiddles and ntt_two_level(Glo, Ghi) for the coset powers at
    every size, as from 2^25 / 2^23 elements on by default."""
    cases, extra = run_child("ntt_two_level", {"LSA_NTT_T1_MB": "0"}, N1_PLANNED)
    table = (1 << 16) * 32                                   # T1 or Gfull of 2^16 points alone
    assert extra["params"]["t1_budget"] == 0
    assert cases["probe"]["resident_bytes"] < table, cases["probe"]
    assert cases["probe"]["domain_tables"] == 1 and cases["probe"]["coset_tables"] == 1
    assert default_ntt_probe()["resident_bytes"] >= table, default_ntt_probe()


def test_n2_table_eviction_by_bytes_under_queued_transforms():
    """LSA_NTT_CACHE_MB=1: the same sequence leaves fewer domains resident than in a default process, where no table of
    these sizes is ever evicted by bytes."""
    _, extra = run_child("ntt_cache", {"LSA_NTT_CACHE_MB": "1"}, N2_PLANNED)
    assert extra["params"]["cache_budget"] == 1 << 20
    assert extra["params"]["domain_tables"] < default_ntt_cache()["domain_tables"], (extra["params"], default_ntt_cache())
    assert default_ntt_cache()["cache_budget"] == 2048 << 20


def test_m1_64_bit_sort_records():
    """LSA_NO_PART=1 LSA_NO_REC32=1: k_scatter_wide<1> / k_fine_sort<u64>, the sort of every call beyond 2^25 pairs."""
    g1_variant({"LSA_NO_PART": "1", "LSA_NO_REC32": "1"}, ["five", "plus1"])


def test_m3_blocking_calls_without_the_bit_trees():
    g1_variant({"LSA_NO_REDUCE_BITS": "1"}, ["five"])


def test_m4_queued_calls_without_the_lane_private_level():
    g1_variant({"LSA_NO_LANE_L1": "1"}, ["queued"])


def test_m5_g2_lane_private_first_level():
    """LSA_G2_LANE_L1=1: k_reduce2_lane<CurveG2> under the second and third of three queued calls."""
    cases, _ = run_child("msm_g2_lane", {"LSA_G2_LANE_L1": "1", "LSA_NO_COMPACT_G2": "1"}, 3)
    ref, _ = run_child("msm_g2_lane", {"LSA_NO_COMPACT_G2": "1"}, 3)
    for name, v in cases.items():
        assert v["affine"] == ref[name]["affine"], name


def test_m6a_narrow_digits_at_2pow16_pairs():
    """LSA_WIDE_BIG_MIN=1048576: 26 narrow digits over 512 buckets, every bucket heavy."""
    g1_variant({"LSA_WIDE_BIG_MIN": "1048576"}, ["five", "plus1"])


def test_m6b_wide_digits_at_4099_pairs():
    """LSA_WIDE_BIG_MIN=4096: 13 wide digits over 2^19 buckets, almost all of them empty."""
    g1_variant({"LSA_WIDE_BIG_MIN": "4096"}, ["n4099"])


def test_m7_g2_bases_through_the_older_conversion():
    """LSA_G2_PREPARE_OLD=1: k_normalize<Fq2> + k_convert_bases instead of k_prepare_g2."""
    run_child("g2_prepare", {"LSA_G2_PREPARE_OLD": "1"}, 4)


def test_f1_eval_mle_by_fold_passes():
    run_child("mle_fold", {"LSA_MLE_DOT": "0"}, 8, args=((16, 17, 20, 21),))


def test_f1_eval_mle_by_fold_passes_without_graphs():
    run_child("mle_fold", {"LSA_MLE_DOT": "0", "LSA_FR_GRAPHS": "0"}, 4, args=((16, 20),))


def test_f2_batch_exp_without_kept_tables():
    run_child("bexp_no_tables", {"LSA_BEXP_TABLES": "0"}, 2 * (4 * 2 + 1))


def test_f2_batch_exp_with_eight_kept_tables():
    run_child("bexp_eight_tables", {"LSA_BEXP_TABLES": "8"}, 2 * 11)
