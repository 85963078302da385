"""GPU: the bucket accumulation's loads after the rotation of its loop (k_accumulate<CurveG1, 1 | 2>, k_accumulate_heavy<CurveG1>;
csrc/msm_accumulate.h, "kernel 4").  Iteration j of a lane requests entry word j+2 and the base of entry j+1 unconditionally, on an index
clamped to the lane's last entry, and the head of a list requests four words and three bases the same way.  What can go wrong
is the bookkeeping at the ends of a list: a lane that ends while its neighbours go on, lists shorter than the look-ahead, the
list at the end of the entries array, an infinity base where the head or the clamp meets it, state carried between calls.

n = 2^16 on a handle of 2^16 points (which carries the pre-shifted copies by default) is the smallest call that runs the
one-lane kernel.  LSA_NO_COMPACT sends it to the general pipeline and LSA_WIDE_SPLIT=2 gives every bucket two lanes; the library
reads both once per process, so the wide cases run in child interpreters, all cases of a child together (as
tests/test_g1_bucket_addition_gpu.py does).  Bases are k_i * G; every result is compared, after affine normalisation, with the
oracle's multiple of the generator by sum_i s_i * k_i.

List lengths are made by construction.  At this size the call has 13 windows of 20 or 19 bits over ONE space of 2^19 buckets
(csrc/msm_plan.h: table_grid, wide_plan_for), a scalar above r/2 is replaced by its negative, and a scalar d << start[k] has the
single non-zero digit d in window k: one entry, in bucket d - 1.  So a bucket's list is as long as the number of scalars that were
given its digit, whichever windows and signs they use.

Each case runs under a limit of its own (faulthandler.dump_traceback_later(..., exit=True)); the tests that wait for a child rely
on subprocess's timeout, which kills the child."""
import faulthandler
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as o

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = o.R
N = 1 << 16
A0, B0 = 0x1F2E3D4C5B6A7988 << 60 | 0x11, 0x9E3779B97F4A7C15 << 20 | 0x3
LIMIT_S = 120
HEAVY_CHUNK = 512                           # csrc/msm_plan.h


# ------------------------------------------------------------------ the digit plan of a wide call (mirror of csrc/msm_plan.h)
def windows(n_table):
    """(start, width) of the 13 wide windows: table_grid() / wide_plan_for(big = true)"""
    nbig = 12 if n_table >= 6 << 20 else 13
    base, rem = divmod(255, nbig)
    out, bit = [], 0
    for k in range(nbig):
        w = base + (1 if k < rem else 0)
        out.append((bit, w))
        bit += w
    return out


WIN = windows(N)
C_BITS = max(w for _, w in WIN)
# A raw digit of 2^(c-1) in a widest window is recoded to -2^(c-1), the LAST bucket of the space, and carries 1 into the next
# window (an entry more for bucket 0).
LAST_BUCKET_DIGIT = 1 << (C_BITS - 1)


def heavy_threshold(n):
    """plan_pipeline(): above this population a bucket goes to k_accumulate_heavy (wide digits, 2^(c-1) > 4096 buckets)"""
    nfull = sum(1 for _, w in WIN if w == C_BITS)
    pop = n * (nfull + 2 * (len(WIN) - nfull)) // (1 << (C_BITS - 1)) + 1
    return max(2 * pop + 32, 64)


def entry_scalar(d, t):
    """The t-th scalar given digit d: window and sign vary with d and t.  Digits stay below 2^16, which every window holds without
    recoding and which keeps the top window's scalars below r/2; LAST_BUCKET_DIGIT is the one exception."""
    k = (d + t) % len(WIN)
    if d == LAST_BUCKET_DIGIT:
        k = t % (sum(1 for _, w in WIN if w == C_BITS) - 1)         # a widest window whose successor takes the carry
        assert WIN[k][1] == C_BITS and WIN[k + 1][1] >= 2
    else:
        assert d < 1 << (WIN[k][1] - 1) and (d << WIN[k][0]) < R // 2
    s = d << WIN[k][0]
    return R - s if (d + 2 * t) % 3 == 0 else s


def scalars_of(spec, seed):
    """spec: (digit, population) pairs -> 2^16 scalars in a fixed shuffled order (the rest zero: no entry at all)"""
    sc = [entry_scalar(d, t) for d, c in spec for t in range(c)]
    assert len(sc) <= N and len({d for d, _ in spec}) == len(spec)
    sc += [0] * (N - len(sc))
    perm = np.random.default_rng(seed).permutation(N)
    return [sc[int(p)] for p in perm]


def mixed_spec():
    """lengths 1 .. 5, 4369 buckets each (15 * 4369 = 2^16 - 1; 4369 = 68 * 64 + 17, so in the order by population the run of every
    length ends inside a wavefront: its lanes end at different iterations)"""
    m = (N - 1) // 15
    return [(1 + (length - 1) * m + i, length) for length in range(1, 6) for i in range(m)]


def last_list_spec(length):
    """the mixed lists, one of them moved to the LAST bucket (the end of the entries array), `length` entries long"""
    spec = mixed_spec()
    at = next(i for i, (_, c) in enumerate(spec) if c == length)
    spec[at] = (LAST_BUCKET_DIGIT, length)
    return spec


def heavy_spec():
    """populations at the threshold (the longest list of k_accumulate) and one above it (a chunk of k_accumulate_heavy in which lane 0
    has two entries and lanes 1 .. thr have one), two chunks whose last stride of 64 is partly empty (1000 = 512 + 7 * 64 + 40),
    a second chunk of exactly one stride, and lists of three as filler"""
    thr = heavy_threshold(N)
    spec = [(30001, thr), (30002, thr + 1), (30003, 1000), (30004, HEAVY_CHUNK + 64)]
    fill = (N - sum(c for _, c in spec)) // 3
    return spec + [(1 + i, 3) for i in range(fill)]


def mont_array(ints):
    buf = b"".join((x % R * o.MONT % R).to_bytes(32, "little") for x in ints)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


def canon(pt):
    return o.g1_canonical_affine(pt)


def expected(scalars, dlogs):
    k = sum(s * d for s, d in zip(scalars, dlogs)) % R
    return canon(o.g1_mul(o.generator("g1"), o.fr_mont(k)))


def progression(n=N):
    return o.arith_bases("g1", A0, B0, n), [(A0 + i * B0) % R for i in range(n)]


def infinity_case():
    """Lists of five, all members of a list in one window at consecutive base positions.  By the bucket's number mod 16: member 0 .. 4
    is the infinity point (whichever order the sort leaves the entries in, infinity stands at the positions 0, 1, 2, second-to-last and
    last of some lists); all five are; or two members are P and -P, every pair of positions in turn (one of them the first two
    entries, which cancel in the head; the others cancel in the loop, on an accumulator that becomes infinity)."""
    pts, dlogs = progression()
    neg = o.arith_bases("g1", R - A0, R - B0, N)
    pairs = list(itertools.combinations(range(5), 2))
    bases, dl, sc = pts.copy(), list(dlogs), [0] * N
    for b in range((N - 1) // 5):
        d, v, first = b + 1, (b + 1) % 16, 5 * b
        s = (d << WIN[d % len(WIN)][0])
        for t in range(5):
            sc[first + t] = R - s if d % 2 else s
        if v < 5:
            bases[first + v] = 0
            dl[first + v] = 0
        elif v == 5:
            bases[first:first + 5] = 0
            dl[first:first + 5] = [0] * 5
        else:
            a, c = pairs[v - 6]
            bases[first + c] = neg[first + a]
            dl[first + c] = (R - dlogs[first + a]) % R
    return bases, sc, dl


def run_wide(B, scalars):
    """one blocking MSM of 2^16 pairs"""
    import torch
    d_s = torch.from_numpy(mont_array(scalars).view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    return canon(B.msm(d_s))


def wide_cases(lsa, names):
    """-> {case: passed}.  One handle over the progression serves every case but 'infinity_positions'."""
    import torch
    out = {}
    lsa.set_table_threshold(0)
    bases, dlogs = progression()
    vectors = {
        "mixed_lengths": lambda: scalars_of(mixed_spec(), 1),
        "last_list_of_one": lambda: scalars_of(last_list_spec(1), 2),
        "last_list_of_two": lambda: scalars_of(last_list_spec(2), 3),
        "heavy_edges": lambda: scalars_of(heavy_spec(), 4),
        "one_value": lambda: [0x0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F0F % R] * N,
    }
    B = lsa.Bases("g1", bases)
    try:
        assert B.has_table()
        for name in names:
            if name == "infinity_positions":
                continue                                                # bases of its own, below
            faulthandler.dump_traceback_later(LIMIT_S, exit=True)      # re-arms: each case has its own limit
            if name in vectors:
                sc = vectors[name]()
                out[name] = run_wide(B, sc) == expected(sc, dlogs)
            elif name == "queued_calls":
                # four calls back to back, one join: nothing of a call's walk may reach the next one's
                scs = [scalars_of(mixed_spec(), 11), scalars_of(heavy_spec(), 12), scalars_of(last_list_spec(1), 13), o.random_scalars(N, seed=14)[1]]
                dev = [torch.from_numpy(mont_array(sc).view(np.int64)).to("cuda:0") for sc in scs]
                outs = torch.zeros((len(scs), 12), dtype=torch.int64, device="cuda:0")
                torch.cuda.synchronize()
                for i in range(len(scs)):
                    B.msm_async(dev[i], outs[i])
                lsa.synchronize()
                got = outs.cpu().numpy().view(np.uint64)
                for i, sc in enumerate(scs):
                    out["%s[%d]" % (name, i)] = canon(got[i]) == expected(sc, dlogs)
            else:
                raise KeyError(name)
            faulthandler.cancel_dump_traceback_later()
            print("CASE", name, flush=True)
    finally:
        B.close()
    if "infinity_positions" in names:
        faulthandler.dump_traceback_later(LIMIT_S, exit=True)
        ibases, sc, dl = infinity_case()
        B = lsa.Bases("g1", ibases)
        try:
            out["infinity_positions"] = run_wide(B, sc) == expected(sc, dl)
        finally:
            B.close()
        faulthandler.cancel_dump_traceback_later()
    return out


ONE_LANE = ["mixed_lengths", "last_list_of_one", "last_list_of_two", "heavy_edges", "one_value", "queued_calls", "infinity_positions"]
TWO_LANES = ["mixed_lengths", "last_list_of_two", "infinity_positions"]

SNIPPET = r"""
import faulthandler, json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import legosnark_amd as lsa
import test_accumulate_prefetch_gpu as T
faulthandler.dump_traceback_later(T.LIMIT_S, exit=True)      # set-up under a limit too
lsa.init(0)
print("RESULT " + json.dumps(T.wide_cases(lsa, %(names)r)))
"""


def run_child(names, **switches):
    env = dict(os.environ, LSA_NO_COMPACT="1", **switches)
    r = subprocess.run([sys.executable, "-c", SNIPPET % {"root": ROOT, "names": names}], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=(len(names) + 1) * LIMIT_S + 60)
    assert r.returncode == 0, r.stdout[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])


def check(out, names):
    want = {n for n in names if n != "queued_calls"} | ({"queued_calls[%d]" % i for i in range(4)} if "queued_calls" in names else set())
    assert set(out) == want
    for name in sorted(want):
        assert out[name], name


def test_the_plan_this_file_builds_its_lists_on():
    """13 windows, 2^19 buckets, and the heavy threshold of plan_pipeline() for 2^16 pairs: if these move, the lists above are not
    what their names say."""
    assert len(WIN) == 13 and C_BITS == 20 and sum(w for _, w in WIN) == 255
    assert heavy_threshold(N) == 64
    assert sum(c for _, c in mixed_spec()) == N - 1 and sum(c for _, c in heavy_spec()) == N
    assert max(d for d, _ in mixed_spec() + heavy_spec()) < 1 << 16


def test_one_lane_per_bucket():
    """k_accumulate<CurveG1, 1> and k_accumulate_heavy on the general wide pipeline: every case of this file."""
    check(run_child(ONE_LANE), ONE_LANE)


def test_two_lanes_per_bucket_on_the_wide_path():
    """LSA_WIDE_SPLIT=2: k_accumulate<CurveG1, 2>, each lane on every second entry -- lists of 1 .. 5 leave a lane 0 .. 3 entries."""
    check(run_child(TWO_LANES, LSA_WIDE_SPLIT="2"), TWO_LANES)


@pytest.fixture
def watchdog():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.mark.parametrize("bits", [254, 40])
def test_plain_path_two_lanes(lsa, watchdog, bits):
    """n = 2^12 on a handle without the copies: GLV halves, two lanes per bucket, entries with the endo bit.  Uniform scalars fill
    every window (bucket populations around 16, odd and even); 40-bit ones leave the upper windows to a few long lists."""
    import torch
    n = 1 << 12
    bases, dlogs = progression(n)
    lsa.set_table_threshold(1 << 30)
    try:
        B = lsa.Bases("g1", bases)
        assert not B.has_table()
        mont, sc = o.random_scalars(n, seed=4096 + bits, bits=bits)
        d_s = torch.from_numpy(mont.view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        got = canon(B.msm(d_s))
        B.close()
    finally:
        lsa.set_table_threshold(0)
    assert got == expected(sc, dlogs)
