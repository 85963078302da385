"""GPU: the tail slots of the MSM pipelines outside their default mode.

Every MSM runs its tail on one of up to eight slots (csrc/msm_slots.hip: msm_slot_begin, the hand-over, msm_slot_finish); the large
pipeline (msm.hip) and the compact one (msm_compact.hip) share that bookkeeping and differ in when they grow a slot, where they wait
before they publish, and when they move on to the next slot.  LSA_NO_OVERLAP=1 runs every tail on the caller's stream,
LSA_TAIL_SLOTS=2 makes the slots wrap around after two calls; both are read once per process, so each variant is its own
interpreter.  Each child queues, without synchronising in between, calls of both pipelines that share destinations and a
sort, then one blocking call; every result is checked by the discrete-log identity
MSM(s, (a + i b) G) = (sum s_i (a + i b)) G.

G1 calls of up to 2^17 pairs over a table take the compact pipeline by default, so in the first three variants the large
pipeline runs the segmented call and the commitment pair; with LSA_COMPACT_MAX=4096 the calls of 70000 and 65537 pairs take
it too (partitioned sort; the second queued one with the lane-private first reduction level; the blocking one with its
tail inline)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = r"""
import json, sys
import numpy as np
import torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import legosnark_amd as lsa
import oracle_lib as o
lsa.init(0)
R = o.R
N, M = 70000, 2500
a, b = 0x1234567 << 100 | 5, 0x7654321 << 64 | 9
a2, b2 = 0x2B992DDFA23249D6 << 40 | 11, 0x517CC1B727220A95 << 16 | 1
lsa.set_table_threshold(1)
B = lsa.Bases("g1", o.arith_bases("g1", a, b, N))
P1 = lsa.Bases("g1", o.arith_bases("g1", a2, b2, M))
P2 = lsa.Bases("g2", o.arith_bases("g2", a2, b2, M))
assert B.has_table() and P1.has_table() and P2.has_table()
sc, ints = o.random_scalars(N, seed=11)
d = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
dev = lambda rows, w: torch.zeros((rows, w), dtype=torch.int64, device="cuda:0")
out0, out1, outs, c1, c2 = dev(1, 12), dev(1, 12), dev(3, 12), dev(1, 12), dev(1, 24)
lens = [0, 65, 2999]
offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
torch.cuda.synchronize()

B.msm_async(d, out0, n=N)                 # large or compact pipeline (see the test module)
B.msm_async(d, out0, n=300)               # compact pipeline, same destination: this one must be what out0 holds
B.msm_segments_async(d, offs, outs)       # large pipeline, three bucket spaces
lsa.commit_async(P1, P2, d, c1, c2, n=M)  # large pipeline twice, the G1 half on the G2 half's sort
B.msm_async(d, out1, n=N)
B.msm_async(d, out1, n=65537)             # same destination again
lsa.synchronize()
blocking = B.msm(d, n=N)                  # tail on the caller's stream

def dlog(aa, bb, lo, m):
    return sum(ints[lo + i] * (aa + i * bb) for i in range(m)) %% R
g1, g2 = o.generator("g1"), o.generator("g2")
def ok1(pt, k):
    return o.g1_canonical_affine(pt) == o.g1_canonical_affine(o.g1_mul(g1, o.fr_mont(k)))
host = lambda t: t.cpu().numpy().view(np.uint64)
res = {
    "out0_holds_n300": ok1(host(out0)[0], dlog(a, b, 0, 300)),
    "out1_holds_n65537": ok1(host(out1)[0], dlog(a, b, 0, 65537)),
    "commit_g1": ok1(host(c1)[0], dlog(a2, b2, 0, M)),
    "commit_g2": o.g2_canonical_affine(host(c2)[0]) == o.g2_canonical_affine(o.g2_mul(g2, o.fr_mont(dlog(a2, b2, 0, M)))),
    "blocking_n70000": ok1(blocking, dlog(a, b, 0, N)),
}
for j, m in enumerate(lens):
    res["segment_%%d_len_%%d" %% (j, m)] = ok1(host(outs)[j], dlog(a, b, int(offs[j]), m))
print("RESULT " + json.dumps(res))
"""

EXPECTED = {"out0_holds_n300", "out1_holds_n65537", "commit_g1", "commit_g2", "blocking_n70000", "segment_0_len_0", "segment_1_len_65", "segment_2_len_2999"}


@pytest.mark.parametrize("compact_max", [None, "4096"], ids=["compact_default", "compact_max_4096"])
@pytest.mark.parametrize("mode", [{}, {"LSA_NO_OVERLAP": "1"}, {"LSA_TAIL_SLOTS": "2"}], ids=["default", "no_overlap", "two_slots"])
def test_queued_and_blocking_calls_in_every_slot_mode(mode, compact_max):
    env = {k: v for k, v in os.environ.items() if k not in ("LSA_NO_OVERLAP", "LSA_TAIL_SLOTS", "LSA_COMPACT_MAX")}
    env.update(mode)
    if compact_max:
        env["LSA_COMPACT_MAX"] = compact_max
    # one child, one attempt: a child that fails or is killed is the finding
    r = subprocess.run([sys.executable, "-c", SNIPPET % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert set(res) == EXPECTED
    assert all(res.values()), res
