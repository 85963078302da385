"""The CRS cache's accounting as a whole: one fixed script of lsa.msm calls over seeded vectors, and after every call the
cache's counters (hits, misses, resident bytes, entries) and what the call reported about itself (cache_hit, table,
table_building), compared with tests/golden/crs_cache_trace.json.  The script takes every path of the cache at the
smallest size at which it exists: same-pointer, content and prefix hits, the small lookups by unit and by point, the
three ways an entry goes (stale under its pointer, over a new budget, trimmed after an insert), the prefix tables of
both groups, the adoption of a background table, and the sampled mode.  Every MSM result is checked against the
oracle too, so the trace cannot pass on wrong points.

LSA_CRS_TRACE_RECORD=<file> writes the trace to <file> instead of comparing it (the committed JSON was recorded that
way at the commit before the cache moved into csrc/crs_cache.hip)."""
import json
import os

import numpy as np
import pytest

import oracle_lib as o

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crs_cache_trace.json")


def canon(group, pt):
    return o.g1_canonical_affine(pt) if group == "g1" else o.g2_canonical_affine(pt)


@pytest.fixture()
def fresh_cache(lsa):
    lsa.crs_cache_configure(lsa.CRS_CACHE_FULL, 8 << 30)
    lsa.crs_cache_clear()
    lsa.crs_cache_table_after(0)          # no background builds unless a step asks for one: the trace is timing-free
    lsa.set_table_threshold(0)
    yield lsa
    lsa.crs_cache_configure(lsa.CRS_CACHE_FULL, 8 << 30)
    lsa.crs_cache_clear()
    lsa.crs_cache_table_after(23)
    lsa.set_table_threshold(0)


def test_the_accounting_of_a_scripted_sequence_is_the_recorded_one(fresh_cache):
    lsa = fresh_cache
    start = lsa.crs_cache_stats()
    trace = []
    alive = []                             # every vector stays allocated: no address is handed out twice

    def vec(group, seed, n):
        v = np.ascontiguousarray(o.arith_bases(group, seed, 3, n))
        alive.append(v)
        return v

    def state(label, host=("cache_hit", "table", "table_building")):
        c, h = lsa.crs_cache_stats(), lsa.msm_host_stats()
        trace.append({"step": label, "hits": c["hits"] - start["hits"], "misses": c["misses"] - start["misses"],
                      "resident_bytes": c["resident_bytes"], "entries": c["entries"], **{k: int(h[k]) for k in host}})
        return c["resident_bytes"]

    def call(label, group, bases, n, check=True, record=True):
        got = lsa.msm(group, bases, sc[:n])
        if check:
            assert canon(group, got) == canon(group, o.multi_exp(group, bases[:n], sc[:n], mode="mixed")), label
        return state(label) if record else None

    sc, _ = o.random_scalars(1088, seed=21)
    # 2. G1 at CRS_MIN_POINTS: miss, then hit
    a = vec("g1", 1001, 1024)
    call("g1 1024 miss", "g1", a, 1024)
    call("g1 1024 hit", "g1", a, 1024)
    # 3. the same bytes at a new address: content hit, the entry is re-keyed to the copy
    a2 = a.copy()
    alive.append(a2)
    assert a2.ctypes.data != a.ctypes.data
    call("g1 1024 copy: content hit", "g1", a2, 1024)
    # 4. one word changed in place: a miss that drops the stale entry under this pointer (the changed point is not on the
    # curve, so that one result has nothing to be compared with); the word restored: a miss again, the result checked
    a2[700, 0] ^= np.uint64(1)
    call("g1 1024 one word changed: miss, stale entry dropped", "g1", a2, 1024, check=False)
    a2[700, 0] ^= np.uint64(1)
    call("g1 1024 word restored: miss, stale entry dropped", "g1", a2, 1024)
    # 5. prefixes of a longer vector under its pointer
    before_p = trace[-1]["resident_bytes"]
    p = vec("g1", 1002, 1088)
    size_p = call("g1 1088 miss", "g1", p, 1088) - before_p
    call("g1 1088[:1024] prefix hit", "g1", p, 1024)
    call("g1 1088[:1030] not comparable: miss, new entry", "g1", p, 1030)
    call("g1 1088[:1000] small, partial last unit: refused", "g1", p, 1000)
    call("g1 1088[:512] small, by unit", "g1", p, 512)
    call("g1 1088[:40] small, by point", "g1", p, 40)
    # 6. G2: its prefix table comes with the second request that could use one
    before_q = trace[-1]["resident_bytes"]
    q = vec("g2", 1003, 1024)
    call("g2 1024 miss", "g2", q, 1024)
    call("g2 1024 hit", "g2", q, 1024)
    size_q = call("g2 1024 hit again", "g2", q, 1024) - before_q
    # 7. a budget that holds the two most recently used entries (the 1088-point one and the G2 one): the others go,
    # oldest first; then one more insert: the trim after it takes the oldest but never the new entry
    assert trace[-1]["entries"] == 4
    lsa.crs_cache_configure(lsa.CRS_CACHE_FULL, size_p + size_q)
    state("budget for two entries", host=())
    c = vec("g1", 1004, 1024)
    call("g1 1024 insert over budget: trim keeps it", "g1", c, 1024)
    # 8. the pre-shifted copies of the whole entry: started by a hit, adopted by wait_tables (nothing is recorded while
    # the build may be in flight), used by the next hit
    lsa.crs_cache_table_after(1)
    lsa.set_table_threshold(1024)
    before_t = trace[-1]["resident_bytes"]
    call("", "g1", c, 1024, record=False)
    lsa.crs_cache_wait_tables()
    after_t = state("g1 1024 hit started the build; after wait_tables", host=("cache_hit",))
    call("g1 1024 hit over the copies", "g1", c, 1024)
    assert trace[-1]["table"] == 1 and after_t > before_t
    lsa.crs_cache_table_after(0)
    lsa.set_table_threshold(0)
    # 9. sampled mode: fingerprints are not comparable, everything goes; index 0 is a sampled position
    lsa.crs_cache_configure(lsa.CRS_CACHE_SAMPLED, 0)
    state("sampled mode", host=())
    d = vec("g1", 1005, 1024)
    call("sampled: miss", "g1", d, 1024)
    call("sampled: hit", "g1", d, 1024)
    d[0] = d[5]
    call("sampled: point 0 changed, miss", "g1", d, 1024)
    # 10.
    lsa.crs_cache_clear()
    state("clear", host=())
    assert trace[-1]["entries"] == 0 and trace[-1]["resident_bytes"] == 0

    record_to = os.environ.get("LSA_CRS_TRACE_RECORD")
    if record_to:
        with open(record_to, "w") as f:
            json.dump(trace, f, indent=1)
            f.write("\n")
        return
    with open(GOLDEN) as f:
        want = json.load(f)
    for got_row, want_row in zip(trace, want):
        assert got_row == want_row
    assert len(trace) == len(want)
