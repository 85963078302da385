"""The G2 line-table cache's accounting as a whole: one fixed script of pairing calls over seeded points, and after
every call the cache's four counters (hits, misses, resident, evictions), compared with
tests/golden/g2_table_cache_trace.json.  The script takes every route of the pairing entry points and every way a key
comes and goes: points at first sight (the fused kernel fills their tables), the same points again, blobs and the same
blobs at other addresses, mixed terms with a repeated Q inside one call, capacities 2, 0 and 16, a failing call followed
by a valid one, prefetches one by one into a cache of 8 and their Miller call, promises kept by the next Miller call, a
prefetch of a resident point, and a call under a forced chunk of 2.  Every Miller value is checked against the oracle
too, so the trace cannot pass on wrong values.

LSA_G2_TRACE_RECORD=<file> writes the trace to <file> instead of comparing it (the committed JSON was recorded that
way at the commit before the cache's rules moved into csrc/g2_table_index.h)."""
import json
import os

import numpy as np
import pytest

import oracle_lib as o

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g2_table_cache_trace.json")
NQ = 12


def test_the_counters_of_a_scripted_sequence_are_the_recorded_ones(lsa):
    import legosnark_amd
    Q = o.arith_bases("g2", 9100, 7, NQ)                    # un-normalised Jacobian
    Q[1] = o.generator("g2")                                 # Z = 1
    Q[3] = 0                                                 # infinity
    P = o.arith_bases("g1", 9101, 5, NQ)
    pre, val = {}, {}

    def want(pi, qi):                                        # the oracle's Miller value of (P[pi], Q[qi]), computed once
        if (pi, qi) not in val:
            if qi not in pre:
                pre[qi] = o.precompute_g2(Q[qi])
            val[(pi, qi)] = o.miller_loop_precomp(P[pi], pre[qi])
        return val[(pi, qi)]

    def want_products(pis, qis, flags, off):
        out = []
        for j in range(len(off) - 1):
            acc = o.fq12_one()
            for i in range(int(off[j]), int(off[j + 1])):
                f = want(pis[i], qis[i])
                acc = o.fq12_mul(acc, o.fq12_unitary_inverse(f) if flags[i] & 1 else f)
            out.append(acc)
        return np.array(out)

    trace = []
    start = None

    def state(label):
        s = lsa.g2_table_cache_stats()
        trace.append({"step": label, "hits": s["hits"] - start["hits"], "misses": s["misses"] - start["misses"],
                      "resident": s["resident"], "evictions": s["evictions"] - start["evictions"]})

    def points(label, pis, qis):
        got = lsa.miller_loop(P[pis], Q[qis])
        for k, (pi, qi) in enumerate(zip(pis, qis)):
            assert np.array_equal(got[k], want(pi, qi)), (label, k)
        state(label)

    def blobs(label, pis, tabs, qis, index=None):
        got = lsa.miller_loop_precomp(P[pis], tabs, index)
        for k, (pi, qi) in enumerate(zip(pis, qis)):
            assert np.array_equal(got[k], want(pi, qi)), (label, k)
        state(label)

    r6 = list(range(6))
    try:
        lsa.pairing_set_chunk(0)
        lsa.g2_table_cache(4096)
        start = lsa.g2_table_cache_stats()
        state("cache of 4096, empty")
        # 1. points: first sight, again, half of them new
        points("six points at first sight", r6, r6)
        points("the same six points", r6, r6)
        points("two resident points and two new ones", [0, 1, 2, 3], [4, 5, 6, 7])
        points("one pair alone, resident", [5], [2])
        # 2. blobs: first sight, the same bytes elsewhere
        tabs = lsa.g2_precompute(Q)
        state("g2_precompute of all twelve: not the cache's business")
        blobs("four blobs at first sight", [0, 1, 2, 3], tabs[8:12], [8, 9, 10, 11])
        blobs("the same four blobs at other addresses", [0, 1, 2, 3], tabs[8:12].copy(), [8, 9, 10, 11])
        # 3. mixed terms, a Q repeated inside the call as a point, as a blob, and as both (two keys); an empty product
        # first and in the middle; conjugated terms
        pis = [0, 1, 2, 3, 4, 5, 6, 7, 8]
        qis = [0, 0, 8, 8, 9, 2, 2, 3, 3]
        index = [-1, -1, 8, 8, -1, -1, 2, 3, 3]
        flags = np.array([0, 1, 0, 0, 1, 0, 1, 1, 0], dtype=np.uint8)
        off = np.array([0, 0, 3, 3, 7, 9], dtype=np.uint64)
        got = lsa.pairing_terms(P[pis], off, g2=Q[qis], tables=tabs, index=index, flags=flags, final_exp=False)
        assert np.array_equal(got, want_products(pis, qis, flags, off))
        state("nine mixed terms in five products")
        # 4. capacity 2: four of six tables live in scratch; eviction across calls
        lsa.g2_table_cache(2)
        state("cache of 2")
        points("six points into two slots", r6, r6)
        points("the last three of them", [3, 4, 5], [3, 4, 5])
        points("all six again", r6, r6)
        blobs("three blobs into two slots", [0, 1, 2], tabs[6:9], [6, 7, 8])
        # 5. capacity 0: nothing is looked up
        lsa.g2_table_cache(0)
        state("cache off")
        points("six points, cache off", r6, r6)
        blobs("blobs, cache off, one of them twice", [0, 1, 2], tabs, [8, 9, 8], index=[8, 9, 8])
        lsa.g2_tables_prefetch(Q[0:2])
        state("a prefetch, cache off")
        # 6. capacity 16: a failing call, then a valid one over the same blobs and over the same points
        lsa.g2_table_cache(16)
        state("cache of 16")
        off5 = np.arange(6, dtype=np.uint64)
        with pytest.raises(legosnark_amd.LsaError):
            lsa.pairing_terms(P[0:5], off5, g2=None, tables=tabs, index=[0, 1, 2, -1, 4], final_exp=False)
        state("a call whose fourth term has neither a point nor a blob")
        got = lsa.pairing_terms(P[0:5], off5, tables=tabs, index=[0, 1, 2, 3, 4], final_exp=False)
        assert np.array_equal(got, want_products(range(5), range(5), [0] * 5, off5))
        state("the same call with all five blobs")
        with pytest.raises(legosnark_amd.LsaError):
            lsa.pairing_terms(P[0:5], np.array([0, 3, 2, 5], dtype=np.uint64), g2=Q[0:5], final_exp=False)
        state("a call whose offsets decrease")
        points("five points after it", [0, 1, 2, 3, 4], [0, 1, 2, 3, 4])
        # 7. a cache of 8 (smaller than four prefetch batches: every promise is kept at once), ten prefetches one by one
        lsa.g2_table_cache(8)
        state("cache of 8")
        for qi in range(10):
            lsa.g2_tables_prefetch(Q[qi].reshape(1, 24))
            state("prefetch of point %d" % qi)
        points("the ten prefetched points", list(range(10)), list(range(10)))
        lsa.g2_tables_prefetch(Q[7].reshape(1, 24))           # (the ten thrashed the eight slots: 0 .. 7 stayed)
        state("prefetch of a resident point")
        lsa.g2_tables_prefetch(Q[9].reshape(1, 24))
        state("prefetch of a point that lost its slot")
        # 8. a large cache: promises wait for the Miller call
        lsa.g2_table_cache(4096)
        state("cache of 4096 again")
        for qi in (5, 6, 7):
            lsa.g2_tables_prefetch(Q[qi].reshape(1, 24))
            state("promise of point %d" % qi)
        points("the three promised points and one more", [0, 1, 2, 3], [5, 6, 7, 8])
        lsa.g2_tables_prefetch(Q[10:12])
        state("two promises")
        lsa.g2_table_cache(16)
        state("cache of 16: the promises are dropped")
        # 9. a forced chunk of 2: the table route builds the tables of new points itself
        lsa.pairing_set_chunk(2)
        pis = [0, 1, 2, 3, 4, 5, 6]
        qis = [10, 11, 10, 4, 4, 4, 11]
        flags = np.array([0, 0, 1, 0, 1, 0, 0], dtype=np.uint8)
        off = np.array([0, 5, 5, 7], dtype=np.uint64)
        got = lsa.pairing_terms(P[pis], off, g2=Q[qis], flags=flags, final_exp=False)
        assert np.array_equal(got, want_products(pis, qis, flags, off))
        state("seven terms, two pairs per accumulator, three new points")
        got = lsa.pairing_terms(P[pis], off, g2=Q[qis], flags=flags, final_exp=True)
        ref = want_products(pis, qis, flags, off)
        assert np.array_equal(got, np.array([o.final_exponentiation(f) for f in ref]))
        state("the same with final exponentiations, all resident")
        lsa.pairing_set_chunk(0)
        # 10. one check: two terms, one conjugated, one value through the final exponentiation
        off1 = np.array([0, 2], dtype=np.uint64)
        got = lsa.pairing_terms(P[[0, 1]], off1, g2=Q[[10, 9]], flags=[0, 1], final_exp=True)
        assert np.array_equal(got[0], o.final_exponentiation(want_products([0, 1], [10, 9], [0, 1], off1)[0]))
        state("one check of two terms, one point new")
    finally:
        lsa.pairing_set_chunk(0)
        lsa.g2_table_cache(4096)

    record_to = os.environ.get("LSA_G2_TRACE_RECORD")
    if record_to:
        with open(record_to, "w") as f:
            json.dump(trace, f, indent=1)
            f.write("\n")
        return
    with open(GOLDEN) as f:
        golden = json.load(f)
    for got_row, want_row in zip(trace, golden):
        assert got_row == want_row
    assert len(trace) == len(golden)
