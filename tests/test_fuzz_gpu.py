"""GPU suite: deterministic randomised parity -- every operation kind of tests/fuzz_parity.py x three fixed seeds x a fixed
number of randomly drawn cases, each compared with the CPU oracle (tests/oracle_lib.py; large resident MSMs by the
known-discrete-log identity over oracle-made bases).

The other GPU tests pin chosen shapes; these draw sizes, sub-ranges, segment lists, thresholds and contents, among them
the scalars at the edges of the signed-digit recoder (fuzz_parity.edge_scalars).  The same commit always runs the same
cases: the case seeds are a function of (kind, seed) alone (fuzz_parity.case_seeds), and a failure names kind, case seed
and shape, so that

    import random, fuzz_parity as fz, legosnark_amd as lsa; lsa.init(0)
    fz.KINDS[kind](random.Random(case_seed), lsa)

replays it.  Conditions, not measurements: a case that raises fails, none is skipped, and the number executed must be the
number planned.  tests/test_fuzz_harness.py shows on the CPU that every kind fails when the library is one bit off.

Cost: 30 kinds x 3 seeds x 50 cases = 4500 cases in 90 tests, and 3 x 300 interleaved ones (test_fuzz_parity_interleaved).
Oracle side alone (drawing the inputs and the oracle's answers, the library replaced by a stand-in whose own time is
subtracted), 50 cases of the first seed on a development CPU: ORACLE_SECONDS below -- 20.4 s for the ten kinds the script
had, 14.3 s for the nine that came with the resident handles, 10.0 s for the eleven of the later provers and of key loading
(the slowest of those, scalar_mul_batch_g2, 3.5 s), about 45 s per seed and 135 s for the three.  Wall time of the whole
module on an MI355X box (its CPU is the faster one): 66 s for the 93 tests; the slowest are an interleaved sequence (3.5 s
for its 300 cases) and fr_fold (3.2 s), the slowest new kind scalar_mul_batch_g2 (2.2 s), so no kind had to be made
smaller."""
import pytest

import fuzz_parity as fz

pytestmark = pytest.mark.gpu

SEEDS = [20261016, 7, 314159]
CASES = 50

# measured, for the record (nothing asserts them): seconds for 50 cases of SEEDS[0], oracle side only
ORACLE_SECONDS = {"final_exp": 0.7, "eq_table": 0.6, "msm": 2.6, "batch_exp": 2.9, "scalar_mul_batch": 2.7, "pairing_terms": 0.7, "ntt": 0.4, "ntt_step": 0.7,
                  "fr_fold": 8.2, "sumcheck_round": 0.9, "resident_msm": 5.1, "segments": 2.3, "commit": 5.4, "sparse_matrix_msm": 0.1, "normalize": 0.2,
                  "sum_async": 0.2, "fq12_product": 0.1, "pairing_precomp": 0.7, "fr_scale_upper": 0.2,
                  "hadamard_quotient": 2.0, "lagrange": 1.4, "fr_matvec": 0.4, "fr_matmul": 0.2, "fr_sparse_matvec": 0.2, "qap_witness": 1.1, "decompress": 0.5,
                  "validate_points": 0.2, "compress": 0.2, "scalar_mul_batch_g2": 3.5, "sparse_matrix_msm_g2": 0.3}
GPU_WALL_SECONDS = 66


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kind", [name for name, _, _ in fz.CASES])
def test_fuzz_parity(lsa, kind, seed):
    executed, failed = fz.run_kind(lsa, kind, seed, CASES)
    assert executed == CASES, "%s seed %d: %d of %d cases ran" % (kind, seed, executed, CASES)
    assert not failed, "%s seed %d: %d of %d cases failed: %s" % (
        kind, seed, len(failed), CASES, "; ".join("case seed %d (%s)" % (s, what) for s, what in failed[:8]))


INTERLEAVED_PER_KIND = 10


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_parity_interleaved(lsa, seed):
    """All kinds in one shuffled sequence (300 cases per seed): a call that is only wrong after some OTHER entry point ran --
    as the witness recursion's unzeroed last entry was, found by the script's interleaved loop and by no run of one kind
    after the other.  Here the quotient and the witness map meet fr_ntt / fr_ntt_step on ntt.hip's shared table caches and
    change the domain under the step domain's table of 1 / Z, and every file's grow-only staging moves between calls."""
    plan = fz.interleaved_plan(seed, INTERLEAVED_PER_KIND)
    executed, failed = 0, []
    for kind, case_seed in plan:
        ok, what = fz.run_case(lsa, fz.KINDS[kind], case_seed)
        executed += 1
        if not ok:
            failed.append((kind, case_seed, what))
    assert executed == len(plan) == INTERLEAVED_PER_KIND * len(fz.CASES)
    assert not failed, "seed %d: %d of %d cases failed: %s" % (
        seed, len(failed), executed, "; ".join("%s case seed %d (%s)" % f for f in failed[:8]))
