"""CPU suite: every LSA_* environment switch the library reads is accounted for.

A switch that selects a kernel or a code path is only as good as the test that sets it: the paths behind LSA_NTT_T1_MB=0,
LSA_NO_REC32 and a dozen others shipped documented and unexercised until tests/test_switch_paths_gpu.py.  This file keeps the
list closed.  Every string literal "LSA_..." under legosnark_amd/csrc (they are all names handed to getenv, directly or through
a helper) must appear in TABLE below with either
  * test: the id of a test that SETS the switch in a child's environment -- the module must exist, define that test and name
    the switch; or
  * reason: one line on why no test sets it -- it selects no computation (tracing, warm-up sizes, thread counts), or it is the
    start-up value of a setting the suite drives through the API call named in the reason, or a size threshold between two
    paths the suite runs on both sides of at the default value;
and in INTEGRATION.md's table of switches.  A switch added later without a test or a reason fails here."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "legosnark_amd", "csrc")

SP = "test_switch_paths_gpu::"
TABLE = {
    # ---- switches a test sets
    "LSA_NTT_T1_MB": {"test": SP + "test_n1_two_level_twiddle_and_coset_lookups"},
    "LSA_NTT_CACHE_MB": {"test": SP + "test_n2_table_eviction_by_bytes_under_queued_transforms"},
    "LSA_NO_REC32": {"test": SP + "test_m1_64_bit_sort_records"},
    "LSA_NO_PART": {"test": "test_sort_paths_gpu::test_partitioned_and_scatter_sorts_agree"},
    "LSA_NO_REDUCE_BITS": {"test": SP + "test_m3_blocking_calls_without_the_bit_trees"},
    "LSA_NO_LANE_L1": {"test": SP + "test_m4_queued_calls_without_the_lane_private_level"},
    "LSA_G2_LANE_L1": {"test": SP + "test_m5_g2_lane_private_first_level"},
    "LSA_WIDE_BIG_MIN": {"test": SP + "test_m6a_narrow_digits_at_2pow16_pairs"},
    "LSA_G2_PREPARE_OLD": {"test": SP + "test_m7_g2_bases_through_the_older_conversion"},
    "LSA_MLE_DOT": {"test": SP + "test_f1_eval_mle_by_fold_passes"},
    "LSA_BEXP_TABLES": {"test": SP + "test_f2_batch_exp_without_kept_tables"},
    "LSA_FR_GRAPHS": {"test": "test_fr_vec_gpu::test_fold_schedules_behind_their_switches_give_the_oracles_bytes"},
    "LSA_SC3": {"test": "test_fr_vec_gpu::test_sumcheck_three_tables_both_kernels"},
    "LSA_NO_COMPACT": {"test": "test_g1_bucket_addition_gpu::test_wide_path_one_lane_kernel_and_heavy_kernels"},
    "LSA_NO_COMPACT_G2": {"test": SP + "test_m5_g2_lane_private_first_level"},
    "LSA_COMPACT_MAX": {"test": "test_msm_slot_modes_gpu::test_queued_and_blocking_calls_in_every_slot_mode"},
    "LSA_NO_OVERLAP": {"test": "test_msm_slot_modes_gpu::test_queued_and_blocking_calls_in_every_slot_mode"},
    "LSA_TAIL_SLOTS": {"test": "test_msm_slot_modes_gpu::test_queued_and_blocking_calls_in_every_slot_mode"},
    "LSA_WIDE_SPLIT": {"test": "test_accumulate_prefetch_gpu::test_two_lanes_per_bucket_on_the_wide_path"},
    "LSA_G2_PAIR": {"test": "test_g2_pair_kernel_gpu::test_pair_kernel_matches_the_oracle"},
    "LSA_MILLER_KERNEL": {"test": "test_pairing_gpu::test_every_miller_kernel_vs_oracle"},
    "LSA_MILLER_NAF": {"test": "test_pairing_gpu::test_signed_digit_miller_loop_gives_the_same_gt"},
    "LSA_FUSED_LOCKSTEP": {"test": "test_pairing_gpu::test_signed_digit_miller_loop_gives_the_same_gt"},
    "LSA_FE_HELPER": {"test": "test_pairing_gpu::test_final_exponentiation_of_arbitrary_elements"},
    "LSA_MILLER_TAB": {"test": "test_pairing_precomp_gpu::test_the_older_kernels_behind_their_switches_give_the_same_bytes"},
    "LSA_MILLER_ROWS": {"test": "test_pairing_precomp_gpu::test_the_older_kernels_behind_their_switches_give_the_same_bytes"},
    "LSA_MILLER_SPLIT": {"test": "test_pairing_precomp_gpu::test_the_older_kernels_behind_their_switches_give_the_same_bytes"},
    "LSA_H2D": {"test": "test_host_copies_gpu::test_staged_direct_and_default_copies_agree"},
    "LSA_COMM_LOOPBACK": {"test": "test_comm::test_multi_rank_step_on_one_gpu_with_loopback_peers"},
    "LSA_TRACE": {"test": "test_shutdown_cycle_gpu::test_two_init_shutdown_cycles_grow_and_free_the_same_staging"},
    "LSA_WARM": {"test": "test_shutdown_cycle_gpu::test_two_init_shutdown_cycles_grow_and_free_the_same_staging"},
    # ---- switches no test sets
    "LSA_WARM_MB": {"reason": "size of the workspaces lsa_init allocates ahead of the first call: no kernel depends on it"},
    "LSA_HASH_THREADS": {"reason": "host threads of the CRS cache's content fingerprint: the same digest from any number of them (tests/cpp/test_crs_index.cc)"},
    "LSA_H2D_THREADS": {"reason": "host threads that share a staged copy's memcpy: the bytes copied are the same"},
    "LSA_H2D_STREAMS": {"reason": "copy streams beside lsa_stream(): ordering of the same copies, no computation"},
    "LSA_H2D_SLOT_KB": {"reason": "size of a pinned staging slot: the same copies in other pieces"},
    "LSA_H2D_DIRECT_AFTER": {"reason": "sightings of a large buffer before its copies go direct: both copy paths run under LSA_H2D in tests/test_host_copies_gpu.py"},
    "LSA_CRS_CACHE": {"reason": "start-up value of lsa_crs_cache_configure(), which tests/test_crs_cache_gpu.py drives through every mode"},
    "LSA_CRS_CACHE_MB": {"reason": "start-up value of the byte budget lsa_crs_cache_configure() takes (tests/test_crs_cache_gpu.py)"},
    "LSA_CRS_TABLE_AFTER": {"reason": "start-up value of lsa_crs_cache_table_after(), which the CRS cache tests set"},
    "LSA_CRS_PREFIX_TABLE": {"reason": "length of the prefix that gets copies on a first small request: a size; tests/test_msm_compact_gpu.py runs with and without the prefix table"},
    "LSA_CRS_PREFIX_AFTER_G2": {"reason": "requests served from the plain layout before a G2 prefix table is built: both layouts run in tests/test_msm_compact_g2_gpu.py"},
    "LSA_PRECOMPUTE": {"reason": "0 keeps every handle on the plain layout, which handles built under lsa_msm_set_table_threshold(1 << 30) take in the suite"},
    "LSA_PRECOMPUTE_MIN": {"reason": "start-up value of lsa_msm_set_table_threshold(), which the MSM tests set"},
    "LSA_COMPACT_MAX_G2": {"reason": "size threshold between the compact and the general G2 pipeline: both sides run at the default (tests/test_msm_compact_g2_gpu.py)"},
    "LSA_G2_TABLES": {"reason": "start-up capacity of the G2 line-table cache, which lsa_g2_table_cache() sets in tests/test_pairing_precomp_gpu.py"},
    "LSA_G2_PREFETCH_BATCH": {"reason": "how many promised line tables wait before they are built: when, not what"},
}


def switches_read():
    """{switch: [files]} over every source file of the library."""
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "**", "*"), recursive=True)):
        if not path.endswith((".hip", ".h", ".cc", ".cpp", ".hpp")):
            continue
        for name in re.findall(r'"(LSA_[A-Z0-9_]+)"', open(path, errors="ignore").read()):
            found.setdefault(name, []).append(os.path.relpath(path, ROOT))
    return found


def test_the_scan_finds_the_switches():
    found = switches_read()
    assert len(found) >= 40 and "LSA_NTT_T1_MB" in found and "LSA_G2_LANE_L1" in found and "LSA_TRACE" in found


def test_every_switch_read_has_a_test_or_a_reason():
    found = switches_read()
    missing = sorted(set(found) - set(TABLE))
    assert not missing, "switches without a test or a reason: %s" % {m: found[m] for m in missing}
    stale = sorted(set(TABLE) - set(found))
    assert not stale, "table entries for switches nothing reads any more: %s" % stale
    for name, entry in TABLE.items():
        assert set(entry) in ({"test"}, {"reason"}), name
        if "reason" in entry:
            assert len(entry["reason"]) >= 20 and "\n" not in entry["reason"], name


def test_every_named_test_exists_and_names_its_switch():
    for name, entry in TABLE.items():
        if "test" not in entry:
            continue
        module, test = entry["test"].split("::")
        path = os.path.join(ROOT, "tests", module + ".py")
        assert os.path.exists(path), (name, path)
        text = open(path).read()
        assert re.search(r"^def %s\(" % re.escape(test), text, flags=re.M), (name, entry["test"])
        assert name in text, "%s does not mention %s" % (module, name)


def test_every_switch_is_in_the_integration_table():
    rows = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if l.startswith("| `LSA_")]
    documented = set()
    for row in rows:
        documented |= set(re.findall(r"LSA_[A-Z0-9_]+", re.split(r"(?<!\\)\|", row)[1]))      # the first cell (\| is a literal bar)
    missing = sorted(set(switches_read()) - documented)
    assert not missing, "not in INTEGRATION.md's table of switches: %s" % missing


def test_ntt_params_answer_without_a_device():
    """lsa_fr_ntt_param: the default budgets, an empty cache, 0 for an unknown selector."""
    import legosnark_amd as lsa
    if not any(k in os.environ for k in ("LSA_NTT_CACHE_MB", "LSA_NTT_T1_MB")):
        p = lsa.fr_ntt_params()
        assert p["cache_budget"] == 2048 << 20 and p["t1_budget"] == 512 << 20
    assert lsa.lib().lsa_fr_ntt_param(99) == 0 and lsa.lib().lsa_fr_ntt_param(-1) == 0
