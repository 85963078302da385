// legosnark_amd/csrc/crs_cache.h -- what the host-vector MSM entry points (capi.hip: msm_host_local) see of the CRS
// cache.  The cache itself -- its entries, threads and device buffers -- is private to crs_cache.hip, where it is described.
#pragma once
#include <stddef.h>
#include "../../include/legosnark_amd.h"

namespace lsa {
struct CrsEntry;
// whether a vector of n points goes through the cache (on, and n >= CRS_MIN_POINTS); reads the environment at first use
bool crs_wanted(size_t n);
// the fingerprint of the n points (point_bytes each) at bases_jac: begun on the cache's hashing threads, so that the
// caller can upload the scalars meanwhile; finished with this thread's help.  Every begin needs its finish, on error
// paths too: the workers read the caller's buffer.  (Sampled mode: both do nothing.)
void crs_fingerprint_begin(const void *bases_jac, size_t n, size_t point_bytes);
void crs_fingerprint_finish();
// n >= CRS_MIN_POINTS, after crs_fingerprint_finish: the resident entry that holds these points, inserted
// (uploaded and normalised on lsa_stream()) when there is none; *hit: it was there
int crs_lookup_or_insert(const void *bases_jac, size_t n, int group, CrsEntry **out, bool *hit);
// n < CRS_MIN_POINTS: the entry these points are a verified prefix of; nullptr: none (nothing is inserted)
CrsEntry *crs_lookup_small(const void *bases_jac, size_t n, int group);
// the device bases an MSM over the first n points of `e` runs on -- the entry's own layout or, built here on
// lsa_stream() when due, its prefix table -- and st.table / st.table_building
int crs_bases_for(CrsEntry *e, size_t n, const void **d_bases, size_t *table_stride, lsa_host_stats &st);
void crs_after_drain();        // lsa_stream() has just drained: frees what adopted tables left behind
void crs_shutdown();           // lsa_shutdown: every entry goes, both kinds of thread stop
}  // namespace lsa
