/* launch.h — every ytql_launch_* wrapper, declared once. kernels.hip defines
 * them and evaluator.cpp calls them; both include this header, so the
 * compiler checks each definition against the declaration its callers see
 * (the linkage is C: a mismatch would otherwise still link). */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"
#include "inlist.h"
#include "../../include/ytql_gpu.h"

extern "C" {
hipError_t ytql_launch_parse_segments(const ytql::DevSeg*, int, ytql::SegEx*, unsigned*, unsigned*, unsigned long long*, unsigned long long*, hipStream_t);
hipError_t ytql_launch_scan_nullflags(const ytql::DevSeg*, const ytql::SegEx*, int, unsigned*, hipStream_t);
hipError_t ytql_launch_scan_zzrange(const ytql::DevSeg*, const ytql::SegEx*, int, int, int,
                                    unsigned long long*, hipStream_t);
hipError_t ytql_launch_scan_partition(const ytql::PartParams*, const ytql::DevSeg*, const ytql::SegEx*,
                                      const ytql::FastCol*, ytql::TableHdr*, unsigned long long*,
                                      void*, unsigned long long*, uint64_t*,
                                      int, hipStream_t);
hipError_t ytql_launch_bucket_agg(const void*, const unsigned long long*, int64_t,
                                  const uint64_t*, const unsigned long long*, int64_t,
                                  ytql::OutGroup*, unsigned long long*, int64_t, int,
                                  ytql::TableHdr*, int, int, int, int,
                                  uint64_t, uint64_t, int, hipStream_t);
hipError_t ytql_launch_bucket_agg_direct(const void*, const unsigned long long*, int64_t,
                                         const uint64_t*, const unsigned long long*, int64_t,
                                         ytql::OutGroup*, unsigned long long*, int64_t, int,
                                         ytql::TableHdr*, int, int, int, int,
                                         uint64_t, uint64_t, int, int, hipStream_t);
hipError_t ytql_launch_topk_hist(const ytql::DevPlan*, const ytql::DevSeg*, const ytql::SegEx*,
                                 const int32_t*, const int32_t*, int64_t,
                                 const ytql::JoinDev*, const ytql::JoinDev*,
                                 const ytql::TopkPass*, unsigned long long*,
                                 unsigned long long*, unsigned*, hipStream_t);
hipError_t ytql_launch_topk_gather(const ytql::DevPlan*, const ytql::DevSeg*, const ytql::SegEx*,
                                   const int32_t*, const int32_t*, int64_t,
                                   const ytql::JoinDev*, const ytql::JoinDev*,
                                   const ytql::TopkGather*,
                                   int64_t*, unsigned long long*,
                                   int64_t*, unsigned long long*,
                                   int64_t*, unsigned long long*,
                                   unsigned*, hipStream_t);
hipError_t ytql_launch_topk_materialize(const ytql::DevPlan*, const ytql::DevSeg*, const ytql::SegEx*,
                                        const int32_t*, const int32_t*,
                                        const ytql::JoinDev*, const ytql::JoinDev*,
                                        const int64_t*, int64_t, ytql::DevOutVal*,
                                        unsigned*, hipStream_t);
hipError_t ytql_launch_topk_hist_fast(const ytql::DevSeg*, const ytql::SegEx*, int, int,
                                      int64_t, int, int, const ytql::TopkPass*,
                                      unsigned long long*, unsigned long long*,
                                      hipStream_t);
hipError_t ytql_launch_topk_gather_fast(const ytql::DevSeg*, const ytql::SegEx*, int, int,
                                        int64_t, int, int, const ytql::TopkGather*,
                                        int64_t*, unsigned long long*,
                                        int64_t*, unsigned long long*,
                                        int64_t*, unsigned long long*,
                                        hipStream_t);
hipError_t ytql_launch_versioned_read(const ytql::VSegDev*, int, int64_t, uint64_t,
                                      uint64_t*, uint8_t*, uint8_t*, uint8_t*,
                                      hipStream_t);
hipError_t ytql_launch_vis_count(const uint8_t*, int64_t,
                                 unsigned long long*, int, hipStream_t);
hipError_t ytql_launch_unvcol_to_arrays(const ytql::DevSeg*, const ytql::SegEx*, int, int,
                                        int64_t, uint64_t*, uint8_t*,
                                        unsigned*, hipStream_t);
hipError_t ytql_launch_vis_scatter(const uint8_t*, const uint8_t*,
                                   const uint64_t*, int64_t,
                                   const unsigned long long*, uint64_t,
                                   const int64_t*, char*, int, int, hipStream_t);
hipError_t ytql_launch_join_build(const ytql::JoinDev*, int64_t, uint64_t*,
                                  long long*, unsigned long long*, unsigned*,
                                  hipStream_t);
hipError_t ytql_launch_join_chain(const ytql::JoinDev*, int64_t, unsigned*,
                                   hipStream_t);
hipError_t ytql_launch_strjoin_build(const ytql::JoinDev*, int64_t, uint64_t*,
                                     long long*, unsigned long long*, unsigned*,
                                     unsigned long long*, hipStream_t);
hipError_t ytql_launch_strjoin_chain(const ytql::JoinDev*, int64_t, unsigned*,
                                     hipStream_t);
hipError_t ytql_launch_strjoin_entries(const ytql::DevSeg*, const ytql::SegEx*, int, int,
                                       const int64_t*, int64_t, const ytql::JoinDev*,
                                       int32_t*, hipStream_t);
hipError_t ytql_launch_scan_project(const ytql::DevPlan*, const ytql::DevSeg*, const ytql::SegEx*,
                                    const int32_t*, const int32_t*, int64_t,
                                    int64_t, const ytql::JoinDev*, const ytql::JoinDev*,
                                    ytql::DevOutVal*, uint8_t*, unsigned*, hipStream_t);
hipError_t ytql_launch_proj_offsets(const ytql::DevSeg*, const ytql::SegEx*, ytql::DevOutVal*,
                                    const uint8_t*, int64_t, int, unsigned,
                                    ytql::ProjTot*, ytql::ProjTot*, hipStream_t);
hipError_t ytql_launch_proj_scatter(const ytql::DevOutVal*, const uint8_t*, int64_t,
                                    int, unsigned, int, const ytql::ProjTot*,
                                    ytql::DevOutVal*, ytql::StrGatherRec*, hipStream_t);
hipError_t ytql_launch_str_reclen(const ytql::DevSeg*, const ytql::SegEx*, ytql::StrGatherRec*,
                                  int64_t, hipStream_t);
hipError_t ytql_launch_str_gather(const ytql::DevSeg*, const ytql::SegEx*,
                                  const ytql::StrGatherRec*, int64_t, char*, uint64_t,
                                  hipStream_t);
hipError_t ytql_launch_scan_generic(const ytql::DevPlan*, const ytql::DevSeg*, const ytql::SegEx*,
                                    const int32_t*, const int32_t*, int64_t,
                                    const ytql::JoinDev*, const ytql::JoinDev*,
                                    ytql::TableHdr*, unsigned long long*, unsigned*,
                                    const ytql::StrKeyDev*, hipStream_t);
hipError_t ytql_launch_scan_fast(const ytql::FastParams*, const ytql::DevSeg*, const ytql::SegEx*,
                                 const ytql::FastCol*, ytql::TableHdr*, unsigned long long*,
                                 unsigned long long*, size_t, int, hipStream_t);
hipError_t ytql_launch_compact(ytql::TableHdr*, ytql::TableHdr*, const unsigned long long*, int,
                               ytql::OutGroup*, unsigned long long*, uint64_t, hipStream_t);
hipError_t ytql_launch_part_count(const ytql::OutGroup*, int64_t, int, int,
                                  unsigned long long*, hipStream_t);
hipError_t ytql_launch_part_scatter(const ytql::OutGroup*, int64_t, int, int, int,
                                    int, unsigned long long*, YtStateRow*,
                                    hipStream_t);
hipError_t ytql_launch_merge_states(const YtStateRow*, int64_t, int, int,
                                    int, ytql::TableHdr*, unsigned long long*,
                                    hipStream_t);
hipError_t ytql_launch_strgrp_accum(const ytql::StrGroupParams*, const ytql::DevSeg*, const ytql::SegEx*,
                                    const int64_t*, unsigned long long*, ytql::TableHdr*,
                                    hipStream_t);
hipError_t ytql_launch_strgrp_hash(const ytql::DevSeg*, const ytql::SegEx*, int, int,
                                   const int64_t*, uint64_t*, uint64_t*,
                                   ulonglong2*, int64_t, hipStream_t);
hipError_t ytql_launch_strgrp_merge(const ytql::DevSeg*, const ytql::SegEx*, int, int,
                                    const int64_t*, const unsigned long long*,
                                    const uint64_t*, const uint64_t*,
                                    const ulonglong2*, ytql::StrSlot*, uint64_t, int,
                                    ytql::TableHdr*, int64_t, hipStream_t);
hipError_t ytql_launch_strgrp_compact(const ytql::DevSeg*, const ytql::SegEx*, int,
                                      const ytql::StrSlot*, uint64_t, ytql::OutStrGroup*,
                                      unsigned long long*, char*, unsigned long long*,
                                      uint64_t, ytql::TableHdr*, hipStream_t);
hipError_t ytql_launch_strkey_claim(const ytql::DevSeg*, const ytql::SegEx*, int, int,
                                    const int64_t*, const uint64_t*, const uint64_t*,
                                    const ulonglong2*, ytql::StrSlot*, uint64_t,
                                    uint32_t*, ytql::TableHdr*, int64_t, hipStream_t);
hipError_t ytql_launch_strkey_compact(const ytql::DevSeg*, const ytql::SegEx*, int,
                                      ytql::StrSlot*, uint64_t, ytql::StrKeyId*,
                                      unsigned long long*, char*, unsigned long long*,
                                      uint64_t, ytql::TableHdr*, hipStream_t);
hipError_t ytql_launch_strkey_remap(const ytql::StrSlot*, uint32_t*, int64_t,
                                    hipStream_t);
hipError_t ytql_launch_strpred_entries(const ytql::DevSeg*, const ytql::SegEx*, int, int,
                                       const int64_t*, int64_t, int, int,
                                       const char*, int64_t, uint64_t*,
                                       hipStream_t);
hipError_t ytql_launch_inlist_str_entries(const ytql::DevSeg*, const ytql::SegEx*, int, int,
                                          const int64_t*, int64_t,
                                          const ytql::InStrSlot*, uint64_t, const char*,
                                          int, uint64_t*, hipStream_t);
hipError_t ytql_launch_strgen_accum(const ytql::DevPlan*, const ytql::DevSeg*, const ytql::SegEx*,
                                    const int32_t*, const int32_t*, int, int64_t,
                                    const int64_t*, unsigned long long*,
                                    ytql::TableHdr*, unsigned*, hipStream_t);
hipError_t ytql_launch_strgen_merge(const ytql::DevSeg*, const ytql::SegEx*, int, int,
                                    const int64_t*, const unsigned long long*,
                                    const ytql::StrGenAggs*, const uint64_t*,
                                    const uint64_t*, const ulonglong2*,
                                    ytql::StrSlot*, uint64_t, unsigned long long*,
                                    ytql::TableHdr*, int64_t, hipStream_t);
hipError_t ytql_launch_strgen_gather(ytql::OutStrGroup*, int64_t,
                                     const unsigned long long*, uint64_t, int,
                                     ytql::OutStrAgg*, int, int, hipStream_t);
hipError_t ytql_launch_strst_count(const ytql::OutStrGroup*, int64_t, const char*,
                                   int, unsigned long long*,
                                   unsigned long long*, hipStream_t);
hipError_t ytql_launch_strst_scatter(const ytql::OutStrGroup*, int64_t, const char*,
                                     int, int, unsigned long long*,
                                     unsigned long long*, YtStateRow*, char*,
                                     const unsigned long long*, hipStream_t);
hipError_t ytql_launch_strst_hash(const YtStateRow*, int64_t, const int64_t*,
                                  const unsigned long long*, int, const char*,
                                  uint64_t*, uint64_t*, ulonglong2*,
                                  uint64_t*, hipStream_t);
hipError_t ytql_launch_strst_merge(const YtStateRow*, int64_t, const char*,
                                   const uint64_t*, const uint64_t*,
                                   const ulonglong2*, const uint64_t*, int,
                                   ytql::StrSlot*, uint64_t, ytql::TableHdr*, hipStream_t);
hipError_t ytql_launch_strst_compact(const ytql::StrSlot*, uint64_t,
                                     const uint64_t*, const char*,
                                     ytql::OutStrState*, unsigned long long*,
                                     char*, unsigned long long*, uint64_t,
                                     ytql::TableHdr*, hipStream_t);
}
