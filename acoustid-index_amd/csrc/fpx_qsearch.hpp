// fpx_qsearch.hpp -- k_search_query: IndexReader.search (src/Index.zig:170-177) for ONE QUERY PER WORKGROUP over a packed group --
// dedupSorted (:489-499), FileSegment.search for all sixteen segments (src/FileSegment.zig:135-180), SearchResults.incr and the
// min_score filter of finish (src/common.zig:121-145) in one kernel, the query's hit records never leaving the CU.
// Part of the fpx_search.hip translation unit (after fpx_pgroup.hpp and fpx_score_bin.hpp, whose line layout and candidate hand-over it shares).
// fpx_qframe.hpp, behind this file, holds the same LDS layout, counting tail and hand-over ONCE for k_search_side and k_search_words (sizes
// asserted equal to the ones here); this kernel keeps its own text of them -- qs_cold_args(), the next query's loads, CLS and LOW run through it.
//
// Rounds 2-5 ran the batch as a pipeline over ALL its query hashes: keys made and ordered by hash bucket (two kernels + a radix pass),
// one probe kernel that drops the hit records -- 7 per query hash on the 100 M index, 237 MB per batch of 8192 -- into bins in HBM, one
// scoring kernel that reads them back twice.  Measured (profiles/r05_*): the probe kernel sits at 0.78 of the rate this chip serves
// memory REQUESTS at, and 29 % of its requests are the records' writes; the order of the keys buys it 8 % (profiles/r06_locality.txt:
// 0.409 ms with the keys ordered by their top 8 hash bits, 0.444 in query order -- every line read anywhere in 137 GB).  So the records
// stay where they are produced: a workgroup owns a query, reads its ~1000 lines (random HBM requests, the only ones left), appends the
// docs to a record array in LDS and counts them in a filter of 16-bit cells as it goes; the docs whose cell reaches the query's floor are
// counted exactly in a small LDS table (the records are read again -- from LDS) and leave as candidates for k_finish.  No keys, no sort,
// no bins: HBM sees the line reads and a few bytes of results.
//
// The rounds, EIGHT LANES TO A LINE (the unfiltered instantiations): a round is a hash per lane, but a hash's line is fetched ONCE and
// WHOLE by the eight lanes of its lane's group -- load instruction k of eight: every group reads the line of the hash its lane k holds,
// lane `sub` words 4 sub .. 4 sub + 3 --, all 64 lines of a wave's round under way at once in 32 registers per lane.  The per-lane walk
// made about three ACCESSES per hash -- a load instruction touching a distinct line: the head, the 16-byte pieces of the words, the
// overflow offset -- and the second trip waited for the first; this one makes one, and no trip depends on another.  (The calibration
// kernels, k_bw_pattern in profiles/r07_kernel_stats.csv, suggest that the chip serves 72 - 76 G accesses per second whatever they carry:
// a hypothesis -- counted, profiles/r10_tcp_accesses.txt, the per-lane walk made 3.4 accesses per hash at 0.85 of that rate, this one 2.5.)
// The hash's own lane takes the head from its group's lane 0 and the `ext` offset from lane 7, does the head's arithmetic
// and the per-hash statistics once; what the group needs of it goes back ready-made -- two words indexed by the LINE's word number: which
// words are the hash's, which of them second words of doubles; and, before the loads, the line's number in the group --, and every lane
// classifies its own four words of each line where they landed: every inline word is walked, only lists and words in `ext` are tasks.
// The filtered form keeps the per-lane walk (a word's column is bookkeeping of its own) -- but for k_search_filt (`COOP`, option
// filt_coop = 1) and k_search_low_coop (`LOW | COOP`, with option low_wg = 3): the same rounds for a filtered group, a word's column
// looked for only where the group's union dead-set bitmap says so.
//
// Taken by run_batch for snapshots that are ONE packed group and nothing else (the resident index between merges), every column searched,
// no superseded docs, queries of up to QS_MAX_HASHES hashes with a floor above 2; a query whose records outgrow the LDS array (hot
// hashes: hundreds of docs per list) fails the batch over to the pipeline above (CTR_BINFAIL), which stays the path for everything else.
//
// THE FAMILY: ten kernels over one body, qs_body<V> -- V a qs_variant that NAMES what is on; what a form changes sits under
// `if constexpr (<its flag>)`.  Every kernel takes the same two by-value parameters (QSearchArgs, GroupArgs): qs_cold_args()'s layout
// holds for all of them.  NS: columns of a line (8 | 16); QS: per-query statistics; MEM: the memory segments' table (an instantiation of
// its own: the look-up costs the usual one registers); FILT: a group with superseded docs and/or columns outside the snapshot.
//
//   kernel <parameters>                 | flags (qs_variant)  | context option = value            | launched by                             | lacks
//   ------------------------------------+---------------------+-----------------------------------+-----------------------------------------+----------------------------------
//   k_search_query    <NS,QS,MEM,FILT>  | --                  | query_wg = 1 (FILT: 2)            | run_query_wg, the first (only) group    | low floors
//   k_search_classes  <NS,MEM>          | CLS  (QS on)        | hot_wg = 1                        | redo_hot_queries, the redo list's       | FILT, low floors, the queue of
//                                       |                     |                                   | entries behind k_search_query           | queries, four workgroups per CU
//   k_search_low      <NS,QS,MEM>       | LOW                 | low_wg = 1                        | run_query_wg, first group of a batch    | redo list (hot_wg ignored), FILT
//                                       |                     |                                   | that HAS a floor of 1 or 2              |
//   k_search_low_filt <NS,QS,MEM>       | LOW  (FILT on)      | low_wg = 2 under query_wg = 2     | the same, a filtered first group        | redo list
//   k_search_filt     <NS,QS,MEM>       | COOP (FILT on)      | filt_coop = 1 under query_wg = 2  | run_query_wg, ONE filtered group whose  | redo list, low floors
//                                       |                     |                                   | snapshot holds the union bitmap         |
//   k_search_low_coop <NS,QS,MEM>       | LOW | COOP (FILT on)| low_wg = 3 with filt_coop = 1     | the same, a batch that HAS a floor of   | redo list
//                                       |                     | under query_wg = 2                | 1 or 2                                  |
//   k_search_next     <NS,QS,FILT>      | NEXT                | groups_wg = 1                     | run_query_wg, groups 1 ..               | redo list, MEM, low floors
//   k_search_low_next <NS,QS,FILT>      | LOW | NEXT          | groups_wg = 2 with low_wg         | run_query_wg, groups 1 .. of a batch    | redo list, MEM
//                                       |                     |                                   | with a floor of 1 or 2                  |
//   k_search_window   <NS,MEM,FILT>     | SHARE               | shard_wg = 1 (FILT: 2)            | shard_probe_impl (fpx_shard_probe)      | QS, redo list, low floors,
//                                       |                     |                                   |                                         | filter, table, candidates
//   k_search_packed   <NS,MEM,FILT>     | SHARE | PACK        | shard_pack = 1 under shard_wg     | shard_probe_impl, longest query of at   | the same
//                                       |                     |                                   | most QS_PACK_MAX hashes                 |
//
// What the rows rest on:
// CLS -- a query whose records outgrew the array is named in the batch's redo list, with nothing counted for it, and walked once per DOC
//   CLASS, keeping one class of records each time: a doc's postings are all in one class, so each pass counts exactly and the passes'
//   candidates are disjoint.  The batch stays here and nothing backs off.  The rare path: a query's walk C times over (its lines are in
//   the L2 after the first).
// LOW -- the legacy protocol's min_score 1, HTTP queries of 40 hashes or fewer.  For those the filter and the table are no use -- every
//   doc counted is at or above the floor --: their tail SORTS the record array in place and reads the scores off the runs, only the top
//   max_results leave; a query of the same batch with a floor above 2 takes the usual tail.  Launched for such a batch only.  With FILT
//   (k_search_low_filt -- a name of its own: k_search_low keeps its three parameters) nothing more is needed: the filtered walk drops a
//   superseded doc where it would be emitted, a column outside the snapshot gives no record, the memory segments' table holds live
//   postings only -- when s_count is final the record array holds live docs only, which is all the sorted tail asks for.  Its scratch is
//   the filter's area, which the task queue left before (tcols, behind the queue, was last read by the last task).  Blocks, docs, qstats
//   and the histograms stay the filtered form's (counted before supersession).  No redo list under LOW: a query over QS_REC_CAP records
//   (FILT: or over the filtered queue's QS_TASKS_FILT tasks) hands the batch to the pipeline, with the back-off.
// FILT -- every word knows its column, as in k_probe_pgroup's per-column walk: a column outside `active` gives no record and no
//   statistic, a doc of a column with a dead set is dropped after it was counted (CTR_DOCS counts before supersession).
// COOP -- the filtered job by the unfiltered form's rounds, eight lanes to a line.  What the per-lane walk needed every word's column for
//   is done without: the hash's lane takes the words of columns outside the snapshot out of the line's mask before it is broadcast; a
//   kept doc is tested against the group's UNION dead-set bitmap of the snapshot (bit doc - gmin, exactly what the word holds), and only a
//   doc whose bit is set -- a superseded one, or its live rewrite in a newer column -- finds its column (pm | dm << 16 and start from the
//   hash's lane) and runs the column's exact test; a list's task carries its column the same way, `ext` words' tasks theirs from the
//   hash's lane.  The tasks phase is the filtered form's, with the union test in front of every exact one.  Everything else that is
//   filtered keeps the per-lane walk.
// LOW | COOP -- the two compose without new machinery: LOW changes only the query's tail, COOP only the rounds and the tasks' tests, and
//   COOP leaves live docs only in the record array as the per-lane filtered walk does -- a kept word whose union bit is clear is live in
//   every column, one whose bit is set ran its column's exact test before it was emitted --, which is all the sorted tail asks for.
//   Nothing of the rounds or the tasks is live in the filter's area or the queue when the tail takes them as scratch: the tasks loop ends
//   behind a barrier with every task and its tcols word read, the filter's atomics behind the tail's first.  A query of the same launch
//   with a floor above 2 takes the usual tail.  Registers: what the tail makes of the lane's number is taken afresh there (lt, llane), as
//   load_pair's `t` and the filter loop's `tc4` are, and the relative floor is worked out in 32 bits -- held from the kernel's start
//   across the rounds they were 20 bytes of scratch at 16 columns.  The union bitmap rides where the redo list would: LOW has none.
// NEXT -- a snapshot of several packed groups is walked group by group, a launch each on the batch's stream.  A doc lives in one segment,
//   hence in one group: every launch counts its docs whole and the launches' candidates are disjoint, so they only have to meet in the
//   same slots and the same shared list -- the hand-over CHAINS behind what the launch before left in qcand_n[q], and qstats[q] is
//   added to.  Everything else a launch reports is additive already (atomic adds and maxima into the batch's counters and sets).  The
//   memory segments ride on the first group's launch.
// LOW | NEXT -- the sorted tail's candidates -- each group's top max_results under its own raised floor, a superset of what k_finish
//   keeps of the group -- go through the same buffer, flags and shared list into the chained hand-over.  What the composition rests on:
//   the records become absolute ids with the gmin of THIS launch's group (the kernel's own GroupArgs); the sorted tail leaves its
//   candidates where the usual one does -- cbuf, s_ccnt, s_cshared and the shared list --, its scratch is the filter's area, and it never
//   touches s_claimed / s_full, which the chained hand-over takes behind the tail's last barrier; a query without a record here (or with
//   fewer than its floor) skips both tails with s_ccnt = 0, and the hand-over then leaves the earlier launches' slots, count and mark as
//   they are.  The floor a launch raises by its own group's best score is a lower bound of the one k_finish applies, and the union of
//   every group's top max_results in (score descending, id ascending) order holds the snapshot's.
// SHARE -- a rank's HASH-WINDOW slice of ONE group, for a step of the sharded bin protocol.  The dedup loop's window test leaves the other
//   windows' hashes to their ranks; what a rank owes the protocol is the query's RECORDS, not its counts -- they go to the query's bin of
//   2^QS_SHARE_BQ queries in the caller's send buffer, in bin_store's form (fpx_partition.hpp), one reservation per query.  MEM: the
//   same table on every rank; only the window's hashes are looked up.  The record protocol keeps the low floors.
// SHARE | PACK -- a rank of N sees 1 / N of a query's hashes: a hash outside the window never enters the set, the first occurrences
//   inside it get dense places 0 .. m - 1 (a list in LDS, where the set was), every lane takes its hashes of the up to four rounds back
//   from there, and the rounds are ceil(m / 256), not ceil(n / 256); a wave without a probe in a round skips its walk.  A lane to every
//   PROBE, not to every hash of a round: one round at 4 and 8 ranks where k_search_window walks four, three waves in four idle in it at 8.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "fpx_internal.h"

namespace fpx {

#ifndef FPX_QS_WG
#define FPX_QS_WG 256
#endif
#ifndef FPX_QS_WAVES
#define FPX_QS_WAVES 4
#endif
#ifndef FPX_QS_REC_CAP
#define FPX_QS_REC_CAP 8192
#endif
#ifndef FPX_QS_FLOG2
#define FPX_QS_FLOG2 11
#endif
constexpr uint32_t QS_WG = FPX_QS_WG;
constexpr uint32_t QS_REC_CAP = FPX_QS_REC_CAP;    // records of a query held in LDS (the 100 M index: 6 200 per query of 1000 hashes)
constexpr uint32_t QS_FLOG2 = FPX_QS_FLOG2;        // the filter: 2^11 16-bit cells
constexpr uint32_t QS_TLOG2 = 8;                   // the exact table: 2^8 slots of doc << 32 | count
constexpr uint32_t QS_MAX_HASHES = QS_REC_CAP >= 8192u ? 4096u : 2048u;   // longest query taken (its hash set: up to QS_REC_CAP slots, before the records move in)
constexpr uint32_t QS_MAX_ROUNDS = 32;             // (a lane remembers which of its rounds' hashes are probes in one word)
#ifndef FPX_QS_WORDS
#define FPX_QS_WORDS 12
#endif
#ifndef FPX_QS_CH
#define FPX_QS_CH 2
#endif
constexpr uint32_t QS_WORDS = FPX_QS_WORDS;                  // (FILT) words of a hash walked by its lane (16-byte pieces of its line); the rest are tasks
constexpr uint32_t QS_CH = FPX_QS_CH;                      // rounds whose hashes a lane holds together ((FILT) whose line heads are under way together)
constexpr uint32_t QS_TASKS = (((size_t)2u << QS_FLOG2) + ((size_t)8u << QS_TLOG2)) / 8u;      // deferred lists / words of a query (8 bytes each: they live where the filter and the exact table will)
constexpr uint32_t QS_TASK_WORDS = 8;              // words a deferred "words" task carries at most (a list's task: its header + seven docs)
constexpr uint32_t QS_TASKS_FILT = QS_TASKS * 8u / 12u;      // (FILT) the same bytes hold fewer tasks: each has a word of its words' columns behind the queue
static_assert(QS_MAX_HASHES * 2u <= QS_REC_CAP, "the dedup set lives where the records will");
static_assert((QS_MAX_HASHES + QS_WG - 1u) / QS_WG <= QS_MAX_ROUNDS, "rounds per query");
static_assert(QS_WORDS % 4 == 0 && QS_WORDS <= 16, "the words are fetched in 16-byte pieces; a lane's masks of them are 16 bits");
#ifndef FPX_QS_DYN
#define FPX_QS_DYN 1               // 1: a launch's workgroups take their queries from a counter (after their first two); 0: every gridDim.x-th
#endif
#ifndef FPX_QS_STAGGER
#define FPX_QS_STAGGER 1           // delays of 3.4 us between the start of a CU's workgroups (0: none)
#endif
constexpr uint32_t QS_STAGGER = FPX_QS_STAGGER;
#ifndef FPX_QS_WGS_PER_CU
#define FPX_QS_WGS_PER_CU 4
#endif
constexpr uint32_t QS_WGS_PER_CU = FPX_QS_WGS_PER_CU;       // workgroups a CU holds (its 160 KB of LDS, 128 registers per lane): the kernel's grid is that many per CU
// [records + a sink word | filter | exact table (before: the task queue) | candidate buffer]
constexpr size_t QS_LDS_BYTES = ((size_t)QS_REC_CAP + 4u) * 4u + ((size_t)2u << QS_FLOG2) + ((size_t)8u << QS_TLOG2) + (size_t)SB_CAND * 8u;

struct QSearchArgs {
    const uint32_t* hashes_base; const uint64_t* offsets;      // hashes_base[i]: the hash at ABSOLUTE position i of the batch; offsets[q] absolute
    const uint32_t* opts;                                      // [B][4]: max_results, floor, pct, raw length
    uint32_t q_begin, q_end, sb;                               // the launch's queries [q_begin, q_end) of the batch; sb: bits of the score field in a candidate key
    // Members in ONE LINE of a union share storage: a kernel that has no use for a member carries something of its own there under its
    // own name, and the struct -- with it every other kernel's argument offsets, which qs_cold_args() reads by -- stays as it is.
    //   SHARE (k_search_window, k_search_packed: no candidates, no slots, no redo list): bins, bin_cap, bin_fill, bin_rec32; qcand is null
    //   COOP (k_search_filt, k_search_low_coop: no redo list -- hot_wg is unfiltered-only, and LOW has none): dead_union, dead_union_last
    union { uint64_t* cands; uint64_t* bins; };                // the shared candidate list (queries with more candidates than slots) | the step's bins: [bin][bin_cap] records of 4 or 8 bytes
    union { uint64_t cand_cap; uint64_t bin_cap; };            // its capacity | a bin's capacity in RECORDS
    uint64_t* qcand;                                           // the queries' own candidate slots ...
    union { uint32_t* qcand_n; uint32_t* bin_fill; };          // ... and their counts | the bins' fill counters (BIN_STRIDE words apart)
    unsigned long long* counters;
    unsigned long long* stat_sets;                             // [LEAN_STAT_SETS][8] statistics + [LEAN_STAT_SETS][HIST_SLOTS] histogram slots
    unsigned long long* qstats;                                // [B] blocks | docs << 32, or null
    const uint32_t* cancel;
    // a live index's memory segments: their ONE hash-sorted table of live postings (fpx_probe_small.hpp: k_probe_memtab), or null
    const uint64_t* mem_tab; const uint32_t* mem_bucket; const uint32_t* mem_bits;
    // the launch's queue of queries: a workgroup's first two are blockIdx.x and blockIdx.x + gridDim.x, the others q_begin + 2 gridDim.x + (what
    // this counter hands out) -- or null: every gridDim.x-th
    unsigned int* next_q;
    uint32_t stagger;                                          // delays of 3.4 us between the start of a CU's workgroups (0: none)
    // (option hot_wg = 1, unfiltered) the batch's redo list, or null: a query whose records outgrow the LDS array is named here --
    // q | its record total << 32, through CTR_REDO -- for k_search_classes instead of failing the batch (redo_cap: entries the list takes)
    // | the group's union dead-set bitmap of the snapshot (32-bit words, bit doc - gmin; Snapshot::dead_union), or null: no column has a dead set
    union { unsigned long long* redo; const uint32_t* dead_union; };
    // | 1: 4-byte records (bin_record32), 0: 8-byte ones | the number of the bitmap's LAST word (a word beyond it is not read)
    union { uint32_t redo_cap; uint32_t bin_rec32; uint32_t dead_union_last; };
};

// The kernel's arguments as its two by-value parameters lay them out in the kernel-argument segment.  Most of them are needed once per
// query, at its head or tail; held in scalar registers for the whole kernel they crowded out the rounds' own scalars (90 spilled into lanes
// of eight vector registers, which in turn spilled to scratch).  Those are read where they are used: qs_cold_args() is the segment's
// address behind a barrier to hoisting, so that a load through it stays at its use and costs no register elsewhere.
struct QSKernargs { QSearchArgs a; GroupArgs ga; };
static_assert(sizeof(QSearchArgs) == 160 && offsetof(QSearchArgs, cands) == 40 && offsetof(QSearchArgs, qcand_n) == 64 && offsetof(QSearchArgs, next_q) == 128 &&
              offsetof(QSearchArgs, redo) == 144 && offsetof(QSearchArgs, redo_cap) == 152, "QSearchArgs' layout is the kernels' argument segment: a member is renamed or shared, never moved");
typedef const __attribute__((address_space(4))) QSKernargs* qs_kargs_t;
__device__ __forceinline__ qs_kargs_t qs_cold_args()
{
    qs_kargs_t p = (qs_kargs_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

#define FPX_QS_OCC __attribute__((amdgpu_waves_per_eu(FPX_QS_WAVES)))
#define FPX_LDS __attribute__((address_space(3)))
typedef uint32_t u32x3_t __attribute__((ext_vector_type(3)));
__device__ __forceinline__ uint3 gload_u3(const uint32_t* p)            // the first three words of a line (16-byte aligned)
{
    const u32x3_t v = *(const FPX_GLOBAL u32x3_t*)p;
    return make_uint3(v.x, v.y, v.z);
}
__device__ __forceinline__ uint32_t qs_cell(uint32_t doc) { return (doc ^ (doc >> QS_FLOG2)) & ((1u << QS_FLOG2) - 1u); }
// a deferred task: the address of a list, or of up to eight words of a hash that its lane did not walk (beyond its own, or overflowed from
// the line into `ext`) -- bits 0..45: address >> 2, 46..48: words - 1, 49..56: which of them are second words of doubles, 57..62: the
// hash's chunk (a list reference among the words counts from the chunk's `ext`), 63: a list.  (FILT: a list's column in bits 46..49; a
// words task's columns -- word j in bits 4j .. 4j+3 -- in a parallel array behind the queue)
__device__ __forceinline__ unsigned long long qs_task_list(const uint32_t* p, uint32_t chunk)
{
    return ((unsigned long long)p >> 2) | ((unsigned long long)chunk << 57) | (1ull << 63);
}
__device__ __forceinline__ unsigned long long qs_task_words(const uint32_t* p, uint32_t cnt, uint32_t second, uint32_t chunk)
{
    return ((unsigned long long)p >> 2) | ((unsigned long long)(cnt - 1u) << 46) | ((unsigned long long)(second & 0xFFu) << 49) | ((unsigned long long)chunk << 57);
}
__device__ __forceinline__ const uint32_t* qs_task_ptr(unsigned long long e) { return reinterpret_cast<const uint32_t*>((e & ((1ull << 46) - 1ull)) << 2); }
// (FILT) the columns of words j0 .. j0 + cnt - 1 of a hash (cnt <= 8) -- its columns pm ascending, a double (dm) two words of one --, word
// j0 + t in bits 4t .. 4t+3
__device__ __forceinline__ uint32_t qs_word_cols(uint32_t pm, uint32_t dm, uint32_t j0, uint32_t cnt)
{
    uint32_t cols = 0, rest = pm, i = 0, w = 0;
    while (rest != 0u && w < j0 + cnt) {
        const uint32_t s = (uint32_t)__builtin_ctz(rest), span = 1u + ((dm >> i) & 1u);
        for (uint32_t t = 0; t < span; ++t, ++w) if (w >= j0 && w < j0 + cnt) cols |= s << (4u * (w - j0));
        ++i; rest &= rest - 1u;
    }
    return cols;
}

// ---- eight lanes to a line (the unfiltered rounds): lane l belongs to group l >> 3 and is its lane sub = l & 7.
// qs_group_bcast<K>: the value of lane K of every group, in all eight of its lanes (a swizzle on the LDS crossbar: and-mask 0x18 keeps the
// group, or-mask K names the lane; a wave half is 32 lanes, the pattern serves both).  qs_from_sub0<K> / qs_from_sub7<K>: lane K of every
// group gets the value of the group's lane 0 / lane 7 (a row shift on the DPP crossbar -- a row is two groups --; the other lanes get
// something they do not look at).  All three want the whole wave active.
template <uint32_t K> __device__ __forceinline__ uint32_t qs_group_bcast(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (int)((K << 5) | 0x18u));
}
template <uint32_t K> __device__ __forceinline__ uint32_t qs_from_sub0(uint32_t v)
{
    if constexpr (K == 0u) return v;
    else return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 | (int)K, 0xF, 0xF, true);          // row_shr:K
}
template <uint32_t K> __device__ __forceinline__ uint32_t qs_from_sub7(uint32_t v)
{
    if constexpr (K == 7u) return v;
    else return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x100 | (int)(7u - K), 0xF, 0xF, true);   // row_shl:7-K
}
template <uint32_t K> struct qs_idx { static constexpr uint32_t value = K; };
template <uint32_t K = 0, class F> __device__ __forceinline__ void qs_for8(F&& f)
{
    if constexpr (K < 8u) { f(qs_idx<K>{}); qs_for8<K + 1u>(f); }
}

// (FPX_QS_PROF: an experiment build -- wave 0 of every workgroup adds the clocks it spent between the kernel's phases to the batch's
// counters [16 ..], which the host prints; tools/build_variant.sh qs_prof -DFPX_QS_PROF=1)
#ifdef FPX_QS_PROF
#define QS_MARK(i) do { if (tid == 0) { const unsigned long long t_ = clock64(); atomicAdd(&qs_cold_args()->a.counters[CTR_HIST + (i)], t_ - t_prev); t_prev = t_; } } while (0)
// (finer marks inside a phase, slots [6 ..]: QS_SUB0 starts a stretch, QS_SUB(i) adds the clocks since the last of either to slot i; QS_ARRIVED
// makes every wave wait right there for the loads whose values it names -- the stretch behind it is that wait and nothing else.  The
// unfiltered rounds feed slots 7 and 10 only (a round has no heads-then-words stretch: slots 8 and 9 stay zero).  The waits
// and the marks' own atomics stretch a query by half: the finer clocks compare builds, they are not shares of the product's time)
#define QS_SUB0() do { if (tid == 0) t_sub = clock64(); } while (0)
#define QS_SUB(i) do { if (tid == 0) { const unsigned long long t_ = clock64(); atomicAdd(&qs_cold_args()->a.counters[CTR_HIST + (i)], t_ - t_sub); t_sub = t_; } } while (0)
#define QS_ARRIVED2(x, y) asm volatile("" :: "v"(x), "v"(y))
#define QS_ARRIVED4(x) asm volatile("" :: "v"((x)[0]), "v"((x)[1]), "v"((x)[2]), "v"((x)[3]))
#else
#define QS_MARK(i) do { } while (0)
#define QS_SUB0() do { } while (0)
#define QS_SUB(i) do { } while (0)
#define QS_ARRIVED2(x, y) do { } while (0)
#define QS_ARRIVED4(x) do { } while (0)
#endif
constexpr uint32_t QS_MAX_CLASSES = 32;           // (CLS) doc classes a redone query is searched in at most
constexpr uint32_t QS_LIST_AHEAD = 8;             // (CLS) loads of 64 docs of a long list that a wave has under way at once
// a record's doc class: bits of the doc's hash that neither the exact table's slot (h2 & TMASK) nor its pass selector ((h2 >> 16) % passes,
// passes <= 64) looks at -- and qs_cell takes the doc's own bits, not its hash's --, so a class fills the filter and the table evenly
__device__ __forceinline__ uint32_t qs_class(uint32_t rec) { return mix32(rec) >> 27; }
static_assert(QS_MAX_CLASSES == 32u, "qs_class gives five bits");
constexpr uint32_t QS_LOW_CHUNK = 8;              // (LOW) records a lane sorts in registers (two 16-byte pieces): the network's strides below it cost no barrier
constexpr uint32_t QS_SHARE_BQ = 3;               // (SHARE) queries per bin: fpx_search.hip's SHARD_BQ
constexpr uint32_t QS_SHARE_STRIDE = 32;          // (SHARE) 32-bit words between the bins' fill counters: fpx_partition.hpp's BIN_STRIDE
constexpr uint32_t QS_PACK_MAX = 4u * QS_WG;      // (PACK) longest query taken: what hq[] holds.  A longer one hands the step back (CTR_BINFAIL 1)

// A kernel of the family, NAMED: what every one has a value for (NS, QS, MEM, FILT), and the forms that are on (the head comment's table).
// Which forms go together is this type's business: an illegal combination fails where it is written.
enum : uint32_t { QS_F_CLS = 1u, QS_F_LOW = 2u, QS_F_NEXT = 4u, QS_F_SHARE = 8u, QS_F_PACK = 16u, QS_F_COOP = 32u };
template <int NS_, bool QS_, bool MEM_, bool FILT_, uint32_t FORM = 0u>
struct qs_variant {
    static constexpr int NS = NS_;
    static constexpr bool QS = QS_, MEM = MEM_, FILT = FILT_;
    static constexpr bool CLS = (FORM & QS_F_CLS) != 0u, LOW = (FORM & QS_F_LOW) != 0u, NEXT = (FORM & QS_F_NEXT) != 0u;
    static constexpr bool SHARE = (FORM & QS_F_SHARE) != 0u, PACK = (FORM & QS_F_PACK) != 0u, COOP = (FORM & QS_F_COOP) != 0u;
    static_assert(NS == 8 || NS == 16, "columns of a line");
    static_assert(!COOP || (FILT && !CLS && !NEXT && !SHARE), "the filtered walk eight lanes to a line: k_search_filt, and with the sorted tail k_search_low_coop");
    static_assert(!SHARE || (!QS && !CLS && !LOW && !NEXT), "a window's walk for the bin protocol: no per-query statistics, no doc classes, no sorted tail, one group");
    static_assert(!PACK || SHARE, "packed probes: a window's walk only (without a window nearly every hash is a probe)");
    static_assert(!PACK || 2u * QS_PACK_MAX <= QS_REC_CAP, "the packed list and its memory-table bits live at the record array's bottom");
    static_assert(!NEXT || (!CLS && !MEM), "a later group's walk: no doc classes, no memory table (they ride on the first group's launch)");
    static_assert(!(CLS && FILT), "doc classes: the unfiltered walk only");
    static_assert(!LOW || (!CLS && QS_WG == 256u && QS_REC_CAP >= 512u && (QS_REC_CAP & (QS_REC_CAP - 1u)) == 0u),
                  "low floors: no doc classes; the sorted tail's scans are written for 256 lanes and a power-of-two array");
};

template <class V>
__device__ __forceinline__ void qs_body(const QSearchArgs& a, const GroupArgs& ga)
{
    constexpr int NS = V::NS;
    constexpr bool QS = V::QS, MEM = V::MEM, FILT = V::FILT, CLS = V::CLS, LOW = V::LOW, NEXT = V::NEXT, SHARE = V::SHARE, PACK = V::PACK, COOP = V::COOP;
#ifdef FPX_QS_PROF
    unsigned long long t_prev = clock64(), t_sub = 0;
#endif
    constexpr uint32_t HVL = NS == 16 ? 2u : 3u;        // log2 of the hash values per line
    constexpr uint32_t T = 1u << QS_TLOG2, TMASK = T - 1u;
    extern __shared__ __align__(16) uint8_t qs_dyn[];
    uint32_t* const recs = reinterpret_cast<uint32_t*>(qs_dyn);                                         // [QS_REC_CAP] docs (+ a sink); before: the query's hash set
    uint32_t* const filter = recs + QS_REC_CAP + 4u;                                                    // 2^(QS_FLOG2 - 1) words of two cells
    unsigned long long* const table = reinterpret_cast<unsigned long long*>(filter + (1u << (QS_FLOG2 - 1u)));
    unsigned long long* const tasks = reinterpret_cast<unsigned long long*>(filter);                   // (until the records are complete)
    constexpr uint32_t TCAP = FILT ? QS_TASKS_FILT : QS_TASKS;                                          // tasks the queue holds
    uint32_t* const tcols = reinterpret_cast<uint32_t*>(tasks + QS_TASKS_FILT);                         // (FILT) [TCAP] a words task's columns
    uint64_t* const cbuf = reinterpret_cast<uint64_t*>(table + T);                                      // [SB_CAND]
    __shared__ uint32_t s_count, s_ntask, s_over_recs, s_seen_ones, s_cancel, s_claimed, s_full, s_ccnt, s_cshared, s_cbase_lo, s_cbase_hi;
    __shared__ unsigned long long wg_blocks, wg_docs, wg_probes, wg_reads;
    __shared__ uint32_t wg_h[HIST_SLOTS];
    __shared__ uint32_t s_first[FUSE_MAX], s_last[FUSE_MAX];
    __shared__ const uint32_t* s_ext[GROUP_CHUNKS];
    __shared__ uint32_t s_q2;                           // the query after the next one (handed out by the launch's counter)
    __shared__ uint32_t s_dseg[FUSE_MAX];               // (FILT) a column's descriptor in ga.segs where it has superseded docs, else ~0

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const GroupDesc* g = &ga.g;
    // The workgroup STAYS: it takes query blockIdx.x, then blockIdx.x + gridDim.x, then what the launch's counter hands out (the host launches as
    // many workgroups as the chip holds at once; a workgroup that starts late -- behind another batch's kernel -- or draws long queries takes fewer).
    // What a query's start waits for -- its offsets, then its hashes: two latencies in a row, the second one HBM's -- is asked for while
    // the queries before it are at work: the offsets of the query after the next one as soon as the counter has named it (under this query's
    // counting), the next query's hashes -- the first four rounds' at once -- under this query's tasks and counting.
    // (CLS: [q_begin, q_end) are ENTRIES of the redo list -- q | record total << 32 --, a workgroup takes every gridDim.x-th: no queue, no
    // stagger and nothing asked for a query ahead, this is the rare path)
    uint32_t ent = a.q_begin + blockIdx.x;
    uint32_t q = ent, q_recs = 0u;
    // (CLS) the query's doc classes: the smallest power of two C with (its record total) / C <= QS_REC_CAP / 2 -- the factor of 2 is
    // room for unequal classes --, known as soon as the entry is read
    uint32_t ncls = 1u;
    // (an entry is one word for the whole workgroup, read by a vector load -- the list is written by the kernel before --: named uniform,
    // so that the query's number, length and classes stay in scalar registers as k_search_query's do)
    auto take_entry = [&]() {
        const unsigned long long e = qs_cold_args()->a.redo[ent];
        q = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)e); q_recs = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(e >> 32));
        ncls = 1u;
        while ((unsigned long long)ncls * (QS_REC_CAP / 2u) < (unsigned long long)q_recs) ncls *= 2u;
    };
    if constexpr (CLS) take_entry();
    (void)q_recs;
    uint32_t qn = q + gridDim.x;                        // the query after this one ...
    uint32_t n, nn = 0u;
    uint64_t nq_lo = 0;                                 // ... and where its hashes are (nn of them)
    const uint32_t* qh;
    if constexpr (CLS) {
        const uint64_t q_lo = a.offsets[q];
        n = (uint32_t)(a.offsets[q + 1] - q_lo);
        qh = a.hashes_base + q_lo;
        qn = 0xFFFFFFFFu;
    } else {
        const uint64_t q_lo = a.offsets[q];
        n = (uint32_t)(a.offsets[q + 1] - q_lo);
        qh = a.hashes_base + q_lo;
        if (qn < a.q_end) { nq_lo = a.offsets[qn]; nn = (uint32_t)(a.offsets[qn + 1] - nq_lo); }
    }
    {
        const qs_kargs_t ka = qs_cold_args();
        if (tid < FUSE_MAX) { s_first[tid] = ka->ga.g.first_hash[tid]; s_last[tid] = ka->ga.g.last_hash[tid]; }
        if (tid < GROUP_CHUNKS) s_ext[tid] = tid < ka->ga.g.nchunks ? ka->ga.g.ext_tab[tid] : nullptr;
        if (FILT && tid < FUSE_MAX) s_dseg[tid] = ka->ga.g.has_dead[tid] != 0u ? ka->ga.g.seg_index[tid] : 0xFFFFFFFFu;
    }
    // (records are docs - gmin inside the workgroup -- what the line's words hold --; gmin is added once per candidate at hand-over.  Only the
    // supersession test (FILT) and the memory segments' absolute docs (MEM) need it before that)
    const uint32_t gmin = (FILT || MEM) ? g->gmin : 0u;
    (void)gmin;
    // ---- a query's hashes are read ONCE, into registers, before the query starts: hq[] holds the lane's hashes of two pairs of rounds --
    //      the whole query up to 1024 hashes.  Dedup reads them there and so do the rounds (nobody else has touched those lines of the
    //      batch's hash array: read where they are needed they are a miss in HBM with the whole workgroup waiting, then a trip to the L2
    //      again in front of the second pair's heads).  A longer query's later pairs follow a pair ahead: in dedup into nx[] while the pair
    //      before is inserted, in the rounds into hq[2..3] while hq[0..1] are probed -- the window rolls (static indices: no scratch).
    //      The heads of a pair's lines (position bits, double flags) are asked for at the top of its rounds, after dedup, both at once: a
    //      duplicate's line and a hash outside the window are not fetched at all.
    uint32_t hq[2u * QS_CH];
    uint3 hd[QS_CH];                                    // (FILT: the per-lane walk's line heads; issue_heads, words_of and probe below are that walk)
    auto line_of = [&](uint32_t h) -> const uint32_t* { return g->lines + (size_t)((h >> HVL) - g->line0) * GROUP_LINE_WORDS; };
    // (the lane's hashes of pair c of a query of n_ hashes at qh_)
    auto load_pair = [&](const uint32_t* qh_, uint32_t n_, uint32_t c, uint32_t& h0, uint32_t& h1) {
        // ((COOP) the lane's number is taken afresh: held across the kernel, tid + 512 and tid + 768 -- the second pair's places -- were the
        // registers k_search_filt<16, ..> did not have, and went to scratch)
        uint32_t t = tid;
        if constexpr (COOP) asm volatile("" : "+v"(t));
        const uint32_t i = c * QS_CH * QS_WG + t;
        h0 = i < n_ ? gload_u32(qh_ + i) : 0u;
        h1 = i + QS_WG < n_ ? gload_u32(qh_ + i + QS_WG) : 0u;
    };
    // (of the pair in hq[0..1]; v0, v1: which of the two are probes.  A lane without a probe reads the group's first line, which nobody
    // looks at -- one address per wave, a hit in the L2 --: a load under a branch comes with its unpacking and the wait for it inside the
    // branch, and the pair's two trips to HBM would follow one another)
    auto issue_heads = [&](bool v0, bool v1) {
        hd[0] = gload_u3(v0 ? line_of(hq[0]) : g->lines);
        hd[1] = gload_u3(v1 ? line_of(hq[1]) : g->lines);
    };
    load_pair(qh, n, 0u, hq[0], hq[1]);
    load_pair(qh, n, 1u, hq[2], hq[3]);
    // (the cancel flag as lane 0 sees it, asked for a query ahead like the rest: cancel_requested() in two halves)
    uint32_t c_host = 0u;
    unsigned long long c_dev = 0ull;
    auto ask_cancel = [&]() {
        const qs_kargs_t ka = qs_cold_args();
        const uint32_t* const cancel = ka->a.cancel;
        if (tid == 0u && cancel != nullptr) {
            if ((blockIdx.x & 63u) == 0u) c_host = __hip_atomic_load(cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            c_dev = __hip_atomic_load(&ka->a.counters[CTR_CANCEL], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    ask_cancel();
  // Queries of one length keep a CU's four workgroups in LOCKSTEP -- all four in their rounds (the memory system's turn), then all four counting
  // (the LDS's and the VALU's) --: the workgroups of the chip's second, third and fourth wave of residents start a few microseconds apart
  // (s_sleep 127 = 3.4 us, `slot` times).  Measured, one batch of 8192 x 1000 in flight: 0.445 -> 0.430 ms (0.426 with twice the delay, 0.431 with four
  // times: the last workgroups' late start is the batch's tail).  Three batches in flight desynchronise one another -- a kernel's workgroups
  // start as the one before lets go of the CUs, one by one, PROVIDED its workgroups end one by one: with the queries handed out by a counter
  // they end together and the next kernel starts in lockstep again (0.412 -> 0.43 ms per batch, and jittery).  So the host asks for both -- the
  // counter and the delays -- only for a batch that finds the device to itself (run_batch: Ctx::qs_running).
  // Only where a workgroup has four or more queries ahead of it: a small batch is one query's latency.
  if (const uint32_t stagger = qs_cold_args()->a.stagger; !CLS && stagger != 0u && a.q_end - a.q_begin >= 4u * gridDim.x)
      for (uint32_t i = 0; i < ((blockIdx.x >> 8) & 3u) * stagger; ++i) __builtin_amdgcn_s_sleep(127);
  for (;;) {
    if constexpr (CLS) {
        // (uniform, before the query's first barrier) more classes than a query gets: the batch goes the long way.  The workgroup's other
        // entries are left undone with it -- the host hands the whole batch to the pipeline on CTR_BINFAIL
        if (ncls > QS_MAX_CLASSES) {
            if (tid == 0) atomicMax(&qs_cold_args()->a.counters[CTR_BINFAIL], 1ull);
            return;
        }
    }
    if constexpr (PACK) {
        // (uniform, before the query's first barrier) a query that hq[] does not hold whole is not this kernel's: the host keeps such a
        // batch on k_search_window -- a wrong launch hands the step back, as a query over the record array does, and stores nothing
        if (n > QS_PACK_MAX) {
            if (tid == 0) atomicMax(&qs_cold_args()->a.counters[CTR_BINFAIL], 1ull);
            return;
        }
    }
    const uint32_t rounds = (n + QS_WG - 1u) / QS_WG, nchunks = (rounds + QS_CH - 1u) / QS_CH;
    // the query's hash set: 2^sbits >= 2 n slots
    uint32_t sbits = 8u;
    while ((1u << sbits) < 2u * n) ++sbits;
    if (tid < HIST_SLOTS) wg_h[tid] = 0u;
    for (uint32_t i = tid; i < (1u << sbits); i += QS_WG) recs[i] = 0xFFFFFFFFu;
    if (tid == 0) {
        s_count = 0u; s_ntask = 0u; s_over_recs = 0u; s_seen_ones = 0u; s_ccnt = 0u; s_cshared = 0u;
        if constexpr (PACK) s_claimed = 0u;               // (the counting passes' word, idle under SHARE: the packed probes' count)
        wg_blocks = 0; wg_docs = 0; wg_probes = 0; wg_reads = 0;
        // cancel point (src/FileSegment.zig:144), once per query, before its first probe: what ask_cancel() read
        if (c_host != 0u) { atomicExch(&qs_cold_args()->a.counters[CTR_CANCEL], 1ull); c_dev = 1ull; }
        s_cancel = c_dev != 0ull ? 1u : 0u;
    }
    __syncthreads();
    if (s_cancel) return;
    QS_MARK(0);
    // ---- dedupSorted (src/Index.zig:171-172,489-499): the first occurrence of a hash is the probe, later ones are dropped.  A lane notes
    //      which of its rounds' hashes are probes (a hash-window slice of the group leaves the other hashes to another rank)
    uint32_t vmask = 0u;
    uint32_t mmask = 0u;                                // (MEM) ... and which of them the memory segments' table may hold: a bit per 256 hash values
    uint32_t nx[QS_CH] = {0u, 0u};                      // (a query of more than 1024 hashes: the pair after the one being inserted)
    for (uint32_t c = 0; c < nchunks; ++c) {
        uint32_t hc[QS_CH];
        uint32_t mb[QS_CH];
#pragma unroll
        for (uint32_t u = 0; u < QS_CH; ++u) hc[u] = c == 0u ? hq[u] : c == 1u ? hq[QS_CH + u] : nx[u];       // (uniform)
        if (c != 0u) { QS_SUB0(); QS_ARRIVED2(hc[0], hc[1]); QS_SUB(6); }
        if (c != 0u && c + 1u < nchunks) load_pair(qh, n, c + 1u, nx[0], nx[1]);
        if constexpr (MEM) {                            // (their bit words travel under the set's compare-and-swaps)
#pragma unroll
            for (uint32_t u = 0; u < QS_CH; ++u) {
                const uint32_t i = (c * QS_CH + u) * QS_WG + tid;
                mb[u] = (i < n && a.mem_bits != nullptr) ? gload_u32(a.mem_bits + ((hc[u] >> MEMTAB_FILTER_SHIFT) >> 5)) : 0xFFFFFFFFu;
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < QS_CH; ++u) {
            const uint32_t i = (c * QS_CH + u) * QS_WG + tid;
            if (i >= n) continue;
            const uint32_t h = hc[u];
            // (PACK) the window FIRST: another rank's hash makes no atomic and takes no slot (a duplicate of a hash of the window is in the window)
            if constexpr (PACK) { if (h < g->win_lo || h > g->win_hi) continue; }
            bool dup;
            if (h == 0xFFFFFFFFu) dup = atomicExch(&s_seen_ones, 1u) != 0u;     // (the set's empty mark is kept apart)
            else {
                uint32_t slot = (h * 0x9E3779B1u) >> (32u - sbits);
                for (;;) {
                    const uint32_t old = atomicCAS(&recs[slot], 0xFFFFFFFFu, h);
                    if (old == 0xFFFFFFFFu) { dup = false; break; }
                    if (old == h) { dup = true; break; }
                    slot = (slot + 1u) & ((1u << sbits) - 1u);
                }
            }
            if (!dup && h >= g->win_lo && h <= g->win_hi) {
                vmask |= 1u << (c * QS_CH + u);
                if constexpr (MEM) mmask |= ((mb[u] >> ((h >> MEMTAB_FILTER_SHIFT) & 31u)) & 1u) << (c * QS_CH + u);
            }
        }
    }
    (void)mmask;
    __syncthreads();                                    // (the set is done with: its slots are the record array now)
    // ---- (PACK) the window's probes get DENSE places: one scan per wave on the DPP crossbar and one LDS atomic per wave (the order is
    //      free: the bins are compared as sets), the hash to a list at the bottom of the record array -- free until the first round --,
    //      (MEM) its memory-table bit to a second list behind it; then every lane takes its hashes of the up to four rounds back into
    //      hq[0..3].  What indexed by the hash's RAW position -- vmask, mmask -- is remade for the packed one.
    // (`cnt` places per lane out of `counter`, one reservation per wave: the records' below, and the packed probes')
    auto reserve_in = [&](uint32_t* counter, uint32_t cnt) -> uint32_t {
        const uint32_t incl = scan16(cnt);
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)incl, 15), r1 = (uint32_t)__builtin_amdgcn_readlane((int)incl, 31),
                       r2 = (uint32_t)__builtin_amdgcn_readlane((int)incl, 47), r3 = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t total = r0 + r1 + r2 + r3;
        uint32_t wbase = 0;
        if (total != 0u) {                                                       // (wave-uniform)
            if (lane == 0u) wbase = atomicAdd(counter, total);
            wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)wbase);
        }
        const uint32_t row = lane >> 4;
        return wbase + (row >= 1u ? r0 : 0u) + (row >= 2u ? r1 : 0u) + (row >= 3u ? r2 : 0u) + (incl - cnt);
    };
    uint32_t prounds = rounds, pnchunks = nchunks;      // the rounds that are walked
    if constexpr (PACK) {
        uint32_t at = reserve_in(&s_claimed, (uint32_t)__popc(vmask));      // (< m <= n <= QS_PACK_MAX)
#pragma unroll
        for (uint32_t r = 0; r < 2u * QS_CH; ++r)
            if (((vmask >> r) & 1u) != 0u) {
                recs[at] = hq[r];
                if constexpr (MEM) recs[QS_PACK_MAX + at] = (mmask >> r) & 1u;
                ++at;
            }
        __syncthreads();                                // (the list is whole)
        const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_claimed);
        vmask = 0u; mmask = 0u;
#pragma unroll
        for (uint32_t r = 0; r < 2u * QS_CH; ++r) {
            const uint32_t i = r * QS_WG + tid;
            const bool has = i < m;
            hq[r] = has ? recs[i] : 0u;
            vmask |= (has ? 1u : 0u) << r;
            if constexpr (MEM) mmask |= (has ? recs[QS_PACK_MAX + i] : 0u) << r;
        }
        prounds = (m + QS_WG - 1u) / QS_WG; pnchunks = (prounds + QS_CH - 1u) / QS_CH;
        __syncthreads();                                // (everybody has its hashes: the array takes records now)
    }
    QS_MARK(1);

    // ---- (CLS) pass `cls` of the query's ncls classes walks the query again and keeps the records of that class only: a doc's postings
    //      are all in one class, so a pass's counts are exact and the passes' candidates are disjoint.  The hash set above is built once.
    const uint32_t cmask = ncls - 1u;
    (void)cmask;
    const bool has_next = qn < a.q_end;                      // (uniform; CLS: never -- qn names no query)
    // (what the tail learns about the query after the next one, for the hand-over behind the passes)
    uint32_t q2 = 0u;
    bool has_q2 = false;
    uint64_t o2_lo = 0;
    uint32_t o2_hi = 0u;                                    // (the low word of its end: a query is shorter than 2^32 hashes)
  for (uint32_t cls = 0; cls < ncls; ++cls) {
    if constexpr (CLS) {
        if (cls != 0u) {
            __syncthreads();                            // (the pass before has read its records, its table and its flags)
            if (tid == 0) { s_count = 0u; s_ntask = 0u; }
            load_pair(qh, n, 0u, hq[0], hq[1]);         // (the rounds' first pair again: the pass before left its last one there)
            __syncthreads();
        }
    }
    // (a record of this pass: every emission site asks -- the rounds' words, the tasks' words and lists, the wave-walked lists, the memory table)
    auto in_class = [&](uint32_t rec) -> bool { return (qs_class(rec) & cmask) == cls; };
    (void)in_class;
    const uint32_t active = g->active, nactive = (uint32_t)__popc(active);
    uint32_t my_blocks = 0, my_docs = 0, my_probes = 0, my_reads = 0;
    // (FILT) a doc of column s that a newer segment supersedes (src/common.zig:158; the column's dead set, k_probe_pgroup's test)
    auto dead_in = [&](uint32_t s, uint32_t doc) -> bool {
        const uint32_t di = s_dseg[s];
        return di != 0xFFFFFFFFu && is_dead_seg(ga.segs[di], doc);
    };
    // (COOP) the group's UNION dead-set bitmap of this snapshot -- bit doc - gmin: some column's dead set holds the doc --, words 0 .. ub_last,
    // or null: no column has a dead set (QSearchArgs::dead_union / dead_union_last).  A doc whose bit is
    // clear is live whatever its column; one whose bit is set asks its own column's set (dead_in)
    const uint32_t* ub = nullptr;
    uint32_t ub_last = 0u;
    if constexpr (COOP) { ub = a.dead_union; ub_last = a.dead_union_last; }
    auto union_hit = [&](uint32_t rel) -> bool {            // (rel: doc - gmin, what a word holds)
        const uint32_t i = rel >> 5;
        return ub != nullptr && i <= ub_last && ((gload_u32(ub + i) >> (rel & 31u)) & 1u) != 0u;
    };
    (void)ub; (void)ub_last; (void)union_hit;
    // ---- records.  `n` docs of the lane (mask km over d[]) join the query's array: one reservation per wave -- a scan on the DPP
    //      crossbar: the whole wave is here (fpx_pgroup.hpp x5) --, doc j at pos + (docs of the lane before it).  No branch and no select
    //      per slot: the slots are stored from the LAST down, a slot without a doc to where the nearest doc BELOW it goes -- a place of the
    //      lane's own that the doc itself, stored later, overwrites (a lane's stores to LDS keep their order); one with no doc below it, and
    //      every slot of a lane without docs, to the sink word behind the array.  The filter is counted later, over the array (every lane busy).
    // (a round reserves its records and its tasks with ONE scan: the two counts side by side in a word -- a wave has at most 64 x 32
    // records and far fewer than 2^16 tasks --, an atomic per counter)
    auto reserve_both = [&](uint32_t cnt, uint32_t nt, uint32_t& tat) -> uint32_t {
        const uint32_t both = cnt | (nt << 16);
        const uint32_t incl = scan16(both);
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)incl, 15), r1 = (uint32_t)__builtin_amdgcn_readlane((int)incl, 31),
                       r2 = (uint32_t)__builtin_amdgcn_readlane((int)incl, 47), r3 = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t total = r0 + r1 + r2 + r3;
        uint32_t rbase = 0, tbase = 0;
        if ((total & 0xFFFFu) != 0u) {                                           // (wave-uniform)
            if (lane == 0u) rbase = atomicAdd(&s_count, total & 0xFFFFu);
            rbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)rbase);
        }
        if ((total >> 16) != 0u) {
            if (lane == 0u) tbase = atomicAdd(&s_ntask, total >> 16);
            tbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)tbase);
        }
        const uint32_t row = lane >> 4;
        const uint32_t before = (row >= 1u ? r0 : 0u) + (row >= 2u ? r1 : 0u) + (row >= 3u ? r2 : 0u) + (incl - both);
        tat = tbase + (before >> 16);
        return rbase + (before & 0xFFFFu);
    };
    auto emit_at = [&](uint32_t km, const auto& d, uint32_t cnt, uint32_t pos) {            // (km: bits 0 .. N-1 only; cnt of them, from pos)
        constexpr uint32_t N = sizeof(d) / sizeof(uint32_t);
        if (cnt != 0u && pos + cnt > QS_REC_CAP) { s_over_recs = 1u; km = 0u; cnt = 0u; }      // (more records than the array takes: the batch goes the long way)
        const uint32_t first = cnt != 0u ? pos : QS_REC_CAP, sink = QS_REC_CAP - first;
        // (the lane's base in LDS -- the array's address and `first` -- is made ONCE, as a 32-bit LDS address in a vector register: a
        // slot's address is then one shift-and-add of it (v_lshl_add_u32) where the array's scalar base, the shifted index and the
        // shifted `first` cost a shift and a three-operand add per slot.  (CLS keeps the generic form: with the memory table's
        // registers its sixteen-column rounds are at the 128 a lane has, and the base held across the stores spilled one)
        auto last_of = [&](uint32_t j) -> uint32_t { return (uint32_t)__popc(km & ((2u << j) - 1u)) - 1u; };      // the last doc up to slot j among the lane's (none: 0xFFFFFFFF)
        if constexpr (CLS) {
#pragma unroll
            for (uint32_t j = N; j-- != 0u;) recs[first + min(last_of(j), sink)] = d[j];
        } else {
            FPX_LDS uint32_t* const base = (FPX_LDS uint32_t*)(recs + first);
#pragma unroll
            for (uint32_t j = N; j-- != 0u;) base[min(last_of(j), sink)] = d[j];
        }
    };
    auto emit = [&](uint32_t km, const auto& d) {
        const uint32_t cnt = (uint32_t)__popc(km);
        emit_at(km, d, cnt, reserve_in(&s_count, cnt));
    };
    // (one record of some lanes of the wave: the wave's turns, long lists)
    auto emit1 = [&](bool kp, uint32_t doc) {
        if constexpr (CLS) kp = kp && in_class(doc);
        const unsigned long long m = __ballot((int)kp);
        if (m == 0ull) return;
        uint32_t base = 0;
        if (lane == (uint32_t)__builtin_ctzll(m)) base = atomicAdd(&s_count, (uint32_t)__popcll(m));
        base = __shfl(base, (int)__builtin_ctzll(m));
        if (kp) {
            const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (at < QS_REC_CAP) recs[at] = doc; else s_over_recs = 1u;
        }
    };
    // a task joins the queue (a full queue: the batch goes the long way)
    auto push_task = [&](unsigned long long e) {
        const uint32_t at = atomicAdd(&s_ntask, 1u);
        if (at < TCAP) tasks[at] = e; else s_over_recs = 1u;
    };

    // ---- FileSegment.search for every column, a hash per lane and round (fpx_pgroup.hpp: the line's layout)
    // (the words of a hash the lane walks itself -- up to QS_WORDS, as far as they are in the line -- asked for as soon as the line's head is
    // there: the line is still in the L2 then.  Asked for a few rounds later -- round 6's first form fetched all heads up front -- the line
    // had been evicted and was fetched from memory AGAIN: 2.27 requests per query hash, profiles/r06_bench.json)
    // (... and what the walk needs of the head's arithmetic, packed: start | mine << 7 | nwords << 11 | inl << 17, and pm | dm << 16)
    // (ov: where the hash's words run past the line's inline part, the offset of the rest in `ext` -- the line's last word -- travels
    // with the words: probe forms its overflow tasks' address from a register)
    auto words_of = [&](uint32_t h, uint3 head, bool valid, uint32_t (&gw)[QS_WORDS], uint32_t& hx, uint32_t& hy, uint32_t& ov) {
        const uint64_t bits = valid ? (((uint64_t)head.y << 32) | head.x) : 0ull;
        const uint32_t dfl = valid ? head.z : 0u;
        const uint32_t sh = (h & ((1u << HVL) - 1u)) * (uint32_t)NS;
        const uint32_t pm = (uint32_t)(bits >> sh) & ((1u << NS) - 1u);
        const uint32_t pos0 = (uint32_t)__popcll(bits & ((1ull << sh) - 1ull));
        const uint32_t k = (uint32_t)__popc(pm);
        const uint32_t dbl_before = pos0 >= 32u ? (uint32_t)__popc(dfl) : (uint32_t)__popc(dfl & ((1u << pos0) - 1u));
        const uint32_t dm = pos0 >= 32u ? 0u : ((dfl >> pos0) & ((1u << k) - 1u));
        const uint32_t nwords = k + (uint32_t)__popc(dm);
        const uint32_t n_line = (uint32_t)__popcll(bits) + (uint32_t)__popc(dfl);
        const uint32_t inl = n_line > GROUP_INLINE ? GROUP_INLINE - 1u : GROUP_INLINE;
        const uint32_t start = pos0 + dbl_before;
        const uint32_t mine = min(min(nwords, QS_WORDS), start < inl ? inl - start : 0u);
#pragma unroll
        for (uint32_t i = 0; i < QS_WORDS; ++i) gw[i] = 0xFFFFFFFFu;
        const uint32_t* lp = line_of(h) + 3u + start;
#pragma unroll
        for (uint32_t i = 0; i < QS_WORDS / 4; ++i) {
            if (mine > 4u * i) {
                const uint4 v = gload_u4_a4(lp + 4u * i);
                gw[4 * i] = v.x; gw[4 * i + 1] = v.y; gw[4 * i + 2] = v.z; gw[4 * i + 3] = v.w;
            }
        }
        ov = start + nwords > inl ? gload_u32(line_of(h) + (GROUP_LINE_WORDS - 1u)) : 0u;
        hx = start | (mine << 7) | (nwords << 11) | (inl << 17);          // (start <= 96, mine <= 12, nwords <= 32, inl <= 29)
        hy = pm | (dm << 16);
    };
    auto probe = [&](uint32_t h, uint32_t hx, uint32_t hy, bool valid, uint32_t (&gw)[QS_WORDS], uint32_t ov) {
        if (valid) { my_probes += nactive; my_reads += 2u; }
        const uint32_t pm = hy & 0xFFFFu, dm = hy >> 16;
        const uint32_t start = hx & 127u, mine = (hx >> 7) & 15u, nwords = (hx >> 11) & 63u, inl = (hx >> 17) & 31u;
        // (outside [first_hash, last_hash] the reference visits no block, src/FileSegment.zig:164,153)
        uint32_t inr = active;
        if (h < g->lo_all || h > g->hi_all) {          // (rare: the columns' bounds stay in LDS -- read through an index the compiler cannot
            inr = 0u;                                  // see through, or it keeps all 2 NS of them in registers across the rounds)
            uint32_t z = 0u;
            asm volatile("" : "+v"(z));
#pragma unroll
            for (uint32_t s = 0; s < NS; ++s) inr |= (h >= s_first[z + s] && h <= s_last[z + s]) ? (1u << s) : 0u;
        }
        if (!valid) inr = 0u;
        my_blocks += (uint32_t)__popc(inr & active & ~pm);         // absent: the reference visits one block, finds nothing and stops
        // second words of doubles: the t-th double, at position i, has its second word at i + t + 1
        uint32_t second = 0;
        for (uint32_t d = dm, t = 0; d != 0u; d &= d - 1u, ++t) second |= 1u << ((uint32_t)__builtin_ctz(d) + t + 1u);
        uint32_t negm = 0, gapm = 0;
#pragma unroll
        for (uint32_t j = 0; j < QS_WORDS; ++j) {
            const uint32_t word = gw[j];
            negm |= (word >> 31) << j;                                          // a gap position and a list reference have bit 31
            gapm |= (word == 0xFFFFFFFFu ? 1u : 0u) << j;
        }
        const uint32_t vm = (1u << mine) - 1u;
        uint32_t keep = vm & ~negm;                                             // the docs among the lane's words
        uint32_t lmask = vm & negm & ~gapm;                                     // its list references
        // (FILT) the walked words by their column (k_probe_pgroup's walk, a column's one or two words at a time): words of a column outside
        // the snapshot are nothing; dmask: the words whose column has superseded docs.  (A word's own column, where it is needed -- a
        // doc of such a column, a list reference --, is walked to again: no register holds the twelve)
        uint32_t dmask = 0;
        if constexpr (FILT) {
            uint32_t amask = 0;
            for (uint32_t r = pm, i = 0, w = 0; r != 0u && w < mine; r &= r - 1u, ++i) {
                const uint32_t s = (uint32_t)__builtin_ctz(r), span = 1u + ((dm >> i) & 1u), bits = ((1u << span) - 1u) << w;
                amask |= ((active >> s) & 1u) != 0u ? bits : 0u;
                dmask |= s_dseg[s] != 0xFFFFFFFFu ? bits : 0u;
                w += span;
            }
            keep &= amask; lmask &= amask;
        }
        my_docs += (uint32_t)__popc(keep);
        my_blocks += (uint32_t)__popc(keep & ~second);
        // (the scan histograms: a double is ONE observation of two docs, counted where its second word is -- the upper half of my_probes)
        if constexpr (SCAN_HIST && (FPX_SH_BITS & 2)) my_probes += (uint32_t)__popc(keep & second) << 16;
        if constexpr (FILT) {                                                   // (counted above: CTR_DOCS counts before supersession)
            for (uint32_t m = keep & dmask; m != 0u; m &= m - 1u) {
                const uint32_t j0 = (uint32_t)__builtin_ctz(m);
                uint32_t doc = 0;
#pragma unroll
                for (uint32_t j = 0; j < QS_WORDS; ++j) doc = j == j0 ? gw[j] : doc;
                if (dead_in(qs_word_cols(pm, dm, j0, 1u), gmin + doc)) keep &= ~(1u << j0);
            }
        }
        // ---- what the round does not wait for joins the query's task queue -- the hash's lists (their heads are other lines: HBM), its
        //      words beyond the lane's own and those that overflowed the line into `ext` --; the workgroup takes the tasks up together
        //      once its rounds are done
        // (their places in the queue: one reservation per wave, a scan on the DPP crossbar -- a lane's own atomic on the one counter is compiled
        // into a serial loop over the wave's lanes)
        const uint32_t in_line = (nwords != mine && start + mine < inl) ? min(nwords - mine, inl - (start + mine)) : 0u;
        const uint32_t in_ext = nwords - mine - in_line;
        const uint32_t nt = (uint32_t)__popc(lmask) + (in_line + QS_TASK_WORDS - 1u) / QS_TASK_WORDS + (in_ext + QS_TASK_WORDS - 1u) / QS_TASK_WORDS;
        uint32_t tat;
        const uint32_t nrec = (uint32_t)__popc(keep);
        emit_at(keep, gw, nrec, reserve_both(nrec, nt, tat));
        if (nt != 0u) {
            if (tat + nt > TCAP) { s_over_recs = 1u; tat = TCAP; }                // (a full queue: the batch goes the long way)
            auto put_task = [&](unsigned long long e) { if (tat < TCAP) tasks[tat] = e; ++tat; };
            auto put_words = [&](unsigned long long e, uint32_t j0, uint32_t c) {
                if constexpr (FILT) { if (tat < TCAP) tcols[tat] = qs_word_cols(pm, dm, j0, c); }
                put_task(e);
            };
            const uint32_t chunk = (h >> GROUP_CHUNK_LOG2) - g->chunk0;
            const uint32_t* ext = s_ext[chunk];
            uint32_t lm = lmask;
            while (lm != 0u) {
                const uint32_t j0 = (uint32_t)__builtin_ctz(lm);
                lm &= lm - 1u;
                uint32_t e = 0;
#pragma unroll
                for (uint32_t j = 0; j < QS_WORDS; ++j) e = j == j0 ? gw[j] : e;
                put_task(qs_task_list(ext + (e & 0x7FFFFFFFu), chunk) | (FILT ? ((unsigned long long)qs_word_cols(pm, dm, j0, 1u) << 46) : 0ull));
            }
            uint32_t j = mine;
            // ... words still in the line (the hash has more than the lane walks)
            while (j < mine + in_line) {
                const uint32_t c = min(mine + in_line - j, QS_TASK_WORDS);
                put_words(qs_task_words(line_of(h) + 3u + start + j, c, second >> j, chunk), j, c);
                j += c;
            }
            // ... and behind its end, in `ext` at the offset the line's last word holds (ov: words_of asked for it)
            if (j < nwords) {
                const uint32_t* ob = ext + ov;
                while (j < nwords) {                     // (start + j >= inl here)
                    const uint32_t c = min(nwords - j, QS_TASK_WORDS);
                    put_words(qs_task_words(ob + (start + j - inl), c, second >> j, chunk), j, c);
                    j += c;
                }
                my_reads += 2u;
            }
        }
    };

    // ---- the same for a snapshot that searches every column and has no superseded docs (!FILT): EIGHT LANES TO A LINE.  A round is still a
    //      hash per lane (h; valid: it is a probe), but a hash's line is fetched ONCE and WHOLE, by the eight lanes of its lane's group:
    //      load instruction k has every group read the line of the hash its lane k holds, lane `sub` words 4 sub .. 4 sub + 3 -- one
    //      access of the vector-memory front end per line where the per-lane walk made three (head, pieces, offset), and no second trip
    //      that depends on the first.  All 64 lines of the wave's round are under way at once, 32 registers per lane.
    //      Then: (1) every lane gets the head (lane 0's first three words) and the `ext` offset (lane 7's last) of ITS OWN hash's line and
    //      does the head's arithmetic and the per-hash statistics once, as the per-lane walk did; (2) the hash's words as a mask over
    //      the line's 32 words, and the second words among them, go back to the group, four lines at a time, and every lane takes its
    //      nibble of each: word w = 4 sub + t sits at position p = w - 3 and belongs to the hash iff start <= p < min(start + nwords, inl)
    //      -- worked out once, by the hash's lane, not by each of the eight for each line --; (3) ONE
    //      reservation per wave for the round's records and tasks, the records stored from the lane's 32 registers.  Every inline word
    //      is walked where it landed: only lists and words in `ext` are tasks.
    auto round_coop = [&](uint32_t h, bool valid) {
        const uint32_t sub = lane & 7u;
        uint32_t L[32];
        {
            // what is per HASH is made once, by its lane: the number of its line in the group -- 0 for a hash that is no probe: the
            // group's first line, one address, no HBM, no load under a branch --; a load is then that number from lane k, a shift and
            // an add to the lane's own base (the byte offset reaches 2^37: only the line's number travels in 32 bits)
            const uint32_t li = valid ? (h >> HVL) - g->line0 : 0u;
            const uint8_t* const lb = reinterpret_cast<const uint8_t*>(g->lines) + 16u * sub;
            uint32_t lk[8];
            qs_for8([&](auto kc) { constexpr uint32_t k = decltype(kc)::value; lk[k] = qs_group_bcast<k>(li); });
            // (the eight broadcasts are under way together, one wait for the crossbar: the registers they land in are the lines' own)
            asm volatile("" : "+v"(lk[0]), "+v"(lk[1]), "+v"(lk[2]), "+v"(lk[3]), "+v"(lk[4]), "+v"(lk[5]), "+v"(lk[6]), "+v"(lk[7]));
            qs_for8([&](auto kc) {
                constexpr uint32_t k = decltype(kc)::value;
                const uint4 v = gload_u4(lb + ((uint64_t)lk[k] * (GROUP_LINE_WORDS * 4u)));
                L[4 * k] = v.x; L[4 * k + 1] = v.y; L[4 * k + 2] = v.z; L[4 * k + 3] = v.w;
            });
        }
        // (all eight are under way before any is looked at)
        asm volatile("" : "+v"(L[0]), "+v"(L[1]), "+v"(L[2]), "+v"(L[3]), "+v"(L[4]), "+v"(L[5]), "+v"(L[6]), "+v"(L[7]),
                          "+v"(L[8]), "+v"(L[9]), "+v"(L[10]), "+v"(L[11]), "+v"(L[12]), "+v"(L[13]), "+v"(L[14]), "+v"(L[15]));
        asm volatile("" : "+v"(L[16]), "+v"(L[17]), "+v"(L[18]), "+v"(L[19]), "+v"(L[20]), "+v"(L[21]), "+v"(L[22]), "+v"(L[23]),
                          "+v"(L[24]), "+v"(L[25]), "+v"(L[26]), "+v"(L[27]), "+v"(L[28]), "+v"(L[29]), "+v"(L[30]), "+v"(L[31]));
        // (CLS) which of the lane's 32 words, read as docs, are of this pass's class: asked here, word by word, while little else is
        // live (thirty-two hashes side by side cost the registers the rounds do not have)
        uint32_t cm32 = CLS ? 0u : 0xFFFFFFFFu;
        if constexpr (CLS) {
#pragma unroll
            for (uint32_t j = 32u; j-- != 0u;) {
                cm32 = (cm32 << 1) | (in_class(L[j]) ? 1u : 0u);     // (from the last word down, a bit at a time: a mask per word would be a register per word)
                asm volatile("" : "+v"(cm32), "+v"(L[j]));
            }
        }
        // (1) the lane's own hash: its line is number `sub` of its group
        uint32_t hx = 0, hy = 0, hz = 0, ov = 0;
        qs_for8([&](auto kc) {
            constexpr uint32_t k = decltype(kc)::value;
            const uint32_t x = qs_from_sub0<k>(L[4 * k]), y = qs_from_sub0<k>(L[4 * k + 1]), z = qs_from_sub0<k>(L[4 * k + 2]), o = qs_from_sub7<k>(L[4 * k + 3]);
            const bool me = sub == k;
            hx = me ? x : hx; hy = me ? y : hy; hz = me ? z : hz; ov = me ? o : ov;
        });
        const uint64_t bits = valid ? (((uint64_t)hy << 32) | hx) : 0ull;
        const uint32_t dfl = valid ? hz : 0u;
        const uint32_t sh = (h & ((1u << HVL) - 1u)) * (uint32_t)NS;
        const uint32_t pm = (uint32_t)(bits >> sh) & ((1u << NS) - 1u);
        const uint32_t pos0 = (uint32_t)__popcll(bits & ((1ull << sh) - 1ull));
        const uint32_t kk = (uint32_t)__popc(pm);
        const uint32_t dbl_before = pos0 >= 32u ? (uint32_t)__popc(dfl) : (uint32_t)__popc(dfl & ((1u << pos0) - 1u));
        const uint32_t dm = pos0 >= 32u ? 0u : ((dfl >> pos0) & ((1u << kk) - 1u));
        const uint32_t nwords = kk + (uint32_t)__popc(dm);
        const uint32_t n_line = (uint32_t)__popcll(bits) + (uint32_t)__popc(dfl);
        const uint32_t inl = n_line > GROUP_INLINE ? GROUP_INLINE - 1u : GROUP_INLINE;
        const uint32_t start = pos0 + dbl_before;
        // second words of doubles: the t-th double, at position i, has its second word at i + t + 1
        uint32_t second = 0;
        for (uint32_t d = dm, t = 0; d != 0u; d &= d - 1u, ++t) second |= 1u << ((uint32_t)__builtin_ctz(d) + t + 1u);
        // what is per hash is counted here, by its one lane
        if (valid) { my_probes += nactive; my_reads += 2u; }
        uint32_t inr = active;
        if (h < g->lo_all || h > g->hi_all) {          // (rare: see probe)
            inr = 0u;
            uint32_t z = 0u;
            asm volatile("" : "+v"(z));
#pragma unroll
            for (uint32_t s = 0; s < NS; ++s) inr |= (h >= s_first[z + s] && h <= s_last[z + s]) ? (1u << s) : 0u;
        }
        if (!valid) inr = 0u;
        my_blocks += (uint32_t)__popc(inr & active & ~pm);         // absent: the reference visits one block, finds nothing and stops
        // its words behind the line's inline part are in `ext`, at the offset in the line's last word: tasks of up to eight words
        const uint32_t in_line = min(nwords, start < inl ? inl - start : 0u);
        const uint32_t in_ext = nwords - in_line;
        if (in_ext != 0u) my_reads += 2u;
        const uint32_t chunk = ((h >> GROUP_CHUNK_LOG2) - g->chunk0) & 63u;
        // (2) the hash's words as the LINE sees them, made once by its lane: bit w of wr = word w of the line (position w - 3) belongs to
        // the hash -- words start + 3 .. start + in_line + 2, at most word 31: inl <= 29 --, bit w of ws = it is the second word of a
        // double (a hash without an inline word: in_line = 0, nothing, whatever the shift; ws is not cut to wr: it is only ever looked at
        // under `keep`, which is).  Both go to the group, line by line, and a lane's share of line k is nibble `sub` of each, put at
        // nibble k of its own masks.
        const uint32_t wb = (start + 3u) & 31u;
        uint32_t wr = ((1u << in_line) - 1u) << wb;
        uint32_t ws = second << wb;
        // (FILT) a word of a column outside the snapshot is not the hash's: never kept, never a list, never counted -- the hash's lane
        // walks its columns once (probe's amask, over the words in the line) where any of them is masked
        if constexpr (FILT) {
            if ((pm & ~active) != 0u) {
                uint32_t am = 0u;
                for (uint32_t r = pm, i = 0, w = 0; r != 0u && w < in_line; r &= r - 1u, ++i) {
                    const uint32_t s = (uint32_t)__builtin_ctz(r), span = 1u + ((dm >> i) & 1u);
                    am |= ((active >> s) & 1u) != 0u ? ((1u << span) - 1u) << w : 0u;
                    w += span;
                }
                wr &= am << wb;
            }
        }
        uint32_t rm32 = 0, sec32 = 0;                    // the lane's words (register 4 k + t) that belong to their line's hash; second words among them
        const uint32_t nb = 4u * sub;
        // (four lines at a time -- eight broadcasts, one wait --: sixteen broadcasts at once cost sixteen registers)
        auto four_lines = [&](auto kc) {
            constexpr uint32_t k = decltype(kc)::value;
            const uint32_t r0 = qs_group_bcast<k>(wr), r1 = qs_group_bcast<k + 1u>(wr), r2 = qs_group_bcast<k + 2u>(wr), r3 = qs_group_bcast<k + 3u>(wr);
            const uint32_t s0 = qs_group_bcast<k>(ws), s1 = qs_group_bcast<k + 1u>(ws), s2 = qs_group_bcast<k + 2u>(ws), s3 = qs_group_bcast<k + 3u>(ws);
            auto nib = [&](uint32_t v) -> uint32_t { return __builtin_amdgcn_ubfe(v, nb, 4u); };
            rm32 |= (nib(r0) << (4u * k)) | (nib(r1) << (4u * k + 4u)) | (nib(r2) << (4u * k + 8u)) | (nib(r3) << (4u * k + 12u));
            sec32 |= (nib(s0) << (4u * k)) | (nib(s1) << (4u * k + 4u)) | (nib(s2) << (4u * k + 8u)) | (nib(s3) << (4u * k + 12u));
            asm volatile("" : "+v"(wr), "+v"(ws), "+v"(rm32), "+v"(sec32));
        };
        four_lines(qs_idx<0u>{});
        four_lines(qs_idx<4u>{});
        uint32_t neg32 = 0;                                                   // a gap position and a list reference have bit 31
#pragma unroll
        for (uint32_t j = 32; j-- != 0u;) neg32 = __builtin_amdgcn_alignbit(neg32, L[j], 31);
        const uint32_t keep = rm32 & ~neg32;
        uint32_t cand = rm32 & neg32;                                         // list references and gap positions
        uint32_t nrec = (uint32_t)__popc(keep);
        my_docs += nrec;
        my_blocks += (uint32_t)__popc(keep & ~sec32);
        // (CLS) what the walk SAW is counted above, whatever the class; the records are this pass's class only
        uint32_t kept = keep & cm32;
        if constexpr (CLS) nrec = (uint32_t)__popc(kept);
        // (the scan histograms: a double is ONE observation of two docs, counted where its second word is -- the upper half of my_probes)
        if constexpr (SCAN_HIST && (FPX_SH_BITS & 2)) my_probes += (uint32_t)__popc(keep & sec32) << 16;
        // the lane's register j0 (selects, first of its line's four, then among those: no register array is indexed by a lane's own number)
        auto word_at = [&](uint32_t j0) -> uint32_t {
            uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
            const uint32_t k0 = j0 >> 2;
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k) {
                const bool me = k0 == k;
                w0 = me ? L[4 * k] : w0; w1 = me ? L[4 * k + 1] : w1; w2 = me ? L[4 * k + 2] : w2; w3 = me ? L[4 * k + 3] : w3;
            }
            const uint32_t lo = (j0 & 1u) ? w1 : w0, hi = (j0 & 1u) ? w3 : w2;
            return (j0 & 2u) ? hi : lo;
        };
        // (FILT) what the word's lane needs of its line's hash to name the word's column: pm | dm << 16 and start, from the hash's lane
        // -- number j0 >> 2 of the group --, next to the chunk.  The whole wave is here.  -> the column of the lane's register j0
        const uint32_t pmdm = pm | (dm << 16);
        (void)pmdm;
        auto col_of = [&](uint32_t j0, bool want) -> uint32_t {
            const int src = (int)((lane & 56u) | (j0 >> 2));
            const uint32_t pd = (uint32_t)__shfl((int)pmdm, src), st = (uint32_t)__shfl((int)start, src);
            return want ? qs_word_cols(pd & 0xFFFFu, pd >> 16, nb + (j0 & 3u) - 3u - st, 1u) : 0u;
        };
        (void)col_of;
        // (FILT) supersession, behind the counting above (CTR_DOCS counts before it): every kept doc word against the UNION bitmap, eight
        // loads of a lane under way together and no column needed; only a word whose bit is set -- hardly any: noted in hit32, taken up
        // behind the loop -- finds its column and runs the exact test.  A null bitmap: no column has a dead set, nothing to test.
        if constexpr (FILT) {
            if (ub != nullptr) {                                                   // (uniform)
                uint32_t left = keep, hit32 = 0u;                                  // hit32: the lane's registers whose union bit is set
                while (__ballot((int)(left != 0u)) != 0ull) {
                    // (a word's place in its bitmap word waits for the load packed, eight bits each: the word itself does not stay live)
                    uint32_t bv[8], it = left, shp[2] = {0u, 0u}, inm = 0u;
#pragma unroll
                    for (uint32_t u = 0; u < 8u; ++u) {
                        const bool has = it != 0u;
                        const uint32_t w = word_at(has ? (uint32_t)__builtin_ctz(it) : 0u);
                        it &= it - 1u;
                        // (a lane without an eighth word reads the bitmap's first: one address, a hit, no load under a branch)
                        const bool in = has && (w >> 5) <= ub_last;
                        bv[u] = gload_u32(reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(ub) + (in ? (w >> 5) << 2 : 0u)));
                        shp[u >> 2] |= (w & 31u) << (8u * (u & 3u));
                        inm |= (in ? 1u : 0u) << u;
                        asm volatile("" : "+v"(shp[u >> 2]), "+v"(inm));
                    }
                    uint32_t hm = 0u;
#pragma unroll
                    for (uint32_t u = 0; u < 8u; ++u) hm |= ((bv[u] >> ((shp[u >> 2] >> (8u * (u & 3u))) & 31u)) & 1u) << u;
                    hm &= inm;
                    if (hm != 0u) {                                                // (rare, and the lane's own business: which registers those were)
                        uint32_t jt = left;
                        for (uint32_t u = 0; u < 8u && jt != 0u; ++u, jt &= jt - 1u) hit32 |= ((hm >> u) & 1u) << (uint32_t)__builtin_ctz(jt);
                    }
                    left = it;
                }
                // (rare: a superseded doc, or its live rewrite -- the wave makes a turn per such word of its fullest lane)
                while (__ballot((int)(hit32 != 0u)) != 0ull) {
                    const bool hit = hit32 != 0u;
                    const uint32_t j0 = hit ? (uint32_t)__builtin_ctz(hit32) : 0u;
                    hit32 &= hit32 - 1u;
                    const uint32_t s = col_of(j0, hit);
                    if (hit && dead_in(s, gmin + word_at(j0))) kept &= ~(1u << j0);
                }
                nrec = (uint32_t)__popc(kept);
            }
        }
        // a list's task is pushed by the lane that owns the word: its first two lists out of the wave's reservation (le: the address's
        // word offset in `ext`, lc: the hash's chunk -- its lane's, number j0 >> 2 of the group), a third one by itself
        // (a gap mark among the lane's words takes one of the two turns without giving a task: a lane with two gaps before a list pushes
        // that list by itself, through the per-lane atomic -- correct, and how often the headline's data does it is not measured)
        uint32_t le[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, lc[2] = {0u, 0u};
        auto next_list = [&](uint32_t& e, uint32_t& c) {                       // (the whole wave is here)
            const uint32_t j0 = cand != 0u ? (uint32_t)__builtin_ctz(cand) : 0u;
            c = (uint32_t)__shfl((int)chunk, (int)((lane & 56u) | (j0 >> 2)));
            if constexpr (FILT) c |= col_of(j0, cand != 0u) << 8;               // ((FILT) the list's column rides above the chunk)
            e = cand != 0u ? word_at(j0) : 0xFFFFFFFFu;                        // (0xFFFFFFFF: a gap position, or nothing)
            cand &= cand - 1u;
        };
        // (FILT) a list's task carries its column in bits 46..49 (the unfiltered form's pushes keep their own text, below: behind a
        // lambda of both forms their instruction stream moved by two instructions)
        auto list_task_filt = [&](uint32_t e, uint32_t c) -> unsigned long long {
            return qs_task_list(s_ext[c & 63u] + (e & 0x7FFFFFFFu), c & 63u) | ((unsigned long long)(c >> 8) << 46);
        };
        (void)list_task_filt;
        if (__ballot((int)(cand != 0u)) != 0ull) {
            next_list(le[0], lc[0]);
            if (__ballot((int)(cand != 0u)) != 0ull) next_list(le[1], lc[1]);
        }
        const uint32_t nt = (le[0] != 0xFFFFFFFFu ? 1u : 0u) + (le[1] != 0xFFFFFFFFu ? 1u : 0u) + (in_ext + QS_TASK_WORDS - 1u) / QS_TASK_WORDS;
        // (3)
        uint32_t tat;
        emit_at(kept, L, nrec, reserve_both(nrec, nt, tat));
        if (nt != 0u) {
            if (tat + nt > TCAP) { s_over_recs = 1u; tat = TCAP; }                // (a full queue: the batch goes the long way)
            auto put_task = [&](unsigned long long e) { if (tat < TCAP) tasks[tat] = e; ++tat; };
#pragma unroll
            for (uint32_t u = 0; u < 2u; ++u)
                if (le[u] != 0xFFFFFFFFu) {
                    if constexpr (FILT) put_task(list_task_filt(le[u], lc[u]));
                    else put_task(qs_task_list(s_ext[lc[u]] + (le[u] & 0x7FFFFFFFu), lc[u]));
                }
            if (in_ext != 0u) {
                const uint32_t* ob = s_ext[chunk] + ov;
                for (uint32_t j = in_line; j < nwords;) {                      // (start + j >= inl here)
                    const uint32_t c = min(nwords - j, QS_TASK_WORDS);
                    if constexpr (FILT) { if (tat < TCAP) tcols[tat] = qs_word_cols(pm, dm, j, c); }      // (the words' columns, as probe's put_words)
                    put_task(qs_task_words(ob + (start + j - inl), c, second >> j, chunk));
                    j += c;
                }
            }
        }
        while (__ballot((int)(cand != 0u)) != 0ull) {                            // (a lane with three lists among its words: hardly ever)
            uint32_t e, c;
            next_list(e, c);
            if constexpr (FILT) { if (e != 0xFFFFFFFFu) push_task(list_task_filt(e, c)); }
            else if (e != 0xFFFFFFFFu) push_task(qs_task_list(s_ext[c] + (e & 0x7FFFFFFFu), c));
        }
    };

    // (PACK) the memory table's look-up for the PACKED hashes, before the rounds while hq[0..3] still hold all of them (behind the rounds
    // the lane's registers have rolled, and a position in the batch's array no longer names the lane's hash): the look-up below, word for word
    // -- a text of its own on purpose: one look-up with the hash's source as a parameter moved the instruction stream and the SGPR spills
    // (30 -> 34, 42 -> 50) of every older MEM instantiation
    auto mem_packed = [&]() {
        if (__ballot((int)((mmask & 15u) != 0u)) == 0ull) return;                  // (wave-uniform)
        uint32_t blo[4], bhi[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
            const bool act = ((mmask >> u) & 1u) != 0u;
            const uint32_t b = hq[u] >> (32u - MEMTAB_BITS);
            blo[u] = act ? gload_u32(a.mem_bucket + b) : 0u;
            bhi[u] = act ? gload_u32(a.mem_bucket + b + 1u) : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u)
            for (uint32_t i = blo[u]; i < bhi[u]; ++i) {
                const uint64_t it = gload_u64(a.mem_tab + i);
                if ((uint32_t)(it >> 32) > hq[u]) break;
                if ((uint32_t)(it >> 32) == hq[u]) {
                    const uint32_t at = atomicAdd(&s_count, 1u);
                    if (at < QS_REC_CAP) recs[at] = (uint32_t)it - gmin; else s_over_recs = 1u;
                }
            }
    };
    (void)mem_packed;

    static_assert(QS_CH == 2, "the rounds run in pairs");
    if constexpr (MEM && PACK) mem_packed();
    for (uint32_t c = 0; c < pnchunks; ++c) {
        if constexpr (!FILT || COOP) {
            // a round after the other, each with its 64 lines per wave under way at once (the lane's registers hold one round's)
            QS_SUB0();
            QS_ARRIVED2(hq[0], hq[1]);
            QS_SUB(7);
            // (PACK: the probes sit in lanes 0 .. m - 1 -- a wave whose 64 lanes hold none in a round skips that round's walk: no barrier
            // between here and the end of the rounds, and everything in the walk is the wave's own)
            const bool v0 = ((vmask >> (c * QS_CH)) & 1u) != 0u, v1 = ((vmask >> (c * QS_CH + 1u)) & 1u) != 0u;
            if (!PACK || __ballot((int)v0) != 0ull) round_coop(hq[0], v0);
            if (c * QS_CH + 1u < prounds && (!PACK || __ballot((int)v1) != 0ull)) round_coop(hq[1], v1);      // (uniform)
            QS_SUB(10);
        } else {
        // two rounds at a time, their hashes in hq[0..1]: their line heads, then -- as the heads arrive -- the words of both (and the offset
        // of an overflowing line's rest), then both rounds out of registers
        QS_SUB0();
        QS_ARRIVED2(hq[0], hq[1]);
        QS_SUB(7);
        const bool v0 = ((vmask >> (c * QS_CH)) & 1u) != 0u, v1 = ((vmask >> (c * QS_CH + 1u)) & 1u) != 0u;
        if (!PACK || __ballot((int)(v0 || v1)) != 0ull) {      // (PACK: a wave without a probe in the pair skips it -- wave-uniform)
        issue_heads(v0, v1);
        // (BOTH heads are under way before either is looked at: what follows sees the six words only behind this point)
        asm volatile("" : "+v"(hd[0].x), "+v"(hd[0].y), "+v"(hd[0].z), "+v"(hd[1].x), "+v"(hd[1].y), "+v"(hd[1].z));
        QS_SUB(8);
        uint32_t gw0[QS_WORDS], gw1[QS_WORDS], hx0, hy0, hx1, hy1;
        uint32_t ov0, ov1;
        words_of(hq[0], hd[0], v0, gw0, hx0, hy0, ov0);
        words_of(hq[1], hd[1], v1, gw1, hx1, hy1, ov1);
        asm volatile("" : "+v"(ov0), "+v"(ov1));             // (likewise: the second hash's words set out before the first one's offset is waited for)
        QS_ARRIVED4(gw0); QS_ARRIVED4(gw0 + 4); QS_ARRIVED4(gw0 + 8); QS_ARRIVED4(gw1); QS_ARRIVED4(gw1 + 4); QS_ARRIVED4(gw1 + 8);
        QS_SUB(9);
        probe(hq[0], hx0, hy0, v0, gw0, ov0);
        if (c * QS_CH + 1u < prounds) probe(hq[1], hx1, hy1, v1, gw1, ov1);              // (uniform)
        }
        QS_SUB(10);
        }
        // (the window rolls: the next pair moves up, the one after it -- a query of more than 1024 hashes -- sets out)
        // ((CLS) no window: the next pair is asked for when this one is done -- two registers the class masks need, on the rare path)
        if constexpr (CLS) { if (c + 1u < nchunks) load_pair(qh, n, c + 1u, hq[0], hq[1]); }
        else {
            hq[0] = hq[2]; hq[1] = hq[3];
            if (c + 2u < pnchunks) load_pair(qh, n, c + 2u, hq[2], hq[3]);
        }
    }
    // ---- MemorySegment.search (src/MemorySegment.zig:44-54) for all memory segments at once: the query's probes looked up in the snapshot's
    //      table of their live postings -- a bit per 256 hash values says "nothing there" for nine probes in ten --, four rounds' loads out
    //      together; every matching item is a record (a doc a newer segment supersedes was dropped when the table was built)
    if constexpr (MEM && !PACK) {
        for (uint32_t c0 = 0; c0 < rounds; c0 += 4u) {
            if (__ballot((int)(((mmask >> c0) & 15u) != 0u)) == 0ull) continue;          // (wave-uniform: nine probes in ten have nothing there)
            uint32_t mh[4], blo[4], bhi[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) {
                const bool act = ((mmask >> (c0 + u)) & 1u) != 0u;
                mh[u] = act ? gload_u32(qh + (c0 + u) * QS_WG + tid) : 0u;
                const uint32_t b = mh[u] >> (32u - MEMTAB_BITS);
                blo[u] = act ? gload_u32(a.mem_bucket + b) : 0u;
                bhi[u] = act ? gload_u32(a.mem_bucket + b + 1u) : 0u;
            }
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u)
                for (uint32_t i = blo[u]; i < bhi[u]; ++i) {                       // (a bucket holds a posting or two)
                    const uint64_t it = gload_u64(a.mem_tab + i);
                    if ((uint32_t)(it >> 32) > mh[u]) break;
                    if ((uint32_t)(it >> 32) == mh[u] && (!CLS || in_class((uint32_t)it - gmin))) {
                        const uint32_t at = atomicAdd(&s_count, 1u);
                        if (at < QS_REC_CAP) recs[at] = (uint32_t)it - gmin; else s_over_recs = 1u;      // (a memory segment's doc may lie below gmin: modulo 2^32)
                    }
                }
        }
    }
    __syncthreads();
    QS_MARK(2);
    // ---- the NEXT query's hashes set out now (the hash registers are free; its offsets have been here since the query before this one):
    //      they travel under this query's tasks and counting
    // (... and the query after THAT is asked of the launch's counter: the answer has the tasks to arrive in)
    uint32_t r2 = 0u;
    if (tid == 0u) { unsigned int* const next_q = qs_cold_args()->a.next_q; if (next_q != nullptr) r2 = atomicAdd(next_q, 1u); }
    QS_SUB0();
    QS_ARRIVED2(nn, (uint32_t)nq_lo); QS_SUB(11);
    // (this query's floor, which the exact pass will want: every lane asks for the one word -- a vector load stays in flight
    // under the LDS work, a scalar one would be waited for with the next LDS read)
    uint32_t floor_v;
    {
        uint32_t qv = q;
        asm volatile("" : "+v"(qv));
        floor_v = gload_u32(qs_cold_args()->a.opts + (size_t)qv * 4u + 1u);
    }
    if (has_next) {
        const uint32_t* const qhn = a.hashes_base + nq_lo;
        load_pair(qhn, nn, 0u, hq[0], hq[1]);
        load_pair(qhn, nn, 1u, hq[2], hq[3]);
    }
    // ---- the deferred tasks, a task per lane: every list head and overflow piece of the query is asked for at once.  (A list inside
    //      overflowing words is a task of the next pass.)
    {
        uint32_t t_lo = 0;
        for (;;) {
            const uint32_t t_hi = min(s_ntask, TCAP);                            // (uniform: read behind a barrier ...
            __syncthreads();                                                      // ... and nobody pushes before everybody has read it)
            if (t_lo >= t_hi) break;
            for (uint32_t t0 = t_lo; t0 < t_hi; t0 += QS_WG) {
                const bool has = t0 + tid < t_hi;
                const unsigned long long e = has ? tasks[t0 + tid] : 0ull;
                const bool is_list = has && (e >> 63) != 0ull;
                const uint32_t* p = qs_task_ptr(e);
                // (FILT) a list's column; a words task's columns
                const uint32_t lcol = FILT ? (uint32_t)(e >> 46) & 15u : 0u;
                const uint32_t tc = (FILT && has && !is_list) ? tcols[t0 + tid] : 0u;
                uint32_t d[QS_TASK_WORDS];
#pragma unroll
                for (uint32_t j = 0; j < QS_TASK_WORDS; ++j) d[j] = 0xFFFFFFFFu;
                const uint32_t cnt = !has ? 0u : is_list ? 8u : ((uint32_t)(e >> 46) & 7u) + 1u;          // words to fetch: a list's header + seven, or the task's
#pragma unroll
                for (uint32_t i = 0; i < QS_TASK_WORDS / 4; ++i) {
                    if (cnt > 4u * i) {
                        const uint4 v = gload_u4_a4(p + 4u * i);
                        d[4 * i] = v.x; d[4 * i + 1] = v.y; d[4 * i + 2] = v.z; d[4 * i + 3] = v.w;
                    }
                }
                uint32_t km = 0, lm = 0;
                bool long_list = false;
                uint32_t eff = 0, Tl = 0, xin = 0;
                if (is_list) {
                    // header: docs the reference RETURNS | blocks it VISITS << 16 | T << 19 [T: the list's full length follows]; then the docs
                    const uint32_t hdr = d[0];
                    eff = hdr & 0xFFFFu; Tl = (hdr >> 19) & 1u;
                    xin = min(eff, Tl ? 6u : 7u);
                    km = ((1u << xin) - 1u) << (1u + Tl);
                    my_blocks += (hdr >> 16) & 7u; my_docs += eff; my_reads += 2u;
                    hist_observe(wg_h, eff, (hdr >> 16) & 7u);
                    long_list = eff > xin;
                    if (long_list) my_reads += ((eff - xin + 31u) >> 5) * 2u;
                } else if (has) {
                    const uint32_t second = (uint32_t)(e >> 49) & 0xFFu;
                    uint32_t vm = (1u << cnt) - 1u, negm = 0, gapm = 0;
#pragma unroll
                    for (uint32_t j = 0; j < QS_TASK_WORDS; ++j) {
                        if constexpr (FILT) vm &= ~((((active >> ((tc >> (4u * j)) & 15u)) & 1u) ^ 1u) << j);
                        negm |= (d[j] >> 31) << j;
                        gapm |= (d[j] == 0xFFFFFFFFu ? 1u : 0u) << j;
                    }
                    km = vm & ~negm;
                    lm = vm & negm & ~gapm;
                    my_docs += (uint32_t)__popc(km); my_blocks += (uint32_t)__popc(km & ~second);
                    if constexpr (SCAN_HIST && (FPX_SH_BITS & 2)) my_probes += (uint32_t)__popc(km & second) << 16;
                }
                if constexpr (FILT) {                   // (counted above: before supersession)
                    for (uint32_t m = km; m != 0u; m &= m - 1u) {
                        const uint32_t j0 = (uint32_t)__builtin_ctz(m);
                        const uint32_t s = is_list ? lcol : (tc >> (4u * j0)) & 15u;
                        if (s_dseg[s] == 0xFFFFFFFFu) continue;
                        uint32_t doc = 0;
#pragma unroll
                        for (uint32_t j = 0; j < QS_TASK_WORDS; ++j) doc = j == j0 ? d[j] : doc;
                        if constexpr (COOP) { if (!union_hit(doc)) continue; }      // (the union bitmap first: a clear bit is live in every column)
                        if (dead_in(s, gmin + doc)) km &= ~(1u << j0);
                    }
                }
                if constexpr (CLS) {                    // (counted above, whatever the class)
                    uint32_t cm = 0u;
#pragma unroll
                    for (uint32_t j = QS_TASK_WORDS; j-- != 0u;) cm = (cm << 1) | (in_class(d[j]) ? 1u : 0u);
                    km &= cm;
                }
                emit(km, d);
                while (lm != 0u) {                      // (a list inside the words: the next pass's)
                    const uint32_t j0 = (uint32_t)__builtin_ctz(lm);
                    lm &= lm - 1u;
                    uint32_t w = 0;
#pragma unroll
                    for (uint32_t j = 0; j < QS_TASK_WORDS; ++j) w = j == j0 ? d[j] : w;
                    const uint32_t chunk = (uint32_t)(e >> 57) & 63u;
                    push_task(qs_task_list(s_ext[chunk] + (w & 0x7FFFFFFFu), chunk) | (FILT ? ((unsigned long long)((tc >> (4u * j0)) & 15u) << 46) : 0ull));
                }
                // lists longer than their head: the wave reads them on, 64 docs at a time
                unsigned long long ml = __ballot((int)long_list);
                while (ml != 0ull) {
                    const int src = (int)__builtin_ctzll(ml);
                    ml &= ml - 1ull;
                    const uint32_t* list = reinterpret_cast<const uint32_t*>(((uint64_t)__shfl((uint32_t)((uint64_t)p >> 32), src) << 32) | __shfl((uint32_t)(uint64_t)p, src));
                    const uint32_t eff_s = __shfl(eff, src), T_s = __shfl(Tl, src), from = __shfl(xin, src);
                    const uint32_t col_s = FILT ? (uint32_t)__shfl(lcol, src) : 0u;
                    if constexpr (CLS) {
                        // (a redone query IS its long lists -- a hot hash is a list of 1000 docs in every column -- and a wave walks them one
                        // after the other, a trip to memory per 64 docs.  Here QS_LIST_AHEAD x 64 docs are asked for before the first is
                        // looked at: a step of 8192 queries, 8 of them with 32 such lists each, 3.92 -> 3.17 ms, profiles/r11_hot_wg.txt)
                        for (uint32_t o2 = from; o2 < eff_s; o2 += 64u * QS_LIST_AHEAD) {
                            uint32_t dv[QS_LIST_AHEAD];
#pragma unroll
                            for (uint32_t u = 0; u < QS_LIST_AHEAD; ++u)
                                dv[u] = o2 + 64u * u + lane < eff_s ? gload_u32(list + 1u + T_s + o2 + 64u * u + lane) : 0u;
#pragma unroll
                            for (uint32_t u = 0; u < QS_LIST_AHEAD; ++u) emit1(o2 + 64u * u + lane < eff_s, dv[u]);
                        }
                    } else
                    for (uint32_t o2 = from; o2 < eff_s; o2 += 64u) {
                        bool kp = o2 + lane < eff_s;
                        const uint32_t dv = kp ? gload_u32(list + 1u + T_s + o2 + lane) : 0u;
                        if constexpr (FILT && COOP) { if (kp && union_hit(dv)) kp = !dead_in(col_s, gmin + dv); }
                        else if constexpr (FILT) { if (kp) kp = !dead_in(col_s, gmin + dv); }
                        emit1(kp, dv);
                    }
                }
            }
            t_lo = t_hi;
            __syncthreads();
        }
    }

    // (every task has been read: the queue's slots become the filter and the exact table)
    if constexpr (!SHARE) {
    for (uint32_t i = tid; i < (1u << (QS_FLOG2 - 1u)); i += QS_WG) filter[i] = 0u;
    for (uint32_t s = tid; s < T; s += QS_WG) table[s] = 0ull;
    }
    // ---- the query's statistics (what FileSegment.search observes per hash, summed: src/FileSegment.zig:177-178)
    {
        auto wave_total = [&](uint32_t v) -> unsigned long long {
            const uint32_t incl = scan16(v);
            return (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)incl, 15) + (uint32_t)__builtin_amdgcn_readlane((int)incl, 31) +
                   (uint32_t)__builtin_amdgcn_readlane((int)incl, 47) + (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        };
        const unsigned long long w_reads = wave_total(my_reads), w_blocks = wave_total(my_blocks), w_docs = wave_total(my_docs), w_probes = wave_total(my_probes & 0xFFFFu);
        const uint32_t w_doubles = (uint32_t)wave_total(my_probes >> 16);
        // (the counter's answer -- the query after the next one -- goes to the workgroup behind the barrier below)
        if (tid == 0u) s_q2 = qs_cold_args()->a.next_q != nullptr ? a.q_begin + 2u * gridDim.x + r2 : qn + gridDim.x;
        if (lane == 0u && (!CLS || cls == 0u)) {           // (CLS: every pass sees the same blocks and docs; the first one reports them)
            if (w_doubles) atomicAdd(&wg_h[0], w_doubles);
            if (w_reads) atomicAdd(&wg_reads, w_reads);
            if (w_blocks) atomicAdd(&wg_blocks, w_blocks);
            if (w_docs) atomicAdd(&wg_docs, w_docs);
            if (w_probes) atomicAdd(&wg_probes, w_probes);
        }
    }
    __syncthreads();                                    // (the records are complete, the filter and the table are clear)
    QS_MARK(3);
    // ---- the offsets of the query after the next one set out as soon as it is known, and the next query's cancel flag: they travel under
    //      this query's counting (vector loads of one address, as the floor's above)
    q2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_q2);
    has_q2 = has_next && q2 < a.q_end;                      // (uniform)
    if (has_q2) {
        uint32_t qv = q2;
        asm volatile("" : "+v"(qv));
        o2_lo = gload_u64(a.offsets + qv); o2_hi = gload_u32(reinterpret_cast<const uint32_t*>(a.offsets + qv + 1u));
    }
    if (has_next) ask_cancel();
    const uint32_t nrec = min(s_count, QS_REC_CAP);
    // ---- SearchResults.incr (src/common.zig:121-129), first the filter: every record into its doc's cell
    // (four records per lane and turn, read as one 16-byte piece: the loop is a chain of LDS latencies -- a record, then its cell)
    // (a lane's four are all records in every turn but the query's last: only that one tests record by record)
    uint32_t tc4 = tid * 4u;                                 // ((COOP) likewise: the loop's first address is made here, not held from the kernel's start)
    if constexpr (COOP) asm volatile("" : "+v"(tc4));
    if constexpr (!SHARE)
    for (uint32_t i = tc4; i < nrec; i += QS_WG * 4u) {
        const uint4 r4 = *reinterpret_cast<const uint4*>(recs + i);             // (the array ends with four spare words)
        const uint32_t r[4] = {r4.x, r4.y, r4.z, r4.w};
        if (i + 3u < nrec) {
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) {
                const uint32_t c = qs_cell(r[u]);
                atomicAdd(&filter[c >> 1], 1u << (16u * (c & 1u)));
            }
        } else {
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) {
                const uint32_t c = qs_cell(r[u]);
                if (i + u < nrec) atomicAdd(&filter[c >> 1], 1u << (16u * (c & 1u)));
            }
        }
    }
    const qs_kargs_t kt = qs_cold_args();               // (the tail's arguments: read here, once per query)
    // (s_over_recs and the counts are final: the barrier above.)  A query whose records outgrew the array, where the batch has a redo list
    // (option hot_wg, unfiltered): it is named there with its record total -- s_count went on counting past the array's end -- and gives
    // NO statistic and no candidate here: k_search_classes redoes it and owns them all.  A query whose TASK QUEUE overflowed has no total
    // (the tasks beyond the queue were never read) and would overflow the same queue in every class: that one fails the batch as before.
    const bool q_stats = !CLS || cls == 0u;                  // (CLS: blocks, docs, probes, reads and the histograms in one pass only)
    bool q_redo = false;
    if constexpr (!FILT && !CLS && !NEXT && !SHARE) {      // (SHARE: no redo list -- the member carries something else)
        if (s_over_recs != 0u || s_count > QS_REC_CAP) q_redo = kt->a.redo != nullptr && s_ntask <= TCAP;
    }
    if (tid == 0 && q_redo) {
        const unsigned long long at = atomicAdd(&kt->a.counters[CTR_REDO], 1ull);
        if (at < (unsigned long long)kt->a.redo_cap) kt->a.redo[at] = (unsigned long long)q | ((unsigned long long)s_count << 32);
    }
    if (tid == 0 && !q_redo) {
        unsigned long long* st = kt->a.stat_sets + (size_t)(q % LEAN_STAT_SETS) * 8u;
        if (q_stats) {
            if (wg_reads) atomicAdd(&st[4], wg_reads);
            if (wg_blocks) atomicAdd(&st[1], wg_blocks);
            const uint32_t block_size = kt->ga.g.block_size;
            if (wg_blocks && block_size != 512u) atomicAdd(&st[5], wg_blocks * (unsigned long long)block_size - wg_blocks * 512ull);
            if (wg_docs) atomicAdd(&st[2], wg_docs);
            if (wg_probes) atomicAdd(&st[3], wg_probes);
        }
        if (s_count) atomicAdd(&st[7], (unsigned long long)s_count);                  // the query's hit records ((CLS) this class's: summed over the passes)
        if constexpr (QS && NEXT) { unsigned long long* const qstats = kt->a.qstats; if (qstats) qstats[q] += wg_blocks | (wg_docs << 32); }   // (the query is this workgroup's alone; the launch before is over)
        else if constexpr (QS) { if (q_stats) { unsigned long long* const qstats = kt->a.qstats; if (qstats) qstats[q] = wg_blocks | (wg_docs << 32); } }
        if (s_over_recs || s_count > QS_REC_CAP) atomicMax(&kt->a.counters[CTR_BINFAIL], 1ull);
    }
    if (tid < HIST_SLOTS - 1u && q_stats && !q_redo) {       // (slot 15: hist_observe's sink)
        const unsigned long long v = tid == HIST_COUNT ? wg_probes : tid == HIST_DOCS ? wg_docs : tid == HIST_BLOCKS ? wg_blocks : (unsigned long long)wg_h[tid];
        if (v != 0ull) atomicAdd(&kt->a.stat_sets[(size_t)LEAN_STAT_SETS * 8u + (size_t)(q % LEAN_STAT_SETS) * HIST_SLOTS + tid], v);
    }
    // ---- ... then the floor of finish (src/common.zig:131-145): a doc can only reach the floor if its cell did; those records are
    //      counted exactly, in `passes` loads over classes of them when they are more than the table takes
    const uint32_t floor_q = (uint32_t)__builtin_amdgcn_readfirstlane((int)floor_v);
    const uint32_t sb = kt->a.sb;
    const uint64_t smax = sb >= 32u ? 0xFFFFFFFFull : ((1ull << sb) - 1ull);
    const bool low_q = LOW && floor_q <= 2u;                 // (uniform: the query's own floor chooses its tail)
    if constexpr (LOW) {
      // ---- a floor of 1 or 2: every counted doc is a candidate for the table, so there is no table.  (1) the records become absolute
      //      ids (+ gmin modulo 2^32: a memory segment's doc below gmin was a large value; compareResults' tie-break, src/common.zig:169-171,
      //      is on the real id); (2) they are SORTED ascending in place, a bitonic network over P = the next power of two, the places
      //      [nrec, P) padded with 0xFFFFFFFF -- a legal id, but pads are the maximum: the first nrec places hold exactly the records --;
      //      (3) a doc's score is the length of its run, M the longest; (4) the floor is raised to E = max(floor, rel_floor(M, pct)) --
      //      finish's relative cut on what this call sees: a part's best is a lower bound of the whole snapshot's, as k_score's
      //      count-only round argues --; (5) of the docs at or above E only what finish can return leaves: with more than K = max_results
      //      of them, those above the K-th's score T and, of the docs AT T, the first K - N(> T) in array order, which is id order.
      //      k_finish gets a superset of what it keeps, in the usual keys.  The filter's area is scratch: a histogram of min(score, 255),
      //      the waves' totals, M, T and the quota.
      if (low_q && s_over_recs == 0u && !q_redo && nrec != 0u && nrec >= floor_q && kt->a.opts[(size_t)q * 4u] != 0u) {
        // ((COOP) the lane's number is taken afresh for the tail, as load_pair's `t` and the filter's `tc4` are: what the tail makes of it --
        // lsc's slot of the lane's wave, the slot lane 255 writes T to, half a dozen comparisons -- does not change from query to query,
        // was made at the kernel's start and held across the rounds: in k_search_low_coop<16, ..> that was 20 bytes of scratch.  Every
        // other kernel's lt and llane ARE its tid and lane)
        uint32_t lt_own = tid;
        if constexpr (COOP) asm volatile("" : "+v"(lt_own));
        const uint32_t llane_own = lt_own & 63u;
        const uint32_t& lt = COOP ? lt_own : tid;
        const uint32_t& llane = COOP ? llane_own : lane;
        const uint32_t kmax = kt->a.opts[(size_t)q * 4u], pct = kt->a.opts[(size_t)q * 4u + 2u];
        const uint32_t gmin_c = kt->ga.g.gmin;
        uint32_t* const lhist = filter;                      // [256]: docs by min(score, 255)
        uint32_t* const lsc = filter + 256u;                 // [0..3] a scan's wave totals, [4] M, [5] T, [6] the quota at T
        uint32_t P = 512u;
        while (P < nrec) P <<= 1;                            // (<= QS_REC_CAP)
        __syncthreads();                                     // (the filter's atomics and everybody's reads of the records are done)
        for (uint32_t i = lt; i < P; i += QS_WG) recs[i] = i < nrec ? recs[i] + gmin_c : 0xFFFFFFFFu;
        lhist[lt] = 0u;
        if (lt < 8u) lsc[lt] = 0u;
        __syncthreads();
        // (2) the network.  A lane keeps QS_LOW_CHUNK consecutive places in registers for the strides below that -- no barrier between
        // them --; the strides from QS_LOW_CHUNK up are four compare-exchanges per lane and turn on 16-byte pieces, a barrier each
        auto cx = [](uint32_t& x, uint32_t& y, bool up) {
            const uint32_t lo = min(x, y), hi = max(x, y);
            x = up ? lo : hi; y = up ? hi : lo;
        };
        auto chunk_sort = [&](uint32_t k) {                  // k == 0: the merge steps 2, 4 and 8 whole; else step k's strides 4, 2, 1
            for (uint32_t c = lt; c < P / QS_LOW_CHUNK; c += QS_WG) {
                uint4* const at = reinterpret_cast<uint4*>(recs + c * QS_LOW_CHUNK);
                const uint4 x0 = at[0], x1 = at[1];
                uint32_t v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
                if (k == 0u) {
#pragma unroll
                    for (uint32_t kk = 2u; kk <= 8u; kk <<= 1)
#pragma unroll
                        for (uint32_t j = kk >> 1; j != 0u; j >>= 1)
#pragma unroll
                            for (uint32_t i = 0; i < 8u; ++i)
                                if ((i & j) == 0u) cx(v[i], v[i | j], kk == 8u ? (c & 1u) == 0u : (i & kk) == 0u);
                } else {
                    const bool up = ((c * QS_LOW_CHUNK) & k) == 0u;
#pragma unroll
                    for (uint32_t j = 4u; j != 0u; j >>= 1)
#pragma unroll
                        for (uint32_t i = 0; i < 8u; ++i)
                            if ((i & j) == 0u) cx(v[i], v[i | j], up);
                }
                at[0] = make_uint4(v[0], v[1], v[2], v[3]); at[1] = make_uint4(v[4], v[5], v[6], v[7]);
            }
        };
        static_assert(QS_LOW_CHUNK == 8u, "chunk_sort is written for eight places");
        chunk_sort(0u);
        __syncthreads();
        for (uint32_t k = 2u * QS_LOW_CHUNK; k <= P; k <<= 1) {
            for (uint32_t j = k >> 1; j >= QS_LOW_CHUNK; j >>= 1) {
                for (uint32_t w = lt; w < P / 8u; w += QS_WG) {
                    const uint32_t t0 = 4u * w, i = ((t0 & ~(j - 1u)) << 1) | (t0 & (j - 1u));       // (four pairs side by side: j >= 8)
                    uint4* const pa = reinterpret_cast<uint4*>(recs + i);
                    uint4* const pb = reinterpret_cast<uint4*>(recs + i + j);
                    uint4 x = *pa, y = *pb;
                    const bool up = (i & k) == 0u;
                    cx(x.x, y.x, up); cx(x.y, y.y, up); cx(x.z, y.z, up); cx(x.w, y.w, up);
                    *pa = x; *pb = y;
                }
                __syncthreads();
            }
            chunk_sort(k);
            __syncthreads();
        }
        // (3) runs.  A lane takes C consecutive places -- C odd: the lanes' places fall into different banks --; a run belongs to the
        // lane that holds its head, its length is one, or found by bisection (the array is sorted: a run ends where the doc does)
        const uint32_t C = ((nrec + QS_WG - 1u) / QS_WG) | 1u;
        const uint32_t i0 = min(lt * C, nrec), i1 = min(i0 + C, nrec);
        auto run_len = [&](uint32_t i, uint32_t doc) -> uint32_t {
            if (i + 1u >= nrec || recs[i + 1u] != doc) return 1u;
            uint32_t lo = i + 2u, hi = nrec;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (recs[mid] == doc) lo = mid + 1u; else hi = mid;
            }
            return lo - i;
        };
        auto for_runs = [&](auto&& f) {                      // f(doc, score) for every run whose head is among the lane's places
            uint32_t prev = (i0 != 0u && i0 < nrec) ? recs[i0 - 1u] : 0u;
            for (uint32_t i = i0; i < i1; ++i) {
                const uint32_t doc = recs[i];
                if (i == 0u || doc != prev) f(doc, run_len(i, doc));
                prev = doc;
            }
        };
        auto wave_incl = [&](uint32_t v) -> uint32_t {       // (the whole wave is here)
            const uint32_t incl = scan16(v);
            const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)incl, 15), r1 = (uint32_t)__builtin_amdgcn_readlane((int)incl, 31),
                           r2 = (uint32_t)__builtin_amdgcn_readlane((int)incl, 47);
            const uint32_t row = llane >> 4;
            return incl + (row >= 1u ? r0 : 0u) + (row >= 2u ? r1 : 0u) + (row >= 3u ? r2 : 0u);
        };
        {
            uint32_t ones = 0u, best = 0u;
            for_runs([&](uint32_t, uint32_t len) {
                best = max(best, len);
                if (len == 1u) ++ones; else atomicAdd(&lhist[min(len, 255u)], 1u);
            });
            if (ones != 0u) atomicAdd(&lhist[1], ones);
            if (best != 0u) atomicMax(&lsc[4], best);
        }
        __syncthreads();
        // (4)
        const uint32_t best_q = lsc[4];
        // ((COOP) rel_floor's 64-bit comparison is made on the VALU against a constant in two vector registers, which the compiler set up
        // at the kernel's start and kept -- the MEM instantiations at 16 columns spilled them: 12 bytes of scratch.  In 32 bits here:
        // best_q <= QS_REC_CAP = 2^13 and the percentage is cut at 2^19 - 1, where the relative floor is above 5242 x best_q already --
        // beyond any score, as with the uncut percentage: best_q < cut either way, and nothing else looks at cut then)
        static_assert(!COOP || QS_REC_CAP <= (1u << 13), "the relative floor in 32 bits");
        const uint32_t rel = COOP ? best_q * min(pct, (1u << 19) - 1u) / 100u : rel_floor(best_q, pct);
        const uint32_t cut = max(floor_q, rel);
        if (best_q >= cut) {                                 // (uniform)
            // (5) lane t: S(t) = docs at or above the cut whose slot is >= t.  T is the slot where S reaches K; slot 255 holds every
            // score from 255 up, so there nothing is cut (a superset: at most 8192 / 255 docs).  With K or fewer docs nobody writes: T = 0
            const uint32_t cb = min(cut, 255u);
            const uint32_t hm = lt >= cb ? lhist[lt] : 0u;
            const uint32_t wi = wave_incl(hm);
            if (llane == 63u) lsc[lt >> 6] = wi;
            __syncthreads();
            const uint32_t t0 = lsc[0], t1 = lsc[1], t2 = lsc[2], t3 = lsc[3], wv = lt >> 6;
            const uint32_t incl = wi + (wv >= 1u ? t0 : 0u) + (wv >= 2u ? t1 : 0u) + (wv >= 3u ? t2 : 0u);
            const uint32_t above = t0 + t1 + t2 + t3 - incl;                       // S(t + 1)
            if (above + hm >= kmax && above < kmax) {
                lsc[5] = lt == 255u ? 254u : lt;
                lsc[6] = lt == 255u ? 0u : kmax - above;
            }
            __syncthreads();
            const uint32_t tcut = lsc[5], quota = lsc[6];
            uint32_t rank = 0u;                              // docs AT tcut in the places before the lane's
            if (quota != 0u) {                               // (uniform)
                uint32_t mine = 0u;
                for_runs([&](uint32_t, uint32_t len) { mine += len == tcut ? 1u : 0u; });
                const uint32_t mi = wave_incl(mine);
                if (llane == 63u) lsc[lt >> 6] = mi;         // (the totals above were read before the last barrier)
                __syncthreads();
                rank = mi - mine + (wv >= 1u ? lsc[0] : 0u) + (wv >= 2u ? lsc[1] : 0u) + (wv >= 3u ? lsc[2] : 0u);
            }
            // the existing hand-over: the query's buffer in LDS (its first SB_CAND), the rest to the shared list
            for_runs([&](uint32_t doc, uint32_t count) {
                if (count < cut || count < tcut) return;
                if (count == tcut && rank++ >= quota) return;
                if ((uint64_t)count > smax) atomicMax(&kt->a.counters[CTR_MAXSCORE], (unsigned long long)count);
                const uint64_t sc = (uint64_t)count > smax ? smax : (uint64_t)count;
                const uint64_t qpart = sb >= 32u ? 0ull : ((uint64_t)q << (32u + sb));
                const uint64_t key = qpart | ((smax - sc) << 32) | doc;
                const uint32_t at = atomicAdd(&s_ccnt, 1u);
                if (at < SB_CAND) cbuf[at] = key;
                else {
                    const unsigned long long gi = atomicAdd(&kt->a.counters[CTR_CANDS], 1ull);
                    if (gi < kt->a.cand_cap) kt->a.cands[gi] = key;
                    s_cshared = 1u;
                }
            });
        }
      }
    }
    if constexpr (SHARE) {
        // ---- (SHARE) the query's records of this window leave for its bin, bin q >> QS_SHARE_BQ of the step's send buffer (QSearchArgs:
        //      bins, bin_cap, bin_fill, bin_rec32).  ONE reservation per query -- nrec is final: the barrier above --, the base
        //      to the workgroup through LDS; every lane copies.  A place at or beyond the capacity is not stored, the fill counter runs
        //      past it: k_cell_counts and the host learn the need from it.  The record is bin_store's (fpx_partition.hpp): narrow,
        //      doc << 3 | q & 7 -- a doc that leaves no room, or would read as "no record", raises CTR_BINFAIL to 3 and the host redoes
        //      the step wide --; wide, q << 32 | doc.  A query whose records outgrew the array (or whose task queue overflowed) stores
        //      nothing: CTR_BINFAIL is 1 (the statistics above) and the host redoes the step on the pipeline.  No padding.
        (void)floor_q; (void)smax; (void)low_q; (void)filter; (void)table; (void)cbuf; (void)TMASK;
        if (s_over_recs == 0u && s_count <= QS_REC_CAP && nrec != 0u) {      // (uniform: LDS words behind a barrier)
            const uint32_t bn = q >> QS_SHARE_BQ;
            if (tid == 0) s_cbase_lo = atomicAdd(&kt->a.bin_fill[(size_t)bn * QS_SHARE_STRIDE], nrec);
            __syncthreads();
            const uint64_t base = s_cbase_lo, cap = kt->a.bin_cap;
            const uint32_t gmin_c = kt->ga.g.gmin;
            if (kt->a.bin_rec32 != 0u) {                                       // (uniform)
                uint32_t* const dst = reinterpret_cast<uint32_t*>(kt->a.bins) + (size_t)bn * cap;
                bool wide = false;
                for (uint32_t i = tid; i < nrec; i += QS_WG) {
                    const uint32_t doc = recs[i] + gmin_c;
                    if (base + i < cap) {
                        wide = wide || (doc >> (32u - QS_SHARE_BQ)) != 0u || doc == (0xFFFFFFFFu >> QS_SHARE_BQ);
                        dst[base + i] = (doc << QS_SHARE_BQ) | (q & ((1u << QS_SHARE_BQ) - 1u));
                    }
                }
                if (wide) atomicMax(&kt->a.counters[CTR_BINFAIL], 3ull);
            } else {
                uint64_t* const dst = kt->a.bins + (size_t)bn * cap;
                for (uint32_t i = tid; i < nrec; i += QS_WG)
                    if (base + i < cap) dst[base + i] = ((uint64_t)q << 32) | (uint32_t)(recs[i] + gmin_c);
            }
        }
    } else
    if (!low_q && s_over_recs == 0u && !q_redo && nrec != 0u && nrec >= floor_q) {
        if (tid == 0) { s_claimed = 0u; s_full = 0u; }
        __syncthreads();                                // (the filter's counts are complete behind this barrier)
        // (a) the SWEEP: four records per lane and turn and their four cells, nothing else -- a record whose cell reaches the floor is a
        // bit of the lane's mask, bit 4 turn + u for record turn * 4 QS_WG + 4 tid + u.  Made once per query (and class): the filter does
        // not change between the passes.  Only the query's last turn tests record by record.
        static_assert((QS_REC_CAP + QS_WG * 4u - 1u) / (QS_WG * 4u) <= 8u, "a lane's turns over a query's records: at most 8, four bits of its mask each");
        uint32_t surv = 0u;
        uint32_t t4 = tid * 4u;
        asm volatile("" : "+v"(t4));
        for (uint32_t i4 = t4, sh = 0u; i4 < nrec; i4 += QS_WG * 4u, sh += 4u) {
            const uint4 r4 = *reinterpret_cast<const uint4*>(recs + i4);
            const uint32_t r[4] = {r4.x, r4.y, r4.z, r4.w};
            uint32_t cnt4[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) { const uint32_t c = qs_cell(r[u]); cnt4[u] = (filter[c >> 1] >> (16u * (c & 1u))) & 0xFFFFu; }
            uint32_t m4 = 0u;
            if (i4 + 3u < nrec) {
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) m4 |= (cnt4[u] >= floor_q ? 1u : 0u) << u;
            } else {
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) m4 |= (i4 + u < nrec && cnt4[u] >= floor_q ? 1u : 0u) << u;
            }
            surv |= m4 << sh;
        }
        uint32_t passes = 1u;
        for (uint32_t pass = 0; pass < passes; ++pass) {
            // (b) the DRAIN: a lane with a bit left takes its lowest one, reads that record back and counts it in the table; the wave
            // makes as many trips as its fullest lane has bits.  Every pass drains a copy of the mask.
            for (uint32_t left = surv; __ballot((int)(left != 0u)) != 0ull;) {
                if (left != 0u) {
                    const uint32_t bit = (uint32_t)__builtin_ctz(left);
                    left &= left - 1u;
                    const uint32_t doc = recs[(bit >> 2) * (QS_WG * 4u) + t4 + (bit & 3u)];
                    const uint32_t h2 = mix32(doc);
                    if (passes == 1u || (h2 >> 16) % passes == pass) {
                        const unsigned long long keyhi = (unsigned long long)doc << 32;
                        uint32_t s = h2 & TMASK;
                        for (uint32_t tries = 0;; ++tries) {
                            if (tries == T) { s_full = 1u; break; }
                            unsigned long long cur = table[s];
                            if (cur == 0ull) {
                                const unsigned long long prev = atomicCAS(&table[s], 0ull, keyhi | 1ull);
                                if (prev == 0ull) { atomicAdd(&s_claimed, 1u); break; }
                                cur = prev;
                            }
                            if ((cur >> 32) == (keyhi >> 32)) { atomicAdd(&table[s], 1ull); break; }
                            s = (s + 1u) & TMASK;
                        }
                    }
                }
            }
            __syncthreads();
            if (pass == 0u && (s_claimed > T * 3u / 4u || s_full != 0u) && passes < 64u) {
                __syncthreads();                        // (everybody has read the flags)
                for (uint32_t s = tid; s < T; s += QS_WG) table[s] = 0ull;
                if (tid == 0) { s_claimed = 0u; s_full = 0u; }
                passes *= 2u; pass = 0xFFFFFFFFu;       // (++pass: 0 again; nothing has been emitted yet)
                __syncthreads();
                continue;
            }
            const qs_kargs_t kc = qs_cold_args();
            if (s_full != 0u && tid == 0) atomicMax(&kc->a.counters[CTR_BINFAIL], 1ull);
            const uint32_t gmin_c = kc->ga.g.gmin;
            // candidates: count >= the floor -> the query's buffer in LDS (its first SB_CAND), the rest to the shared list
            for (uint32_t s = tid; s < T; s += QS_WG) {
                const unsigned long long e = table[s];
                if (e == 0ull) continue;
                const uint32_t count = (uint32_t)e, doc = gmin_c + (uint32_t)(e >> 32);       // (the table's key is doc - gmin)
                if (count < floor_q) continue;
                if ((uint64_t)count > smax) atomicMax(&kc->a.counters[CTR_MAXSCORE], (unsigned long long)count);
                const uint64_t sc = (uint64_t)count > smax ? smax : (uint64_t)count;
                const uint64_t qpart = sb >= 32u ? 0ull : ((uint64_t)q << (32u + sb));
                const uint64_t key = qpart | ((smax - sc) << 32) | doc;
                const uint32_t at = atomicAdd(&s_ccnt, 1u);
                if (at < SB_CAND) cbuf[at] = key;
                else {
                    const unsigned long long gi = atomicAdd(&kc->a.counters[CTR_CANDS], 1ull);
                    if (gi < kc->a.cand_cap) kc->a.cands[gi] = key;
                    s_cshared = 1u;
                }
            }
            if (pass + 1u < passes) {                   // (the next pass's table and flags)
                __syncthreads();
                for (uint32_t s = tid; s < T; s += QS_WG) table[s] = 0ull;
                if (tid == 0) { s_claimed = 0u; s_full = 0u; }
                __syncthreads();
            }
        }
    }
  }   // (the classes: one pass unless CLS.  The candidates of all of them are in the buffer and the shared list: s_ccnt was not reset)
    // ---- hand-over: up to QCAND_SLOTS candidates stay in the query's own slots, more move to the shared list entirely
    __syncthreads();
    QS_MARK(4);
    const uint32_t cn = min(s_ccnt, SB_CAND);
    (void)cn;
    if constexpr (SHARE) {
        // (no candidates: the query's slots and their count are not this kernel's -- the members carry the bins)
    } else if constexpr (NEXT) {
        const qs_kargs_t kh = qs_cold_args();
        // ---- (NEXT) the CHAINED hand-over.  prev: what the launch before on this stream left for the query -- a kernel boundary lies
        //      between, a plain load sees it.  (1) prev overflowed: this launch's candidates follow the others into the shared list, the
        //      mark stays.  (2) nothing of the query went to the shared list here and prev + cn fit the slots: slots [prev, prev + cn).
        //      (3) the query overflows NOW: its prev slots and the buffer's cn move to the shared list together, one reservation.
        //      prev indexes nothing unchecked: a workgroup of the first launch that returned at its cancel point wrote no count (a fresh
        //      allocation may hold anything) -- whatever is neither the mark nor a count of slots is taken for full slots.
        //      (s_claimed and s_full are the counting passes' and idle here: the carried count and the case, for the workgroup)
        if (tid == 0) {
            uint32_t prev = kh->a.qcand_n[q];
            const bool was = prev == QCAND_OVERFLOWED;
            prev = was ? 0u : min(prev, QCAND_SLOTS);
            const bool to_slots = !was && s_cshared == 0u && prev + cn <= QCAND_SLOTS;
            if (!to_slots) {
                if (prev + cn != 0u) {
                    const unsigned long long gi = atomicAdd(&kh->a.counters[CTR_CANDS], (unsigned long long)(prev + cn));
                    s_cbase_lo = (uint32_t)gi; s_cbase_hi = (uint32_t)(gi >> 32);
                }
                if (!was) kh->a.qcand_n[q] = QCAND_OVERFLOWED;
            } else kh->a.qcand_n[q] = prev + cn;
            s_claimed = prev; s_full = to_slots ? 1u : 0u;
        }
        __syncthreads();
        const uint32_t prev = s_claimed;
        const bool to_slots = s_full != 0u;
        const uint64_t base = ((uint64_t)s_cbase_hi << 32) | s_cbase_lo;
        if (tid < cn) {
            const uint64_t key = cbuf[tid];
            if (to_slots) kh->a.qcand[(size_t)q * QCAND_SLOTS + prev + tid] = key;      // (prev + cn <= QCAND_SLOTS)
            else if (base + tid < kh->a.cand_cap) kh->a.cands[base + tid] = key;
        }
        static_assert(SB_CAND + QCAND_SLOTS <= QS_WG, "the carried slots move by lanes of their own");
        if (const uint32_t t = tid - SB_CAND; !to_slots && t < prev) {                   // (prev <= QCAND_SLOTS; tid < SB_CAND wraps to a large t)
            const uint64_t gi = base + cn + t;
            if (gi < kh->a.cand_cap) kh->a.cands[gi] = kh->a.qcand[(size_t)q * QCAND_SLOTS + t];
        }
    } else {
    const bool shared = s_cshared != 0u || cn > QCAND_SLOTS;
    const qs_kargs_t kh = qs_cold_args();
    if (tid == 0) {
        if (shared && cn != 0u) {
            const unsigned long long gi = atomicAdd(&kh->a.counters[CTR_CANDS], (unsigned long long)cn);
            s_cbase_lo = (uint32_t)gi; s_cbase_hi = (uint32_t)(gi >> 32);
        }
        kh->a.qcand_n[q] = shared ? QCAND_OVERFLOWED : cn;
    }
    __syncthreads();
    if (tid < cn) {
        const uint64_t key = cbuf[tid];
        if (!shared) kh->a.qcand[(size_t)q * QCAND_SLOTS + tid] = key;
        else {
            const uint64_t gi = (((uint64_t)s_cbase_hi << 32) | s_cbase_lo) + tid;
            if (gi < kh->a.cand_cap) kh->a.cands[gi] = key;
        }
    }
    }
    QS_MARK(5);
    if constexpr (CLS) {                                // the workgroup's next entry of the redo list
        ent += gridDim.x;
        if (ent >= a.q_end) break;
        take_entry();
        const uint64_t q_lo = a.offsets[q];
        n = (uint32_t)(a.offsets[q + 1] - q_lo);
        qh = a.hashes_base + q_lo;
        load_pair(qh, n, 0u, hq[0], hq[1]);
        load_pair(qh, n, 1u, hq[2], hq[3]);
        ask_cancel();
    } else {
        if (!has_next) break;
        q = qn; n = nn; qh = a.hashes_base + nq_lo;
        qn = q2; nn = 0u; nq_lo = 0;
        if (has_q2) {
            nq_lo = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(o2_lo >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)o2_lo);
            nn = (uint32_t)__builtin_amdgcn_readfirstlane((int)(o2_hi - (uint32_t)o2_lo));
        }
    }
    __syncthreads();                                    // (the candidate buffer and the flags have been read: the next query may reset them)
  }
}

// The ten kernels (the head comment's table): a wrapper names what is on.
template <int NS, bool QS, bool MEM, bool FILT>
__global__ __launch_bounds__(QS_WG) FPX_QS_OCC void k_search_query(QSearchArgs a, GroupArgs ga)
{
    qs_body<qs_variant<NS, QS, MEM, FILT>>(a, ga);
}
template <int NS, bool MEM>
__global__ __launch_bounds__(QS_WG) FPX_QS_OCC void k_search_classes(QSearchArgs a, GroupArgs ga)
{
    qs_body<qs_variant<NS, true, MEM, false, QS_F_CLS>>(a, ga);
}
template <int NS, bool QS, bool MEM>
__global__ __launch_bounds__(QS_WG) FPX_QS_OCC void k_search_low(QSearchArgs a, GroupArgs ga)
{
    qs_body<qs_variant<NS, QS, MEM, false, QS_F_LOW>>(a, ga);
}
template <int NS, bool QS, bool MEM>
__global__ __launch_bounds__(QS_WG) FPX_QS_OCC void k_search_low_filt(QSearchArgs a, GroupArgs ga)
{
    qs_body<qs_variant<NS, QS, MEM, true, QS_F_LOW>>(a, ga);
}
template <int NS, bool QS, bool MEM>
__global__ __launch_bounds__(QS_WG) FPX_QS_OCC void k_search_filt(QSearchArgs a, GroupArgs ga)
{
    qs_body<qs_variant<NS, QS, MEM, true, QS_F_COOP>>(a, ga);
}
template <int NS, bool QS, bool MEM>
__global__ __launch_bounds__(QS_WG) FPX_QS_OCC void k_search_low_coop(QSearchArgs a, GroupArgs ga)
{
    qs_body<qs_variant<NS, QS, MEM, true, QS_F_LOW | QS_F_COOP>>(a, ga);
}
template <int NS, bool QS, bool FILT>
__global__ __launch_bounds__(QS_WG) FPX_QS_OCC void k_search_next(QSearchArgs a, GroupArgs ga)
{
    qs_body<qs_variant<NS, QS, false, FILT, QS_F_NEXT>>(a, ga);
}
template <int NS, bool QS, bool FILT>
__global__ __launch_bounds__(QS_WG) FPX_QS_OCC void k_search_low_next(QSearchArgs a, GroupArgs ga)
{
    qs_body<qs_variant<NS, QS, false, FILT, QS_F_LOW | QS_F_NEXT>>(a, ga);
}
template <int NS, bool MEM, bool FILT>
__global__ __launch_bounds__(QS_WG) FPX_QS_OCC void k_search_window(QSearchArgs a, GroupArgs ga)
{
    qs_body<qs_variant<NS, false, MEM, FILT, QS_F_SHARE>>(a, ga);
}
template <int NS, bool MEM, bool FILT>
__global__ __launch_bounds__(QS_WG) FPX_QS_OCC void k_search_packed(QSearchArgs a, GroupArgs ga)
{
    qs_body<qs_variant<NS, false, MEM, FILT, QS_F_SHARE | QS_F_PACK>>(a, ga);
}

// zeroes what a batch of k_search_query adds to: the batch's counters and the statistics sets (one launch instead of two memsets)
__global__ __launch_bounds__(256) void k_qs_zero(unsigned long long* counters, unsigned int* words, uint32_t nwords)
{
    const uint32_t i0 = blockIdx.x * 256u + threadIdx.x;
    if (i0 < CTR_COUNT) counters[i0] = 0ull;
    for (uint32_t i = i0; i < nwords; i += gridDim.x * 256u) words[i] = 0u;
}

}  // namespace fpx
