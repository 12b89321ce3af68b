// fpx_qframe.hpp -- the frame that k_search_side (fpx_qside.hpp) and k_search_words (fpx_qwords.hpp) stand in: everything of a
// query-per-workgroup kernel except its walk.  The LDS layout, the arguments every such kernel takes, the workgroup's state, and over that
// state: the query's reset and cancel point, the hash set of dedupSorted (src/Index.zig:489-499), the records' reservations, the query's
// statistics, and the tail -- SearchResults.incr and the min_score filter of finish (src/common.zig:121-145), the candidate buffer, the
// hand-over to k_finish -- with the workgroup's statistics flush behind it.  A kernel reads: frame set-up, its walk, frame tail.
// Part of the fpx_search.hip translation unit (after fpx_qsearch.hpp, whose layout, counting and candidate format these are).
//
// What is NOT here, and why:
//  - k_search_query (fpx_qsearch.hpp) keeps its own copy of all of this: its tail reads its arguments through qs_cold_args(), has the next
//    query's loads threaded through it and carries the CLS and LOW forms.  QSearchArgs keeps its own members for the same reason
//    (qs_cold_args() reads the kernel-argument segment by that struct's layout).
//  - dedupSorted's loop over a lane's rounds stays in the kernels, around qf_later_occurrence: k_search_words requests the memory table's
//    filter word BEFORE the set is probed, so that it arrives under the probe, and tests the hash window after it; a hook called for a
//    first occurrence would move that load behind the probe.
//  - tot_bytes, the sum of the visited blocks' sizes, is k_search_side's own (its segments differ in block size; a group has one): the
//    kernels hand qf_flush what their blocks cost beyond 512 bytes each.
//  - k_search_words' `reserve` (a round's records, placed by a scan) and its memory-table lookup (a copy of qs_body's) belong to its walk.
#pragma once
#include <hip/hip_runtime.h>

#include "fpx_internal.h"

namespace fpx {

constexpr uint32_t QF_WG = 256;
constexpr uint32_t QF_REC_CAP = 8192;              // records of a query held in LDS; before: the query's hash set
constexpr uint32_t QF_WGS_PER_CU = 4;              // (LDS: 39 KB per workgroup)
// the dynamic LDS of a workgroup: [records + four spare words | filter | exact table | candidate buffer]
struct QFrameLds {
    uint32_t recs[QF_REC_CAP + 4u];                // docs (+ four spare words)
    uint32_t filter[1u << (QS_FLOG2 - 1u)];        // words of two cells
    unsigned long long table[1u << QS_TLOG2];      // doc << 32 | count
    uint64_t cbuf[SB_CAND];
};
constexpr size_t QF_LDS_BYTES = sizeof(QFrameLds);
static_assert(QF_LDS_BYTES == QS_LDS_BYTES && QF_REC_CAP == QS_REC_CAP && QF_WG == QS_WG, "k_search_query's layout");
static_assert(QS_MAX_HASHES * 2u <= QF_REC_CAP, "the dedup set lives where the records will");
static_assert((QS_MAX_HASHES + QF_WG - 1u) / QF_WG <= 32u, "a lane remembers which of its rounds' hashes are probes in one word");

// what every such kernel is told (SideArgs and WordsArgs begin with it)
struct QFrameArgs {
    const uint32_t* hashes_base; const uint64_t* offsets;      // hashes_base[i]: the hash at ABSOLUTE position i of the batch; offsets[q] absolute
    const uint32_t* opts;                                      // [B][4]: max_results, floor, pct, raw length
    uint32_t B, sb;                                            // queries; bits of the score field in a candidate key
    uint64_t* cands; uint64_t cand_cap;                        // the shared candidate list (queries with more candidates than slots)
    uint64_t* qcand; uint32_t* qcand_n;                        // the queries' own candidate slots
    unsigned long long* counters;
    unsigned long long* stat_sets;                             // [LEAN_STAT_SETS][8] statistics + [LEAN_STAT_SETS][HIST_SLOTS] histogram slots
    unsigned long long* qstats;                                // [B] blocks | docs << 32, or null
    const uint32_t* cancel;
};

// the workgroup's state: ONE __shared__ object of each kernel.  (The order of the words: s_claimed | s_full and s_ccnt | s_cshared are
// zeroed together; as neighbours each pair became ONE 64-bit store, and the compiler kept a pair of zero registers for them through the
// whole kernel -- two vector registers more in the filtered k_search_words)
struct QFrame {
    uint32_t s_count, s_over_recs, s_seen_ones, s_cancel, s_claimed, s_ccnt, s_full, s_cshared, s_cbase_lo, s_cbase_hi;
    unsigned long long wg_blocks, wg_docs;                                                   // the query's
    unsigned long long tot_blocks, tot_docs, tot_probes, tot_reads, tot_recs;                // the workgroup's, over all its queries
    uint32_t wg_h[HIST_SLOTS];                                                               // ... and its scan histogram slots (hist_observe)
};
// a query as its workgroup sees it: n hashes at qh, a hash per lane in each of `rounds`, a hash set of 2^sbits slots
struct QFrameQuery { const uint32_t* qh; uint32_t n, rounds, sbits; bool cancelled; };

// once per kernel, before the first query
__device__ __forceinline__ void qf_init(QFrame& fr, uint32_t tid)
{
    if (tid < HIST_SLOTS) fr.wg_h[tid] = 0u;
    if (tid == 0) { fr.tot_blocks = 0; fr.tot_docs = 0; fr.tot_probes = 0; fr.tot_reads = 0; fr.tot_recs = 0; }
}

// one record of some lanes of the wave: ONE reservation per wave (a lane's own atomic on the one counter is compiled into a serial loop
// over the wave's lanes: experiments/README.md)
__device__ __forceinline__ void qf_emit1(QFrame& fr, QFrameLds& L, uint32_t lane, bool kp, uint32_t doc)
{
    const unsigned long long m = __ballot((int)kp);
    if (m == 0ull) return;
    uint32_t base = 0;
    if (lane == (uint32_t)__builtin_ctzll(m)) base = atomicAdd(&fr.s_count, (uint32_t)__popcll(m));
    base = __shfl(base, (int)__builtin_ctzll(m));
    if (kp) {
        const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (at < QF_REC_CAP) L.recs[at] = doc; else fr.s_over_recs = 1u;       // (more records than the array takes: the host redoes the batch or part on the pipeline)
    }
}
__device__ __forceinline__ unsigned long long qf_wave_total(uint32_t v)
{
    const uint32_t incl = scan16(v);                                     // (the whole wave is here)
    return (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)incl, 15) + (uint32_t)__builtin_amdgcn_readlane((int)incl, 31) +
           (uint32_t)__builtin_amdgcn_readlane((int)incl, 47) + (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
}

// the head of a query: its hashes, the LDS reset, the cancel point (cancelled: the kernel returns)
__device__ __forceinline__ QFrameQuery qf_begin_query(QFrame& fr, QFrameLds& L, const QFrameArgs& a, uint32_t q, uint32_t tid)
{
    constexpr uint32_t T = 1u << QS_TLOG2;
    const uint64_t q_lo = a.offsets[q];
    const uint32_t n_raw = (uint32_t)(a.offsets[q + 1] - q_lo);
    const bool too_long = n_raw > QS_MAX_HASHES;          // (the host takes no such batch; a query that long would overrun its hash set)
    const uint32_t n = too_long ? 0u : n_raw;
    const uint32_t* qh = a.hashes_base + q_lo;
    const uint32_t rounds = (n + QF_WG - 1u) / QF_WG;
    // the query's hash set: 2^sbits >= 2 n slots
    uint32_t sbits = 8u;
    while ((1u << sbits) < 2u * n) ++sbits;
    __syncthreads();                                    // (the query before: its candidate buffer and flags have been read)
    for (uint32_t i = tid; i < (1u << sbits); i += QF_WG) L.recs[i] = 0xFFFFFFFFu;
    for (uint32_t i = tid; i < (1u << (QS_FLOG2 - 1u)); i += QF_WG) L.filter[i] = 0u;
    for (uint32_t s = tid; s < T; s += QF_WG) L.table[s] = 0ull;
    if (tid == 0) {
        fr.s_count = 0u; fr.s_over_recs = too_long ? 1u : 0u; fr.s_seen_ones = 0u; fr.s_ccnt = 0u; fr.s_cshared = 0u;
        fr.wg_blocks = 0; fr.wg_docs = 0;
        fr.s_cancel = cancel_requested(a.cancel, a.counters) ? 1u : 0u;      // cancel point (src/FileSegment.zig:144), once per query
    }
    __syncthreads();
    return QFrameQuery{qh, n, rounds, sbits, fr.s_cancel != 0u};
}

// dedupSorted (src/Index.zig:171-172,489-499), one hash: the first occurrence of a hash is the probe, later ones are dropped
__device__ __forceinline__ bool qf_later_occurrence(QFrame& fr, QFrameLds& L, uint32_t sbits, uint32_t h)
{
    bool dup;
    if (h == 0xFFFFFFFFu) dup = atomicExch(&fr.s_seen_ones, 1u) != 0u;     // (the set's empty mark is kept apart)
    else {
        uint32_t slot = (h * 0x9E3779B1u) >> (32u - sbits);
        for (;;) {
            const uint32_t old = atomicCAS(&L.recs[slot], 0xFFFFFFFFu, h);
            if (old == 0xFFFFFFFFu) { dup = false; break; }
            if (old == h) { dup = true; break; }
            slot = (slot + 1u) & ((1u << sbits) - 1u);
        }
    }
    return dup;
}

// the query's statistics (what FileSegment.search observes per hash, summed: src/FileSegment.zig:177-178): a wave's totals
__device__ __forceinline__ void qf_query_stats(QFrame& fr, uint32_t lane, unsigned long long w_reads, unsigned long long w_blocks, unsigned long long w_docs,
                                               unsigned long long w_probes)
{
    if (lane == 0u) {
        if (w_reads) atomicAdd(&fr.tot_reads, w_reads);
        if (w_blocks) { atomicAdd(&fr.wg_blocks, w_blocks); atomicAdd(&fr.tot_blocks, w_blocks); }
        if (w_docs) { atomicAdd(&fr.wg_docs, w_docs); atomicAdd(&fr.tot_docs, w_docs); }
        if (w_probes) atomicAdd(&fr.tot_probes, w_probes);
    }
}

// the tail of a query, behind its walk: the records counted, those at the floor counted exactly, the candidates handed over
__device__ __forceinline__ void qf_count_and_hand_over(QFrame& fr, QFrameLds& L, const QFrameArgs& a, uint32_t q, uint32_t tid)
{
    constexpr uint32_t T = 1u << QS_TLOG2, TMASK = T - 1u;
    uint32_t* const recs = L.recs;
    uint32_t* const filter = L.filter;
    unsigned long long* const table = L.table;
    uint64_t* const cbuf = L.cbuf;
    __syncthreads();                                    // (the records are complete)
    const uint32_t nrec = min(fr.s_count, QF_REC_CAP);
    // ---- SearchResults.incr (src/common.zig:121-129), first the filter: every record into its doc's cell
    for (uint32_t i = tid * 4u; i < nrec; i += QF_WG * 4u) {
        const uint4 r4 = *reinterpret_cast<const uint4*>(recs + i);             // (the array ends with four spare words)
        const uint32_t r[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
            const uint32_t c = qs_cell(r[u]);
            if (i + u < nrec) atomicAdd(&filter[c >> 1], 1u << (16u * (c & 1u)));
        }
    }
    if (tid == 0) {
        fr.tot_recs += (unsigned long long)fr.s_count;                          // the query's hit records
        if (a.qstats) a.qstats[q] = fr.wg_blocks | (fr.wg_docs << 32);
        if (fr.s_over_recs || fr.s_count > QF_REC_CAP) atomicMax(&a.counters[CTR_BINFAIL], 1ull);
    }
    // ---- ... then the floor of finish (src/common.zig:131-145): a doc can only reach the floor if its cell did; those records are
    //      counted exactly, in `passes` loads over classes of them when they are more than the table takes
    const uint32_t floor_q = a.opts[q * 4u + 1u];
    const uint32_t sb = a.sb;
    const uint64_t smax = sb >= 32u ? 0xFFFFFFFFull : ((1ull << sb) - 1ull);
    if (fr.s_over_recs == 0u && nrec != 0u && nrec >= floor_q) {
        uint32_t passes = 1u;
        for (uint32_t pass = 0; pass < passes; ++pass) {
            if (pass != 0u) {
                __syncthreads();
                for (uint32_t s = tid; s < T; s += QF_WG) table[s] = 0ull;
            }
            if (tid == 0) { fr.s_claimed = 0u; fr.s_full = 0u; }
            __syncthreads();                            // (the first pass: the filter's counts are complete behind this barrier)
            for (uint32_t i4 = tid * 4u; i4 < nrec; i4 += QF_WG * 4u) {
                const uint4 r4 = *reinterpret_cast<const uint4*>(recs + i4);
                const uint32_t r[4] = {r4.x, r4.y, r4.z, r4.w};
                uint32_t cnt4[4];
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) { const uint32_t c = qs_cell(r[u]); cnt4[u] = (filter[c >> 1] >> (16u * (c & 1u))) & 0xFFFFu; }
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) {
                    const uint32_t doc = r[u];
                    if (i4 + u >= nrec || cnt4[u] < floor_q) continue;
                    const uint32_t h2 = mix32(doc);
                    if (passes > 1u && (h2 >> 16) % passes != pass) continue;
                    const unsigned long long keyhi = (unsigned long long)doc << 32;
                    uint32_t s = h2 & TMASK;
                    for (uint32_t tries = 0;; ++tries) {
                        if (tries == T) { fr.s_full = 1u; break; }
                        unsigned long long cur = table[s];
                        if (cur == 0ull) {
                            const unsigned long long prev = atomicCAS(&table[s], 0ull, keyhi | 1ull);
                            if (prev == 0ull) { atomicAdd(&fr.s_claimed, 1u); break; }
                            cur = prev;
                        }
                        if ((cur >> 32) == (keyhi >> 32)) { atomicAdd(&table[s], 1ull); break; }
                        s = (s + 1u) & TMASK;
                    }
                }
            }
            __syncthreads();
            if (pass == 0u && (fr.s_claimed > T * 3u / 4u || fr.s_full != 0u) && passes < 64u) {
                const uint32_t np = passes * 2u;
                __syncthreads();
                for (uint32_t s = tid; s < T; s += QF_WG) table[s] = 0ull;
                passes = np; pass = 0xFFFFFFFFu;           // (++pass: 0 again; nothing has been emitted yet)
                continue;
            }
            if (fr.s_full != 0u && tid == 0) atomicMax(&a.counters[CTR_BINFAIL], 1ull);
            // candidates: count >= the floor -> the query's buffer in LDS (its first SB_CAND), the rest to the shared list
            for (uint32_t s = tid; s < T; s += QF_WG) {
                const unsigned long long e = table[s];
                if (e == 0ull) continue;
                const uint32_t count = (uint32_t)e, doc = (uint32_t)(e >> 32);
                if (count < floor_q) continue;
                if ((uint64_t)count > smax) atomicMax(&a.counters[CTR_MAXSCORE], (unsigned long long)count);
                const uint64_t sc = (uint64_t)count > smax ? smax : (uint64_t)count;
                const uint64_t qpart = sb >= 32u ? 0ull : ((uint64_t)q << (32u + sb));
                const uint64_t key = qpart | ((smax - sc) << 32) | doc;
                const uint32_t at = atomicAdd(&fr.s_ccnt, 1u);
                if (at < SB_CAND) cbuf[at] = key;
                else {
                    const unsigned long long gi = atomicAdd(&a.counters[CTR_CANDS], 1ull);
                    if (gi < a.cand_cap) a.cands[gi] = key;
                    fr.s_cshared = 1u;
                }
            }
        }
    }
    // ---- hand-over: up to QCAND_SLOTS candidates stay in the query's own slots, more move to the shared list entirely
    __syncthreads();
    const uint32_t cn = min(fr.s_ccnt, SB_CAND);
    const bool shared = fr.s_cshared != 0u || cn > QCAND_SLOTS;
    if (tid == 0) {
        if (shared && cn != 0u) {
            const unsigned long long gi = atomicAdd(&a.counters[CTR_CANDS], (unsigned long long)cn);
            fr.s_cbase_lo = (uint32_t)gi; fr.s_cbase_hi = (uint32_t)(gi >> 32);
        }
        a.qcand_n[q] = shared ? QCAND_OVERFLOWED : cn;
    }
    __syncthreads();
    if (tid < cn) {
        const uint64_t key = cbuf[tid];
        if (!shared) a.qcand[(size_t)q * QCAND_SLOTS + tid] = key;
        else {
            const uint64_t gi = (((uint64_t)fr.s_cbase_hi << 32) | fr.s_cbase_lo) + tid;
            if (gi < a.cand_cap) a.cands[gi] = key;
        }
    }
}

// the workgroup's statistics, once, behind a barrier after its last query: its set of the spread statistics (the host prices the sets'
// blocks at 512 bytes; blocks of another size add the difference -- mod 2^64, bytes_off: the kernel's to say -- to slot 5) and the scan
// histograms' slots behind them
__device__ __forceinline__ void qf_flush(QFrame& fr, const QFrameArgs& a, uint32_t tid, unsigned long long bytes_off)
{
    if (tid == 0) {
        unsigned long long* st = a.stat_sets + (size_t)(blockIdx.x % LEAN_STAT_SETS) * 8u;
        if (fr.tot_reads) atomicAdd(&st[4], fr.tot_reads);
        if (fr.tot_blocks) atomicAdd(&st[1], fr.tot_blocks);
        if (bytes_off) atomicAdd(&st[5], bytes_off);
        if (fr.tot_docs) atomicAdd(&st[2], fr.tot_docs);
        if (fr.tot_probes) atomicAdd(&st[3], fr.tot_probes);
        if (fr.tot_recs) atomicAdd(&st[7], fr.tot_recs);
    }
    if (tid < HIST_SLOTS - 1u) {                             // (slot 15: hist_observe's sink)
        const unsigned long long v = tid == HIST_COUNT ? fr.tot_probes : tid == HIST_DOCS ? fr.tot_docs : tid == HIST_BLOCKS ? fr.tot_blocks : (unsigned long long)fr.wg_h[tid];
        if (v != 0ull) atomicAdd(&a.stat_sets[(size_t)LEAN_STAT_SETS * 8u + (size_t)(blockIdx.x % LEAN_STAT_SETS) * HIST_SLOTS + tid], v);
    }
}

}  // namespace fpx
