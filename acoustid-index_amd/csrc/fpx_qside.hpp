// fpx_qside.hpp -- k_search_side: the file segments NEXT TO the group of a live index -- fresh checkpoints kept decoded (fpx_probe_small.hpp),
// a merged segment that is direct-addressed on its own (fpx_direct.hpp) -- searched ONE QUERY PER WORKGROUP, as k_search_query
// (fpx_qsearch.hpp) searches the group: dedupSorted (src/Index.zig:489-499), FileSegment.search for every side segment
// (src/FileSegment.zig:135-180), SearchResults.incr and the min_score filter of finish (src/common.zig:121-145) in one kernel.
// Part of the fpx_search.hip translation unit (after fpx_qsearch.hpp, whose LDS layout, counting and candidate hand-over it copies).
//
// The pipeline runs keys, a radix pass, k_probe_small, k_probe_direct, the partition and k_score over ALL the batch's hashes to bring the
// few thousand records these segments hold for a batch.  Here a workgroup owns a query and stays (every gridDim.x-th query): the query's
// hashes go into a hash set in LDS, every unique hash is a lane's, looked up in every side segment in turn -- the first loads of a chunk
// of segments out together --, the docs are appended to a record array in LDS (absolute doc ids), counted in a filter of 16-bit cells and,
// where a cell reaches the query's floor, exactly in a small table; candidates leave in k_search_query's format for k_finish.
//
// Taken by run_batch (option side_wg = 1) for a snapshot -- a part 1, or a whole young index -- that holds small decoded and
// direct-addressed-alone segments only, nothing of them a hash-window slice.  The record array holds SIDE_REC_CAP = 8192 docs: what the
// dedup set of the longest query taken needs anyway (2 x QS_MAX_HASHES slots).  The reference's caps let ONE hash bring up to 1000 docs
// plus a block's worth from ONE segment (src/FileSegment.zig:171-174), so a single hot hash fits several times over next to a query's
// ordinary records (a handful per query of a live index); a query with eight or more such hashes does not, raises CTR_BINFAIL, and the
// host redoes that snapshot or part on the pipeline (FPX_REDO_QS) -- sizing the array for 4096 hot hashes is not possible in LDS.
#pragma once
#include <hip/hip_runtime.h>

#include "fpx_internal.h"

namespace fpx {

constexpr uint32_t SIDE_WG = 256;
constexpr uint32_t SIDE_REC_CAP = 8192;            // records of a query held in LDS; before: the query's hash set
constexpr uint32_t SIDE_SMALL_CH = 4;              // small segments whose loads are under way together
constexpr uint32_t SIDE_SOLO_CH = 2;               // direct-addressed segments likewise
constexpr uint32_t SIDE_WGS_PER_CU = 4;            // (LDS: 39 KB per workgroup)
// [records + four spare words | filter | exact table | candidate buffer]
constexpr size_t SIDE_LDS_BYTES = ((size_t)SIDE_REC_CAP + 4u) * 4u + ((size_t)2u << QS_FLOG2) + ((size_t)8u << QS_TLOG2) + (size_t)SB_CAND * 8u;
static_assert(QS_MAX_HASHES * 2u <= SIDE_REC_CAP, "the dedup set lives where the records will");
static_assert((QS_MAX_HASHES + SIDE_WG - 1u) / SIDE_WG <= 32u, "a lane remembers which of its rounds' hashes are probes in one word");

struct SideArgs {
    const uint32_t* hashes_base; const uint64_t* offsets;      // hashes_base[i]: the hash at ABSOLUTE position i of the batch; offsets[q] absolute
    const uint32_t* opts;                                      // [B][4]: max_results, floor, pct, raw length
    uint32_t B, sb;                                            // queries; bits of the score field in a candidate key
    uint64_t* cands; uint64_t cand_cap;                        // the shared candidate list (queries with more candidates than slots)
    uint64_t* qcand; uint32_t* qcand_n;                        // the queries' own candidate slots
    unsigned long long* counters;
    unsigned long long* stat_sets;                             // [LEAN_STAT_SETS][8] statistics + [LEAN_STAT_SETS][HIST_SLOTS] histogram slots
    unsigned long long* qstats;                                // [B] blocks | docs << 32, or null
    const uint32_t* cancel;
    const SegDesc* small; uint32_t n_small;                    // the snapshot's small decoded segments (Snapshot::d_small)
    const SegDesc* solo; uint32_t n_solo;                      // ... and its direct-addressed segments outside any group (Snapshot::d_solo)
};

__global__ __launch_bounds__(SIDE_WG) void k_search_side(SideArgs a)
{
    constexpr uint32_t T = 1u << QS_TLOG2, TMASK = T - 1u;
    extern __shared__ __align__(16) uint8_t side_dyn[];
    uint32_t* const recs = reinterpret_cast<uint32_t*>(side_dyn);                                       // [SIDE_REC_CAP] docs (+ four spare words)
    uint32_t* const filter = recs + SIDE_REC_CAP + 4u;                                                  // 2^(QS_FLOG2 - 1) words of two cells
    unsigned long long* const table = reinterpret_cast<unsigned long long*>(filter + (1u << (QS_FLOG2 - 1u)));
    uint64_t* const cbuf = reinterpret_cast<uint64_t*>(table + T);                                      // [SB_CAND]
    __shared__ uint32_t s_count, s_over_recs, s_seen_ones, s_cancel, s_claimed, s_full, s_ccnt, s_cshared, s_cbase_lo, s_cbase_hi;
    __shared__ unsigned long long wg_blocks, wg_docs;                                                   // the query's
    __shared__ unsigned long long tot_blocks, tot_docs, tot_probes, tot_reads, tot_bytes, tot_recs;     // the workgroup's, over all its queries
    __shared__ uint32_t wg_h[HIST_SLOTS];                                                               // ... and its scan histogram slots (hist_observe)

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < HIST_SLOTS) wg_h[tid] = 0u;
    if (tid == 0) { tot_blocks = 0; tot_docs = 0; tot_probes = 0; tot_reads = 0; tot_bytes = 0; tot_recs = 0; }

    // one record of some lanes of the wave: ONE reservation per wave (a lane's own atomic on the one counter is compiled into a serial loop
    // over the wave's lanes: experiments/README.md)
    auto emit1 = [&](bool kp, uint32_t doc) {
        const unsigned long long m = __ballot((int)kp);
        if (m == 0ull) return;
        uint32_t base = 0;
        if (lane == (uint32_t)__builtin_ctzll(m)) base = atomicAdd(&s_count, (uint32_t)__popcll(m));
        base = __shfl(base, (int)__builtin_ctzll(m));
        if (kp) {
            const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (at < SIDE_REC_CAP) recs[at] = doc; else s_over_recs = 1u;      // (more records than the array takes: the host redoes the part on the pipeline)
        }
    };
    auto wave_total = [&](uint32_t v) -> unsigned long long {
        const uint32_t incl = scan16(v);                                     // (the whole wave is here)
        return (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)incl, 15) + (uint32_t)__builtin_amdgcn_readlane((int)incl, 31) +
               (uint32_t)__builtin_amdgcn_readlane((int)incl, 47) + (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    };

    for (uint32_t q = blockIdx.x; q < a.B; q += gridDim.x) {
        const uint64_t q_lo = a.offsets[q];
        const uint32_t n_raw = (uint32_t)(a.offsets[q + 1] - q_lo);
        const bool too_long = n_raw > QS_MAX_HASHES;          // (the host takes no such batch; a query that long would overrun its hash set)
        const uint32_t n = too_long ? 0u : n_raw;
        const uint32_t* qh = a.hashes_base + q_lo;
        const uint32_t rounds = (n + SIDE_WG - 1u) / SIDE_WG;
        // the query's hash set: 2^sbits >= 2 n slots
        uint32_t sbits = 8u;
        while ((1u << sbits) < 2u * n) ++sbits;
        __syncthreads();                                    // (the query before: its candidate buffer and flags have been read)
        for (uint32_t i = tid; i < (1u << sbits); i += SIDE_WG) recs[i] = 0xFFFFFFFFu;
        for (uint32_t i = tid; i < (1u << (QS_FLOG2 - 1u)); i += SIDE_WG) filter[i] = 0u;
        for (uint32_t s = tid; s < T; s += SIDE_WG) table[s] = 0ull;
        if (tid == 0) {
            s_count = 0u; s_over_recs = too_long ? 1u : 0u; s_seen_ones = 0u; s_ccnt = 0u; s_cshared = 0u;
            wg_blocks = 0; wg_docs = 0;
            s_cancel = cancel_requested(a.cancel, a.counters) ? 1u : 0u;      // cancel point (src/FileSegment.zig:144), once per query
        }
        __syncthreads();
        if (s_cancel) return;
        // ---- dedupSorted (src/Index.zig:171-172,489-499): the first occurrence of a hash is the probe, later ones are dropped.  A lane notes
        //      which of its rounds' hashes are probes
        uint32_t vmask = 0u;
        for (uint32_t r = 0; r < rounds; ++r) {
            const uint32_t i = r * SIDE_WG + tid;
            if (i >= n) continue;
            const uint32_t h = gload_u32(qh + i);
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
            if (!dup) vmask |= 1u << r;
        }
        __syncthreads();                                    // (the set is done with: its slots are the record array now)

        uint32_t my_blocks = 0, my_docs = 0, my_probes = 0, my_reads = 0, my_bytes = 0;
        // ---- FileSegment.search for every side segment, a hash per lane and round
        for (uint32_t r = 0; r < rounds; ++r) {
            const bool valid = ((vmask >> r) & 1u) != 0u;
            const uint32_t h = valid ? gload_u32(qh + r * SIDE_WG + tid) : 0u;

            // -- small decoded segments (k_probe_small's logic, its keys-per-thread dimension turned into segments): the cell codes ...
            auto small_first = [&](uint32_t s0, uint32_t (&cw)[SIDE_SMALL_CH]) {
#pragma unroll
                for (uint32_t k = 0; k < SIDE_SMALL_CH; ++k) {
                    cw[k] = 0u;
                    if (s0 + k >= a.n_small) continue;                             // (uniform)
                    const SegDesc& seg = a.small[s0 + k];
                    if (valid) cw[k] = gload_u32(seg.scode + ((h >> seg.cshift) >> 4));
                }
            };
            // ... then bucket bounds, the search to the first item >= h, the block-first bits and the walk
            auto small_rest = [&](uint32_t s0, const uint32_t (&cw)[SIDE_SMALL_CH]) {
                uint32_t lo[SIDE_SMALL_CH], hi[SIDE_SMALL_CH], run_n[SIDE_SMALL_CH];
                bool act[SIDE_SMALL_CH];
                // seven hashes in eight fall into a cell without items: its code says what the reference's walk would have cost
#pragma unroll
                for (uint32_t k = 0; k < SIDE_SMALL_CH; ++k) {
                    act[k] = valid && s0 + k < a.n_small;
                    lo[k] = 0u; hi[k] = 0u; run_n[k] = 0u;
                    if (!act[k]) continue;
                    const SegDesc& seg = a.small[s0 + k];
                    my_probes += 1u;
                    const uint32_t code = (cw[k] >> (((h >> seg.cshift) & 15u) * 2u)) & 3u;
                    if (code == 0u) continue;
                    act[k] = false;
                    if (code == 1u) { my_blocks += 1u; my_bytes += seg.block_size; }
                }
#pragma unroll
                for (uint32_t k = 0; k < SIDE_SMALL_CH; ++k) {
                    if (!act[k]) continue;
                    const SegDesc& seg = a.small[s0 + k];
                    const uint32_t bk = h >> seg.sshift;
                    lo[k] = gload_u32(seg.sbucket + bk);
                    hi[k] = gload_u32(seg.sbucket + bk + 1u);
                    my_reads += 2u;
                }
                for (;;) {
                    bool more = false;
                    uint32_t v[SIDE_SMALL_CH];
#pragma unroll
                    for (uint32_t k = 0; k < SIDE_SMALL_CH; ++k)         // (a segment past the last one has lo == hi: its descriptor is not read)
                        v[k] = lo[k] < hi[k] ? (uint32_t)(gload_u64(a.small[min(s0 + k, a.n_small - 1u)].items + ((lo[k] + hi[k]) >> 1)) >> 32) : 0u;
#pragma unroll
                    for (uint32_t k = 0; k < SIDE_SMALL_CH; ++k) {
                        if (lo[k] < hi[k]) { const uint32_t m = (lo[k] + hi[k]) >> 1; if (v[k] < h) lo[k] = m + 1u; else hi[k] = m; }
                        more = more || lo[k] < hi[k];
                    }
                    if (!more) break;
                }
                uint64_t it[SIDE_SMALL_CH];
                uint32_t fw[SIDE_SMALL_CH];
#pragma unroll
                for (uint32_t k = 0; k < SIDE_SMALL_CH; ++k) {
                    it[k] = 0ull; fw[k] = 0u;
                    if (!act[k]) continue;
                    const SegDesc& seg = a.small[s0 + k];
                    act[k] = lo[k] < seg.num_items;                                  // (above every block: nothing is visited, :153)
                    if (!act[k]) continue;
                    it[k] = gload_u64(seg.items + lo[k]);
                    fw[k] = gload_u32(seg.sfirst + (lo[k] >> 5));
                }
#pragma unroll
                for (uint32_t k = 0; k < SIDE_SMALL_CH; ++k) {
                    if (!act[k]) continue;
                    const SegDesc& seg = a.small[s0 + k];
                    const uint32_t i = lo[k], nit = seg.num_items, block_size = seg.block_size;
                    if ((uint32_t)(it[k] >> 32) != h) {
                        // absent: the walk visits the block of item i, finds nothing and stops -- unless i opens its block (the gap before it, :164)
                        if (((fw[k] >> (i & 31u)) & 1u) == 0u) { my_blocks += 1u; my_bytes += block_size; }
                        continue;
                    }
                    // the run's docs that count: a block more each time it crosses a block-first item, until four blocks or past 1000 docs (:171-174)
                    uint32_t nb = 1, nd = 1;
                    for (uint32_t j = i + 1u; j < nit; ++j) {
                        if ((uint32_t)(gload_u64(seg.items + j) >> 32) != h) break;
                        if (((gload_u32(seg.sfirst + (j >> 5)) >> (j & 31u)) & 1u) != 0u) {
                            if (nb >= (uint32_t)MAX_BLOCKS_PER_HASH || nd > (uint32_t)MAX_DOCS_PER_HASH) break;
                            ++nb;
                        }
                        ++nd;
                    }
                    my_blocks += nb; my_docs += nd; my_bytes += nb * block_size; my_reads += 2u + ((nd + 15u) >> 4) * 2u;
                    if (nd > 1u || nb > 1u) hist_observe(wg_h, nd, nb);
                    run_n[k] = nd;
                }
                // the runs' docs join the query's records: the first of each lane's, then the longer runs read on by the wave, 64 docs at a
                // time.  (A doc that a newer segment supersedes has been counted above: CTR_DOCS counts before supersession)
#pragma unroll
                for (uint32_t k = 0; k < SIDE_SMALL_CH; ++k) {
                    if (s0 + k >= a.n_small) continue;                             // (uniform)
                    const SegDesc& seg = a.small[s0 + k];
                    const bool filt = seg.num_dead != 0u;
                    const uint32_t d0 = (uint32_t)it[k];
                    bool kp = run_n[k] != 0u;
                    if (kp && filt) kp = !is_dead_seg(seg, d0);
                    emit1(kp, d0);
                    unsigned long long ml = __ballot((int)(run_n[k] > 1u));
                    while (ml != 0ull) {
                        const int src = (int)__builtin_ctzll(ml);
                        ml &= ml - 1ull;
                        const uint32_t i_s = __shfl(lo[k], src), n_s = __shfl(run_n[k], src);
                        for (uint32_t o = 1u; o < n_s; o += 64u) {
                            bool kp2 = o + lane < n_s;
                            const uint32_t dv = kp2 ? (uint32_t)gload_u64(seg.items + i_s + o + lane) : 0u;
                            if (kp2 && filt) kp2 = !is_dead_seg(seg, dv);
                            emit1(kp2, dv);
                        }
                    }
                }
            };
            // -- segments that are direct-addressed on their own (k_probe_direct's logic): the 64-byte records ...
            auto solo_first = [&](uint32_t s0, uint32_t (&bw)[SIDE_SOLO_CH], uint4 (&ax)[SIDE_SOLO_CH], bool (&vld)[SIDE_SOLO_CH]) {
#pragma unroll
                for (uint32_t k = 0; k < SIDE_SOLO_CH; ++k) {
                    bw[k] = 0u; ax[k] = make_uint4(0, 0, 0, 0); vld[k] = false;
                    if (s0 + k >= a.n_solo) continue;                              // (uniform)
                    const SegDesc& seg = a.solo[s0 + k];
                    if (!valid) continue;
                    my_probes += 1u;
                    // (before the segment's first hash and beyond its last one: absent, nothing visited, src/FileSegment.zig:164,153)
                    if (h < seg.first_hash || h > seg.last_hash) continue;
                    vld[k] = true;
                    const uint32_t* rec = seg.drec + (size_t)(h >> 8) * 16u;
                    bw[k] = gload_u32(rec + ((h >> 5) & 7u));
                    ax[k] = gload_u4(reinterpret_cast<const uint8_t*>(rec + 8));
                }
            };
            // ... then the rank into `primary`, the gap word, the list's head and the lists longer than it
            auto solo_rest = [&](uint32_t s0, const uint32_t (&bw)[SIDE_SOLO_CH], const uint4 (&ax)[SIDE_SOLO_CH], const bool (&vld)[SIDE_SOLO_CH]) {
                bool present[SIDE_SOLO_CH];
                uint32_t d[SIDE_SOLO_CH];
                uint4 x[SIDE_SOLO_CH];
#pragma unroll
                for (uint32_t k = 0; k < SIDE_SOLO_CH; ++k) {
                    const uint32_t pos = h & 255u, w = pos >> 5, bit = pos & 31u;
                    present[k] = vld[k] && ((bw[k] >> bit) & 1u) != 0u;
                    d[k] = 0xFFFFFFFFu;
                    if (present[k]) {
                        const SegDesc& seg = a.solo[s0 + k];
                        const uint32_t pre = ((w < 4u ? ax[k].y : ax[k].z) >> (8u * (w & 3u))) & 0xFFu;
                        const uint32_t rank = ax[k].x + pre + (uint32_t)__popc(bw[k] & ((1u << bit) - 1u));
                        d[k] = gload_u32(seg.primary + rank);
                        my_reads += 2u;
                    } else if (vld[k]) {
                        my_blocks += 1u; my_bytes += a.solo[s0 + k].block_size;      // a clear bit: the reference visits one block, finds nothing and stops
                    }
                }
#pragma unroll
                for (uint32_t k = 0; k < SIDE_SOLO_CH; ++k) {
                    present[k] = present[k] && d[k] != 0xFFFFFFFFu;                  // (a gap position: nothing visited)
                    x[k] = make_uint4(0, 0, 0, 0);
                    if (present[k] && (d[k] >> 31)) {
                        const SegDesc& seg = a.solo[s0 + k];
                        x[k] = gload_u4_a4(seg.extras + ((size_t)(d[k] & 0x7FFFFFFFu) << seg.extras_shift));
                        my_reads += 2u;
                    }
                }
#pragma unroll
                for (uint32_t k = 0; k < SIDE_SOLO_CH; ++k) {
                    if (s0 + k >= a.n_solo) continue;                              // (uniform)
                    const SegDesc& seg = a.solo[s0 + k];
                    const bool filt = seg.num_dead != 0u;
                    const uint32_t base_doc = seg.min_doc_id;
                    const bool multi = present[k] && (d[k] >> 31) != 0u;
                    // header: docs the reference RETURNS | blocks it VISITS << 16 | T << 19 [T: the list's full length follows]; then the docs
                    const uint32_t eff = multi ? (x[k].x & 0xFFFFu) : (present[k] ? 1u : 0u);
                    const uint32_t Tl = (x[k].x >> 19) & 1u;
                    if (present[k]) {
                        const uint32_t nbk = multi ? ((x[k].x >> 16) & 7u) : 1u;
                        my_blocks += nbk; my_bytes += nbk * seg.block_size; my_docs += eff;
                    }
                    if (multi) hist_observe(wg_h, eff, (x[k].x >> 16) & 7u);
                    const uint32_t d0 = multi ? (Tl ? x[k].z : x[k].y) : d[k];
                    const uint32_t d1 = Tl ? x[k].w : x[k].z;
                    auto emit_live = [&](bool kp, uint32_t doc) {                  // (counted above: before supersession)
                        if (kp && filt) kp = !is_dead_seg(seg, doc);
                        emit1(kp, doc);
                    };
                    emit_live(eff >= 1u, base_doc + d0);
                    emit_live(multi && eff >= 2u, base_doc + d1);
                    emit_live(multi && eff >= 3u && Tl == 0u, base_doc + x[k].w);
                    // longer lists: the wave reads them on together, 64 docs at a time
                    const uint32_t in_regs = Tl ? 2u : 3u;
                    const bool long_list = multi && eff > in_regs;
                    if (long_list) my_reads += ((eff + 31u) >> 5) * 2u;
                    unsigned long long ml = __ballot((int)long_list);
                    while (ml != 0ull) {
                        const int src = (int)__builtin_ctzll(ml);
                        ml &= ml - 1ull;
                        const uint32_t xs = __shfl(d[k] & 0x7FFFFFFFu, src), es = __shfl(eff, src), ts = __shfl(Tl, src);
                        for (uint32_t o = ts ? 2u : 3u; o < es; o += 64u) {
                            const bool kp = o + lane < es;
                            const uint32_t dv = kp ? gload_u32(seg.extras + ((size_t)xs << seg.extras_shift) + 1u + ts + o + lane) : 0u;
                            emit_live(kp, base_doc + dv);
                        }
                    }
                }
            };

            // the first loads of BOTH kinds go out together; a chain of one load latency per segment is what a lane's time would be otherwise.
            // LIMIT: that holds for the first SIDE_SMALL_CH small and SIDE_SOLO_CH direct-addressed segments -- a live index has a few
            // checkpoints and one merged segment between two merges --; a snapshot with more runs the further chunks one after the other,
            // each with its own chain, and the direct-addressed chunk's second step waits behind the small chunk's walks
            uint32_t cw[SIDE_SMALL_CH], bw[SIDE_SOLO_CH];
            uint4 ax[SIDE_SOLO_CH];
            bool vld[SIDE_SOLO_CH];
            small_first(0u, cw);
            solo_first(0u, bw, ax, vld);
            if (a.n_small != 0u) small_rest(0u, cw);
            if (a.n_solo != 0u) solo_rest(0u, bw, ax, vld);
            for (uint32_t s0 = SIDE_SMALL_CH; s0 < a.n_small; s0 += SIDE_SMALL_CH) { small_first(s0, cw); small_rest(s0, cw); }
            for (uint32_t s0 = SIDE_SOLO_CH; s0 < a.n_solo; s0 += SIDE_SOLO_CH) { solo_first(s0, bw, ax, vld); solo_rest(s0, bw, ax, vld); }
        }
        // ---- the query's statistics (what FileSegment.search observes per hash, summed: src/FileSegment.zig:177-178)
        {
            const unsigned long long w_reads = wave_total(my_reads), w_blocks = wave_total(my_blocks), w_docs = wave_total(my_docs),
                                     w_probes = wave_total(my_probes), w_bytes = wave_total(my_bytes);
            if (lane == 0u) {
                if (w_reads) atomicAdd(&tot_reads, w_reads);
                if (w_blocks) { atomicAdd(&wg_blocks, w_blocks); atomicAdd(&tot_blocks, w_blocks); atomicAdd(&tot_bytes, w_bytes); }
                if (w_docs) { atomicAdd(&wg_docs, w_docs); atomicAdd(&tot_docs, w_docs); }
                if (w_probes) atomicAdd(&tot_probes, w_probes);
            }
        }
        __syncthreads();                                    // (the records are complete)
        const uint32_t nrec = min(s_count, SIDE_REC_CAP);
        // ---- SearchResults.incr (src/common.zig:121-129), first the filter: every record into its doc's cell
        for (uint32_t i = tid * 4u; i < nrec; i += SIDE_WG * 4u) {
            const uint4 r4 = *reinterpret_cast<const uint4*>(recs + i);             // (the array ends with four spare words)
            const uint32_t r[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) {
                const uint32_t c = qs_cell(r[u]);
                if (i + u < nrec) atomicAdd(&filter[c >> 1], 1u << (16u * (c & 1u)));
            }
        }
        if (tid == 0) {
            tot_recs += (unsigned long long)s_count;                                // the query's hit records
            if (a.qstats) a.qstats[q] = wg_blocks | (wg_docs << 32);
            if (s_over_recs || s_count > SIDE_REC_CAP) atomicMax(&a.counters[CTR_BINFAIL], 1ull);
        }
        // ---- ... then the floor of finish (src/common.zig:131-145): a doc can only reach the floor if its cell did; those records are
        //      counted exactly, in `passes` loads over classes of them when they are more than the table takes
        const uint32_t floor_q = a.opts[q * 4u + 1u];
        const uint32_t sb = a.sb;
        const uint64_t smax = sb >= 32u ? 0xFFFFFFFFull : ((1ull << sb) - 1ull);
        if (s_over_recs == 0u && nrec != 0u && nrec >= floor_q) {
            uint32_t passes = 1u;
            for (uint32_t pass = 0; pass < passes; ++pass) {
                if (pass != 0u) {
                    __syncthreads();
                    for (uint32_t s = tid; s < T; s += SIDE_WG) table[s] = 0ull;
                }
                if (tid == 0) { s_claimed = 0u; s_full = 0u; }
                __syncthreads();                            // (the first pass: the filter's counts are complete behind this barrier)
                for (uint32_t i4 = tid * 4u; i4 < nrec; i4 += SIDE_WG * 4u) {
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
                __syncthreads();
                if (pass == 0u && (s_claimed > T * 3u / 4u || s_full != 0u) && passes < 64u) {
                    const uint32_t np = passes * 2u;
                    __syncthreads();
                    for (uint32_t s = tid; s < T; s += SIDE_WG) table[s] = 0ull;
                    passes = np; pass = 0xFFFFFFFFu;           // (++pass: 0 again; nothing has been emitted yet)
                    continue;
                }
                if (s_full != 0u && tid == 0) atomicMax(&a.counters[CTR_BINFAIL], 1ull);
                // candidates: count >= the floor -> the query's buffer in LDS (its first SB_CAND), the rest to the shared list
                for (uint32_t s = tid; s < T; s += SIDE_WG) {
                    const unsigned long long e = table[s];
                    if (e == 0ull) continue;
                    const uint32_t count = (uint32_t)e, doc = (uint32_t)(e >> 32);
                    if (count < floor_q) continue;
                    if ((uint64_t)count > smax) atomicMax(&a.counters[CTR_MAXSCORE], (unsigned long long)count);
                    const uint64_t sc = (uint64_t)count > smax ? smax : (uint64_t)count;
                    const uint64_t qpart = sb >= 32u ? 0ull : ((uint64_t)q << (32u + sb));
                    const uint64_t key = qpart | ((smax - sc) << 32) | doc;
                    const uint32_t at = atomicAdd(&s_ccnt, 1u);
                    if (at < SB_CAND) cbuf[at] = key;
                    else {
                        const unsigned long long gi = atomicAdd(&a.counters[CTR_CANDS], 1ull);
                        if (gi < a.cand_cap) a.cands[gi] = key;
                        s_cshared = 1u;
                    }
                }
            }
        }
        // ---- hand-over: up to QCAND_SLOTS candidates stay in the query's own slots, more move to the shared list entirely
        __syncthreads();
        const uint32_t cn = min(s_ccnt, SB_CAND);
        const bool shared = s_cshared != 0u || cn > QCAND_SLOTS;
        if (tid == 0) {
            if (shared && cn != 0u) {
                const unsigned long long gi = atomicAdd(&a.counters[CTR_CANDS], (unsigned long long)cn);
                s_cbase_lo = (uint32_t)gi; s_cbase_hi = (uint32_t)(gi >> 32);
            }
            a.qcand_n[q] = shared ? QCAND_OVERFLOWED : cn;
        }
        __syncthreads();
        if (tid < cn) {
            const uint64_t key = cbuf[tid];
            if (!shared) a.qcand[(size_t)q * QCAND_SLOTS + tid] = key;
            else {
                const uint64_t gi = (((uint64_t)s_cbase_hi << 32) | s_cbase_lo) + tid;
                if (gi < a.cand_cap) a.cands[gi] = key;
            }
        }
    }
    // ---- the workgroup's statistics, once: its set of the spread statistics (the host prices the sets' blocks at 512 bytes; blocks of
    //      another size add the difference -- mod 2^64 -- to slot 5) and the scan histograms' slots behind them
    __syncthreads();
    if (tid == 0) {
        unsigned long long* st = a.stat_sets + (size_t)(blockIdx.x % LEAN_STAT_SETS) * 8u;
        if (tot_reads) atomicAdd(&st[4], tot_reads);
        if (tot_blocks) atomicAdd(&st[1], tot_blocks);
        if (tot_bytes != tot_blocks * 512ull) atomicAdd(&st[5], tot_bytes - tot_blocks * 512ull);
        if (tot_docs) atomicAdd(&st[2], tot_docs);
        if (tot_probes) atomicAdd(&st[3], tot_probes);
        if (tot_recs) atomicAdd(&st[7], tot_recs);
    }
    if (tid < HIST_SLOTS - 1u) {                             // (slot 15: hist_observe's sink)
        const unsigned long long v = tid == HIST_COUNT ? tot_probes : tid == HIST_DOCS ? tot_docs : tid == HIST_BLOCKS ? tot_blocks : (unsigned long long)wg_h[tid];
        if (v != 0ull) atomicAdd(&a.stat_sets[(size_t)LEAN_STAT_SETS * 8u + (size_t)(blockIdx.x % LEAN_STAT_SETS) * HIST_SLOTS + tid], v);
    }
}

}  // namespace fpx
