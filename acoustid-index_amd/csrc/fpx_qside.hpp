// fpx_qside.hpp -- k_search_side: the file segments NEXT TO the group of a live index -- fresh checkpoints kept decoded (fpx_probe_small.hpp),
// a merged segment that is direct-addressed on its own (fpx_direct.hpp) -- searched ONE QUERY PER WORKGROUP, as k_search_query
// (fpx_qsearch.hpp) searches the group: dedupSorted (src/Index.zig:489-499), FileSegment.search for every side segment
// (src/FileSegment.zig:135-180), SearchResults.incr and the min_score filter of finish (src/common.zig:121-145) in one kernel.
// Part of the fpx_search.hip translation unit (after fpx_qframe.hpp: the LDS layout, the query's reset, the hash set, counting, the candidate
// hand-over and the statistics flush are that header's, shared with k_search_words; this file is the kernel's walk).
//
// The pipeline runs keys, a radix pass, k_probe_small, k_probe_direct, the partition and k_score over ALL the batch's hashes to bring the
// few thousand records these segments hold for a batch.  Here a workgroup owns a query and stays (every gridDim.x-th query): the query's
// hashes go into a hash set in LDS, every unique hash is a lane's, looked up in every side segment in turn -- the first loads of a chunk
// of segments out together --, the docs are appended to a record array in LDS (absolute doc ids), counted in a filter of 16-bit cells and,
// where a cell reaches the query's floor, exactly in a small table; candidates leave in k_search_query's format for k_finish.
//
// Taken by run_batch (option side_wg = 1) for a snapshot -- a part 1, or a whole young index -- that holds small decoded and
// direct-addressed-alone segments only, nothing of them a hash-window slice.  The record array holds QF_REC_CAP = 8192 docs: what the
// dedup set of the longest query taken needs anyway (2 x QS_MAX_HASHES slots).  The reference's caps let ONE hash bring up to 1000 docs
// plus a block's worth from ONE segment (src/FileSegment.zig:171-174), so a single hot hash fits several times over next to a query's
// ordinary records (a handful per query of a live index); a query with eight or more such hashes does not, raises CTR_BINFAIL, and the
// host redoes that snapshot or part on the pipeline (FPX_REDO_QS) -- sizing the array for 4096 hot hashes is not possible in LDS.
#pragma once
#include <hip/hip_runtime.h>

#include "fpx_internal.h"

namespace fpx {

constexpr uint32_t SIDE_SMALL_CH = 4;              // small segments whose loads are under way together
constexpr uint32_t SIDE_SOLO_CH = 2;               // direct-addressed segments likewise

struct SideArgs {
    QFrameArgs f;
    const SegDesc* small; uint32_t n_small;                    // the snapshot's small decoded segments (Snapshot::d_small)
    const SegDesc* solo; uint32_t n_solo;                      // ... and its direct-addressed segments outside any group (Snapshot::d_solo)
};

__global__ __launch_bounds__(QF_WG) void k_search_side(SideArgs a)
{
    extern __shared__ __align__(16) uint8_t side_dyn[];
    QFrameLds& L = *reinterpret_cast<QFrameLds*>(side_dyn);
    __shared__ QFrame fr;
    __shared__ unsigned long long tot_bytes;              // the workgroup's, over all its queries: what its visited blocks hold (the segments' block sizes differ)

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    qf_init(fr, tid);
    if (tid == 0) tot_bytes = 0;
    auto emit1 = [&](bool kp, uint32_t doc) { qf_emit1(fr, L, lane, kp, doc); };

    for (uint32_t q = blockIdx.x; q < a.f.B; q += gridDim.x) {
        const QFrameQuery fq = qf_begin_query(fr, L, a.f, q, tid);
        if (fq.cancelled) return;
        const uint32_t* const qh = fq.qh;
        const uint32_t n = fq.n, rounds = fq.rounds;
        // ---- dedupSorted (src/Index.zig:171-172,489-499).  A lane notes which of its rounds' hashes are probes
        uint32_t vmask = 0u;
        for (uint32_t r = 0; r < rounds; ++r) {
            const uint32_t i = r * QF_WG + tid;
            if (i >= n) continue;
            const uint32_t h = gload_u32(qh + i);
            if (!qf_later_occurrence(fr, L, fq.sbits, h)) vmask |= 1u << r;
        }
        __syncthreads();                                    // (the set is done with: its slots are the record array now)

        uint32_t my_blocks = 0, my_docs = 0, my_probes = 0, my_reads = 0, my_bytes = 0;
        // ---- FileSegment.search for every side segment, a hash per lane and round
        for (uint32_t r = 0; r < rounds; ++r) {
            const bool valid = ((vmask >> r) & 1u) != 0u;
            const uint32_t h = valid ? gload_u32(qh + r * QF_WG + tid) : 0u;

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
                    if (nd > 1u || nb > 1u) hist_observe(fr.wg_h, nd, nb);
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
                    if (multi) hist_observe(fr.wg_h, eff, (x[k].x >> 16) & 7u);
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
        // ---- the query's statistics, and with them what its blocks hold
        {
            const unsigned long long w_reads = qf_wave_total(my_reads), w_blocks = qf_wave_total(my_blocks), w_docs = qf_wave_total(my_docs),
                                     w_probes = qf_wave_total(my_probes), w_bytes = qf_wave_total(my_bytes);
            qf_query_stats(fr, lane, w_reads, w_blocks, w_docs, w_probes);
            if (lane == 0u && w_blocks) atomicAdd(&tot_bytes, w_bytes);
        }
        qf_count_and_hand_over(fr, L, a.f, q, tid);
    }
    __syncthreads();
    qf_flush(fr, a.f, tid, tot_bytes - fr.tot_blocks * 512ull);
}

}  // namespace fpx
