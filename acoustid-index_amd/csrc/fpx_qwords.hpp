// fpx_qwords.hpp -- k_search_words: a group in DIRECTORY + WORDS form (fpx_group.hpp: one directory line per 32 hash values, the words
// elsewhere, `lists` per chunk -- every group that is not dense enough to be packed, or whose doc ids span 2^31 or more) searched ONE QUERY
// PER WORKGROUP, as k_search_query (fpx_qsearch.hpp) searches the packed group and k_search_side (fpx_qside.hpp) the segments next to it:
// dedupSorted (src/Index.zig:489-499), FileSegment.search for every column (src/FileSegment.zig:135-180), the memory segments' table,
// SearchResults.incr and the min_score filter of finish (src/common.zig:121-145) in one kernel.
// Part of the fpx_search.hip translation unit (after fpx_qframe.hpp: the LDS layout, the query's reset, the hash set, counting, the candidate
// hand-over and the statistics flush are that header's, shared with k_search_side; this file is the kernel's walk and its memory-table lookup).
//
// The pipeline runs keys, a radix pass, k_probe_group, the bins in HBM, k_score_bin and k_finish.  Here a workgroup owns a query and stays
// (every gridDim.x-th query): the query's hashes go into a hash set in LDS, every unique hash is a lane's, walked as k_probe_group walks it
// -- THAT kernel is the normative statement of the walk and of every statistic: pm, pos0, dbl_before, dm, nwords, the absent-column blocks,
// gap words, singles and doubles, list references, the list header, hist_observe, the doubles in the upper half of the probe counter,
// win_lo / win_hi --, the docs are appended to a record array in LDS as ABSOLUTE ids (min_doc[column] + word: this form has no single base),
// counted in a filter of 16-bit cells and, where a cell reaches the query's floor, exactly in a small table; candidates leave in
// k_search_query's format for k_finish.
//
// The form built: the PER-LANE walk.  A lane fetches its own hash's directory line (eight or four 16-byte loads), then the hash's words
// (up to GK_WORDS = 12 in three loads), then the head of its first list: a chain of two or three dependent trips, 32 or 16 line words held
// per lane and round.  One reservation per wave and round in the record array (a scan on the DPP crossbar); the rare rest -- words beyond the
// lane's twelve, further lists, lists longer than their head -- by the whole wave, one ballot reservation per 64 docs.  (A lane group to a
// line -- DESIGN 4.0's finding for the packed form -- is the next step, not this one: DESIGN 4.3.)
//
// Taken by run_batch (option words_wg = 1) for a snapshot that is one such group and nothing else, every column searched and no doc
// superseded; FILT (option words_wg = 2): columns outside `active` give nothing -- no record, no statistic --, a doc of a column with a dead
// set is dropped after it was counted.  The record array holds QF_REC_CAP = 8192 docs; a query that brings more raises CTR_BINFAIL and
// the host redoes the batch on the pipeline (FPX_REDO_QS).
#pragma once
#include <hip/hip_runtime.h>

#include "fpx_internal.h"

namespace fpx {

struct WordsArgs {
    QFrameArgs f;
    // a live index's memory segments: their ONE hash-sorted table of live postings (fpx_probe_small.hpp: k_probe_memtab), or null
    const uint64_t* mem_tab; const uint32_t* mem_bucket; const uint32_t* mem_bits;
};

// (four workgroups per CU: 128 registers per lane)
#define FPX_QW_OCC __attribute__((amdgpu_waves_per_eu(4)))
// (MEM: the snapshot has memory segments.  FILT: the group has superseded docs and/or columns outside the snapshot)
template <int NS, bool MEM, bool FILT>
__global__ __launch_bounds__(QF_WG) FPX_QW_OCC void k_search_words(WordsArgs a, GroupArgs ga)
{
    constexpr int NM = NS - 4;             // words of double bits
    extern __shared__ __align__(16) uint8_t words_dyn[];
    QFrameLds& L = *reinterpret_cast<QFrameLds*>(words_dyn);
    uint32_t* const recs = L.recs;
    __shared__ QFrame fr;
    // per column, indexed by a lane's own column number
    __shared__ uint32_t s_min_doc[FUSE_MAX], s_has_dead[FUSE_MAX], s_seg_index[FUSE_MAX];

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const GroupDesc* g = &ga.g;
    if (tid < FUSE_MAX) { s_min_doc[tid] = g->min_doc[tid]; s_has_dead[tid] = g->has_dead[tid]; s_seg_index[tid] = g->seg_index[tid]; }
    qf_init(fr, tid);
    // (unfiltered: every column in use is searched and none has superseded docs -- the tests below fold away)
    const uint32_t active = FILT ? g->active : 0xFFFFFFFFu, nactive = (uint32_t)__popc(g->active);
    const bool any_dead = FILT && g->any_dead != 0u;

    // the records of a round: ONE reservation per wave -- a scan on the DPP crossbar: the whole wave is here --, the lane's docs from the
    // place it returns (a lane's own atomic on the one counter is compiled into a serial loop over the wave's lanes: experiments/README.md)
    auto reserve = [&](uint32_t cnt) -> uint32_t {
        const uint32_t incl = scan16(cnt);
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)incl, 15), r1 = (uint32_t)__builtin_amdgcn_readlane((int)incl, 31),
                       r2 = (uint32_t)__builtin_amdgcn_readlane((int)incl, 47), r3 = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t total = r0 + r1 + r2 + r3;
        uint32_t wbase = 0;
        if (total != 0u) {                                                       // (wave-uniform)
            if (lane == 0u) wbase = atomicAdd(&fr.s_count, total);
            wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)wbase);
        }
        const uint32_t row = lane >> 4;
        return wbase + (row >= 1u ? r0 : 0u) + (row >= 2u ? r1 : 0u) + (row >= 3u ? r2 : 0u) + (incl - cnt);
    };
    // one record of some lanes of the wave (the wave's turns: words beyond a lane's own, long lists): a ballot, one reservation
    auto emit1 = [&](bool kp, uint32_t doc) { qf_emit1(fr, L, lane, kp, doc); };
    // (FILT) a doc of column s that a newer segment supersedes
    auto dead_in = [&](uint32_t s, uint32_t doc) -> bool {
        if constexpr (!FILT) return false;
        return any_dead && s_has_dead[s] != 0u && is_dead_seg(ga.segs[s_seg_index[s]], doc);
    };

    for (uint32_t q = blockIdx.x; q < a.f.B; q += gridDim.x) {
        const QFrameQuery fq = qf_begin_query(fr, L, a.f, q, tid);
        if (fq.cancelled) return;
        const uint32_t* const qh = fq.qh;
        const uint32_t n = fq.n, rounds = fq.rounds;
        // ---- dedupSorted (src/Index.zig:171-172,489-499).  A lane notes which of its rounds' hashes are probes (a hash-window slice of the
        //      group leaves the other hashes to another rank)
        uint32_t vmask = 0u;
        uint32_t mmask = 0u;                                // (MEM) ... and which of them the memory segments' table may hold: a bit per 256 hash values
        for (uint32_t r = 0; r < rounds; ++r) {
            const uint32_t i = r * QF_WG + tid;
            if (i >= n) continue;
            const uint32_t h = gload_u32(qh + i);
            uint32_t mb = 0xFFFFFFFFu;
            if constexpr (MEM) { if (a.mem_bits != nullptr) mb = gload_u32(a.mem_bits + ((h >> MEMTAB_FILTER_SHIFT) >> 5)); }
            const bool dup = qf_later_occurrence(fr, L, fq.sbits, h);
            if (!dup && h >= g->win_lo && h <= g->win_hi) {
                vmask |= 1u << r;
                if constexpr (MEM) mmask |= ((mb >> ((h >> MEMTAB_FILTER_SHIFT) & 31u)) & 1u) << r;
            }
        }
        (void)mmask;
        __syncthreads();                                    // (the set is done with: its slots are the record array now)

        // (my_probes: the probes in its lower half, the doubles among them in its upper one -- 16 per hash at most, 16 rounds)
        uint32_t my_blocks = 0, my_docs = 0, my_probes = 0, my_reads = 0;
        // ---- FileSegment.search for every column, a hash per lane and round: k_probe_group's walk
        for (uint32_t r = 0; r < rounds; ++r) {
            const bool valid = ((vmask >> r) & 1u) != 0u;
            const uint32_t h = valid ? gload_u32(qh + r * QF_WG + tid) : 0u;
            const uint32_t bit = h & 31u, below = (1u << bit) - 1u;
            // ---- the line
            uint32_t w[2 * NS];
#pragma unroll
            for (uint32_t i = 0; i < 2 * NS; ++i) w[i] = 0u;
            if (valid) {
                const uint8_t* lb = reinterpret_cast<const uint8_t*>(g->lines + (size_t)((h >> 5) - g->line0) * (2u * NS));
#pragma unroll
                for (int i = 0; i < (2 * NS) / 4; ++i) {
                    const uint4 v = gload_u4(lb + 16 * i);
                    w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
                }
                my_probes += nactive;
                my_reads += NS >= 16 ? 2u : 1u;        // (64-byte units)
            }
            // ---- the hash's columns: which have it, where its words start
            uint32_t pm = 0, pos0 = 0, inr = 0;
#pragma unroll
            for (uint32_t s = 0; s < NS; ++s) {
                pm |= ((w[s] >> bit) & 1u) << s;
                pos0 += (uint32_t)__popc(w[s] & below);
                // (outside [first_hash, last_hash] the reference visits no block, src/FileSegment.zig:164,153; unused columns: empty range)
                inr |= (h >= g->first_hash[s] && h <= g->last_hash[s]) ? (1u << s) : 0u;
            }
            if (!valid) { pm = 0u; inr = 0u; }
            my_blocks += (uint32_t)__popc(inr & active & ~pm);         // absent: the reference visits one block, finds nothing and stops
            const uint32_t k = (uint32_t)__popc(pm);
            // doubles: how many lie before the hash's first position, and which of its own positions are
            uint32_t dbl_before = 0, dlo = 0, dhi = 0;
            const uint32_t pw0 = pos0 >> 5;
#pragma unroll
            for (uint32_t j = 0; j < (uint32_t)NM; ++j) {
                const uint32_t m = w[NS + 4 + j];
                const int lim = (int)pos0 - (int)(32u * j);
                const uint32_t mask = lim >= 32 ? 0xFFFFFFFFu : lim <= 0 ? 0u : ((1u << lim) - 1u);
                dbl_before += (uint32_t)__popc(m & mask);
                dlo = j == pw0 ? m : dlo;
                dhi = j == pw0 + 1u ? m : dhi;
            }
            const uint32_t dm = (uint32_t)(((((uint64_t)dhi << 32) | dlo) >> (pos0 & 31u))) & ((1u << k) - 1u);     // (k <= 16)
            const uint32_t nwords = k + (uint32_t)__popc(dm);
            const uint32_t* pw = reinterpret_cast<const uint32_t*>(((uint64_t)w[NS + 1] << 32) | w[NS]) + (pos0 + dbl_before);
            const uint32_t* lists = reinterpret_cast<const uint32_t*>(((uint64_t)w[NS + 3] << 32) | w[NS + 2]);
            // ---- its words: three loads, the second and third only where the hash has that many
            uint32_t gw[GK_WORDS];
#pragma unroll
            for (uint32_t i = 0; i < GK_WORDS; ++i) gw[i] = 0u;
#pragma unroll
            for (uint32_t i = 0; i < GK_WORDS / 4; ++i) {
                if (nwords > 4u * i) {
                    const uint4 v = gload_u4_a4(pw + 4u * i);
                    gw[4 * i] = v.x; gw[4 * i + 1] = v.y; gw[4 * i + 2] = v.z; gw[4 * i + 3] = v.w;
                    my_reads += 2u;
                }
            }
            // ---- walk them: single docs and doubles become records (absolute doc ids), the first list reference gets the lane's slot
            uint32_t docs[GK_WORDS];
            uint32_t keep = 0, n_esc = 0, esc_off = 0, esc_col = 0;
            {
                uint32_t rest = pm, i = 0;
                bool second = false;
#pragma unroll
                for (uint32_t j = 0; j < GK_WORDS; ++j) {
                    const uint32_t word = gw[j];
                    uint32_t doc = 0u;
                    if (j < nwords) {
                        const uint32_t s = (uint32_t)__builtin_ctz(rest);
                        if (word != 0xFFFFFFFFu && ((active >> s) & 1u) != 0u) {                 // (0xFFFFFFFF: a gap position -- nothing visited)
                            if (word >> 31) {
                                if (n_esc == 0u) { esc_off = word & 0x7FFFFFFFu; esc_col = s; }
                                n_esc += 1u;
                            } else {
                                doc = s_min_doc[s] + word;
                                my_blocks += second ? 0u : 1u; my_docs += 1u;
                                if constexpr (SCAN_HIST && (FPX_SH_BITS & 2)) my_probes += second ? (1u << 16) : 0u;     // (a double: ONE observation of two docs, counted at its second word)
                                // (FILT: counted above -- CTR_DOCS counts before supersession)
                                if (!dead_in(s, doc)) keep |= 1u << j;
                            }
                        }
                        if (((dm >> i) & 1u) != 0u && !second) second = true;
                        else { second = false; i += 1u; rest &= rest - 1u; }
                    }
                    docs[j] = doc;
                }
            }
            // the head of the first list: header + up to three docs in one load
            uint4 x = make_uint4(0, 0, 0, 0);
            if (n_esc != 0u) { x = gload_u4_a4(lists + esc_off); my_reads += 2u; }
            uint32_t xkeep = 0;
            const uint32_t xT = (x.x >> 19) & 1u, xeff = x.x & 0xFFFFu, xin = n_esc ? min(xeff, xT ? 2u : 3u) : 0u;
            const uint32_t xmd = s_min_doc[esc_col];
            const uint32_t xd0 = xmd + (xT ? x.z : x.y), xd1 = xmd + (xT ? x.w : x.z), xd2 = xmd + x.w;
            if (n_esc != 0u) {
                my_blocks += (x.x >> 16) & 7u; my_docs += xeff;
                hist_observe(fr.wg_h, xeff, (x.x >> 16) & 7u);
                xkeep = (1u << xin) - 1u;
                if constexpr (FILT) {
                    if ((xkeep & 1u) && dead_in(esc_col, xd0)) xkeep &= ~1u;
                    if ((xkeep & 2u) && dead_in(esc_col, xd1)) xkeep &= ~2u;
                    if ((xkeep & 4u) && dead_in(esc_col, xd2)) xkeep &= ~4u;
                }
            }
            // ---- one reservation per wave and round in the query's record array
            {
                const uint32_t cnt = (uint32_t)__popc(keep) + (uint32_t)__popc(xkeep);
                uint32_t at = reserve(cnt);
                if (cnt != 0u && at + cnt > QF_REC_CAP) { fr.s_over_recs = 1u; keep = 0u; xkeep = 0u; }
#pragma unroll
                for (uint32_t j = 0; j < GK_WORDS; ++j)
                    if ((keep >> j) & 1u) recs[at++] = docs[j];
                if (xkeep & 1u) recs[at++] = xd0;
                if (xkeep & 2u) recs[at++] = xd1;
                if (xkeep & 4u) recs[at++] = xd2;
            }
            // ---- the rare rest, by the whole wave: words beyond the lane's twelve, further lists, lists longer than their head
            {
                const bool more = nwords > GK_WORDS || n_esc > 1u || (n_esc == 1u && xeff > xin);
                unsigned long long mo = __ballot((int)more);
                while (mo != 0ull) {
                    const int src = (int)__builtin_ctzll(mo);
                    mo &= mo - 1ull;
                    const uint32_t pm_s = __shfl(pm, src), dm_s = __shfl(dm, src), nw_s = __shfl(nwords, src);
                    const uint32_t* pw_s = reinterpret_cast<const uint32_t*>(((uint64_t)__shfl((uint32_t)((uint64_t)pw >> 32), src) << 32) | __shfl((uint32_t)(uint64_t)pw, src));
                    const uint32_t* li_s = reinterpret_cast<const uint32_t*>(((uint64_t)__shfl((uint32_t)((uint64_t)lists >> 32), src) << 32) | __shfl((uint32_t)(uint64_t)lists, src));
                    // lane l looks at word l of the hash (nwords <= 32): its column, and whether it is a double's second word
                    uint32_t col = 0, wv = 0xFFFFFFFFu;
                    bool second = false;
                    if (lane < nw_s) {
                        uint32_t rest = pm_s, i = 0, j = 0;
                        for (;;) {
                            col = (uint32_t)__builtin_ctz(rest);
                            const uint32_t span = 1u + ((dm_s >> i) & 1u);
                            if (lane < j + span) { second = lane == j + 1u; break; }
                            j += span; i += 1u; rest &= rest - 1u;
                        }
                        wv = gload_u32(pw_s + lane);
                    }
                    const bool act = lane < nw_s && ((active >> col) & 1u) != 0u && wv != 0xFFFFFFFFu;
                    // singles and doubles beyond the lane's words
                    {
                        const bool plain = act && (wv >> 31) == 0u && lane >= GK_WORDS;
                        const uint32_t doc = s_min_doc[col] + wv;
                        if (plain) {
                            my_blocks += second ? 0u : 1u; my_docs += 1u;
                            if constexpr (SCAN_HIST && (FPX_SH_BITS & 2)) my_probes += second ? (1u << 16) : 0u;
                        }
                        emit1(plain && !dead_in(col, doc), doc);
                    }
                    // the lists, one after the other, 64 docs at a time; of the first one within the lane's words the head has been emitted
                    unsigned long long me = __ballot((int)(act && (wv >> 31) != 0u));
                    bool first = true;
                    while (me != 0ull) {
                        const int el = (int)__builtin_ctzll(me);
                        me &= me - 1ull;
                        const uint32_t off = __shfl(wv, el) & 0x7FFFFFFFu, c2 = __shfl(col, el);
                        const uint32_t* list = li_s + off;
                        const uint32_t hdr = gload_u32(list), eff = hdr & 0xFFFFu, Tl = (hdr >> 19) & 1u;
                        uint32_t from = 0u;
                        if (first && (uint32_t)el < GK_WORDS) from = min(eff, Tl ? 2u : 3u);          // (the lane's slot took these)
                        else if (lane == 0) {
                            my_blocks += (hdr >> 16) & 7u; my_docs += eff; my_reads += 2u;
                            hist_observe(fr.wg_h, eff, (hdr >> 16) & 7u);
                        }
                        first = false;
                        const uint32_t md = s_min_doc[c2];
                        for (uint32_t o2 = from; o2 < eff; o2 += 64u) {
                            bool kp = o2 + lane < eff;
                            const uint32_t dv = md + (kp ? gload_u32(list + 1u + Tl + o2 + lane) : 0u);
                            if (kp && dead_in(c2, dv)) kp = false;
                            emit1(kp, dv);
                        }
                        if (lane == 0 && eff > from) my_reads += ((eff - from + 31u) >> 5) * 2u;
                    }
                }
            }
        }
        // ---- MemorySegment.search (src/MemorySegment.zig:44-54) for all memory segments at once: the query's probes looked up in the
        //      snapshot's table of their live postings -- a bit per 256 hash values says "nothing there" for nine probes in ten --, four rounds'
        //      loads out together; every matching item is a record (a doc a newer segment supersedes was dropped when the table was built)
        if constexpr (MEM) {
            for (uint32_t c0 = 0; c0 < rounds; c0 += 4u) {
                if (__ballot((int)(((mmask >> c0) & 15u) != 0u)) == 0ull) continue;          // (wave-uniform)
                uint32_t mh[4], blo[4], bhi[4];
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) {
                    const bool act = ((mmask >> (c0 + u)) & 1u) != 0u;
                    mh[u] = act ? gload_u32(qh + (c0 + u) * QF_WG + tid) : 0u;
                    const uint32_t b = mh[u] >> (32u - MEMTAB_BITS);
                    blo[u] = act ? gload_u32(a.mem_bucket + b) : 0u;
                    bhi[u] = act ? gload_u32(a.mem_bucket + b + 1u) : 0u;
                }
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u)
                    for (uint32_t i = blo[u]; i < bhi[u]; ++i) {                       // (a bucket holds a posting or two)
                        const uint64_t it = gload_u64(a.mem_tab + i);
                        if ((uint32_t)(it >> 32) > mh[u]) break;
                        if ((uint32_t)(it >> 32) == mh[u]) {
                            const uint32_t at = atomicAdd(&fr.s_count, 1u);
                            if (at < QF_REC_CAP) recs[at] = (uint32_t)it; else fr.s_over_recs = 1u;
                        }
                    }
            }
        }
        // ---- the query's statistics; the doubles leave the probe counter's upper half
        {
            const unsigned long long w_reads = qf_wave_total(my_reads), w_blocks = qf_wave_total(my_blocks), w_docs = qf_wave_total(my_docs),
                                     w_probes = qf_wave_total(my_probes & 0xFFFFu);
            const uint32_t w_doubles = (uint32_t)qf_wave_total(my_probes >> 16);
            if (lane == 0u && w_doubles) atomicAdd(&fr.wg_h[0], w_doubles);      // (two docs: the second bucket of the docs histogram)
            qf_query_stats(fr, lane, w_reads, w_blocks, w_docs, w_probes);
        }
        qf_count_and_hand_over(fr, L, a.f, q, tid);
    }
    // (a group has ONE block size)
    __syncthreads();
    qf_flush(fr, a.f, tid, fr.tot_blocks * (unsigned long long)g->block_size - fr.tot_blocks * 512ull);
}

}  // namespace fpx
