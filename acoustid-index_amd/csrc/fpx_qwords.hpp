// fpx_qwords.hpp -- k_search_words: a group in DIRECTORY + WORDS form (fpx_group.hpp: one directory line per 32 hash values, the words
// elsewhere, `lists` per chunk -- every group that is not dense enough to be packed, or whose doc ids span 2^31 or more) searched ONE QUERY
// PER WORKGROUP, as k_search_query (fpx_qsearch.hpp) searches the packed group and k_search_side (fpx_qside.hpp) the segments next to it:
// dedupSorted (src/Index.zig:489-499), FileSegment.search for every column (src/FileSegment.zig:135-180), the memory segments' table,
// SearchResults.incr and the min_score filter of finish (src/common.zig:121-145) in one kernel.
// Part of the fpx_search.hip translation unit (after fpx_qside.hpp, whose LDS layout, counting and candidate hand-over it copies).
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
// set is dropped after it was counted.  The record array holds WORDS_REC_CAP = 8192 docs; a query that brings more raises CTR_BINFAIL and
// the host redoes the batch on the pipeline (FPX_REDO_QS).
#pragma once
#include <hip/hip_runtime.h>

#include "fpx_internal.h"

namespace fpx {

constexpr uint32_t WORDS_WG = 256;
constexpr uint32_t WORDS_REC_CAP = SIDE_REC_CAP;    // records of a query held in LDS; before: the query's hash set
constexpr uint32_t WORDS_WGS_PER_CU = 4;            // (LDS: 39 KB per workgroup, 128 registers per lane)
constexpr size_t WORDS_LDS_BYTES = SIDE_LDS_BYTES;  // [records + four spare words | filter | exact table | candidate buffer]
static_assert(QS_MAX_HASHES * 2u <= WORDS_REC_CAP, "the dedup set lives where the records will");
static_assert((QS_MAX_HASHES + WORDS_WG - 1u) / WORDS_WG <= 32u, "a lane remembers which of its rounds' hashes are probes in one word");

struct WordsArgs {
    const uint32_t* hashes_base; const uint64_t* offsets;      // hashes_base[i]: the hash at ABSOLUTE position i of the batch; offsets[q] absolute
    const uint32_t* opts;                                      // [B][4]: max_results, floor, pct, raw length
    uint32_t B, sb;                                            // queries; bits of the score field in a candidate key
    uint64_t* cands; uint64_t cand_cap;                        // the shared candidate list (queries with more candidates than slots)
    uint64_t* qcand; uint32_t* qcand_n;                        // the queries' own candidate slots
    unsigned long long* counters;
    unsigned long long* stat_sets;                             // [LEAN_STAT_SETS][8] statistics + [LEAN_STAT_SETS][HIST_SLOTS] histogram slots
    unsigned long long* qstats;                                // [B] blocks | docs << 32, or null
    const uint32_t* cancel;
    // a live index's memory segments: their ONE hash-sorted table of live postings (fpx_probe_small.hpp: k_probe_memtab), or null
    const uint64_t* mem_tab; const uint32_t* mem_bucket; const uint32_t* mem_bits;
};

// (four workgroups per CU: 128 registers per lane)
#define FPX_QW_OCC __attribute__((amdgpu_waves_per_eu(4)))
// (MEM: the snapshot has memory segments.  FILT: the group has superseded docs and/or columns outside the snapshot)
template <int NS, bool MEM, bool FILT>
__global__ __launch_bounds__(WORDS_WG) FPX_QW_OCC void k_search_words(WordsArgs a, GroupArgs ga)
{
    constexpr int NM = NS - 4;             // words of double bits
    constexpr uint32_t T = 1u << QS_TLOG2, TMASK = T - 1u;
    extern __shared__ __align__(16) uint8_t words_dyn[];
    uint32_t* const recs = reinterpret_cast<uint32_t*>(words_dyn);                                      // [WORDS_REC_CAP] docs (+ four spare words)
    uint32_t* const filter = recs + WORDS_REC_CAP + 4u;                                                 // 2^(QS_FLOG2 - 1) words of two cells
    unsigned long long* const table = reinterpret_cast<unsigned long long*>(filter + (1u << (QS_FLOG2 - 1u)));
    uint64_t* const cbuf = reinterpret_cast<uint64_t*>(table + T);                                      // [SB_CAND]
    __shared__ uint32_t s_count, s_over_recs, s_seen_ones, s_cancel, s_claimed, s_full, s_ccnt, s_cshared, s_cbase_lo, s_cbase_hi;
    __shared__ unsigned long long wg_blocks, wg_docs;                                                   // the query's
    __shared__ unsigned long long tot_blocks, tot_docs, tot_probes, tot_reads, tot_recs;                // the workgroup's, over all its queries
    __shared__ uint32_t wg_h[HIST_SLOTS];                                                               // ... and its scan histogram slots (hist_observe)
    // per column, indexed by a lane's own column number
    __shared__ uint32_t s_min_doc[FUSE_MAX], s_has_dead[FUSE_MAX], s_seg_index[FUSE_MAX];

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const GroupDesc* g = &ga.g;
    if (tid < FUSE_MAX) { s_min_doc[tid] = g->min_doc[tid]; s_has_dead[tid] = g->has_dead[tid]; s_seg_index[tid] = g->seg_index[tid]; }
    if (tid < HIST_SLOTS) wg_h[tid] = 0u;
    if (tid == 0) { tot_blocks = 0; tot_docs = 0; tot_probes = 0; tot_reads = 0; tot_recs = 0; }
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
            if (lane == 0u) wbase = atomicAdd(&s_count, total);
            wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)wbase);
        }
        const uint32_t row = lane >> 4;
        return wbase + (row >= 1u ? r0 : 0u) + (row >= 2u ? r1 : 0u) + (row >= 3u ? r2 : 0u) + (incl - cnt);
    };
    // one record of some lanes of the wave (the wave's turns: words beyond a lane's own, long lists): a ballot, one reservation
    auto emit1 = [&](bool kp, uint32_t doc) {
        const unsigned long long m = __ballot((int)kp);
        if (m == 0ull) return;
        uint32_t base = 0;
        if (lane == (uint32_t)__builtin_ctzll(m)) base = atomicAdd(&s_count, (uint32_t)__popcll(m));
        base = __shfl(base, (int)__builtin_ctzll(m));
        if (kp) {
            const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (at < WORDS_REC_CAP) recs[at] = doc; else s_over_recs = 1u;     // (more records than the array takes: the host redoes the batch on the pipeline)
        }
    };
    auto wave_total = [&](uint32_t v) -> unsigned long long {
        const uint32_t incl = scan16(v);                                     // (the whole wave is here)
        return (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)incl, 15) + (uint32_t)__builtin_amdgcn_readlane((int)incl, 31) +
               (uint32_t)__builtin_amdgcn_readlane((int)incl, 47) + (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    };
    // (FILT) a doc of column s that a newer segment supersedes
    auto dead_in = [&](uint32_t s, uint32_t doc) -> bool {
        if constexpr (!FILT) return false;
        return any_dead && s_has_dead[s] != 0u && is_dead_seg(ga.segs[s_seg_index[s]], doc);
    };

    for (uint32_t q = blockIdx.x; q < a.B; q += gridDim.x) {
        const uint64_t q_lo = a.offsets[q];
        const uint32_t n_raw = (uint32_t)(a.offsets[q + 1] - q_lo);
        const bool too_long = n_raw > QS_MAX_HASHES;          // (the host takes no such batch; a query that long would overrun its hash set)
        const uint32_t n = too_long ? 0u : n_raw;
        const uint32_t* qh = a.hashes_base + q_lo;
        const uint32_t rounds = (n + WORDS_WG - 1u) / WORDS_WG;
        // the query's hash set: 2^sbits >= 2 n slots
        uint32_t sbits = 8u;
        while ((1u << sbits) < 2u * n) ++sbits;
        __syncthreads();                                    // (the query before: its candidate buffer and flags have been read)
        for (uint32_t i = tid; i < (1u << sbits); i += WORDS_WG) recs[i] = 0xFFFFFFFFu;
        for (uint32_t i = tid; i < (1u << (QS_FLOG2 - 1u)); i += WORDS_WG) filter[i] = 0u;
        for (uint32_t s = tid; s < T; s += WORDS_WG) table[s] = 0ull;
        if (tid == 0) {
            s_count = 0u; s_over_recs = too_long ? 1u : 0u; s_seen_ones = 0u; s_ccnt = 0u; s_cshared = 0u;
            wg_blocks = 0; wg_docs = 0;
            s_cancel = cancel_requested(a.cancel, a.counters) ? 1u : 0u;      // cancel point (src/FileSegment.zig:144), once per query
        }
        __syncthreads();
        if (s_cancel) return;
        // ---- dedupSorted (src/Index.zig:171-172,489-499): the first occurrence of a hash is the probe, later ones are dropped.  A lane notes
        //      which of its rounds' hashes are probes (a hash-window slice of the group leaves the other hashes to another rank)
        uint32_t vmask = 0u;
        uint32_t mmask = 0u;                                // (MEM) ... and which of them the memory segments' table may hold: a bit per 256 hash values
        for (uint32_t r = 0; r < rounds; ++r) {
            const uint32_t i = r * WORDS_WG + tid;
            if (i >= n) continue;
            const uint32_t h = gload_u32(qh + i);
            uint32_t mb = 0xFFFFFFFFu;
            if constexpr (MEM) { if (a.mem_bits != nullptr) mb = gload_u32(a.mem_bits + ((h >> MEMTAB_FILTER_SHIFT) >> 5)); }
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
            const uint32_t h = valid ? gload_u32(qh + r * WORDS_WG + tid) : 0u;
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
                hist_observe(wg_h, xeff, (x.x >> 16) & 7u);
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
                if (cnt != 0u && at + cnt > WORDS_REC_CAP) { s_over_recs = 1u; keep = 0u; xkeep = 0u; }
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
                            hist_observe(wg_h, eff, (hdr >> 16) & 7u);
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
                    mh[u] = act ? gload_u32(qh + (c0 + u) * WORDS_WG + tid) : 0u;
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
                            const uint32_t at = atomicAdd(&s_count, 1u);
                            if (at < WORDS_REC_CAP) recs[at] = (uint32_t)it; else s_over_recs = 1u;
                        }
                    }
            }
        }
        // ---- the query's statistics (what FileSegment.search observes per hash, summed: src/FileSegment.zig:177-178)
        {
            const unsigned long long w_reads = wave_total(my_reads), w_blocks = wave_total(my_blocks), w_docs = wave_total(my_docs),
                                     w_probes = wave_total(my_probes & 0xFFFFu);
            const uint32_t w_doubles = (uint32_t)wave_total(my_probes >> 16);
            if (lane == 0u) {
                if (w_doubles) atomicAdd(&wg_h[0], w_doubles);                       // (two docs: the second bucket of the docs histogram)
                if (w_reads) atomicAdd(&tot_reads, w_reads);
                if (w_blocks) { atomicAdd(&wg_blocks, w_blocks); atomicAdd(&tot_blocks, w_blocks); }
                if (w_docs) { atomicAdd(&wg_docs, w_docs); atomicAdd(&tot_docs, w_docs); }
                if (w_probes) atomicAdd(&tot_probes, w_probes);
            }
        }
        __syncthreads();                                    // (the records are complete)
        const uint32_t nrec = min(s_count, WORDS_REC_CAP);
        // ---- SearchResults.incr (src/common.zig:121-129), first the filter: every record into its doc's cell
        for (uint32_t i = tid * 4u; i < nrec; i += WORDS_WG * 4u) {
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
            if (s_over_recs || s_count > WORDS_REC_CAP) atomicMax(&a.counters[CTR_BINFAIL], 1ull);
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
                    for (uint32_t s = tid; s < T; s += WORDS_WG) table[s] = 0ull;
                }
                if (tid == 0) { s_claimed = 0u; s_full = 0u; }
                __syncthreads();                            // (the first pass: the filter's counts are complete behind this barrier)
                for (uint32_t i4 = tid * 4u; i4 < nrec; i4 += WORDS_WG * 4u) {
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
                    for (uint32_t s = tid; s < T; s += WORDS_WG) table[s] = 0ull;
                    passes = np; pass = 0xFFFFFFFFu;           // (++pass: 0 again; nothing has been emitted yet)
                    continue;
                }
                if (s_full != 0u && tid == 0) atomicMax(&a.counters[CTR_BINFAIL], 1ull);
                // candidates: count >= the floor -> the query's buffer in LDS (its first SB_CAND), the rest to the shared list
                for (uint32_t s = tid; s < T; s += WORDS_WG) {
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
        if (tot_blocks && g->block_size != 512u) atomicAdd(&st[5], tot_blocks * (unsigned long long)g->block_size - tot_blocks * 512ull);
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
