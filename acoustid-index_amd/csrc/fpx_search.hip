// fpx_search.hip -- the /_search hot path on MI355X (gfx950, wave64).
//
// Reference path being replaced (all CPU, per query, per segment, per hash):
//   IndexReader.search      src/Index.zig:170-177      sort + dedup, drive segments, finish
//   FileSegment.search      src/FileSegment.zig:135-180 block_index lower_bound, <=4 blocks / >1000 docs caps
//   BlockReader.searchHash  src/block.zig:137-158,217-271 StreamVByte 0124 hash decode, equalRange, 1234 docid decode
//   MemorySegment.search    src/MemorySegment.zig:44-54
//   SearchResults.incr/finish src/common.zig:121-171  + Segments.hasNewerCommit src/Index.zig:133-149
//
// GPU formulation (a batch of B queries at once) -- two of them, chosen per batch by run_batch, which fills a Batch and calls one driver:
//   A. a snapshot that is ONE packed group (the resident index between merges): k_search_query (fpx_qsearch.hpp), a QUERY PER WORKGROUP --
//      dedup, the group's lines, counting and the floor in one kernel, the hit records never leaving the CU -- then k_finish, k_publish
//      (run_query_wg; run_side_wg for the file segments next to the group; run_words_wg -- option words_wg, k_search_words in
//      fpx_qwords.hpp -- for a snapshot that is one group in directory + words form).  A batch with queries whose floor is 1 or 2 is B's,
//      or -- option low_wg: 1 an unfiltered packed group, 2 a filtered one too -- run_query_wg's with k_search_low (k_search_low_filt) in
//      k_search_query's place (3: as 2, with k_search_low_coop where filt_coop = 1 would run k_search_filt).  A snapshot of SEVERAL packed groups is B's, or -- option groups_wg = 1 -- run_query_wg's: the groups walked
//      one after the other, k_search_query over the first, k_search_next over the others, one k_finish.  Both together -- several groups
//      and a low floor in the batch -- are B's, or, option groups_wg = 2 with low_wg, run_query_wg's: k_search_low (k_search_low_filt)
//      over the first group, k_search_low_next over the others.
//   B. everything else, the pipeline over all the batch's hashes (make_keys, launch_probes; run_device_sized, run_single or run_general):
//      1. k_make_keys*     (hash, q) keys, packed hash << QB | q; ordered by hash bucket (fpx_keyorder.hpp / fpx_sort.hip) or per query in LDS:
//                          duplicates become adjacent (dedupSorted) and neighbouring probes walk neighbouring lines
//      2. probe kernels    by storage form -- blocks: k_probe (fpx_probe_generic.hpp), k_probe_lean8 (fpx_probe_lean.hpp), k_probe_small;
//                          direct-addressed: k_probe_direct, k_probe_group, k_probe_pgroup; memory segments: k_probe_memtab
//      3. scoring          records binned by the probe kernel and scored a bin per workgroup (k_score_bin), or partitioned by query
//                          (fpx_partition.hpp) and counted by k_score: a counting filter + an exact table in LDS, score >= min_score
//      4. k_finish         (score desc, doc asc), relative cut-off, top-k; k_merge for per-rank partial tables
// Integer gather/scan work: HBM-request-bound, no MFMA.  This file holds the host side: run_batch and the C-ABI implementations.
#include <cstdio>
#include <cstring>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <thread>
#include <type_traits>
#include <vector>

#include "fpx_internal.h"


#include "fpx_kernels_common.hpp"
#include "fpx_keyorder.hpp"
#include "fpx_probe_generic.hpp"
#include "fpx_probe_lean.hpp"
#include "fpx_direct.hpp"
#include "fpx_group.hpp"
#include "fpx_pgroup.hpp"
#include "fpx_probe_small.hpp"
#include "fpx_score.hpp"
#include "fpx_score_bin.hpp"
#include "fpx_qsearch.hpp"
#include "fpx_qframe.hpp"
#include "fpx_qside.hpp"
#include "fpx_qwords.hpp"

namespace fpx {

// ------------------------------------------------------------------------------------------------
// bucket table: bucket[k] = lower_bound(block_index, k << shift), bucket[nb] = num_blocks
// ------------------------------------------------------------------------------------------------
__global__ void k_build_buckets(const uint32_t* __restrict__ block_index, uint32_t num_blocks, uint32_t shift,
                                uint32_t nbuckets, uint32_t* __restrict__ bucket)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nbuckets) return;
    if (k == nbuckets) { bucket[k] = num_blocks; return; }
    const uint32_t h = shift >= 32u ? 0u : (k << shift);
    uint32_t lo = 0, hi = num_blocks;
    while (lo < hi) {
        uint32_t m = (lo + hi) >> 1;
        if (block_index[m] < h) lo = m + 1; else hi = m;
    }
    bucket[k] = lo;
}

int build_bucket_table(Segment* seg, hipStream_t stream)
{
    // about one block per bucket (the table costs 4 B per block, < 1 % of the blocks): the lower_bound that follows the
    // bucket lookup then takes 0-1 dependent loads instead of 3-4 -- 1 % of the lean kernel's time
    uint32_t bits = 0;
    while (bits < 25u && (1ull << bits) < (uint64_t)seg->num_blocks) ++bits;
    seg->num_buckets = 1u << bits;
    seg->bucket_shift = 32u - bits;
    FPX_HIP(dmalloc(&seg->d_bucket, ((size_t)seg->num_buckets + 1) * sizeof(uint32_t)));
    seg->device_bytes += ((size_t)seg->num_buckets + 1) * sizeof(uint32_t);
    const uint32_t n = seg->num_buckets + 1;
    hipLaunchKernelGGL(k_build_buckets, dim3((n + 255) / 256), dim3(256), 0, stream,
                       seg->d_block_index, seg->num_blocks, seg->bucket_shift, seg->num_buckets, seg->d_bucket);
    FPX_HIP(hipGetLastError());
    return FPX_OK;
}

// the snapshot's ONE table of its memory segments' live postings (fpx_probe_small.hpp: k_probe_memtab)
int build_memtab(Snapshot* sn)
{
    uint64_t total = 0, mmax = 0;
    for (const MemDesc& m : sn->h_mem) { total += m.num_items; mmax = std::max<uint64_t>(mmax, m.num_items); }
    if (total == 0) return FPX_OK;                                      // (nothing to look up)
    if (total >= 0xFFFFFFF0ull) { set_error("a snapshot's memory segments hold %llu items: their table's offsets are 32 bits", (unsigned long long)total); return FPX_E_INVAL; }
    uint64_t* buf[2] = {nullptr, nullptr};
    unsigned long long* d_count = nullptr;
    void* d_temp = nullptr;
    uint32_t* d_bucket = nullptr;
    auto fail = [&](int rc) { for (auto* b : buf) if (b) (void)hipFree(b); if (d_count) (void)hipFree(d_count); if (d_temp) (void)hipFree(d_temp); if (d_bucket) (void)hipFree(d_bucket); (void)hipGetLastError(); return rc; };
    const size_t tb = sort_u64_temp_bytes(total, 0, 64);
    if (dmalloc(&buf[0], (total + 1) * 8) != hipSuccess || dmalloc(&buf[1], (total + 1) * 8) != hipSuccess || dmalloc(&d_count, 8) != hipSuccess ||
        dmalloc(&d_temp, tb + 256) != hipSuccess || dmalloc(&d_bucket, ((size_t)(1u << MEMTAB_BITS) + 2) * sizeof(uint32_t)) != hipSuccess)
        return fail(FPX_E_NOMEM);
    hipStream_t st = 0;
    if (hipMemsetAsync(d_count, 0, 8, st) != hipSuccess) return fail(FPX_E_DEVICE);
    const uint32_t gx = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, (mmax + WG - 1) / WG), 1024);
    hipLaunchKernelGGL(k_memtab_gather, dim3(gx, sn->n_mem), dim3(WG), 0, st, (const MemDesc*)sn->d_mem, buf[0], d_count);
    unsigned long long n = 0;
    if (hipMemcpyAsync(&n, d_count, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(FPX_E_DEVICE);
    int cur = 0;
    // (the whole key: Item order, src/segment.zig:90-94 -- hash, then doc)
    if (n > 1 && sort_u64(d_temp, tb + 256, buf[0], buf[1], n, 0, 64, st, &cur) != hipSuccess) return fail(FPX_E_DEVICE);
    hipLaunchKernelGGL(k_memtab_buckets, dim3(((1u << MEMTAB_BITS) + 256) / 256), dim3(256), 0, st, (const uint64_t*)buf[cur], (uint64_t)n, d_bucket);
    // (the presence bits: optional -- without them the kernel starts at the bucket table)
    uint32_t* d_bits = nullptr;
    const size_t bits_bytes = ((size_t)1 << (32u - MEMTAB_FILTER_SHIFT)) / 8u;
    if (n != 0 && dmalloc(&d_bits, bits_bytes) == hipSuccess) {
        if (hipMemsetAsync(d_bits, 0, bits_bytes, st) != hipSuccess) { (void)hipFree(d_bits); d_bits = nullptr; }
        else hipLaunchKernelGGL(k_memtab_bits, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, (const uint64_t*)buf[cur], (uint64_t)n, d_bits);
    }
    (void)hipGetLastError();
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { if (d_bits) (void)hipFree(d_bits); return fail(FPX_E_DEVICE); }
    sn->d_memtab = buf[cur]; sn->d_membucket = d_bucket; sn->n_memtab = n; sn->d_membits = d_bits;
    (void)hipFree(buf[1 - cur]); (void)hipFree(d_count); (void)hipFree(d_temp);
    return FPX_OK;
}

// ------------------------------------------------------------------------------------------------
// workspace
// ------------------------------------------------------------------------------------------------
template <class T>
static int grow(T** p, size_t* cap, size_t need, size_t slack_num = 5, size_t slack_den = 4)
{
    if (need <= *cap) return FPX_OK;
    size_t ncap = need * slack_num / slack_den + 64;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    hipError_t e = dmalloc(reinterpret_cast<void**>(p), ncap * sizeof(T));
    if (e != hipSuccess) { set_error("hipMalloc(%zu bytes) failed: %s", ncap * sizeof(T), hipGetErrorString(e)); return FPX_E_NOMEM; }
    *cap = ncap;
    return FPX_OK;
}

static int grow_pair(uint64_t* p[2], size_t* cap, size_t need)
{
    if (need <= *cap) return FPX_OK;
    size_t c0 = *cap, c1 = *cap;
    int rc = grow(&p[0], &c0, need);
    if (rc) return rc;
    rc = grow(&p[1], &c1, need);
    if (rc) return rc;
    *cap = std::min(c0, c1);
    return FPX_OK;
}

// n keys of pair[0] sorted on their bits [lo, hi), with the workspace's temporary storage; *cur: which of the pair holds them afterwards
static int sort_keys(Workspace* ws, uint64_t* pair[2], uint64_t n, unsigned lo, unsigned hi, hipStream_t st, int* cur)
{
    const size_t tb = sort_u64_temp_bytes(n, lo, hi);
    if (const int rc = grow(reinterpret_cast<uint8_t**>(&ws->d_temp), &ws->cap_temp, tb + 256)) return rc;
    FPX_HIP(sort_u64(ws->d_temp, ws->cap_temp, pair[0], pair[1], n, lo, hi, st, cur));
    return FPX_OK;
}

// ---- the one launcher of kernel templates K<NS, flags...>: run-time flags become compile-time constants, IN ORDER, and that instantiation
// is launched.  The flags at a call site stand in the kernel's OWN template-parameter order, behind ns8 (NS: 8 | 16 columns of a directory
// line).  A flag is a `bool` and nothing else: a pointer or a count in a flag's place does not compile.
template <class F> static void with_flags(F&& f) { f(); }
template <class F, class B, class... Bs> static void with_flags(F&& f, B flag, Bs... rest)
{
    static_assert(std::is_same<B, bool>::value, "a kernel's flag is a bool");
    if (flag) with_flags([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
    else with_flags([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}
template <class F, class... Bs> static void with_ns(bool ns8, F&& f, Bs... flags)
{
    if (ns8) with_flags([&](auto... cs) { f(std::integral_constant<int, 8>{}, cs...); }, flags...);
    else with_flags([&](auto... cs) { f(std::integral_constant<int, 16>{}, cs...); }, flags...);
}
// (a macro: a function template's name cannot be passed as an argument.  a0, a1: the kernel's two by-value parameters)
#define FPX_LAUNCH(K, grid, wg, lds, st, a0, a1, ns8, ...) \
    with_ns(ns8, [&](auto ns, auto... cs) { hipLaunchKernelGGL((K<decltype(ns)::value, decltype(cs)::value...>), grid, dim3(wg), lds, st, a0, a1); }, __VA_ARGS__)
// (the query-per-workgroup family of fpx_qsearch.hpp: one workgroup size, one LDS size)
#define FPX_LAUNCH_QS(K, grid, st, qa, g, ns8, ...) FPX_LAUNCH(K, grid, QS_WG, QS_LDS_BYTES, st, qa, g, ns8, __VA_ARGS__)

// k_probe_group<NS, BINNED, QS> -- records binned in the flush, per-query scan statistics --, or k_probe_pgroup for a dense group: its words
// live in its lines (fpx_pgroup.hpp)
static void launch_probe_group(bool packed, bool ns8, bool binned, bool qs, dim3 grid, hipStream_t st, const ProbeArgs& a, const GroupArgs& g)
{
    const size_t stage = (size_t)FSTAGE_CAP * sizeof(uint64_t);
    if (packed) FPX_LAUNCH(k_probe_pgroup, grid, FK_WG, stage + PK_HEAD_LDS, st, a, g, ns8, binned, qs);      // (+ the prefetched line heads)
    else FPX_LAUNCH(k_probe_group, grid, FK_WG, stage + (binned ? (size_t)FSTAGE_CAP * sizeof(uint16_t) : 0u), st, a, g, ns8, binned, qs);      // (+ ranks)
}

constexpr int FPX_SPLIT = 1;   // internal: candidate key does not fit 64 bits, split the batch
constexpr int FPX_REDO_QS = 3; // internal: the one-workgroup-per-query path gave up (a query's records outgrew its LDS array, scores too wide): the pipeline
constexpr int FPX_REDO = 2;    // internal: the device-sized or the single-query path met something only the general path handles (a full bin, ...)
// (option hot_wg) queries of a batch of B that k_search_classes redoes in doc classes; a batch with more of them goes to the pipeline.
// A policy guess, not a measurement: an eighth of the batch, and a handful for a small one.
constexpr uint32_t QS_REDO_MIN = 4, QS_REDO_SHARE = 8;
constexpr uint32_t qs_redo_limit(uint32_t B) { return B / QS_REDO_SHARE > QS_REDO_MIN ? B / QS_REDO_SHARE : QS_REDO_MIN; }

static unsigned bits_for(uint64_t n)   // number of bits needed to represent values in [0, n)
{
    unsigned b = 0;
    while (b < 64 && (1ull << b) < n) ++b;
    return b;
}

// per-query arrays (offsets, options, result counts) share one capacity
static int ensure_queries(Workspace* ws, size_t B)
{
    if (B + 1 <= ws->cap_queries && ws->d_offsets && ws->d_opts && ws->d_out_n) return FPX_OK;
    const size_t cap = (B + 1) * 5 / 4 + 64;
    if (ws->d_offsets) (void)hipFree(ws->d_offsets);
    if (ws->d_opts) (void)hipFree(ws->d_opts);
    if (ws->d_out_n) (void)hipFree(ws->d_out_n);
    ws->d_offsets = nullptr; ws->d_opts = nullptr; ws->d_out_n = nullptr; ws->cap_queries = 0;
    if (dmalloc(&ws->d_offsets, cap * sizeof(uint64_t)) != hipSuccess ||
        dmalloc(&ws->d_opts, cap * 4 * sizeof(uint32_t)) != hipSuccess ||
        dmalloc(&ws->d_out_n, cap * sizeof(uint32_t)) != hipSuccess) {
        set_error("hipMalloc(query arrays) failed");
        return FPX_E_NOMEM;
    }
    ws->cap_queries = cap;
    return FPX_OK;
}

// a query's effective floor -- src/MultiIndex.zig:304: the default floor uses the RAW query length (before dedup)
static uint32_t query_floor(const fpx_opts& o, uint64_t raw_len) { return o.has_min_score ? o.min_score : (uint32_t)((raw_len + 19) / 20); }
static uint32_t min_floor(const uint64_t* offsets, const fpx_opts* opts, uint32_t B)
{
    uint32_t lo = 0xFFFFFFFFu;
    for (uint32_t q = 0; q < B; ++q) lo = std::min(lo, query_floor(opts[q], offsets[q + 1] - offsets[q]));
    return lo;
}

static void fill_opts(std::vector<uint32_t>& h_opts, const fpx_opts* opts, const uint64_t* offsets, uint32_t B)
{
    h_opts.resize((size_t)B * 4);
    for (uint32_t q = 0; q < B; ++q) {
        const uint64_t raw_len = offsets[q + 1] - offsets[q];
        h_opts[q * 4 + 0] = opts[q].max_results;
        h_opts[q * 4 + 1] = query_floor(opts[q], raw_len);
        h_opts[q * 4 + 2] = opts[q].min_score_pct;
        h_opts[q * 4 + 3] = (uint32_t)raw_len;
    }
}

static double now_ms()
{
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// Wait for the call's stream.  With a deadline the host thread polls instead of blocking: when the deadline passes it
// sets the workspace's cancel word (pinned, mapped into the device), the running kernels leave at their next cancel
// point (cancel_requested), the rest of the queue drains in microseconds, and the call reports error.SearchTimeout
// (src/MultiIndex.zig:314-322) with no partial results -- promptly, not after the batch has run to completion.
static int sync_deadline(Workspace* ws, double t_start, uint32_t timeout_ms)
{
    hipStream_t st = ws->stream;
    if (timeout_ms == 0) { FPX_HIP(hipStreamSynchronize(st)); return FPX_OK; }
    bool fired = *reinterpret_cast<volatile uint32_t*>(ws->h_cancel) != 0u;
    for (uint32_t spins = 0;; ++spins) {
        const hipError_t e = hipStreamQuery(st);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) return hip_fail(e, "hipStreamQuery");
        if (!fired && now_ms() - t_start > (double)timeout_ms) {
            __atomic_store_n(ws->h_cancel, 1u, __ATOMIC_RELEASE);
            fired = true;
        }
        if (spins < 512u) std::this_thread::yield();                       // a single /_search completes within this window
        else std::this_thread::sleep_for(std::chrono::microseconds(fired ? 5 : 40));
    }
    if (fired) { set_error("search timeout"); return FPX_E_TIMEOUT; }
    return FPX_OK;
}
#define FPX_SYNC(ws) do { const int _rc = sync_deadline((ws), t_start, timeout_ms); if (_rc != FPX_OK) return _rc; } while (0)
#define FPX_SYNC_BATCH(b) do { const int _rc = sync_deadline((b).ws, (b).t_start, (b).timeout_ms); if (_rc != FPX_OK) return _rc; } while (0)

// The count table of the batch's key order (fpx_keyorder.hpp): `bits` hash bits below the `win_bits` a hash window fixes, fewer
// when the table would outgrow KO_MAX_CELLS.  Layout of ws->d_kocnt: [B x nb counts | nb totals | pad | the key count (u64)].
static int key_order_setup(Workspace* ws, uint32_t B, unsigned win_bits, unsigned bits, KeyOrder* ko, unsigned long long** P_dev, hipStream_t st, bool rows = false)
{
    const uint32_t G = (B + KO_GROUP - 1u) / KO_GROUP;
    bits = std::min(bits, 8u);                       // KO_MAX_BUCKETS
    while (bits > 0u && ((uint64_t)G << bits) > KO_MAX_CELLS) --bits;
    const uint32_t nb = 1u << bits;
    const size_t rows_at = ((size_t)G * nb + nb + 4 + (P_dev ? (size_t)B : 0) + 31) & ~(size_t)31;      // (the queries' rows of counts, a 128-byte boundary)
    const size_t words = rows_at + (rows ? (size_t)B * nb : 0);
    if (words > ws->cap_kocnt) {
        if (ws->d_kocnt) (void)hipFree(ws->d_kocnt);
        ws->d_kocnt = nullptr; ws->cap_kocnt = 0;
        hipError_t e = dmalloc(&ws->d_kocnt, words * sizeof(uint32_t));
        if (e != hipSuccess) { set_error("hipMalloc(%zu bytes) failed: %s", words * sizeof(uint32_t), hipGetErrorString(e)); return FPX_E_NOMEM; }
        ws->cap_kocnt = words;
    }
    ko->cnt = ws->d_kocnt;
    ko->totals = ws->d_kocnt + (size_t)G * nb;
    ko->nb = nb;
    ko->bshift = std::min(31u, 32u - std::min(32u, win_bits + bits));
    if (P_dev) {                                     // (windowed keys: their number lives on the device, per query and in all)
        *P_dev = reinterpret_cast<unsigned long long*>(ws->d_kocnt + (((size_t)G * nb + nb + 1) & ~(size_t)1));
        ko->qn = ws->d_kocnt + (size_t)G * nb + nb + 4;
    }
    ko->qrows = rows ? ws->d_kocnt + rows_at : nullptr;      // (k_group_hist stores every cell of cnt: nothing to zero)
    if (!rows) FPX_HIP(hipMemsetAsync(ko->cnt, 0, (size_t)G * nb * sizeof(uint32_t), st));
    return FPX_OK;
}
// from this many queries on k_make_keys_dedup stores its query's counts as a row and k_group_hist adds the groups' rows (no atomics)
constexpr uint32_t KO_ROWS_MIN_B = 2048;

// What the host looks at after a device-sized batch -- counters, the kernels' statistics, the bins' fill counts -- is written by
// ONE small kernel into page-locked host memory that is mapped into the device, and k_finish writes a small batch's results there
// itself: no copy calls at the end of the stream.  Five hipMemcpyAsync(DeviceToHost) alternated between the copy engines and
// blit kernels, with a cross-engine wait each time: a gap of 40 - 140 us after k_finish, a third of a 1024-query batch's step.
struct PublishArgs {
    const unsigned long long* counters; unsigned long long* h_counters;
    const uint32_t* a_src; uint32_t* a_dst; uint32_t a_n;                       // contiguous words: deferred-list counts + statistics sets
    const uint32_t* b_src; uint32_t* b_dst; uint32_t b_n, b_stride;              // the bins' counts, compacted
};
__global__ __launch_bounds__(256) void k_publish(PublishArgs p)
{
    const uint32_t i0 = blockIdx.x * 256u + threadIdx.x, step = gridDim.x * 256u;
    if (i0 < CTR_COUNT) p.h_counters[i0] = p.counters[i0];
    for (uint32_t i = i0; i < p.a_n; i += step) p.a_dst[i] = p.a_src[i];
    for (uint32_t i = i0; i < p.b_n; i += step) p.b_dst[i] = p.b_src[(size_t)i * p.b_stride];
}
template <typename T> static T* mapped_address(T* host)
{
    void* d = nullptr;
    return hipHostGetDevicePointer(&d, host, 0) == hipSuccess ? static_cast<T*>(d) : nullptr;
}

// Results leave through pinned staging (see Workspace::h_out): enqueue the two copies, and after the stream has been
// waited for, hand the bytes to the caller.  Beyond a megabyte the host's second copy costs more than the driver's slow
// path saves (2.6 MB at batch 8192: +0.08 ms): those go directly, after the wait.
constexpr size_t STAGED_OUT_MAX = (size_t)1 << 20;
static int ensure_h_out(Workspace* ws, size_t bytes)
{
    if (bytes <= ws->cap_h_out) return FPX_OK;
    if (ws->h_out) (void)hipHostFree(ws->h_out);
    ws->h_out = nullptr; ws->cap_h_out = 0;
    const size_t ncap = bytes * 5 / 4 + 4096;
    FPX_HIP(hipHostMalloc(reinterpret_cast<void**>(&ws->h_out), ncap, hipHostMallocMapped));
    ws->cap_h_out = ncap;
    return FPX_OK;
}
static int stage_results(Workspace* ws, uint32_t B, uint32_t out_cap, hipStream_t st, bool* staged)
{
    const size_t bytes = (size_t)B * sizeof(uint32_t) + (size_t)B * out_cap * sizeof(fpx_result);
    *staged = bytes <= STAGED_OUT_MAX;
    if (!*staged) return FPX_OK;
    if (const int rc = ensure_h_out(ws, bytes)) return rc;
    FPX_HIP(hipMemcpyAsync(ws->h_out, ws->d_out_n, (size_t)B * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (out_cap) FPX_HIP(hipMemcpyAsync(ws->h_out + (size_t)B * sizeof(uint32_t), ws->d_out, (size_t)B * out_cap * sizeof(fpx_result), hipMemcpyDeviceToHost, st));
    return FPX_OK;
}
// the same staging, filled by k_finish itself: where it writes a batch's counts and results (mapped addresses of h_out)
static int staged_targets(Workspace* ws, uint32_t B, uint32_t out_cap, bool* staged, uint32_t** d_n, fpx_result** d_res)
{
    const size_t bytes = (size_t)B * sizeof(uint32_t) + (size_t)B * out_cap * sizeof(fpx_result);
    *staged = bytes <= STAGED_OUT_MAX;
    if (!*staged) return FPX_OK;
    if (const int rc = ensure_h_out(ws, bytes)) return rc;
    uint8_t* d = mapped_address(ws->h_out);
    if (!d) { *staged = false; return FPX_OK; }
    *d_n = reinterpret_cast<uint32_t*>(d);
    *d_res = reinterpret_cast<fpx_result*>(d + (size_t)B * sizeof(uint32_t));
    return FPX_OK;
}
static int deliver_results(Workspace* ws, uint32_t B, uint32_t out_cap, bool staged, fpx_result* out, uint32_t* out_n, hipStream_t st)
{
    if (staged) {                                   // (the stream has been synchronised)
        std::memcpy(out_n, ws->h_out, (size_t)B * sizeof(uint32_t));
        if (out_cap) std::memcpy(out, ws->h_out + (size_t)B * sizeof(uint32_t), (size_t)B * out_cap * sizeof(fpx_result));
        return FPX_OK;
    }
    FPX_HIP(hipMemcpyAsync(out_n, ws->d_out_n, (size_t)B * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (out_cap) FPX_HIP(hipMemcpyAsync(out, ws->d_out, (size_t)B * out_cap * sizeof(fpx_result), hipMemcpyDeviceToHost, st));
    FPX_HIP(hipStreamSynchronize(st));
    return FPX_OK;
}

// ------------------------------------------------------------------------------------------------
// batch driver
// ------------------------------------------------------------------------------------------------
// `offsets` are absolute positions into the batch the view [q0, q0+B) belongs to; `hashes` (host) points at
// absolute position 0 and is only read when the batch is not resident.
static uint64_t lean_min_probes(const Ctx* c) { return (uint64_t)std::max<int64_t>(0, ctx_opt(c, OPT_LEAN_MIN)); }

// Hash-range sharding of one segment (second mode) cuts the pipeline at the hit records: a doc's
// postings may come from several GPUs, so the records travel (grouped by doc & (world - 1)) before they are counted.
struct Exchange {
    int mode = 0;                 // 1: probe only, records out;  2: score only, records in
    uint32_t world = 1;           // mode 1: number of destination ranks (power of two)
    uint64_t* d_records = nullptr; uint64_t cap = 0;   // mode 1: destination buffer;  mode 2: source
    uint64_t n = 0;               // mode 2: number of records
    uint64_t* counts = nullptr;   // mode 1: records per destination rank [world]
};

// records sorted by (rec & mask): first index whose destination is >= d, for d = 0 .. world
__global__ void k_dest_bounds(const uint64_t* __restrict__ recs, uint64_t n, uint32_t mask, uint32_t world, uint64_t* __restrict__ bounds)
{
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d > world) return;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t m = (lo + hi) >> 1;
        if (((uint32_t)recs[m] & mask) < d) lo = m + 1; else hi = m;
    }
    bounds[d] = lo;
}

// The scan histogram slots of a batch that has reached the host (fpx_internal.h, HIST_SLOTS): what small launches added to the batch's
// counters + the spread sets behind the statistics sets (`sets`: the [LEAN_STAT_SETS][8] statistics, or null); `probes`: every (hash,
// file segment) walk of the batch -- every probe kernel observes its own, so none is left over (dst[HIST_SLOTS]: counted, not bucketed).
static void gather_hist(uint64_t* dst, const unsigned long long* h_counters, const unsigned long long* sets, uint64_t probes)
{
    for (uint32_t i = 0; i < HIST_SLOTS; ++i) dst[i] = h_counters[CTR_HIST + i];
    // (kernels that keep their statistics in the batch's counters leave the histograms' totals to them: hist_publish)
    dst[HIST_COUNT] += h_counters[CTR_PROBES]; dst[HIST_DOCS] += h_counters[CTR_DOCS]; dst[HIST_BLOCKS] += h_counters[CTR_BLOCKS];
    if (sets) {
        const unsigned long long* hs = sets + (size_t)LEAN_STAT_SETS * 8;
        for (uint32_t k = 0; k < LEAN_STAT_SETS; ++k)
            for (uint32_t i = 0; i < HIST_SLOTS; ++i) dst[i] += hs[(size_t)k * HIST_SLOTS + i];
    }
    dst[HIST_SLOTS] = probes > dst[HIST_COUNT] ? probes - dst[HIST_COUNT] : 0ull;
}
void ctx_hist_add(Ctx* c, const uint64_t* slots, uint64_t unbucketed)
{
    for (uint32_t i = 0; i < HIST_SLOTS; ++i) if (slots[i]) c->scan_hist[i].fetch_add(slots[i], std::memory_order_relaxed);
    if (unbucketed) c->scan_hist[HIST_SLOTS].fetch_add(unbucketed, std::memory_order_relaxed);
}

// which paths an entry of run_batch may take: run_with_redos walks down this list as a path hands the batch back
enum class Try { First, NoQueryWg, GeneralOnly };

// One entry of run_batch: what every path reads.  run_batch fills it once and passes it by reference -- a plain bag of values.
struct Batch {
    Snapshot* snap; Workspace* ws; hipStream_t st;
    const QueryBatch* resident; uint32_t q0;                                    // a batch resident in HBM, and the view's first query in it
    uint32_t B; uint64_t P, base; unsigned qb;                                  // queries, their hashes, the first one's absolute position, bits of q
    const uint32_t* hashes; const uint64_t* offsets; const fpx_opts* opts;      // the caller's host arrays
    const uint32_t* d_hashes_base; const uint64_t* d_offsets; const uint32_t* d_opts;      // ... and where the kernels read them
    bool staged_single;                                                         // one small query, read from mapped host memory: its positions start at 0
    const uint32_t* cancel; double t_start; uint32_t timeout_ms;
    bool partial; fpx_result* out; uint32_t out_cap; uint32_t* out_n; fpx_stats* stats;
    bool want_q; uint64_t* q_blocks; uint64_t* q_docs;                          // per-query scan statistics, when the caller asked for them
    size_t def_cap, def_stat_off, def_words;                                    // the deferred lists' layout (ws->d_def_count)
    uint32_t up_chunks, up_q[Workspace::UP_CHUNKS + 1];                         // a chunked upload: the pieces' query ranges
};

// ---- steps that several paths share --------------------------------------------------------------------------------------------
// the kernels' statistics, LEAN_STAT_SETS copies of 8 slots on separate cache lines (a workgroup adds to set blockIdx.x % LEAN_STAT_SETS), summed
struct StatSums { unsigned long long reads = 0, blocks = 0, docs = 0, probes = 0, dreads = 0, bytes_off = 0, pads = 0, records = 0; };
static StatSums sum_stat_sets(const unsigned long long* ls)
{
    StatSums s;
    for (uint32_t i = 0; i < LEAN_STAT_SETS; ++i) {
        s.reads += ls[i * 8 + 0]; s.blocks += ls[i * 8 + 1]; s.docs += ls[i * 8 + 2]; s.probes += ls[i * 8 + 3]; s.dreads += ls[i * 8 + 4];
        s.bytes_off += ls[i * 8 + 5];            // (block sizes other than 512 in the direct-addressed forms: the difference, mod 2^64)
        s.pads += ls[i * 8 + 6]; s.records += ls[i * 8 + 7];
    }
    return s;
}
static const unsigned long long* host_stat_sets(const Batch& b) { return reinterpret_cast<const unsigned long long*>(b.ws->h_def_count + b.def_stat_off); }
static unsigned long long* device_stat_sets(const Batch& b) { return reinterpret_cast<unsigned long long*>(b.ws->d_def_count + b.def_stat_off); }
// block bytes the probe kernels fetched, where they kept no spread statistics (k_probe_direct / k_probe_group: 64-byte units)
static unsigned long long unspread_fetched_bytes(const Workspace* ws, const Snapshot* snap)
{
    return snap->n_direct ? ws->h_counters[CTR_LEAN_READS] * 64ull + (snap->n_file ? ws->h_counters[CTR_BYTES] : 0ull) : ws->h_counters[CTR_BYTES];
}
// compute units of the context's device: asked of the runtime once per device
static int device_cus(const Ctx* ctx)
{
    static std::atomic<int> cus_of[64];
    int cus = cus_of[(unsigned)ctx->device & 63u].load(std::memory_order_relaxed);
    if (cus == 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = 256; }
        cus_of[(unsigned)ctx->device & 63u].store(cus, std::memory_order_relaxed);
    }
    return cus;
}
// per-query candidate slots: [B][QCAND_SLOTS] keys, then [B] counts, then the list of heavy queries [B], then `extra_words` of the caller's
// (`extra`); and the shared list the queries with more candidates than slots write to, at its first guess
struct CandSlots { uint64_t* qcand = nullptr; uint32_t* qcand_n = nullptr; uint32_t* heavy = nullptr; uint64_t* extra = nullptr; };
static int ensure_cand_slots(Workspace* ws, uint32_t B, size_t extra_words, CandSlots* cs)
{
    const size_t words = (size_t)B * QCAND_SLOTS + 2 * ((size_t)B / 2 + 1);
    if (const int rc = grow(&ws->d_qcand, &ws->cap_qcand, words + extra_words)) return rc;
    cs->qcand = ws->d_qcand;
    cs->qcand_n = reinterpret_cast<uint32_t*>(ws->d_qcand + (size_t)B * QCAND_SLOTS);
    cs->heavy = reinterpret_cast<uint32_t*>(ws->d_qcand + (size_t)B * QCAND_SLOTS + (size_t)B / 2 + 1);
    cs->extra = ws->d_qcand + words;
    const size_t cand_guess0 = std::max<size_t>(1u << 16, (size_t)B * 64);
    return ws->cap_cands < cand_guess0 ? grow_pair(ws->d_cands, &ws->cap_cands, cand_guess0) : FPX_OK;
}
// where k_finish writes: the caller's device table (`partial`), the workspace's, or -- a small batch -- the pinned staging itself
struct ResultsTo { fpx_result* res; uint32_t* n; bool staged; };
static int results_target(Batch& b, ResultsTo* to)
{
    to->res = b.partial ? b.out : b.ws->d_out;
    to->n = b.partial ? b.out_n : b.ws->d_out_n;
    to->staged = false;
    return b.partial ? FPX_OK : staged_targets(b.ws, b.B, b.out_cap, &to->staged, &to->n, &to->res);
}
// k_finish over the batch: `cands[C]` the sorted shared list, the queries' own slots next to it; count_slots: it adds the slots' candidates up
static void launch_finish(Batch& b, const uint64_t* cands, uint64_t C, uint32_t sb, const CandSlots& cs, fpx_result* d_res, uint32_t* d_res_n, bool count_slots)
{
    hipLaunchKernelGGL(k_finish, dim3((b.B + 127) / 128), dim3(128), 0, b.st,
                       cands, C, b.d_opts, b.B, sb, b.partial ? 1 : 0, d_res, b.out_cap, d_res_n,
                       (const uint64_t*)cs.qcand, (const uint32_t*)cs.qcand_n, count_slots ? b.ws->d_counters : nullptr);
}
// some queries have more candidates than slots: sort the shared list's Cf entries and finish again (second round trip)
static int finish_crowded(Batch& b, uint32_t sb, const CandSlots& cs, const ResultsTo& to, uint64_t Cf)
{
    Workspace* ws = b.ws; int rc, ccur = 0;
    if (Cf != 0 && (rc = sort_keys(ws, ws->d_cands, Cf, 0, 64, b.st, &ccur))) return rc;
    if (b.stats) FPX_HIP(hipMemsetAsync(&ws->d_counters[CTR_SLOTCANDS], 0, sizeof(unsigned long long), b.st));
    launch_finish(b, ws->d_cands[ccur], Cf, sb, cs, to.res, to.n, b.stats != nullptr);
    FPX_HIP(hipGetLastError());
    FPX_HIP(hipMemcpyAsync(&ws->h_counters[CTR_SLOTCANDS], &ws->d_counters[CTR_SLOTCANDS], sizeof(unsigned long long), hipMemcpyDeviceToHost, b.st));
    FPX_HIP(hipEventRecord(ws->ev_end, b.st));
    FPX_SYNC_BATCH(b);
    return FPX_OK;
}
// the batch's counters, and with `stat_sets` the deferred lists' counts and the statistics sets, into the host's mapped copies; b_src: the bins' counts too
constexpr size_t BINQ_HEAD = 64 / sizeof(uint32_t);                          // room for the BinArgs the kernels read
static int publish(Batch& b, bool stat_sets, const uint32_t* b_src = nullptr, uint32_t b_n = 0, uint32_t b_stride = 0)
{
    Workspace* ws = b.ws;
    PublishArgs pa{};
    pa.counters = ws->d_counters; pa.h_counters = mapped_address(ws->h_counters);
    pa.a_src = ws->d_def_count; pa.a_dst = stat_sets ? mapped_address(ws->h_def_count) : nullptr; pa.a_n = stat_sets ? (uint32_t)b.def_words : 0u;
    uint32_t* d_hbins = b_src ? mapped_address(ws->h_bins) : nullptr;
    if (b_src) { pa.b_src = b_src; pa.b_dst = d_hbins + BINQ_HEAD; pa.b_n = b_n; pa.b_stride = b_stride; }
    if (!pa.h_counters || (stat_sets && !pa.a_dst) || (b_src && !d_hbins)) { set_error("page-locked host memory is not mapped into the device"); return FPX_E_DEVICE; }
    hipLaunchKernelGGL(k_publish, dim3(4), dim3(256), 0, b.st, pa);
    FPX_HIP(hipGetLastError());
    return FPX_OK;
}
// did a query-per-workgroup kernel hand the batch back?  (a full LDS array: the snapshot's next batches do not try again at once)
static bool handed_back(const Workspace* ws, Snapshot* snap)
{
    if (ws->h_counters[CTR_BINFAIL] == 0 && ws->h_counters[CTR_MAXSCORE] == 0 && ws->h_counters[CTR_CANDS] <= ws->cap_cands) return false;
    if (ws->h_counters[CTR_BINFAIL] != 0) __atomic_store_n(&snap->qs_skip, 32u, __ATOMIC_RELAXED);
    return true;
}
static int deliver_qstats(Batch& b)
{
    if (!b.want_q) return FPX_OK;
    std::vector<unsigned long long> hq(b.B);
    FPX_HIP(hipMemcpy(hq.data(), b.ws->d_qstats, (size_t)b.B * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (uint32_t q = 0; q < b.B; ++q) {
        if (b.q_blocks) b.q_blocks[q] = hq[q] & 0xFFFFFFFFull;
        if (b.q_docs) b.q_docs[q] = hq[q] >> 32;
    }
    return FPX_OK;
}
// k_score's filter and table: a counting filter sized for ~2x the average number of records per query (8 KB .. 64 KB of LDS) + a 16 KB
// exact table.  The filter only has to keep cells that collect < min_score records below the floor: with the usual floor (n / 20 = 50 for
// 1 k-hash queries) a cell may hold several docs' records and still reject them, so a quarter of the size does; the LDS saved more than
// doubles the resident workgroups (k_score is occupancy bound).  With a floor of 1 or 2 (the legacy protocol) nearly every record passes
// it: the LDS goes to a larger exact table instead, so that the count needs 2 passes rather than 6.
static void score_filter_sizes(uint32_t floor_min, uint64_t H, uint32_t B, uint32_t* log2f_out, uint32_t* log2t_out)
{
    uint32_t log2f = 11;
    while (log2f < 14 && (1ull << log2f) < 2 * (H / B + 1)) ++log2f;
    log2f = std::max(11u, log2f - (floor_min >= 8u ? 2u : floor_min >= 3u ? 1u : 0u));
    uint32_t log2t = SCORE_TABLE_LOG2;
    if (floor_min <= 2u && H / B > (1u << SCORE_TABLE_LOG2)) { log2t = 13; log2f = 11; }
    static const hipError_t lds_attrs[3] = {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_score<32, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024),
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_score<8, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024),
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_score<32, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024)};
    (void)lds_attrs;
    *log2f_out = log2f; *log2t_out = log2t;
}
// k_score over the records in `hits`, by the queries' ranges (ws->d_qrange): ROWS rows of a tile; HEAVY: the queries that launch handed over
template <int ROWS, bool HEAVY>
static void launch_score(Batch& b, uint32_t grid, size_t lds, const uint64_t* hits, uint32_t sizes, uint32_t sb, const CandSlots& cs)
{
    hipLaunchKernelGGL((k_score<ROWS, HEAVY>), dim3(grid), dim3(WG), lds, b.st, hits, (const uint64_t*)b.ws->d_qrange, b.d_opts, sizes, sb, b.ws->d_cands[0],
                       (uint64_t)b.ws->cap_cands, b.ws->d_counters, (uint64_t)0, cs.qcand, cs.qcand_n, cs.heavy, b.cancel);
}

// ---- the batch's way to the device -------------------------------------------------------------------------------------------------
// piece c of a chunked upload's hashes, on the copy stream; its event behind it
static int upload_piece(Batch& b, uint32_t c)
{
    Workspace* ws = b.ws;
    const uint64_t h0 = b.offsets[b.up_q[c]] - b.base, h1 = b.offsets[b.up_q[c + 1]] - b.base;
    if (h1 > h0) FPX_HIP(hipMemcpyAsync(ws->d_hashes + h0, b.hashes + b.base + h0, (h1 - h0) * sizeof(uint32_t), hipMemcpyHostToDevice, ws->copy_stream));
    FPX_HIP(hipEventRecord(ws->ev_chunk[c], ws->copy_stream));
    return FPX_OK;
}
// the batch: resident in HBM already, or uploaded from the caller's host buffers (query_wg: the batch goes to k_search_query)
static int place_batch(Batch& b, bool query_wg)
{
    Workspace* ws = b.ws; hipStream_t st = b.st; const uint32_t B = b.B; const uint64_t P = b.P, base = b.base; int rc;
    if (b.resident) {
        b.d_hashes_base = b.resident->d_hashes;
        b.d_offsets = b.resident->d_offsets + b.q0;
        b.d_opts = b.resident->d_opts + (size_t)b.q0 * 4;
        return FPX_OK;
    }
    if (B == 1 && 32 + P * sizeof(uint32_t) <= STAGE_BYTES) {
        // one small query: offsets, options and hashes travel in a single copy from pinned memory, no host sync
        if (!ws->h_stage) {
            FPX_HIP(hipHostMalloc(reinterpret_cast<void**>(&ws->h_stage), STAGE_BYTES, hipHostMallocMapped));
            FPX_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&ws->d_stage), ws->h_stage, 0));
        }
        std::vector<uint32_t> h_opts;
        fill_opts(h_opts, b.opts, b.offsets, 1);
        uint64_t* so = reinterpret_cast<uint64_t*>(ws->h_stage);
        so[0] = 0; so[1] = P;
        std::memcpy(ws->h_stage + 16, h_opts.data(), 16);
        if (P) std::memcpy(ws->h_stage + 32, b.hashes + base, P * sizeof(uint32_t));
        // the kernels read the query straight from pinned host memory (4 KB over PCIe): no copy call
        b.d_hashes_base = reinterpret_cast<const uint32_t*>(ws->d_stage + 32);
        b.d_offsets = reinterpret_cast<const uint64_t*>(ws->d_stage);
        b.d_opts = reinterpret_cast<const uint32_t*>(ws->d_stage + 16);
        b.staged_single = true;
        return FPX_OK;
    }
    if ((rc = grow(&ws->d_hashes, &ws->cap_hashes, (size_t)P + 1))) return rc;
    std::vector<uint32_t>& h_opts = ws->h_opts;
    fill_opts(h_opts, b.opts, b.offsets, B);
    if (query_wg && B >= 1024u && P >= (1u << 20)) {
        // A large batch for k_search_query: every query is a workgroup's own business, so the batch is uploaded in pieces on a stream of
        // its own and the kernel over piece c waits for THAT piece only -- piece c + 1 crosses PCIe under it (33 MB per batch of
        // 8192 x 1000 hashes: 0.6 ms of link time next to 0.45 ms of kernel).  Nothing here waits: the options live in the workspace.
        if (!ws->copy_stream) {
            FPX_HIP(hipStreamCreateWithFlags(&ws->copy_stream, hipStreamNonBlocking));
            for (hipEvent_t& e : ws->ev_chunk) FPX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        hipStream_t cs = ws->copy_stream;
        FPX_HIP(hipMemcpyAsync(ws->d_offsets, b.offsets, ((size_t)B + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, cs));
        FPX_HIP(hipMemcpyAsync(ws->d_opts, h_opts.data(), h_opts.size() * sizeof(uint32_t), hipMemcpyHostToDevice, cs));
        b.up_chunks = Workspace::UP_CHUNKS;
        for (uint32_t c = 0; c <= b.up_chunks; ++c) b.up_q[c] = (uint32_t)((uint64_t)B * c / b.up_chunks);
        // (the first piece now, piece c + 1 right after the kernel over piece c has been launched: a copy out of PAGEABLE memory keeps the
        // calling thread until the runtime has staged it -- with all four enqueued here the first kernel started when the last piece had
        // been staged, 6.1 M queries/s with one caller; page-locked sources do not care)
        if ((rc = upload_piece(b, 0u))) return rc;
    } else {
        // (pageable sources go through the runtime's own staging.  A private page-locked ring per workspace was tried in round 3:
        // 3.8 / 5.2 M queries/s with one / two callers against 4.6 / 6.5 M this way -- the host's extra copy costs more than the
        // runtime's lock; what round 2 measured as "two pageable callers serialise" was the second caller's workspace being
        // allocated inside the timed loop)
        if (P) FPX_HIP(hipMemcpyAsync(ws->d_hashes, b.hashes + base, P * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        FPX_HIP(hipMemcpyAsync(ws->d_offsets, b.offsets, ((size_t)B + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        FPX_HIP(hipMemcpyAsync(ws->d_opts, h_opts.data(), h_opts.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        FPX_HIP(hipStreamSynchronize(st));             // (the caller's arrays may go once the call returns an error further down)
    }
    b.d_hashes_base = ws->d_hashes - base;
    b.d_offsets = ws->d_offsets;
    b.d_opts = ws->d_opts;
    return FPX_OK;
}
// deferred-probe lists of the lean kernel: room for 1/8 of the pairs per segment (typically < 2 % are deferred)
static int ensure_def_lists(Batch& b, bool side_wg)
{
    Snapshot* snap = b.snap; Workspace* ws = b.ws; int rc;
    b.def_cap = std::max<size_t>(4096, (size_t)(b.P / 8));
    if (snap->n_lean || snap->n_direct || side_wg) {            // (k_search_side: the statistics sets behind the counts)
        const size_t need = b.def_cap * std::max(1u, snap->n_lean);
        if ((rc = grow(&ws->d_def_list, &ws->cap_def, need))) return rc;
        if (snap->n_lean > ws->cap_def_segs || !ws->d_def_count) {
            if (ws->d_def_count) (void)hipFree(ws->d_def_count);
            if (ws->h_def_count) (void)hipHostFree(ws->h_def_count);
            ws->d_def_count = nullptr; ws->h_def_count = nullptr; ws->cap_def_segs = 0;
            // [n_lean deferred-list counts, one per 128-B line | LEAN_STAT_SETS x 8 u64 statistics slots of the lean kernel]
            const size_t nseg = std::max(1u, snap->n_lean);
            const size_t words = nseg * DEF_COUNT_STRIDE + LEAN_STAT_WORDS;
            FPX_HIP(dmalloc(&ws->d_def_count, words * sizeof(unsigned int)));
            FPX_HIP(hipHostMalloc(reinterpret_cast<void**>(&ws->h_def_count), words * sizeof(unsigned int), hipHostMallocMapped));
            ws->cap_def_segs = nseg;
        }
    }
    // (for the workspace's capacity, not this snapshot's n_lean: the layout must not move between batches)
    b.def_stat_off = (size_t)ws->cap_def_segs * DEF_COUNT_STRIDE;
    b.def_words = b.def_stat_off + LEAN_STAT_WORDS;
    return FPX_OK;
}

// ---- the query-per-workgroup paths: who takes them --------------------------------------------------------------------------------
// the queries' rule: short enough for the kernels' hash set, and a floor above the legacy protocol's
// (low_ok: floors of 1 and 2 are allowed -- option low_wg, k_search_low's sorted tail --; *has_low: the batch has such a query)
static bool queries_fit_wg(const uint64_t* offsets, const fpx_opts* opts, uint32_t B, bool low_ok = false, bool* has_low = nullptr)
{
    bool low = false;
    for (uint32_t q = 0; q < B; ++q) {
        const uint64_t raw_len = offsets[q + 1] - offsets[q];
        if (raw_len > QS_MAX_HASHES) return false;
        if (query_floor(opts[q], raw_len) <= 2u) {
            if (!low_ok) return false;
            low = true;
        }
    }
    if (has_low) *has_low = low;
    return true;
}
// a group for k_search_query's filtered instantiation: superseded docs, or columns outside the snapshot
static bool group_filtered(const GroupDesc& gd) { return gd.any_dead != 0u || gd.active != (gd.nseg >= 32u ? 0xFFFFFFFFu : ((1u << gd.nseg) - 1u)); }

// ONE WORKGROUP PER QUERY (fpx_qsearch.hpp): the snapshot is one packed group and nothing else, every column of it searched, no superseded
// docs -- the resident index between merges --, the queries short enough for their hash set and their floor above the legacy protocol's.
// Option query_wg 2: a group with superseded docs or columns outside the snapshot too, by the kernel's filtered instantiation (*filt).
// Option low_wg 1: queries with a floor of 1 or 2 too, where the group is NOT filtered (*low: the batch has such a query -- k_search_low);
// 2: where it is filtered too (k_search_low_filt; a filtered group is only ever here under query_wg 2); 3: as 2 -- which kernel a filtered
// group's batch then gets is run_query_wg's business (k_search_low_coop where k_search_filt would be taken, else k_search_low_filt).
static bool low_floors_ok(const Ctx* ctx, bool filtered)
{
    const int64_t low_wg = ctx_opt(ctx, OPT_LOW_WG);
    return low_wg == 2 || low_wg == 3 || (low_wg == 1 && !filtered);
}
// Option groups_wg 1: a snapshot of 2 .. QS_MAX_GROUPS packed groups too -- every one whole-hash-space, nothing else next to them --, walked
// one after the other (run_query_wg: k_search_next).  *filt: ANY of them is filtered (under query_wg 2 only, as for one); no query with a
// floor of 1 or 2, whatever low_wg says.  One group: exactly as before.
// Option groups_wg 2: as 1, and a batch with floors of 1 or 2 too where low_wg allows it (several_groups_low_ok: low_wg 1 when no group
// is filtered, 2 also when any is) -- k_search_low / k_search_low_filt over the first group, k_search_low_next over the others.
static bool several_groups_ok(const Snapshot* snap)
{
    const int64_t groups_wg = ctx_opt(snap->ctx, OPT_GROUPS_WG);
    if (snap->n_group < 2u || snap->n_group > QS_MAX_GROUPS || (groups_wg != 1 && groups_wg != 2)) return false;
    for (uint32_t i = 0; i < snap->n_group; ++i)
        if (!snap->groups[i]->packed || snap->h_group[i].win_lo != 0u || snap->h_group[i].win_hi != 0xFFFFFFFFu) return false;
    return true;
}
static bool several_groups_low_ok(const Ctx* ctx, bool any_filtered)
{
    return ctx_opt(ctx, OPT_GROUPS_WG) == 2 && low_floors_ok(ctx, any_filtered);
}
static bool takes_query_wg(const Snapshot* snap, const uint64_t* offsets, const fpx_opts* opts, uint32_t B, bool* filt, bool* low)
{
    const int64_t query_wg = ctx_opt(snap->ctx, OPT_QUERY_WG);
    if (!(snap->n_file == 0 && snap->n_solo == 0 && snap->n_group >= 1 && snap->n_direct != 0 &&
          (snap->n_mem == 0 || snap->mem_items == 0 || snap->d_memtab != nullptr) && query_wg != 0)) return false;
    if (snap->n_group != 1) {
        if (!several_groups_ok(snap)) return false;
        *filt = false;
        for (uint32_t i = 0; i < snap->n_group; ++i) *filt = *filt || group_filtered(snap->h_group[i]);
        *low = false;
        return (!*filt || query_wg == 2) && queries_fit_wg(offsets, opts, B, several_groups_low_ok(snap->ctx, *filt), low);
    }
    if (!snap->groups[0]->packed) return false;
    *filt = group_filtered(snap->h_group[0]);
    return (!*filt || query_wg == 2) && queries_fit_wg(offsets, opts, B, low_floors_ok(snap->ctx, *filt), low);
}
// ... and the same for the file segments NEXT TO the group (fpx_qside.hpp; option side_wg = 1): a snapshot -- part 1 of a live one, or a
// whole young index -- of small decoded and direct-addressed-alone segments only, none of them a hash-window slice, no group, no
// memory-segment postings.  The queries' rule is parts_take's, so a batch in two parts never splits between paths by query.
static bool takes_side_wg(const Snapshot* snap, const uint64_t* offsets, const fpx_opts* opts, uint32_t B)
{
    if (!(ctx_opt(snap->ctx, OPT_SIDE_WG) == 1 &&
          snap->n_group == 0 && snap->n_lean == 0 && snap->n_gen == 0 && snap->n_file == snap->n_small && snap->n_direct == snap->n_solo &&
          snap->n_small + snap->n_solo != 0 && (snap->n_mem == 0 || snap->mem_items == 0))) return false;
    for (const SegDesc& d : snap->h_file) if (!(d.own_flags == 0u && d.items && d.sbucket && d.sfirst && d.scode)) return false;
    for (const SegDesc& d : snap->h_direct) if (!(d.own_flags == 0u && d.drec && d.primary)) return false;
    return queries_fit_wg(offsets, opts, B);
}
// ... and for a snapshot that is ONE group in DIRECTORY + WORDS form (fpx_qwords.hpp; option words_wg = 1, 2 for a group with superseded
// docs or columns outside the snapshot too: *filt).  A window-sliced group may be taken: the kernel honours win_lo / win_hi.
static bool takes_words_wg(const Snapshot* snap, const uint64_t* offsets, const fpx_opts* opts, uint32_t B, bool* filt)
{
    const int64_t words_wg = ctx_opt(snap->ctx, OPT_WORDS_WG);
    if (!(words_wg != 0 && snap->n_group == 1 && !snap->groups[0]->packed && snap->n_file == 0 && snap->n_solo == 0 && snap->n_direct != 0 &&
          (snap->n_mem == 0 || snap->mem_items == 0 || snap->d_memtab != nullptr))) return false;
    *filt = group_filtered(snap->h_group[0]);
    return (!*filt || words_wg == 2) && queries_fit_wg(offsets, opts, B);
}

// ---- A. a query per workgroup --------------------------------------------------------------------------------------------------------
// a query-per-workgroup path opens: the queries' candidate slots (`extra_words` of the caller's behind them), the counters and statistics
// sets zeroed, the probe's first event -- and the arguments every such kernel takes, from the batch (Args: QFrameArgs | QSearchArgs,
// by their same-named members; which queries a launch takes is the caller's to say)
template <class Args>
static int open_wg_path(Batch& b, size_t extra_words, CandSlots* cs, Args* a)
{
    Workspace* ws = b.ws; int rc;
    if ((rc = ensure_cand_slots(ws, b.B, extra_words, cs))) return rc;
    hipLaunchKernelGGL(k_qs_zero, dim3(8), dim3(256), 0, b.st, ws->d_counters, ws->d_def_count, (uint32_t)b.def_words);
    FPX_HIP(hipEventRecord(ws->ev_probe0, b.st));
    a->hashes_base = b.d_hashes_base; a->offsets = b.d_offsets; a->opts = b.d_opts; a->sb = 32u - b.qb;
    a->cands = ws->d_cands[0]; a->cand_cap = ws->cap_cands; a->qcand = cs->qcand; a->qcand_n = cs->qcand_n;
    a->counters = ws->d_counters; a->stat_sets = device_stat_sets(b);
    a->qstats = b.want_q ? ws->d_qstats : nullptr; a->cancel = b.cancel;
    return FPX_OK;
}
// ... and its first pass closes behind the kernel's launches: k_finish over the queries' own slots, the batch's counters and statistics sets
// into the host's mapped copies, the wait.  FPX_REDO_QS: the kernel handed the batch back (run_with_redos: the pipeline)
static int close_wg_pass(Batch& b, uint32_t sb, const CandSlots& cs, ResultsTo* to)
{
    Workspace* ws = b.ws; int rc;
    FPX_HIP(hipGetLastError());
    FPX_HIP(hipEventRecord(ws->ev_probe1, b.st));
    if ((rc = results_target(b, to))) return rc;
    launch_finish(b, ws->d_cands[0], 0, sb, cs, to->res, to->n, b.stats != nullptr);
    if ((rc = publish(b, true))) return rc;
    FPX_HIP(hipEventRecord(ws->ev_end, b.st));
    FPX_SYNC_BATCH(b);
    return handed_back(ws, b.snap) ? FPX_REDO_QS : FPX_OK;
}
// the end of a query-per-workgroup path: results, the kernel's statistics sets, per-query statistics, the next batch's hints
static int finish_wg_path(Batch& b, const ResultsTo& to, uint64_t Cf, uint32_t path_bits)
{
    Workspace* ws = b.ws; int rc;
    if (!b.partial && (rc = deliver_results(ws, b.B, b.out_cap, to.staged, b.out, b.out_n, b.st))) return rc;
    const unsigned long long* ls = host_stat_sets(b);
    const StatSums s = sum_stat_sets(ls);
    gather_hist(ws->batch_hist, ws->h_counters, ls, s.probes);
    if (fpx_stats* stats = b.stats) {
        float ms = 0.f, total_ms = 0.f;
        (void)hipEventElapsedTime(&ms, ws->ev_probe0, ws->ev_probe1);
        (void)hipEventElapsedTime(&total_ms, ws->ev_begin, ws->ev_end);
        stats->probes += s.probes; stats->scanned_blocks += s.blocks; stats->scanned_docs += s.docs; stats->hits += s.records;
        stats->algorithmic_bytes += s.blocks * 512ull + s.bytes_off;
        stats->candidates += Cf + ws->h_counters[CTR_SLOTCANDS];
        stats->probe_kernel_ms += ms; stats->total_gpu_ms += total_ms; stats->probe_launches += 1;
        stats->probe_kernel_bytes += s.blocks * 512ull + s.bytes_off;
        stats->probe_kernel_fetched_bytes += (s.dreads + 1) / 2 * 128ull;
        stats->path_flags |= 1u | (Cf ? 2u : 0u) | path_bits;
    }
    if ((rc = deliver_qstats(b))) return rc;
    ws->hint_P = b.P; ws->hint_H = std::max<uint64_t>(s.records, 1);          // (sizes the pipeline's bins should a later batch take it)
    ws->hint_misc = 0; ws->hint_def = 0;
    return FPX_OK;
}
// Option hot_wg: the R queries whose records outgrew the LDS array were named in the redo list, with nothing counted and no candidate;
// k_search_classes searches each of them once per doc class (fpx_qsearch.hpp), into the same slots and shared list.  A few of them: the
// batch stays here and nothing backs off.  More than qs_redo_limit(B): the pipeline and the back-off, as before -- a walk per class
// costs more than the pipeline's one once much of a batch is hot, and hot traffic comes in runs.
static int redo_hot_queries(Batch& b, QSearchArgs qa, const GroupArgs& gargs, bool ns8, int cus, uint64_t R)
{
    if (R > qs_redo_limit(b.B) || R > qa.redo_cap) {
        __atomic_store_n(&b.snap->qs_skip, 32u, __ATOMIC_RELAXED);
        return FPX_REDO_QS;
    }
    int rc;
    qa.q_begin = 0u; qa.q_end = (uint32_t)R; qa.next_q = nullptr; qa.stagger = 0u;      // (entries of the list; all pieces of a chunked upload have arrived)
    FPX_LAUNCH_QS(k_search_classes, dim3(std::min<uint32_t>((uint32_t)R, (uint32_t)cus * QS_WGS_PER_CU)), b.st, qa, gargs, ns8, qa.mem_tab != nullptr);
    if ((rc = publish(b, true))) return rc;
    FPX_HIP(hipEventRecord(b.ws->ev_end, b.st));
    FPX_SYNC_BATCH(b);
    return handed_back(b.ws, b.snap) ? FPX_REDO_QS : FPX_OK;
}

// Dedup, probe, count and floor happen in ONE kernel, no keys are made or ordered, no record reaches HBM.  A batch that kernel hands back
// (hot hashes: a query's records outgrow its LDS array) returns FPX_REDO_QS: run_with_redos gives it to the pipeline.
// low: the batch has queries with a floor of 1 or 2 (option low_wg let it in; with filt under low_wg 2 or 3 only) -- k_search_low, or
// k_search_low_filt on a filtered group (low_wg 3: k_search_low_coop where `coop` holds); none of them has a redo list.
// Every other batch is k_search_query's exactly as before, whatever that option says.
// SEVERAL GROUPS (option groups_wg = 1; takes_query_wg): per upload piece the groups are walked one after the other on the batch's stream --
// k_search_query over group 0 (with the memory segments' table), k_search_next over groups 1.., which chain their candidates behind the
// launch before (fpx_qsearch.hpp).  The batch is opened once and closed once, one k_finish; a hand-back from any launch is the batch's.
// No redo list there; filt: ANY group is filtered -- which instantiation a launch is is its own group's business.  Low floors under
// groups_wg = 2 only (with low_wg): k_search_low or k_search_low_filt over group 0, k_search_low_next over the others, path bits 13 and 12.
static_assert(QS_MAX_GROUPS * Workspace::UP_CHUNKS <= DEF_COUNT_STRIDE, "the launches' next_q words -- one per (upload piece, group) -- are the first deferred-list count's line, which k_qs_zero clears");
static int run_query_wg(Batch& b, bool filt, bool low)
{
    Snapshot* snap = b.snap; Workspace* ws = b.ws; hipStream_t st = b.st; const uint32_t B = b.B; int rc;
    const uint32_t ngroups = snap->n_group;
    const bool ns8 = snap->groups[0]->ns == 8u;
    // (option hot_wg = 1, unfiltered: the batch's redo list -- B entries, behind the slots and their counts)
    const bool hot_wg = !filt && !low && ngroups == 1u && ctx_opt(snap->ctx, OPT_HOT_WG) == 1;
    if (low) {
        // (a query with a low floor hands over up to max_results candidates -- the legacy protocol's 500 --, all of them through the shared
        // list once they are more than its slots: the list is sized for that, not for the first guess of 64 per query)
        // (several groups: every launch hands over its own group's top max_results -- up to that many again per group; the slots a
        // launch carries over into the list were counted with the group that filled them)
        size_t want = 0;
        for (uint32_t q = 0; q < B; ++q) {
            const bool low_q = query_floor(b.opts[q], b.offsets[q + 1] - b.offsets[q]) <= 2u;
            want += low_q ? (size_t)ngroups * (std::min<size_t>(b.opts[q].max_results, QS_REC_CAP) + 32u) : 64u;
        }
        if (ws->cap_cands < want && (rc = grow_pair(ws->d_cands, &ws->cap_cands, want))) return rc;
    }
    CandSlots cs;
    QSearchArgs qa{};
    if ((rc = open_wg_path(b, hot_wg ? (size_t)B : 0, &cs, &qa))) return rc;
    struct Running {                                 // batches of this context inside their k_search_query launches, this one included
        std::atomic<int>* c; int before;
        explicit Running(std::atomic<int>* c_) : c(c_), before(c_->fetch_add(1)) {}
        ~Running() { c->fetch_sub(1); }
    } running(&snap->ctx->qs_running);
    const bool alone = running.before == 0;
    qa.q_begin = 0u; qa.q_end = B;
    if (snap->n_mem != 0 && snap->mem_items != 0) { qa.mem_tab = snap->d_memtab; qa.mem_bucket = snap->d_membucket; qa.mem_bits = snap->d_membits; }
    if (hot_wg) { qa.redo = reinterpret_cast<unsigned long long*>(cs.extra); qa.redo_cap = B; }
    // (option filt_coop = 1: ONE filtered packed group, no low floor in the batch, by k_search_filt -- where the snapshot holds the group's
    // union dead-set bitmap (made under filt_coop = 1, the id range narrow enough) or no column has a dead set.  The bitmap shares the
    // redo list's storage, which the filtered form never reads: fpx_qsearch.hpp, QSearchArgs)
    // (option low_wg = 3: a batch WITH a low floor too, by k_search_low_coop -- the same rounds and tasks with k_search_low's sorted tail;
    // under low_wg = 2 such a batch stays k_search_low_filt's, whatever filt_coop says)
    const bool coop = filt && (!low || ctx_opt(snap->ctx, OPT_LOW_WG) == 3) && ngroups == 1u && ctx_opt(snap->ctx, OPT_FILT_COOP) == 1 &&
                      (snap->h_group[0].any_dead == 0u || (snap->dead_union && snap->dead_union->d_bits != nullptr));
    if (coop && snap->h_group[0].any_dead != 0u) {
        qa.dead_union = snap->dead_union->d_bits; qa.dead_union_last = (uint32_t)(snap->dead_union->words - 1u);
    }
    const GroupArgs gargs{snap->h_group[0], snap->d_direct};
    const bool filt0 = group_filtered(snap->h_group[0]), mem = qa.mem_tab != nullptr;
    // as many workgroups as the chip holds at once (LDS: QS_WGS_PER_CU per CU); each takes every gridDim.x-th query
    const int cus = device_cus(snap->ctx);
    const uint32_t up_chunks = b.up_chunks;
    uint32_t next_launches = 0;
    for (uint32_t c = 0; c < std::max(1u, up_chunks); ++c) {
        qa.q_begin = up_chunks ? b.up_q[c] : 0u; qa.q_end = up_chunks ? b.up_q[c + 1] : B;
        if (qa.q_end == qa.q_begin) { if (up_chunks && c + 1u < up_chunks && (rc = upload_piece(b, c + 1u))) return rc; continue; }
        // (alone on the device: the launch's queue of queries -- a word of the deferred lists' counts, zeroed by k_qs_zero, unused on this
        // path -- and a staggered start; next to other batches' kernels neither: fpx_qsearch.hpp says why)
        qa.next_q = (FPX_QS_DYN && alone) ? ws->d_def_count + c : nullptr;
        qa.stagger = alone ? QS_STAGGER : 0u;
        if (up_chunks) FPX_HIP(hipStreamWaitEvent(st, ws->ev_chunk[c], 0));           // (the piece's hashes have arrived; the next piece is on its way)
        const dim3 grid(std::min<uint32_t>(qa.q_end - qa.q_begin, (uint32_t)cus * QS_WGS_PER_CU));
        // (the piece's queries over group 0 -- filtered or not as that group is: with one group, takes_query_wg's `filt` --, with the memory table)
        if (low && coop) FPX_LAUNCH_QS(k_search_low_coop, grid, st, qa, gargs, ns8, b.want_q, mem);
        else if (low && filt0) FPX_LAUNCH_QS(k_search_low_filt, grid, st, qa, gargs, ns8, b.want_q, mem);
        else if (low) FPX_LAUNCH_QS(k_search_low, grid, st, qa, gargs, ns8, b.want_q, mem);
        else if (coop) FPX_LAUNCH_QS(k_search_filt, grid, st, qa, gargs, ns8, b.want_q, mem);
        else FPX_LAUNCH_QS(k_search_query, grid, st, qa, gargs, ns8, b.want_q, mem, filt0);
        if (ngroups > 1u) {
            // (... then over every other group: a launch's queue of queries is a word of its own.
            // low -- option groups_wg = 2 --: the kernels with the sorted tail, each launch filtered or not as its own group is)
            QSearchArgs qn = qa;
            qn.mem_tab = nullptr; qn.mem_bucket = nullptr; qn.mem_bits = nullptr;
            for (uint32_t gi = 1; gi < ngroups; ++gi) {
                qn.next_q = qa.next_q ? ws->d_def_count + (size_t)gi * Workspace::UP_CHUNKS + c : nullptr;
                const bool ns8_g = snap->groups[gi]->ns == 8u, filt_g = group_filtered(snap->h_group[gi]);
                const GroupArgs gargs_g{snap->h_group[gi], snap->d_direct};
                if (low) FPX_LAUNCH_QS(k_search_low_next, grid, st, qn, gargs_g, ns8_g, b.want_q, filt_g);
                else FPX_LAUNCH_QS(k_search_next, grid, st, qn, gargs_g, ns8_g, b.want_q, filt_g);
                ++next_launches;
            }
        }
        if (up_chunks && c + 1u < up_chunks && (rc = upload_piece(b, c + 1u))) return rc;       // (the next piece crosses PCIe under this kernel)
    }
    // (the batch's counters and statistics sets go to the host's mapped copies here, after the first pass, and again after a redo)
    ResultsTo to;
    if ((rc = close_wg_pass(b, qa.sb, cs, &to)) != FPX_OK && rc != FPX_REDO_QS) return rc;
#ifdef FPX_QS_PROF
    fprintf(stderr, "qs_prof clocks/query: setup %.0f dedup %.0f rounds %.0f tasks %.0f count+exact %.0f handover %.0f", ws->h_counters[CTR_HIST] / (double)B, ws->h_counters[CTR_HIST + 1] / (double)B,
            ws->h_counters[CTR_HIST + 2] / (double)B, ws->h_counters[CTR_HIST + 3] / (double)B, ws->h_counters[CTR_HIST + 4] / (double)B, ws->h_counters[CTR_HIST + 5] / (double)B);
    // (the finer marks: waits inside dedup, the rounds and before the tasks)
    fprintf(stderr, " | dedup: hash wait %.0f | rounds: hash wait %.0f heads wait %.0f words wait %.0f probe %.0f | next offsets wait %.0f\n", ws->h_counters[CTR_HIST + 6] / (double)B,
            ws->h_counters[CTR_HIST + 7] / (double)B, ws->h_counters[CTR_HIST + 8] / (double)B, ws->h_counters[CTR_HIST + 9] / (double)B, ws->h_counters[CTR_HIST + 10] / (double)B,
            ws->h_counters[CTR_HIST + 11] / (double)B);
#endif
    if (rc) return rc;                                         // (handed back)
    // (the shared list's length is known to the host only behind a synchronisation of its own: the sort below needs it)
    const uint64_t R = hot_wg ? ws->h_counters[CTR_REDO] : 0;
    if (R != 0 && (rc = redo_hot_queries(b, qa, gargs, ns8, cus, R))) return rc;
    // some queries have more candidates than slots: the second k_finish, which also takes the redone queries' candidates from their slots
    uint64_t Cf = 0;
    if (ws->h_counters[CTR_CANDS] != 0 || R != 0) {
        Cf = ws->h_counters[CTR_CANDS];
        if ((rc = finish_crowded(b, qa.sb, cs, to, Cf))) return rc;
    }
    if ((rc = finish_wg_path(b, to, Cf, 4u | 64u | (filt ? 256u : 0u) | (R != 0 ? 1024u : 0u) | (low ? 4096u : 0u) | (ngroups > 1u ? 8192u : 0u) | (coop ? 65536u : 0u)))) return rc;
    if (b.stats) b.stats->probe_launches += next_launches;
    return FPX_OK;
}

// ... and the file segments next to the group, by k_search_side
static int run_side_wg(Batch& b)
{
    Snapshot* snap = b.snap; const uint32_t B = b.B; int rc;
    CandSlots cs;
    SideArgs sa{};
    if ((rc = open_wg_path(b, 0, &cs, &sa.f))) return rc;
    sa.f.B = B;
    sa.small = snap->d_small; sa.n_small = snap->n_small; sa.solo = snap->d_solo; sa.n_solo = snap->n_solo;
    // as many workgroups as the chip holds at once (LDS: QF_WGS_PER_CU per CU); each takes every gridDim.x-th query
    const int cus = device_cus(snap->ctx);
    hipLaunchKernelGGL(k_search_side, dim3(std::min<uint32_t>(B, (uint32_t)cus * QF_WGS_PER_CU)), dim3(QF_WG), QF_LDS_BYTES, b.st, sa);
    ResultsTo to;
    if ((rc = close_wg_pass(b, sa.f.sb, cs, &to))) return rc;           // (handed back: that snapshot or part alone goes to the pipeline)
    const uint64_t Cf = b.ws->h_counters[CTR_CANDS];
    if (Cf != 0 && (rc = finish_crowded(b, sa.f.sb, cs, to, Cf))) return rc;
    return finish_wg_path(b, to, Cf, 512u);
}

// ... and a group in directory + words form, by k_search_words (the memory segments behind their table with it)
static int run_words_wg(Batch& b, bool filt)
{
    Snapshot* snap = b.snap; const uint32_t B = b.B; int rc;
    CandSlots cs;
    WordsArgs wa{};
    if ((rc = open_wg_path(b, 0, &cs, &wa.f))) return rc;
    wa.f.B = B;
    if (snap->n_mem != 0 && snap->mem_items != 0) { wa.mem_tab = snap->d_memtab; wa.mem_bucket = snap->d_membucket; wa.mem_bits = snap->d_membits; }
    const GroupArgs gargs{snap->h_group[0], snap->d_direct};
    // as many workgroups as the chip holds at once (LDS: QF_WGS_PER_CU per CU); each takes every gridDim.x-th query
    const int cus = device_cus(snap->ctx);
    FPX_LAUNCH(k_search_words, dim3(std::min<uint32_t>(B, (uint32_t)cus * QF_WGS_PER_CU)), QF_WG, QF_LDS_BYTES, b.st, wa, gargs,
               snap->groups[0]->ns == 8u, wa.mem_tab != nullptr, filt);
    ResultsTo to;
    if ((rc = close_wg_pass(b, wa.f.sb, cs, &to))) return rc;           // (handed back: the pipeline)
    const uint64_t Cf = b.ws->h_counters[CTR_CANDS];
    if (Cf != 0 && (rc = finish_crowded(b, wa.f.sb, cs, to, Cf))) return rc;
    return finish_wg_path(b, to, Cf, 4u | 2048u | (filt ? 256u : 0u));
}

// ---- B. the pipeline: steps of its three drivers ----------------------------------------------------------------------------------------
// the batch's (hash, q) keys, ordered; flagged: duplicates were flagged where the keys were made; key_skip: low hash bits the order ignores
struct Keys { const uint64_t* d_pairs; bool flagged; uint32_t key_skip; };

// ---- 1+2: keys, sort by (hash, q)
static int make_keys(Batch& b, bool single_fast, bool score_only, Keys* keys)
{
    Snapshot* snap = b.snap; Workspace* ws = b.ws; hipStream_t st = b.st; const uint64_t* offsets = b.offsets;
    const uint32_t B = b.B; const uint64_t P = b.P, base = b.base; const unsigned qb = b.qb;
    int rc, kcur = 0;
    // (every kernel of the batch must look back over the same bucket width: the coarser order only where the direct-addressed
    // kernels, which take it as a parameter, are the only ones that read the pairs)
    // Snapshots of direct-addressed segments only (their kernels are the only readers of the pairs): duplicates are flagged
    // when the keys are made (k_make_keys_dedup, queries of up to DEDUP_MAX hashes) and the sort takes one pass
    // (memory segments do not stand in the way once the snapshot has their ONE table: k_probe_memtab reads keys in any order)
    bool flagged = snap->n_file == 0 && (snap->n_mem == 0 || snap->d_memtab != nullptr) && snap->n_direct != 0 && !score_only;
    for (uint32_t q = 0; q < B && flagged; ++q) flagged = offsets[q + 1] - offsets[q] <= DEDUP_MAX;
    // (flagged keys are ordered for locality alone: by how many of the top hash bits is the context's choice -- fewer bits, fewer
    // queries per round of a workgroup, larger reservations in their bins)
    const uint32_t key_skip = flagged ? KEY_SORT_SKIP_DIRECT : KEY_SORT_SKIP;      // (flagged keys: the top 8 hash bits -- 8 / 7 / 6 bits measured alike, 5 / 4 slower: round 5)
    // small batches sort their keys per query in ONE kernel (k_make_keys_sorted) instead of batch-wide in eleven launches
    const uint64_t local_sort_max = (uint64_t)std::max<int64_t>(0, ctx_opt(snap->ctx, OPT_LOCAL_SORT_MAX));
    bool local_sort = P && !score_only && !single_fast && !flagged && B >= 2u && P <= local_sort_max && snap->n_small == 0;
    if (local_sort)
        for (uint32_t q = 0; q < B && local_sort; ++q) local_sort = offsets[q + 1] - offsets[q] <= QSORT_MAX;
    if (local_sort) {
        hipLaunchKernelGGL(k_make_keys_sorted, dim3(B), dim3(256), 0, st, b.d_hashes_base, b.d_offsets, B, qb, base, ws->d_keys[0],
                           (snap->n_lean || snap->n_direct) ? ws->d_def_count : nullptr, (uint32_t)b.def_words);
        FPX_HIP(hipGetLastError());
    } else if (P && !score_only) {
        // flagged keys are brought into (hash bucket, query) order by our own counting sort, whose counts k_make_keys_dedup takes
        // on its way (fpx_keyorder.hpp); tiny batches stay in query order (the three launches cost what the order buys)
        const uint64_t order_min = (uint64_t)std::max<int64_t>(0, ctx_opt(snap->ctx, OPT_ORDER_MIN_PAIRS));
        KeyOrder ko{};
        // ... and large ones keep the library's pass: there our three launches cost 0.03 ms more than its five, and two batches in
        // flight no longer fill each other's gaps (8192 queries: 1.16 against 0.97 ms per batch)
        const uint64_t order_max = 1ull << 20;
        const bool own_order = flagged && !single_fast && P >= order_min && P <= order_max;
        if (own_order && (rc = key_order_setup(ws, B, 0u, 32u - key_skip, &ko, nullptr, st, B >= KO_ROWS_MIN_B))) return rc;
        const uint64_t key_base = b.staged_single ? 0ull : base;
        if (flagged)
            hipLaunchKernelGGL(k_make_keys_dedup, dim3(B), dim3(256), 0, st, b.d_hashes_base, b.d_offsets, B, qb, key_base, ws->d_keys[0],
                               single_fast ? ws->d_counters : nullptr, ws->d_def_count, (uint32_t)b.def_words, ko);
        else
            hipLaunchKernelGGL(k_make_keys, dim3(B), dim3(256), 0, st, b.d_hashes_base, b.d_offsets, B, qb, key_base, ws->d_keys[0],
                               single_fast ? ws->d_counters : nullptr, (snap->n_lean || snap->n_direct) ? ws->d_def_count : nullptr, (uint32_t)b.def_words);
        // k_make_keys writes the pairs in (q, position) order and the LSD radix sort is stable, so sorting on the 32 hash
        // bits alone leaves the pairs ordered by (hash, q): equal pairs end up adjacent without sorting the q bits.
        // ... and only the top 32 - KEY_SORT_SKIP of them: block-level locality is all the probes need from the order
        // (a 256-value hash bucket is narrower than a block's hash span), see is_duplicate_pair for the dedup.
        // (flagged keys of a small batch are not sorted at all: the order only serves locality, which batches of up to 2^20
        // pairs -- every probe on lines of its own -- do not have; nor those of a snapshot whose direct-addressed segments are
        // one fused pair -- a rank's share of an index sharded over 8 GPUs: the pass costs 0.1 ms and buys k_probe_fused<2> 0.06;
        // k_probe_direct, whose neighbouring probes share record lines, keeps the order)
        if (own_order) {
            if (ko.qrows) hipLaunchKernelGGL(k_group_hist, dim3((B + KO_GROUP - 1u) / KO_GROUP), dim3(256), 0, st, ko, B);
            hipLaunchKernelGGL(k_bucket_scan, dim3(ko.nb), dim3(256), 0, st, ko, (B + KO_GROUP - 1u) / KO_GROUP);
            hipLaunchKernelGGL(k_scatter_keys, dim3((B + KO_GROUP - 1u) / KO_GROUP), dim3(256), 0, st, ko, (const uint64_t*)ws->d_keys[0], b.d_offsets, key_base, 0u, B, qb,
                               ws->d_keys[1], (unsigned long long*)nullptr);
            FPX_HIP(hipGetLastError());
            kcur = 1;
        } else if (!(flagged && P <= local_sort_max)) {
            if ((rc = sort_keys(ws, ws->d_keys, P, qb + key_skip, 32 + qb, st, &kcur))) return rc;
        }
    }
    keys->d_pairs = ws->d_keys[kcur];
    keys->flagged = flagged;
    keys->key_skip = key_skip;
    return FPX_OK;
}

// the hit records' bins of the device-sized path (fpx_partition.hpp), as its probe kernels need them
struct Bins {
    BinArgs h{};
    bool binned = false; uint32_t sbins = 0;      // k_probe_group bins the records itself, k_score_bin scores a bin per workgroup: that many
    uint32_t ref_cap = 0;                         // references to hot lists a bin takes; 0: hot lists are copied into the bins
    uint32_t* d_bin_count = nullptr; uint32_t* d_qcount = nullptr;
    uint64_t est_H = 0;                           // the batch's records, as the workspace's last batch lets expect
};
// one round of probe launches: what the driver tells it, and what it reports
struct Probes {
    bool single_fast = false; int attempt = 0; bool force_generic = false;
    const Bins* bins = nullptr;           // the device-sized path: the records go to d_hits[1] and the bins, nothing is copied to the host
    bool used_lean = false, spread = false, used_fused = false; uint32_t launches = 0;
};

// ---- 3+4: probes, by the segments' storage forms
static int launch_probes(Batch& b, const Keys& keys, Probes& pr)
{
    Snapshot* snap = b.snap; Workspace* ws = b.ws; hipStream_t st = b.st; const uint64_t P = b.P; const unsigned qb = b.qb;
    const bool single_fast = pr.single_fast, fast = pr.bins != nullptr, binned = fast && pr.bins->binned;
    uint64_t* const d_hits = ws->d_hits[fast ? 1 : 0];                            // (fast: binned into d_hits[0] afterwards)
    const uint32_t key_skip = keys.flagged ? KEY_SKIP_FLAGGED : keys.key_skip;
    pr.used_lean = false; pr.spread = false;
    if (!single_fast) FPX_HIP(hipMemsetAsync(ws->d_counters, 0, CTR_COUNT * sizeof(unsigned long long), st));   // (k_make_keys did it)
    if (b.want_q) FPX_HIP(hipMemsetAsync(ws->d_qstats, 0, (size_t)b.B * sizeof(unsigned long long), st));
    if (P && (snap->n_file || snap->n_direct)) {
        ProbeArgs a;
        a.pairs = keys.d_pairs; a.P = P; a.qb = qb;
        // enough workgroups to fill 256 CUs; long per-wave runs amortise the index walk for big batches
        const uint64_t total = P * snap->n_file;
        // (16 pairs per wave also for tiny batches: a single query is bound by per-workgroup set-up, not by parallelism)
        a.ppw = total >= (1ull << 22) ? 64u : 16u;
        a.rounds = total >= (1ull << 25) ? 2u : 1u;
        a.bsp = ((snap->max_block_size + 15u) & ~15u) + 32u;
        a.hits = d_hits; a.hit_cap = ws->cap_hits; a.counters = ws->d_counters;
        a.def_list = ws->d_def_list; a.def_count = ws->d_def_count; a.def_cap = (uint32_t)b.def_cap; a.ctr_off = 0; a.lean_stats = nullptr; a.cancel = b.cancel;
        a.key_skip = key_skip;
        a.qstats = b.want_q ? ws->d_qstats : nullptr;
        const uint64_t per_wg = (uint64_t)PWAVES * a.ppw * a.rounds;
        const uint32_t gx = (uint32_t)((P + per_wg - 1) / per_wg);
        const size_t lds = STAGE_CAP * sizeof(uint64_t) + sizeof(DecodeLut) + (size_t)PWAVES * 4 * a.bsp;
        // big batches: every kind of file segment has its own kernel
        const bool lean = (snap->n_lean != 0 || snap->n_small != 0) && !pr.force_generic && P < 0x80000000ull && qb <= 24u &&   // pair indices + a tag bit in the deferred lists; 8 spare bits in q
                          total >= lean_min_probes(snap->ctx);
        if (!single_fast) FPX_HIP(hipEventRecord(ws->ev_probe0, st));
        if (pr.attempt > 0 && (snap->n_lean || snap->n_direct))
            FPX_HIP(hipMemsetAsync(ws->d_def_count, 0, b.def_words * sizeof(unsigned int), st));   // (first attempt: k_make_keys)
        if (snap->n_direct) {
            // direct-addressed segments: their kernels serve every batch size -- the grouped ones through their group's
            // directory (fpx_group.hpp: one thread per hash), the others one thread per hash and segment (fpx_direct.hpp)
            const uint32_t n_solo = snap->n_solo;
            const SegDesc* d_solo = snap->d_solo;
            const uint64_t wgs_solo = (P + DK_WG * DK_KPL - 1) / (DK_WG * DK_KPL) * n_solo;
            const uint64_t wgs_group = (P + FK_WG - 1) / FK_WG * snap->n_group;
            // statistics: spread over 64 lines when thousands of workgroups end with them (see LEAN_STAT_SETS)
            pr.spread = !single_fast && wgs_solo + wgs_group >= 1024;
            unsigned long long* stat_sets = pr.spread ? device_stat_sets(b) : nullptr;
            if (snap->n_group) {
                ProbeArgs gk = a;
                gk.segs = snap->d_direct; gk.lean_stats = stat_sets;
                if (binned) { const BinArgs& h = pr.bins->h; gk.bins = h.bins; gk.bin_cap = h.bin_cap; gk.bin_count = h.bin_count; gk.bin_shift = h.shift; gk.rec32 = h.rec32; }
                if (binned) { gk.refs = pr.bins->ref_cap ? ws->d_refs : nullptr; gk.ref_cap = pr.bins->ref_cap; }
                gk.rounds = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(6, wgs_group / 6000));   // (8192 x 1000: 0.626 / 0.580 / 0.566 / 0.564 ms at 2 / 3 / 4 / 6)
                // (hot-hash data -- the previous batch brought 16+ records per key: a workgroup's rounds wait for the waves that copy the
                // long lists; three rounds: 3.5 ms per batch of 8192 on distribution Z where five take 4.4)
                if (fast && pr.bins->est_H > 16ull * P) gk.rounds = std::min(gk.rounds, 3u);
                const uint64_t per_wg_gk = (uint64_t)FK_WG * gk.rounds;
                for (const GroupDesc& gd : snap->h_group) {              // one launch per group: its descriptor is a kernel argument
                    const GroupArgs gargs{gd, snap->d_direct};
                    const dim3 gridg((uint32_t)((P + per_wg_gk - 1) / per_wg_gk));
                    const Group* grp = snap->groups[&gd - snap->h_group.data()].get();
                    launch_probe_group(grp->packed, grp->ns == 8u, binned, gk.qstats != nullptr, gridg, st, gk, gargs);
                }
                pr.used_fused = true;
            }
            if (n_solo) {
                ProbeArgs dk = a;
                dk.segs = d_solo; dk.lean_stats = stat_sets;
                dk.rounds = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(4, wgs_solo / 8192));
                const uint64_t per_wg_dk = (uint64_t)DK_WG * DK_KPL * dk.rounds;
                hipLaunchKernelGGL(k_probe_direct, dim3((uint32_t)((P + per_wg_dk - 1) / per_wg_dk), n_solo), dim3(DK_WG), 0, st, dk);
            }
        }
        if (lean) {
            if (snap->n_lean) {
                // main kernel: k_probe_lean8 over the dense 512-B segments
                pr.spread = true;
                ProbeArgs l = a;
                // rounds of 1024 pairs per workgroup: more rounds amortise the workgroup's set-up (decode tables, barriers) --
                // measured at 8.2 M pairs x 16 segments: 5.48 ms with 1, 5.11 with 2, 5.01 with 6, 5.14 with 16 -- as long
                // as the grid still fills the chip several times over (>= 4096 workgroups)
                const uint64_t wgs_at_1 = (P + 1023) / 1024 * snap->n_lean;
                l.segs = snap->d_lean; l.ctr_off = 8u;
                l.rounds = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(6, wgs_at_1 / 4096));
                l.lean_stats = device_stat_sets(b);
                const size_t lds8 = STAGE_CAP * sizeof(uint64_t) + sizeof(LeanLut) + (size_t)L8_WAVES * 8 * L8_SLOT;
                const uint64_t per_wg_8 = (uint64_t)L8_WAVES * 64u * LEAN_KPL * l.rounds;
                const uint32_t gx8 = (uint32_t)((P + per_wg_8 - 1) / per_wg_8);
                // d_lean lists the segments whose blocks' head (header, hashes, docid control bytes) fits two lines first:
                // they take the partial-fetch instantiation, the rest the whole-block one
                if (snap->n_lean2)
                    hipLaunchKernelGGL(k_probe_lean8<2>, dim3(gx8, snap->n_lean2), dim3(L8_WG), lds8, st, l);
                if (snap->n_lean > snap->n_lean2) {
                    ProbeArgs l4 = l;
                    l4.segs = snap->d_lean + snap->n_lean2;
                    l4.def_list = l.def_list + (size_t)snap->n_lean2 * l.def_cap;
                    l4.def_count = l.def_count + (size_t)snap->n_lean2 * DEF_COUNT_STRIDE;
                    hipLaunchKernelGGL(k_probe_lean8<4>, dim3(gx8, snap->n_lean - snap->n_lean2), dim3(L8_WG), lds8, st, l4);
                }
            }
            FPX_HIP(hipEventRecord(ws->ev_probe1, st));
            // auxiliary passes: the rows the lean kernel deferred, and the segments it does not suit
            if (snap->n_lean) {
                ProbeArgs d = a;
                d.segs = snap->d_lean; d.ppw = 16u; d.rounds = 1u;
                const uint64_t per_wg_d = (uint64_t)PWAVES * d.ppw;
                // persistent workgroups striding over the device-side list: about 1024 of them over all segments
                // ... sized from the longest list of the workspace's previous batch (x4; any grid is correct, the list is
                // walked in strides): the usual lists hold a few dozen rows, and a grid of a thousand 512-thread
                // workgroups that find nothing to do still costs 35 us
                const uint64_t gxd_cap = std::max<uint64_t>(64, (1024 + snap->n_lean - 1) / snap->n_lean);
                const uint64_t want_d = ws->hint_P ? std::max<uint64_t>(1, (4ull * ws->hint_def + per_wg_d - 1) / per_wg_d) : gxd_cap;
                const uint32_t gxd = (uint32_t)std::min<uint64_t>(std::min<uint64_t>((b.def_cap + per_wg_d - 1) / per_wg_d, gxd_cap), want_d);
                hipLaunchKernelGGL((k_probe<true, true>), dim3(gxd, snap->n_lean), dim3(PWG), lds, st, d);
            }
            if (snap->n_small) {
                hipLaunchKernelGGL(k_probe_small, dim3((uint32_t)std::min<uint64_t>((P + (uint64_t)WG * SMALL_KPT - 1) / ((uint64_t)WG * SMALL_KPT), SMALL_GRID)), dim3(WG), 0, st,
                                   snap->d_small, snap->n_small, keys.d_pairs, P, qb, d_hits, (uint64_t)ws->cap_hits, ws->d_counters,
                                   b.want_q ? ws->d_qstats : (unsigned long long*)nullptr);
            }
            if (snap->n_gen) {
                ProbeArgs ge = a;
                ge.segs = snap->d_gen;
                if (snap->gen_all_512) hipLaunchKernelGGL((k_probe<true, false>), dim3(gx, snap->n_gen), dim3(PWG), lds, st, ge);
                else hipLaunchKernelGGL((k_probe<false, false>), dim3(gx, snap->n_gen), dim3(PWG), lds, st, ge);
            }
            FPX_HIP(hipEventRecord(ws->ev_probe2, st));
            pr.used_lean = true;
        } else {
            a.segs = snap->d_file;
            if (snap->n_file) {
                if (snap->all_512) hipLaunchKernelGGL((k_probe<true, false>), dim3(gx, snap->n_file), dim3(PWG), lds, st, a);
                else hipLaunchKernelGGL((k_probe<false, false>), dim3(gx, snap->n_file), dim3(PWG), lds, st, a);
            }
            if (!single_fast) FPX_HIP(hipEventRecord(ws->ev_probe1, st));
        }
        if (pr.spread && !fast)            // (the device-sized path publishes them at its end, with everything else)
            FPX_HIP(hipMemcpyAsync(ws->h_def_count, ws->d_def_count, b.def_words * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
        FPX_HIP(hipGetLastError());
        pr.launches += 1;
    }
    if (P && snap->n_mem && snap->d_memtab) {
        hipLaunchKernelGGL(k_probe_memtab, dim3(memtab_grid(P)), dim3(WG), 0, st, (const uint64_t*)snap->d_memtab, (const uint32_t*)snap->d_membucket,
                           keys.d_pairs, P, qb, key_skip, d_hits, (uint64_t)ws->cap_hits, ws->d_counters,
                           (const unsigned long long*)nullptr, 0ull, (const uint32_t*)snap->d_membits);
        FPX_HIP(hipGetLastError());
    }
    return FPX_OK;
}

// ---- the device-sized path (fpx_partition.hpp): the hit records are binned by query as they are produced, every size downstream is read
//      from device memory, and the batch needs ONE host round trip (two when queries overflow their candidate slots) instead of three.
//      It needs an estimate of the record count to size its bins: the first batch of a workspace takes the general path.  Anything it
//      cannot handle (a full bin, a full deferred list, scores too wide for the candidate key) is noticed after the synchronisation and
//      the batch is redone on the general path (FPX_REDO).
constexpr uint32_t HOT_REF_CAP = 4096;                                       // references to hot lists a bin takes (16 bytes each)
static uint32_t level1_bits(unsigned qb) { return qb > BIN_QUERIES_LOG2 ? qb - BIN_QUERIES_LOG2 : 0u; }

// the bins' form, sizes and buffers; their counts zeroed on the stream
static int size_bins(Batch& b, const Keys& keys, Bins* bins)
{
    Snapshot* snap = b.snap; Workspace* ws = b.ws; const uint32_t B = b.B; const uint64_t P = b.P; int rc;
    BinArgs& h_bin = bins->h;
    // ... and its short form when the records come from groups of direct-addressed segments alone: k_probe_group drops them
    // into bins of 2^BQ queries itself and k_score_bin scores a bin per workgroup (fpx_score_bin.hpp) -- no partition kernels
    // Queries per bin: eight, fewer for batches that would not give k_score_bin ~2048 workgroups otherwise (a workgroup's time is
    // a chain of tile-load latencies: 8192 queries in bins of 4: 170 -> 154 us, 1024 queries in bins of 2: 66 -> 29 us)
    uint32_t bin_q_log2 = 3u;
    while (bin_q_log2 > 1u && (B >> bin_q_log2) < 2048u) --bin_q_log2;
    uint32_t sbins = 0;
    // (segments direct-addressed on their own and memory segments append their records to the misc buffer, which k_bin bins: the
    // snapshot a live index has between merges keeps the one-launch scoring of its groups)
    if (ctx_opt(snap->ctx, OPT_BINNED) != 0 && keys.flagged && snap->n_group != 0 && bin_q_log2 >= 1u && bin_q_log2 <= 4u) {
        sbins = (B + (1u << bin_q_log2) - 1u) >> bin_q_log2;
        // (a floor of 1 or 2 -- the legacy protocol's -- makes every counted doc a candidate: k_score's count-only round, which
        // raises the floor to top * pct / 100 before anything is emitted, handles those)
        bins->binned = min_floor(b.offsets, b.opts, B) > 2u && sbins <= MAX_SBINS;
        if (!bins->binned) sbins = 0;            // (the two-level partition's layout below: its counts must sit where its memset zeroes them)
    }
    bins->sbins = sbins;
    const uint64_t est_H = bins->est_H = (uint64_t)((double)ws->hint_H * (double)P / (double)ws->hint_P) + 1024;
    const size_t want = (size_t)(2 * est_H + (1u << 16)) + (bins->binned ? (size_t)sbins * 8192u : 0u);      // bins get 2x their expected fill
    if (ws->cap_hits < want && (rc = grow_pair(ws->d_hits, &ws->cap_hits, want))) return rc;
    const size_t words = BINQ_HEAD + (size_t)std::max<uint32_t>(MAX_BINS, sbins) * BIN_STRIDE + (size_t)B + 64 + sbins;
    if (words > ws->cap_binq) {
        if (ws->d_binq) (void)hipFree(ws->d_binq);
        if (ws->d_qcursor) (void)hipFree(ws->d_qcursor);
        ws->d_binq = nullptr; ws->d_qcursor = nullptr; ws->cap_binq = 0;
        const size_t ncap = words * 5 / 4;
        FPX_HIP(dmalloc(&ws->d_binq, ncap * sizeof(uint32_t)));
        FPX_HIP(dmalloc(&ws->d_qcursor, ncap * sizeof(unsigned long long)));
        ws->cap_binq = ncap;
    }
    if (!ws->h_bins) FPX_HIP(hipHostMalloc(reinterpret_cast<void**>(&ws->h_bins), (BINQ_HEAD + (size_t)MAX_BINS * BIN_STRIDE + MAX_SBINS) * sizeof(uint32_t), hipHostMallocMapped));
    uint32_t* d_bin_count = bins->d_bin_count = ws->d_binq + BINQ_HEAD;
    bins->d_qcount = d_bin_count + (size_t)std::max<uint32_t>(MAX_BINS, sbins) * BIN_STRIDE;
    h_bin.bins = ws->d_hits[0];
    h_bin.bin_count = d_bin_count;
    if (bins->binned) {
        // 4-byte records where the doc ids leave room for the query's bits inside its bin (fpx_partition.hpp)
        const bool rec32_enabled = ctx_opt(snap->ctx, OPT_REC32) != 0;
        h_bin.rec32 = rec32_enabled && !__atomic_load_n(&snap->rec32_refused, __ATOMIC_RELAXED) &&
                      snap->max_doc_declared < (0xFFFFFFFFu >> bin_q_log2) ? 1u : 0u;
        h_bin.counters = ws->d_counters;
        h_bin.nbins = sbins; h_bin.shift = bin_q_log2;
        // twice the expected share + room for the spread of a small bin; a bin that overflows is seen after the batch's
        // synchronisation and the batch is redone on the general path
        h_bin.bin_cap = std::min<uint64_t>(ws->cap_hits / sbins, std::max<uint64_t>(2 * est_H / sbins + 8192, 16384)) & ~(uint64_t)31;      // (whole lines per bin: reservations padded to BIN_ALIGN records start on a sector)
        FPX_HIP(hipMemsetAsync(d_bin_count, 0, (size_t)sbins * BIN_STRIDE * sizeof(uint32_t), b.st));
        // Hot-hash data (the last batch brought 16+ records per key): the lists of a hot hash -- thousands of docs, the same for every
        // query that holds the hash -- reach the score kernel BY REFERENCE (ProbeArgs::refs): HOT_REF_CAP entries per bin, their
        // counts in the bins' counter lines (zeroed above); a bin with more lists has the rest copied as before
        const int64_t hot_refs = ctx_opt(snap->ctx, OPT_HOT_REFS);
        if (hot_refs > 0 || (hot_refs < 0 && est_H > 16ull * P)) {
            bins->ref_cap = HOT_REF_CAP;
            if ((size_t)sbins * HOT_REF_CAP > ws->cap_refs) {
                if (ws->d_refs) (void)hipFree(ws->d_refs);
                ws->d_refs = nullptr; ws->cap_refs = 0;
                if (dmalloc(&ws->d_refs, (size_t)sbins * HOT_REF_CAP * sizeof(uint4)) == hipSuccess) ws->cap_refs = (size_t)sbins * HOT_REF_CAP;
                else { (void)hipGetLastError(); bins->ref_cap = 0; }              // (no room: the lists are copied)
            }
        }
    } else {
        const uint32_t nb_bits = level1_bits(b.qb);
        h_bin.nbins = 1u << nb_bits; h_bin.shift = b.qb - nb_bits;
        // a bin holds at most 4x its expected share (never more than its slice of the buffer): the level-2 grids are sized by
        // this capacity, and a workspace that has seen a huge batch must not launch that batch's grids for a small one
        h_bin.bin_cap = std::min<uint64_t>(ws->cap_hits / h_bin.nbins, std::max<uint64_t>(4 * est_H / h_bin.nbins, 1u << 16));
        FPX_HIP(hipMemsetAsync(d_bin_count, 0, ((size_t)MAX_BINS * BIN_STRIDE + B) * sizeof(uint32_t), b.st));
    }
    return FPX_OK;
}
// a bin per workgroup: k_score_bin over the bins k_probe_group filled
static void score_bins(Batch& b, const Bins& bins, const CandSlots& cs, uint32_t* d_bin_n)
{
    Snapshot* snap = b.snap; Workspace* ws = b.ws;
    const BinArgs& h_bin = bins.h;
    ScoreBinArgs sa{};
    sa.bins = h_bin.bins; sa.bin_cap = h_bin.rec32 ? h_bin.bin_cap / 2u : h_bin.bin_cap; sa.rec_mode = h_bin.rec32; sa.bin_count = h_bin.bin_count; sa.bq = h_bin.shift; sa.B = b.B;
    sa.nsrc = 1u; sa.src_stride = 0; sa.count_stride = 0; sa.count_step = BIN_STRIDE;
    sa.opts = b.d_opts; sa.sb = 32u - b.qb; sa.cands = ws->d_cands[0]; sa.cand_cap = ws->cap_cands; sa.counters = ws->d_counters;
    sa.qcand = cs.qcand; sa.qcand_n = cs.qcand_n; sa.bin_n = d_bin_n; sa.cancel = b.cancel;
    // bins of hundreds of thousands of records (hot-hash data: 12 x the records of a uniform batch) get a filter of 2^15 32-bit cells
    // -- 128 KB, one workgroup per CU -- that counts them in ONE class: two passes over the bin where the 32-KB filter needs 2 K
    sa.refs = bins.ref_cap ? ws->d_refs : nullptr; sa.ref_cap = bins.ref_cap;
    sa.flog2 = bins.est_H / bins.sbins > 60000ull ? 16u : 0u;
    const size_t sb_lds = ((size_t)8u << SB_TABLE_LOG2) + ((size_t)2u << (sa.flog2 ? sa.flog2 : SB_FILTER_LOG2)) + ((size_t)SB_CAND << h_bin.shift) * 8u;
    {   // (a function's attribute belongs to the device it is set on: once per device, not once per process)
        static std::atomic<uint64_t> attr_done{0};
        const uint64_t bit = 1ull << ((unsigned)snap->ctx->device & 63u);
        if (!(attr_done.load(std::memory_order_acquire) & bit)) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_score_bin<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024);
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_score_bin<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024);
            (void)hipGetLastError();
            attr_done.fetch_or(bit, std::memory_order_release);
        }
    }
    if (bins.ref_cap) hipLaunchKernelGGL(k_score_bin<true>, dim3(bins.sbins), dim3(SB_WG), sb_lds, b.st, sa);
    else hipLaunchKernelGGL(k_score_bin<false>, dim3(bins.sbins), dim3(SB_WG), sb_lds, b.st, sa);
}
// bins -> per-query ranges (level 2 of fpx_partition.hpp), then k_score as on the general path, its LDS split sized from the estimated
// records per query
static int score_two_level(Batch& b, const Bins& bins, const CandSlots& cs, uint32_t sbf)
{
    Workspace* ws = b.ws; hipStream_t st = b.st; const uint32_t B = b.B; const BinArgs& h_bin = bins.h;
    const uint32_t tiles = (uint32_t)std::min<uint64_t>((h_bin.bin_cap + L2_TILE - 1) / L2_TILE, 0x7FFFFFFFull / 256u);
    hipLaunchKernelGGL(k_l2_count, dim3(tiles, h_bin.nbins), dim3(256), 0, st, h_bin, bins.d_qcount, B);
    hipLaunchKernelGGL(k_l2_scan, dim3(1), dim3(1024), 0, st, (const uint32_t*)bins.d_qcount, B, ws->d_qrange, ws->d_qcursor, cs.qcand_n,
                       &ws->d_counters[CTR_TOTAL]);
    hipLaunchKernelGGL(k_l2_scatter, dim3(tiles, h_bin.nbins), dim3(256), 0, st, h_bin, ws->d_qcursor, B, ws->d_hits[1], (uint64_t)ws->cap_hits);
    FPX_HIP(hipGetLastError());
    uint32_t log2f, log2t;
    score_filter_sizes(min_floor(b.offsets, b.opts, B), bins.est_H, B, &log2f, &log2t);
    const bool short_queries = bins.est_H / B <= (uint64_t)WG * 8u;
    const size_t score_lds = ((size_t)8 << log2t) + ((size_t)4 << log2f);
    if (short_queries) launch_score<8, false>(b, B, score_lds, ws->d_hits[1], log2f | (log2t << 8), sbf, cs);
    else launch_score<32, false>(b, B, score_lds, ws->d_hits[1], log2f | (log2t << 8), sbf, cs);
    // the queries it handed over (far more records than the filter was sized for): their number is on the device
    launch_score<32, true>(b, std::min<uint32_t>(B, 256u), score_lds, ws->d_hits[1], log2f | (log2t << 8), sbf, cs);
    return FPX_OK;
}

static int run_device_sized(Batch& b, const Keys& keys)
{
    Snapshot* snap = b.snap; Workspace* ws = b.ws; hipStream_t st = b.st; const uint32_t B = b.B; int rc;
    Bins bins;
    if ((rc = size_bins(b, keys, &bins))) return rc;
    const BinArgs& h_bin = bins.h;
    const bool binned = bins.binned;
    Probes pr;
    pr.bins = &bins;
    if ((rc = launch_probes(b, keys, pr))) return rc;
    const bool spread = pr.spread, used_lean = pr.used_lean;
    // ---- 5': bins -> scores, finish; sizes stay on the device
    // (binned: only what k_probe_group could not place itself is in the misc buffer -- normally nothing; the lists of hot hashes,
    // which go there whole, on skewed data: the grid follows what the workspace's last batch left there)
    const uint32_t bin_grid = binned ? (uint32_t)std::min<uint64_t>(std::max<uint64_t>(64, (2 * ws->hint_misc + BIN_TILE - 1) / BIN_TILE), 8192u)
                                     : (uint32_t)std::min<uint64_t>((2 * bins.est_H + BIN_TILE - 1) / BIN_TILE, 8192u);
    hipLaunchKernelGGL(k_bin, dim3(std::max(1u, bin_grid)), dim3(256), 0, st, h_bin, (const uint64_t*)ws->d_hits[1],
                       (const unsigned long long*)&ws->d_counters[CTR_HITS], (uint64_t)ws->cap_hits);
    if ((rc = grow(&ws->d_qrange, &ws->cap_qrange, (size_t)B * 2 + 2))) return rc;
    CandSlots cs;
    if ((rc = ensure_cand_slots(ws, B, 0, &cs))) return rc;
    uint32_t* d_bin_n = bins.d_qcount + B + 64;
    const uint32_t sbf = 32u - b.qb;
    if (binned) score_bins(b, bins, cs, d_bin_n);
    else if ((rc = score_two_level(b, bins, cs, sbf))) return rc;
    // (the results travel through pinned staging: a copy to the caller's pageable memory would block the host until the
    // stream reaches it, and a blocked host cannot watch the deadline.  Small batches: k_finish writes into the staging itself)
    ResultsTo to;
    if ((rc = results_target(b, &to))) return rc;
    // optimistic finish: every query's candidates fit its own slots (C == 0); redone below after a sort otherwise
    launch_finish(b, ws->d_cands[0], 0, sbf, cs, to.res, to.n, b.stats != nullptr);
    FPX_HIP(hipGetLastError());
    // (not spread: the histogram slots ride in the counters)
    if ((rc = publish(b, spread, binned ? d_bin_n : bins.d_bin_count, binned ? bins.sbins : h_bin.nbins, binned ? 1u : BIN_STRIDE))) return rc;
    FPX_HIP(hipEventRecord(ws->ev_end, st));
    FPX_SYNC_BATCH(b);
    // ---- the one look at what happened
    bool redo = false, hits_short = false;
    uint64_t worst_bin = 0, bin_total = 0;
    for (uint32_t i = 0; i < h_bin.nbins; ++i) {
        const uint64_t c = ws->h_bins[BINQ_HEAD + i];
        worst_bin = std::max<uint64_t>(worst_bin, c);
        bin_total += c;
    }
    const uint64_t misc = ws->h_counters[CTR_HITS];
    const uint64_t ref_docs = (binned && bins.ref_cap) ? ws->h_counters[CTR_TOTAL] : 0;         // (docs of the lists that travelled by reference: records of the batch, in no buffer)
    const uint64_t H = binned ? bin_total + ref_docs : ws->h_counters[CTR_TOTAL];
    if (worst_bin > h_bin.bin_cap || misc > ws->cap_hits || H - ref_docs > ws->cap_hits) { redo = true; hits_short = true; }
    if (used_lean)
        for (uint32_t i = 0; i < snap->n_lean; ++i) redo = redo || ws->h_def_count[(size_t)i * DEF_COUNT_STRIDE] > b.def_cap;
    if (ws->h_counters[CTR_MAXSCORE] != 0 || ws->h_counters[CTR_CANDS] > ws->cap_cands || ws->h_counters[CTR_BINFAIL] != 0) redo = true;
    if (ws->h_counters[CTR_BINFAIL] == 3) __atomic_store_n(const_cast<uint32_t*>(&snap->rec32_refused), 1u, __ATOMIC_RELAXED);      // (a doc id beyond the declared range)
    if (redo) {
        if (hits_short) {           // room for what this batch really produced, so that neither path trips over it again
            const size_t need = (size_t)std::max<uint64_t>(std::max<uint64_t>(worst_bin * h_bin.nbins, misc), H) * 5 / 4 + 1024;
            if (ws->cap_hits < need && (rc = grow_pair(ws->d_hits, &ws->cap_hits, need))) return rc;
        }
        ws->hint_H = 0;             // the estimate was off: the general path measures again
        ws->fast_penalty = 4;
        return FPX_REDO;
    }
    const uint64_t Cf = ws->h_counters[CTR_CANDS];
    if (Cf != 0 && (rc = finish_crowded(b, sbf, cs, to, Cf))) return rc;
    if (!b.partial && (rc = deliver_results(ws, B, b.out_cap, to.staged, b.out, b.out_n, st))) return rc;
    const unsigned long long* ls = spread ? host_stat_sets(b) : nullptr;
    const StatSums s = ls ? sum_stat_sets(ls) : StatSums{};
    gather_hist(ws->batch_hist, ws->h_counters, ls, ws->h_counters[CTR_PROBES] + s.probes);
    if (fpx_stats* stats = b.stats) {
        const unsigned long long reads = s.reads + (spread ? (s.dreads + 1) / 2 : 0ull);
        const unsigned long long pads = ws->h_counters[CTR_PADS] + s.pads;          // ("no record" entries in the bins' counts: fpx_partition.hpp, BIN_ALIGN)
        float ms = 0.f, aux = 0.f, total_ms = 0.f;
        if (b.P && (snap->n_file || snap->n_direct)) {
            (void)hipEventElapsedTime(&ms, ws->ev_probe0, ws->ev_probe1);
            if (used_lean) (void)hipEventElapsedTime(&aux, ws->ev_probe1, ws->ev_probe2);
        }
        (void)hipEventElapsedTime(&total_ms, ws->ev_begin, ws->ev_end);
        stats->probes += ws->h_counters[CTR_PROBES] + s.probes; stats->scanned_blocks += ws->h_counters[CTR_BLOCKS] + s.blocks; stats->scanned_docs += ws->h_counters[CTR_DOCS] + s.docs;
        stats->hits += H - (binned ? std::min<unsigned long long>(pads, H) : 0ull);
        stats->algorithmic_bytes += ws->h_counters[CTR_BYTES] + s.blocks * 512ull + s.bytes_off;
        stats->candidates += Cf + ws->h_counters[CTR_SLOTCANDS];
        stats->probe_kernel_ms += ms; stats->total_gpu_ms += total_ms; stats->probe_aux_ms += aux; stats->probe_launches += pr.launches;
        stats->generic_iters += (uint32_t)ws->h_counters[CTR_GENERIC];
        stats->probe_kernel_bytes += spread ? s.blocks * 512ull + s.bytes_off : ws->h_counters[CTR_BYTES];
        stats->probe_kernel_fetched_bytes += spread ? reads * 128ull : unspread_fetched_bytes(ws, snap);
        stats->path_flags |= 1u | (Cf ? 2u : 0u) | (pr.used_fused ? 4u : 0u) | (binned ? 8u : 0u) | (ref_docs ? 32u : 0u);
    }
    if ((rc = deliver_qstats(b))) return rc;
    ws->hint_P = b.P; ws->hint_H = std::max<uint64_t>(H, 1);
    ws->hint_misc = binned ? misc : 0;
    ws->hint_def = 0;
    if (used_lean) for (uint32_t i = 0; i < snap->n_lean; ++i) ws->hint_def = std::max<uint32_t>(ws->hint_def, ws->h_def_count[(size_t)i * DEF_COUNT_STRIDE]);
    return FPX_OK;
}

// ---- a single /_search (B == 1): latency bound, and every HIP call costs microseconds (and a runtime lock shared with the other host
//      threads).  Its pipeline runs with fixed sizes, reads its inputs from and writes its outputs to device-mapped pinned memory (no
//      copy, memset or event calls), synchronises once, and is checked at the end; anything that does not fit falls back to the general path.
static int run_single(Batch& b, const Keys& keys)
{
    Snapshot* snap = b.snap; Workspace* ws = b.ws; hipStream_t st = b.st; int rc;
    Probes pr;
    pr.single_fast = true;
    if ((rc = launch_probes(b, keys, pr))) return rc;
    if (ws->cap_cands < SINGLE_CANDS && (rc = grow_pair(ws->d_cands, &ws->cap_cands, SINGLE_CANDS))) return rc;
    static const hipError_t lds_attr1 = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_score<32, true>),
                                                            hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    (void)lds_attr1;
    const uint32_t log2f = 13, sb1 = 32u - b.qb;
    hipLaunchKernelGGL((k_score<32, true>), dim3(1), dim3(WG), ((size_t)8 << SCORE_TABLE_LOG2) + ((size_t)4 << log2f), st,
                       (const uint64_t*)ws->d_hits[0], (const uint64_t*)nullptr, b.d_opts, log2f | (SCORE_TABLE_LOG2 << 8), sb1, ws->d_cands[0],
                       (uint64_t)SINGLE_CANDS, ws->d_counters, (uint64_t)ws->cap_hits, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, b.cancel);
    if (!ws->d_ret) FPX_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&ws->d_ret), ws->h_counters, 0));
    hipLaunchKernelGGL(k_finish_single, dim3(1), dim3(256), 0, st, (const uint64_t*)ws->d_cands[0], b.d_opts,
                       (const unsigned long long*)ws->d_counters, b.out_cap, ws->d_ret);
    FPX_HIP(hipGetLastError());
    FPX_SYNC_BATCH(b);      // counters, result count and results are in pinned host memory now
    if (b.timeout_ms && now_ms() - b.t_start > (double)b.timeout_ms) return FPX_E_TIMEOUT;
    const uint64_t H = ws->h_counters[CTR_HITS];
    const bool fits = H <= ws->cap_hits && ws->h_counters[CTR_CANDS] <= SINGLE_CANDS && ws->h_counters[CTR_MAXSCORE] == 0;
    if (!fits) {                           // rare: rerun on the general path (which grows buffers / splits as needed)
        if (H > ws->cap_hits && (rc = grow_pair(ws->d_hits, &ws->cap_hits, (size_t)H + 1024))) return rc;
        return FPX_REDO;
    }
    *b.out_n = (uint32_t)ws->h_counters[CTR_COUNT];
    std::memcpy(b.out, ws->h_counters + CTR_COUNT + 1, (size_t)*b.out_n * sizeof(fpx_result));
    gather_hist(ws->batch_hist, ws->h_counters, nullptr, ws->h_counters[CTR_PROBES]);
    if (fpx_stats* stats = b.stats) {        // counters only: the fast path takes no device timestamps
        stats->probes += ws->h_counters[CTR_PROBES]; stats->scanned_blocks += ws->h_counters[CTR_BLOCKS]; stats->scanned_docs += ws->h_counters[CTR_DOCS];
        stats->hits += H; stats->algorithmic_bytes += ws->h_counters[CTR_BYTES]; stats->candidates += ws->h_counters[CTR_CANDS];
        stats->probe_launches += pr.launches; stats->generic_iters += (uint32_t)ws->h_counters[CTR_GENERIC];
        stats->probe_kernel_bytes += ws->h_counters[CTR_BYTES]; stats->probe_kernel_fetched_bytes += unspread_fetched_bytes(ws, snap);
    }
    return FPX_OK;
}

// ---- the general path: every size comes back to the host before the next step is sized; the exchange modes cut it at the hit records
static void add_stats(fpx_stats* dst, const fpx_stats& s)
{
    dst->probes += s.probes; dst->scanned_blocks += s.scanned_blocks; dst->scanned_docs += s.scanned_docs;
    dst->hits += s.hits; dst->algorithmic_bytes += s.algorithmic_bytes; dst->candidates += s.candidates;
    dst->probe_kernel_ms += s.probe_kernel_ms; dst->total_gpu_ms += s.total_gpu_ms; dst->probe_launches += s.probe_launches; dst->generic_iters += s.generic_iters;
    dst->probe_kernel_bytes += s.probe_kernel_bytes; dst->probe_aux_ms += s.probe_aux_ms;
    dst->probe_kernel_fetched_bytes += s.probe_kernel_fetched_bytes;
    dst->path_flags |= s.path_flags;
}

// exchange mode 1: group the H records by destination rank (doc & (world - 1)) and hand them to the caller
static int hand_records_over(Batch& b, const Exchange* ex, uint64_t H)
{
    Workspace* ws = b.ws; hipStream_t st = b.st; int rc;
    const uint32_t world = ex->world, mask = world - 1u;
    if (world > 1 && H) {
        int hcur = 0;
        if ((rc = sort_keys(ws, ws->d_hits, H, 0, bits_for(world), st, &hcur))) return rc;
        if (hcur != 0) std::swap(ws->d_hits[0], ws->d_hits[1]);
    }
    if ((rc = grow(&ws->d_qrange, &ws->cap_qrange, (size_t)world + 2))) return rc;
    hipLaunchKernelGGL(k_dest_bounds, dim3((world + 1 + 63) / 64), dim3(64), 0, st,
                       (const uint64_t*)ws->d_hits[0], H, mask, world, ws->d_qrange);
    FPX_HIP(hipGetLastError());
    std::vector<uint64_t> hb(world + 1);
    FPX_HIP(hipMemcpyAsync(hb.data(), ws->d_qrange, ((size_t)world + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    const bool fits = H <= ex->cap;
    if (fits && H) FPX_HIP(hipMemcpyAsync(ex->d_records, ws->d_hits[0], H * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    FPX_HIP(hipEventRecord(ws->ev_end, st));
    FPX_SYNC_BATCH(b);
    for (uint32_t d = 0; d < world; ++d) ex->counts[d] = hb[d + 1] - hb[d];
    if (!fits) { set_error("records buffer too small: %llu records (counts are filled in; retry with room for them)", (unsigned long long)H); return FPX_E_INVAL; }
    return FPX_OK;
}

// ---- 5+6: partition the H hit records by query, count per (query, doc) in LDS, keep score >= min_score; sort the candidates by
//      (q, score desc, id asc).  *C of them in the shared list d_cands[*ccur]; FPX_SPLIT: a score does not fit the key's `sb` bits
static int score_general(Batch& b, bool score_only, uint64_t H, uint32_t sb, CandSlots* cs, uint64_t* C_out, int* ccur)
{
    Workspace* ws = b.ws; hipStream_t st = b.st; const uint32_t B = b.B; const unsigned qb = b.qb; int rc;
    // partition of the records by query (order inside a query is irrelevant to the hash-table count)
    if ((rc = grow(&ws->d_qrange, &ws->cap_qrange, (size_t)B * 2 + 2))) return rc;
    if (qb) {
        int hcur = 0;
        if ((rc = sort_keys(ws, ws->d_hits, H, 32, 32 + qb, st, &hcur))) return rc;
        if (hcur != 0) std::swap(ws->d_hits[0], ws->d_hits[1]);   // convention: d_hits[0] holds the data
    }
    if ((rc = ensure_cand_slots(ws, B, 0, cs))) return rc;
    hipLaunchKernelGGL(k_bounds, dim3((B + WG - 1) / WG), dim3(WG), 0, st, (const uint64_t*)ws->d_hits[0], H, B, ws->d_qrange, cs->qcand_n);
    uint32_t log2f, log2t;
    score_filter_sizes(min_floor(b.offsets, b.opts, B), H, B, &log2f, &log2t);
    const bool short_queries = H / B <= (uint64_t)WG * 8u;      // the average query fits one 8-row tile
    const size_t score_lds = ((size_t)8 << log2t) + ((size_t)4 << log2f);
    uint64_t C = 0;
    for (int attempt = 0;; ++attempt) {
        if (attempt > 0) {                    // first attempt: the counters are still zero, k_bounds zeroed the slot counts
            FPX_HIP(hipMemsetAsync(&ws->d_counters[CTR_CANDS], 0, sizeof(unsigned long long), st));
            FPX_HIP(hipMemsetAsync(&ws->d_counters[CTR_MAXSCORE], 0, sizeof(unsigned long long), st));
            FPX_HIP(hipMemsetAsync(&ws->d_counters[CTR_HEAVY], 0, sizeof(unsigned long long), st));
            FPX_HIP(hipMemsetAsync(cs->qcand_n, 0, (size_t)B * sizeof(uint32_t), st));
        }
        if (short_queries) launch_score<8, false>(b, B, score_lds, ws->d_hits[0], log2f | (log2t << 8), sb, *cs);
        else launch_score<32, false>(b, B, score_lds, ws->d_hits[0], log2f | (log2t << 8), sb, *cs);
        FPX_HIP(hipGetLastError());
        FPX_HIP(hipMemcpyAsync(ws->h_counters, ws->d_counters, CTR_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        FPX_SYNC_BATCH(b);
        if (ws->h_counters[CTR_HEAVY] != 0) {
            // queries the launch above handed over (far more records than the filter was sized for): rounds over doc classes
            launch_score<32, true>(b, (uint32_t)std::min<uint64_t>(ws->h_counters[CTR_HEAVY], 1024u), score_lds, ws->d_hits[0], log2f | (log2t << 8), sb, *cs);
            FPX_HIP(hipGetLastError());
            FPX_HIP(hipMemcpyAsync(ws->h_counters, ws->d_counters, CTR_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            FPX_SYNC_BATCH(b);
        }
        C = ws->h_counters[CTR_CANDS];
        if (ws->h_counters[CTR_MAXSCORE] != 0) {              // a score does not fit the key's score field
            if (B <= 1) { set_error("score overflows u32"); return FPX_E_INVAL; }
            if (score_only) { set_error("a score does not fit the candidate key: use smaller query batches"); return FPX_E_INVAL; }
            return FPX_SPLIT;                                  // the caller retries with smaller batches
        }
        if (C <= ws->cap_cands) break;
        if (attempt >= 2) { set_error("candidate buffer overflow persists"); return FPX_E_DEVICE; }
        if ((rc = grow_pair(ws->d_cands, &ws->cap_cands, (size_t)C + 1024))) return rc;
    }
    if (C && (rc = sort_keys(ws, ws->d_cands, C, 0, 64, st, ccur))) return rc;
    *C_out = C;
    return FPX_OK;
}

static int run_general(Batch& b, const Keys& keys, const Exchange* ex)
{
    Snapshot* snap = b.snap; Workspace* ws = b.ws; hipStream_t st = b.st; const uint32_t B = b.B; const uint64_t P = b.P;
    const bool probe_only = ex && ex->mode == 1, score_only = ex && ex->mode == 2;
    int rc;
    fpx_stats gs{};                             // this entry's statistics: added to the caller's at the end
    uint64_t H = 0, C = 0;                      // hit records; candidates in the shared list
    // ---- 3+4: probes (rerun with a larger hit buffer on overflow)
    Probes pr;
    for (pr.attempt = 0;; ++pr.attempt) {
        if ((rc = launch_probes(b, keys, pr))) return rc;
        FPX_HIP(hipMemcpyAsync(ws->h_counters, ws->d_counters, CTR_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        FPX_SYNC_BATCH(b);
        if (pr.spread) {
            // the lean / direct kernels' statistics sets, summed into the slots the code below reads
            const StatSums s = sum_stat_sets(host_stat_sets(b));
            ws->h_counters[CTR_LEAN_READS] = s.reads + (s.dreads + 1) / 2;           // (k_probe_direct counts 64-byte requests)
            ws->h_counters[8 + CTR_BLOCKS] = s.blocks; ws->h_counters[8 + CTR_BYTES] = s.blocks * 512ull + s.bytes_off;
            ws->h_counters[8 + CTR_DOCS] = s.docs; ws->h_counters[8 + CTR_PROBES] = s.probes;
        }
        if (P && (snap->n_file || snap->n_direct)) {
            float ms = 0.f;
            FPX_HIP(hipEventElapsedTime(&ms, ws->ev_probe0, ws->ev_probe1));
            gs.probe_kernel_ms = ms;
            gs.probe_aux_ms = 0.f;
            if (pr.used_lean) FPX_HIP(hipEventElapsedTime(&gs.probe_aux_ms, ws->ev_probe1, ws->ev_probe2));
        }
        H = ws->h_counters[CTR_HITS];
        if (pr.used_lean) {
            bool overflow = false;
            for (uint32_t i = 0; i < snap->n_lean; ++i) overflow = overflow || ws->h_def_count[(size_t)i * DEF_COUNT_STRIDE] > b.def_cap;
            if (overflow) {                 // pathological data: nearly every probe needs the generic path
                if (pr.attempt >= 3) { set_error("deferred list overflow persists"); return FPX_E_DEVICE; }
                pr.force_generic = true;
                continue;
            }
        }
        if (H <= ws->cap_hits) break;
        if (pr.attempt >= 4) { set_error("hit buffer overflow persists (%llu records)", (unsigned long long)H); return FPX_E_DEVICE; }
        if ((rc = grow_pair(ws->d_hits, &ws->cap_hits, (size_t)H + 1024))) return rc;
    }
    const bool spread = pr.spread, used_lean = pr.used_lean;
    if (score_only) {                           // the records come from the exchange instead of the probes above
        H = ex->n;
        if (H > ws->cap_hits && (rc = grow_pair(ws->d_hits, &ws->cap_hits, (size_t)H + 1024))) return rc;
        if (H) FPX_HIP(hipMemcpyAsync(ws->d_hits[0], ex->d_records, H * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    }
    if (b.timeout_ms && now_ms() - b.t_start > (double)b.timeout_ms) return FPX_E_TIMEOUT;
    // statistics: slots 0..7 are written by k_probe (generic / deferred / memory), 8..15 by k_probe_lean8
    gs.scanned_blocks = ws->h_counters[CTR_BLOCKS] + ws->h_counters[8 + CTR_BLOCKS]; gs.scanned_docs = ws->h_counters[CTR_DOCS] + ws->h_counters[8 + CTR_DOCS];
    gs.algorithmic_bytes = ws->h_counters[CTR_BYTES] + ws->h_counters[8 + CTR_BYTES]; gs.probes = ws->h_counters[CTR_PROBES] + ws->h_counters[8 + CTR_PROBES];
    gs.generic_iters = (uint32_t)ws->h_counters[CTR_GENERIC];
    gs.probe_kernel_bytes = spread ? ws->h_counters[8 + CTR_BYTES] : ws->h_counters[CTR_BYTES];
    gs.probe_kernel_fetched_bytes = spread ? ws->h_counters[CTR_LEAN_READS] * 128ull /* (lines) */ : unspread_fetched_bytes(ws, snap);
    gs.hits = H; gs.probe_launches = pr.launches; gs.path_flags = pr.used_fused ? 4u : 0u;
    if (!score_only) gather_hist(ws->batch_hist, ws->h_counters, spread ? host_stat_sets(b) : nullptr, gs.probes);
    auto fill_stats = [&]() {
        if (!b.stats) return;
        (void)hipEventElapsedTime(&gs.total_gpu_ms, ws->ev_begin, ws->ev_end);
        add_stats(b.stats, gs);
    };
    if (probe_only) {
        if ((rc = hand_records_over(b, ex, H))) return rc;
        fill_stats();
        return FPX_OK;
    }
    int ccur = 0;
    const uint32_t sb = 32u - b.qb;             // score field of the candidate key; larger scores -> split the batch
    CandSlots cs;                               // (no records: no slots, and k_finish looks at none)
    if (H && (rc = score_general(b, score_only, H, sb, &cs, &C, &ccur))) return rc;
    if (b.timeout_ms && now_ms() - b.t_start > (double)b.timeout_ms) return FPX_E_TIMEOUT;

    // ---- finish
    const bool count_slots = b.stats && cs.qcand_n;
    launch_finish(b, ws->d_cands[ccur], C, sb, cs, b.partial ? b.out : ws->d_out, b.partial ? b.out_n : ws->d_out_n, count_slots);
    FPX_HIP(hipGetLastError());
    bool staged = false;
    if (!b.partial && (rc = stage_results(ws, B, b.out_cap, st, &staged))) return rc;
    if (count_slots)
        FPX_HIP(hipMemcpyAsync(&ws->h_counters[CTR_SLOTCANDS], &ws->d_counters[CTR_SLOTCANDS], sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    FPX_HIP(hipEventRecord(ws->ev_end, st));
    FPX_SYNC_BATCH(b);
    if (b.timeout_ms && now_ms() - b.t_start > (double)b.timeout_ms) return FPX_E_TIMEOUT;
    if (!b.partial && (rc = deliver_results(ws, B, b.out_cap, staged, b.out, b.out_n, st))) return rc;
    gs.candidates = C + (count_slots ? ws->h_counters[CTR_SLOTCANDS] : 0ull);       // (in the shared list + in the queries' own slots)
    fill_stats();
    if ((rc = deliver_qstats(b))) return rc;
    ws->hint_P = P; ws->hint_H = std::max<uint64_t>(H, 1);       // sizes the device-sized path of the next batch
    ws->hint_def = 0;
    if (used_lean) for (uint32_t i = 0; i < snap->n_lean; ++i) ws->hint_def = std::max<uint32_t>(ws->hint_def, ws->h_def_count[(size_t)i * DEF_COUNT_STRIDE]);
    return FPX_OK;
}

// ---- one batch, one path: fill the Batch, choose, call the path's driver.  FPX_REDO_QS and FPX_REDO may escape to the caller: a caller
//      without an Exchange (the only ones whose batches take the paths that raise them) goes through run_with_redos, which re-enters.
static int run_batch(Snapshot* snap, Workspace* ws, const QueryBatch* resident, uint32_t q0,
                     const uint32_t* hashes, const uint64_t* offsets, uint32_t B,
                     const fpx_opts* opts, uint32_t timeout_ms, bool partial,
                     fpx_result* out, uint32_t out_cap, uint32_t* out_n, fpx_stats* stats, const Exchange* ex = nullptr,
                     Try mode = Try::First, double t_call = 0.0, uint64_t* q_blocks = nullptr, uint64_t* q_docs = nullptr)
{
    const bool score_only = ex && ex->mode == 2;
    const bool no_fast = mode == Try::GeneralOnly, no_qs = mode != Try::First;
    Batch b{};
    b.snap = snap; b.ws = ws; b.st = ws->stream;
    b.resident = resident; b.q0 = q0; b.hashes = hashes; b.offsets = offsets; b.opts = opts; b.B = B;
    // the deadline counts from the API call's entry (one deadline per search, src/MultiIndex.zig:314-322), however often the
    // batch re-enters here (a redo on the general path, the two halves of a split)
    b.t_start = t_call != 0.0 ? t_call : now_ms(); b.timeout_ms = timeout_ms;
    std::memset(ws->batch_hist, 0, sizeof ws->batch_hist);
    __atomic_store_n(ws->h_cancel, 0u, __ATOMIC_RELEASE);           // (the stream is idle: the previous call synchronised it)
    b.cancel = timeout_ms ? ws->d_cancel : nullptr;
    b.base = offsets[0]; b.P = offsets[B] - b.base; b.qb = bits_for(B);                         // (q in [0, B))
    b.partial = partial; b.out = out; b.out_cap = out_cap; b.out_n = out_n; b.stats = stats; b.q_blocks = q_blocks; b.q_docs = q_docs;
    const uint64_t P = b.P;
    int rc;
    if ((rc = ensure_queries(ws, B))) return rc;       // d_out_n (+ staging for non-resident batches)
    if ((rc = grow_pair(ws->d_keys, &ws->cap_keys, (size_t)P + 1))) return rc;
    if (!partial && (rc = grow(&ws->d_out, &ws->cap_out, (size_t)B * out_cap + 1))) return rc;
    static_assert(sizeof(fpx_result) == 8, "fpx_result layout");

    // ---- the path.  A: a query per workgroup, where the snapshot and the queries suit k_search_query or k_search_side (a snapshot has one
    //      group or none: never both) or, under option words_wg, k_search_words; B: the pipeline -- for one query its single-launch form, else device-sized (below) or general
    const bool single_fast = B == 1 && !partial && !ex && !no_fast && P != 0 && out_cap <= SINGLE_OUT_MAX &&
                             (snap->n_lean == 0 || P * snap->n_file < lean_min_probes(snap->ctx));
    bool query_wg = false, words_wg = false, side_wg = false, filt = false, low = false;
    if (!ex && !no_fast && !no_qs && !single_fast && B >= 2u && P != 0 && b.qb <= 24u) {
        query_wg = takes_query_wg(snap, offsets, opts, B, &filt, &low);
        words_wg = !query_wg && takes_words_wg(snap, offsets, opts, B, &filt);
        side_wg = !query_wg && !words_wg && takes_side_wg(snap, offsets, opts, B);
        if (query_wg || words_wg || side_wg) {
            // (after a batch that was handed back: the next ones do not try again at once -- hot-hash traffic comes in runs; the
            // snapshot's own count -- a part 1 is a snapshot of its own)
            const uint32_t skip = __atomic_load_n(&snap->qs_skip, __ATOMIC_RELAXED);
            if (skip != 0u) { __atomic_store_n(&snap->qs_skip, skip - 1u, __ATOMIC_RELAXED); query_wg = words_wg = side_wg = false; }
        }
    }

    if (!single_fast) FPX_HIP(hipEventRecord(ws->ev_begin, b.st));
    if ((rc = place_batch(b, query_wg))) return rc;
    if ((rc = ensure_def_lists(b, side_wg))) return rc;
    // (every memset is a 5-us launch of its own: the batch's zeroing rides in kernels that run anyway where it can)
    Keys keys{};
    if (!query_wg && !words_wg && !side_wg && (rc = make_keys(b, single_fast, score_only, &keys))) return rc;
    // per-query scan statistics, when the caller asked for them (a single query's are the call's totals: search_split)
    b.want_q = (q_blocks || q_docs) && B >= 2u && !score_only;
    if (b.want_q && (rc = grow(&ws->d_qstats, &ws->cap_qstats, (size_t)B + 1))) return rc;
    if (query_wg) return run_query_wg(b, filt, low);
    if (words_wg) return run_words_wg(b, filt);
    if (side_wg) return run_side_wg(b);

    if (ws->cap_hits == 0) {
        size_t want = std::max<size_t>(1u << 20, (size_t)P * std::max<uint32_t>(1u, snap->n_file + snap->n_direct + snap->n_mem));
        if ((rc = grow_pair(ws->d_hits, &ws->cap_hits, want))) return rc;
    }
    bool fast = ctx_opt(snap->ctx, OPT_FAST) != 0 && !ex && !no_fast && !single_fast && B >= 2u && P != 0 && b.qb <= 24u &&
                (1u << level1_bits(b.qb)) <= MAX_BINS && ws->hint_H != 0 && ws->hint_P != 0;
    if (fast && ws->fast_penalty != 0) { ws->fast_penalty -= 1; fast = false; }
    if (fast) return run_device_sized(b, keys);
    if (single_fast) return run_single(b, keys);
    return run_general(b, keys, ex);
}

// one pass, or -- when (query index, score) do not fit the 64-bit candidate key -- two half batches
// would part 0 of the snapshot run this batch a query per workgroup?  (run_batch's own test for it, on the host arrays; a batch it would
// not take gains nothing from two parts.  A part 0 whose group has superseded docs or masked columns -- made under query_wg 2 -- only
// while the option is 2)
static bool parts_take(const Snapshot* snap, const uint64_t* offsets, const fpx_opts* opts, uint32_t B)
{
    // (a part 0 in directory + words form -- made under words_wg -- while THAT option allows it)
    const int64_t query_wg = ctx_opt(snap->ctx, snap->part[0]->groups[0]->packed ? OPT_QUERY_WG : OPT_WORDS_WG);
    if (query_wg == 0) return false;
    const Snapshot* p0 = snap->part[0];
    bool filtered = false;                                       // (ANY group of part 0)
    for (uint32_t i = 0; i < p0->n_group; ++i) filtered = filtered || group_filtered(p0->h_group[i]);
    const bool packed = p0->groups[0]->packed;
    if (query_wg != 2 && filtered) return false;
    if (bits_for(B) > 24u || offsets[B] == offsets[0]) return false;
    // (a part 0 of several groups -- made under groups_wg -- while that option allows it; batches with low floors under groups_wg 2
    // with low_wg only: takes_query_wg's rule)
    if (p0->n_group > 1u) return several_groups_ok(p0) && queries_fit_wg(offsets, opts, B, several_groups_low_ok(snap->ctx, filtered));
    // (floors of 1 and 2: takes_query_wg's rule -- option low_wg, a packed part 0; a filtered one under 2 only)
    return queries_fit_wg(offsets, opts, B, packed && low_floors_ok(snap->ctx, filtered));
}

// one batch on one workspace, redone where a path hands it back; FPX_OK, FPX_SPLIT (the caller halves the batch) or an error
static int run_with_redos(Snapshot* snap, Workspace* ws, const QueryBatch* resident, uint32_t q0, const uint32_t* hashes, const uint64_t* offsets, uint32_t B,
                          const fpx_opts* opts, uint32_t timeout_ms, bool partial, fpx_result* out, uint32_t out_cap, uint32_t* out_n, fpx_stats* local,
                          double t_call, uint64_t* q_blocks, uint64_t* q_docs)
{
    auto run = [&](Try mode) { return run_batch(snap, ws, resident, q0, hashes, offsets, B, opts, timeout_ms, partial, out, out_cap, out_n, local, nullptr, mode, t_call, q_blocks, q_docs); };
    int rc = run(Try::First);
    if (rc == FPX_REDO_QS) {                    // the one-workgroup-per-query path handed the batch back: the pipeline
        *local = fpx_stats{};
        rc = run(Try::NoQueryWg);
    }
    if (rc == FPX_REDO) {                       // the device-sized or the single-query path gave up (after its synchronisation): the general path
        *local = fpx_stats{};
        rc = run(Try::GeneralOnly);
    }
    return rc;
}

// A snapshot in TWO PARTS (fpx_snapshot_create): part 0 -- its one packed group, the memory segments behind their table -- a query per
// workgroup, part 1 -- the file segments next to the group -- by the pipeline, each into a table of its own ([B][cap] rows, no relative
// cut-off yet: `partial`); k_merge puts the tables together as it does the ranks' of a segment-sharded index.  The batch is uploaded ONCE:
// part 1 reads part 0's copy.  FPX_SPLIT: nothing has been delivered, the caller takes the whole snapshot's path (which halves the batch).
static int search_parts(Snapshot* snap, const QueryBatch* resident, const uint32_t* hashes, const uint64_t* offsets, uint32_t B,
                        const fpx_opts* opts, uint32_t timeout_ms, fpx_result* out, uint32_t out_cap, uint32_t* out_n, fpx_stats* stats, double t_call,
                        uint64_t* q_blocks, uint64_t* q_docs)
{
    Ctx* ctx = snap->ctx;
    uint32_t cap = 1;
    for (uint32_t q = 0; q < B; ++q) cap = std::max(cap, std::min(opts[q].max_results, out_cap ? out_cap : 1u));
    Workspace* w0 = ws_acquire(ctx);
    Workspace* w1 = w0 ? ws_acquire(ctx) : nullptr;
    if (!w1) { if (w0) ws_release(ctx, w0); return FPX_E_NOMEM; }
    fpx_stats l0{}, l1{};
    std::vector<uint64_t> qb1, qd1;
    if (q_blocks) qb1.assign(B, 0);
    if (q_docs) qd1.assign(B, 0);
    auto body = [&]() -> int {
        int rc;
        if ((rc = grow(&w0->d_parts, &w0->cap_parts, (size_t)2 * B * cap + 1))) return rc;
        if ((rc = grow(&w0->d_parts_n, &w0->cap_parts_n, (size_t)2 * B + 1))) return rc;
        rc = run_with_redos(snap->part[0], w0, resident, 0, hashes, offsets, B, opts, timeout_ms, true, w0->d_parts, cap, w0->d_parts_n, &l0, t_call, q_blocks, q_docs);
        if (rc != FPX_OK) return rc;
        // (part 1 reads the batch where part 0's run left it: the caller's resident batch, or this call's upload in w0)
        QueryBatch view;
        const QueryBatch* rb = resident;
        if (!rb) {
            view.ctx = ctx; view.B = B; view.d_hashes = w0->d_hashes - offsets[0]; view.d_offsets = w0->d_offsets; view.d_opts = w0->d_opts;
            view.offsets.assign(offsets, offsets + B + 1); view.opts.assign(opts, opts + B);
            rb = &view;
        }
        rc = run_with_redos(snap->part[1], w1, rb, 0, nullptr, rb->offsets.data(), B, rb->opts.data(), timeout_ms, true, w0->d_parts + (size_t)B * cap, cap, w0->d_parts_n + B, &l1,
                            t_call, q_blocks ? qb1.data() : nullptr, q_docs ? qd1.data() : nullptr);
        if (rc != FPX_OK) return rc;
        if (timeout_ms && now_ms() - t_call > (double)timeout_ms) { set_error("search timeout"); return FPX_E_TIMEOUT; }
        return merge_partials_impl(ctx, w0->d_parts, w0->d_parts_n, 2, B, cap, opts, offsets, out, out_cap, out_n);
    };
    const int rc = body();
    if (rc != FPX_OK) {
        (void)hipStreamSynchronize(w0->stream); (void)hipStreamSynchronize(w1->stream);
        if (w0->copy_stream) (void)hipStreamSynchronize(w0->copy_stream);
    } else {
        ctx_hist_add(ctx, w0->batch_hist, w0->batch_hist[HIST_SLOTS]);
        ctx_hist_add(ctx, w1->batch_hist, w1->batch_hist[HIST_SLOTS]);
        for (uint32_t q = 0; q < B; ++q) { if (q_blocks) q_blocks[q] += qb1[q]; if (q_docs) q_docs[q] += qd1[q]; }
        if (stats) { add_stats(stats, l0); add_stats(stats, l1); stats->path_flags |= 128u; }
    }
    ws_release(ctx, w1);
    ws_release(ctx, w0);
    return rc;
}

static int search_split(Snapshot* snap, const QueryBatch* resident, uint32_t q0,
                        const uint32_t* hashes, const uint64_t* offsets, uint32_t B,
                        const fpx_opts* opts, uint32_t timeout_ms, bool partial,
                        fpx_result* out, uint32_t out_cap, uint32_t* out_n, fpx_stats* stats, double t_call,
                        uint64_t* q_blocks = nullptr, uint64_t* q_docs = nullptr)
{
    Workspace* ws = ws_acquire(snap->ctx);
    if (!ws) return FPX_E_NOMEM;
    fpx_stats local{};
    int rc = run_with_redos(snap, ws, resident, q0, hashes, offsets, B, opts, timeout_ms, partial, out, out_cap, out_n, &local, t_call, q_blocks, q_docs);
    if (rc == FPX_OK && B == 1) {               // (one query: its statistics are the call's)
        if (q_blocks) q_blocks[0] = local.scanned_blocks;
        if (q_docs) q_docs[0] = local.scanned_docs;
    }
    if (rc != FPX_OK) { (void)hipStreamSynchronize(ws->stream); if (ws->copy_stream) (void)hipStreamSynchronize(ws->copy_stream); }
    if (rc == FPX_OK) ctx_hist_add(snap->ctx, ws->batch_hist, ws->batch_hist[HIST_SLOTS]);       // (the context's running scan histograms: fpx_ctx_scan_histograms)
    ws_release(snap->ctx, ws);
    if (rc == FPX_OK) { if (stats) add_stats(stats, local); return FPX_OK; }
    if (rc != FPX_SPLIT) return rc;
    if (B <= 1) { set_error("internal: single query cannot be split"); return FPX_E_DEVICE; }
    const uint32_t half = B / 2;
    rc = search_split(snap, resident, q0, hashes, offsets, half, opts, timeout_ms, partial, out, out_cap, out_n, stats, t_call, q_blocks, q_docs);
    if (rc) return rc;
    fpx_result* out2 = out ? out + (size_t)half * out_cap : out;
    return search_split(snap, resident, q0 + half, hashes, offsets + half, B - half, opts + half, timeout_ms, partial,
                        out2, out_cap, out_n + half, stats, t_call, q_blocks ? q_blocks + half : nullptr, q_docs ? q_docs + half : nullptr);
}

int search_batch_impl(Snapshot* snap, const QueryBatch* resident, const uint32_t* hashes, const uint64_t* offsets, uint32_t B,
                      const fpx_opts* opts, uint32_t timeout_ms, bool partial,
                      fpx_result* out, uint32_t out_cap, uint32_t* out_n, fpx_stats* stats, uint64_t* q_blocks, uint64_t* q_docs)
{
    if (resident) { offsets = resident->offsets.data(); opts = resident->opts.data(); B = resident->B; hashes = nullptr; }
    if (!snap || !offsets || !opts || !out_n || (!out && out_cap) || (!resident && B && offsets[B] && !hashes)) {
        set_error("null argument"); return FPX_E_INVAL;
    }
    if (resident && resident->ctx != snap->ctx) { set_error("query batch and snapshot belong to different contexts"); return FPX_E_INVAL; }
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (B == 0) return FPX_OK;
    for (uint32_t q = 0; q < B; ++q) {
        if (offsets[q + 1] < offsets[q]) { set_error("offsets must be non-decreasing"); return FPX_E_INVAL; }
        if (offsets[q + 1] - offsets[q] >= (1ull << 32)) { set_error("query longer than 2^32-1 hashes"); return FPX_E_INVAL; }
    }
    FPX_HIP(hipSetDevice(snap->ctx->device));
    const double t_call = now_ms();
    if (!partial && snap->part[0] && B >= 2u && parts_take(snap, offsets, opts, B)) {
        const int rc = search_parts(snap, resident, hashes, offsets, B, opts, timeout_ms, out, out_cap, out_n, stats, t_call, q_blocks, q_docs);
        if (rc != FPX_SPLIT) return rc;
        if (stats) std::memset(stats, 0, sizeof *stats);
    }
    return search_split(snap, resident, 0, hashes, offsets, B, opts, timeout_ms, partial, out, out_cap, out_n, stats, t_call, q_blocks, q_docs);
}

int probe_records_impl(Snapshot* snap, const QueryBatch* qb, uint32_t world, uint32_t timeout_ms,
                       uint64_t* d_records, uint64_t records_cap, uint64_t* counts, fpx_stats* stats)
{
    if (qb->ctx != snap->ctx) { set_error("query batch and snapshot belong to different contexts"); return FPX_E_INVAL; }
    if (stats) std::memset(stats, 0, sizeof *stats);
    for (uint32_t d = 0; d < world; ++d) counts[d] = 0;
    if (qb->B == 0) return FPX_OK;
    FPX_HIP(hipSetDevice(snap->ctx->device));
    Workspace* ws = ws_acquire(snap->ctx);
    if (!ws) return FPX_E_NOMEM;
    Exchange ex;
    ex.mode = 1; ex.world = world; ex.d_records = d_records; ex.cap = records_cap; ex.counts = counts;
    int rc = run_batch(snap, ws, qb, 0, nullptr, qb->offsets.data(), qb->B, qb->opts.data(), timeout_ms, true,
                       nullptr, 0, nullptr, stats, &ex);
    if (rc != FPX_OK) (void)hipStreamSynchronize(ws->stream);
    ws_release(snap->ctx, ws);
    return rc;
}

int score_records_impl(Ctx* ctx, const QueryBatch* qb, const uint64_t* d_records, uint64_t num_records, uint32_t timeout_ms,
                       fpx_result* d_out, uint32_t out_cap, uint32_t* d_out_n)
{
    if (qb->ctx != ctx) { set_error("query batch belongs to a different context"); return FPX_E_INVAL; }
    if (qb->B == 0) return FPX_OK;
    FPX_HIP(hipSetDevice(ctx->device));
    Workspace* ws = ws_acquire(ctx);
    if (!ws) return FPX_E_NOMEM;
    Snapshot none;                                  // no segments: the probe stage finds nothing to do
    none.ctx = ctx;
    Exchange ex;
    ex.mode = 2; ex.d_records = const_cast<uint64_t*>(d_records); ex.n = num_records;
    int rc = run_batch(&none, ws, qb, 0, nullptr, qb->offsets.data(), qb->B, qb->opts.data(), timeout_ms, true,
                       d_out, out_cap, d_out_n, nullptr, &ex);
    if (rc != FPX_OK) (void)hipStreamSynchronize(ws->stream);
    ws_release(ctx, ws);
    return rc;
}

void query_batch_free(QueryBatch* qb)
{
    if (!qb) return;
    (void)hipSetDevice(qb->ctx->device);
    if (qb->d_hashes) (void)hipFree(qb->d_hashes);
    if (qb->d_offsets) (void)hipFree(qb->d_offsets);
    if (qb->d_opts) (void)hipFree(qb->d_opts);
    delete qb;
}

int query_batch_create_impl(Ctx* ctx, const uint32_t* hashes, const uint64_t* offsets, uint32_t B,
                            const fpx_opts* opts, QueryBatch** out)
{
    *out = nullptr;
    if (!ctx || !offsets || !opts || (B && offsets[B] && !hashes)) { set_error("null argument"); return FPX_E_INVAL; }
    if (offsets[0] != 0) { set_error("offsets[0] must be 0"); return FPX_E_INVAL; }
    for (uint32_t q = 0; q < B; ++q) {
        if (offsets[q + 1] < offsets[q]) { set_error("offsets must be non-decreasing"); return FPX_E_INVAL; }
    }
    FPX_HIP(hipSetDevice(ctx->device));
    QueryBatch* qb = new (std::nothrow) QueryBatch();
    if (!qb) return FPX_E_NOMEM;
    qb->ctx = ctx; qb->B = B;
    qb->offsets.assign(offsets, offsets + B + 1);
    qb->opts.assign(opts, opts + B);
    std::vector<uint32_t> h_opts;
    fill_opts(h_opts, opts, offsets, B);
    const uint64_t P = offsets[B];
    hipError_t e = dmalloc(&qb->d_hashes, (P + 1) * sizeof(uint32_t));
    if (e == hipSuccess) e = dmalloc(&qb->d_offsets, ((size_t)B + 1) * sizeof(uint64_t));
    if (e == hipSuccess) e = dmalloc(&qb->d_opts, ((size_t)B * 4 + 4) * sizeof(uint32_t));
    if (e == hipSuccess && P) e = hipMemcpy(qb->d_hashes, hashes, P * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(qb->d_offsets, offsets, ((size_t)B + 1) * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && B) e = hipMemcpy(qb->d_opts, h_opts.data(), h_opts.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { query_batch_free(qb); return hip_fail(e, "query batch upload"); }
    *out = qb;
    return FPX_OK;
}

int merge_partials_impl(Ctx* ctx, const void* d_parts, const void* d_counts, uint32_t world,
                        uint32_t B, uint32_t part_cap, const fpx_opts* opts, const uint64_t* offsets,
                        fpx_result* out, uint32_t out_cap, uint32_t* out_n)
{
    if (!ctx || !d_parts || !d_counts || !opts || !offsets || !out_n) { set_error("null argument"); return FPX_E_INVAL; }
    if (B == 0) return FPX_OK;
    FPX_HIP(hipSetDevice(ctx->device));
    Workspace* ws = ws_acquire(ctx);
    if (!ws) return FPX_E_NOMEM;
    int rc = FPX_OK;
    auto body = [&]() -> int {
        int r;
        if ((r = ensure_queries(ws, B))) return r;
        if ((r = grow(&ws->d_out, &ws->cap_out, (size_t)B * out_cap + 1))) return r;
        std::vector<uint32_t> h_opts;
        fill_opts(h_opts, opts, offsets, B);
        hipStream_t st = ws->stream;
        FPX_HIP(hipMemcpyAsync(ws->d_opts, h_opts.data(), h_opts.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_merge, dim3((B + 127) / 128), dim3(128), 0, st,
                           (const fpx_result*)d_parts, (const uint32_t*)d_counts, world, B, part_cap, ws->d_opts,
                           ws->d_out, out_cap, ws->d_out_n);
        FPX_HIP(hipGetLastError());
        bool staged = false;
        if ((r = stage_results(ws, B, out_cap, st, &staged))) return r;
        FPX_HIP(hipStreamSynchronize(st));
        return deliver_results(ws, B, out_cap, staged, out, out_n, st);
    };
    rc = body();
    ws_release(ctx, ws);
    return rc;
}

// ------------------------------------------------------------------------------------------------
// An index sharded by HASH RANGE: every rank holds the same window of the hash space of ALL segments (its slice
// of their group), so a rank makes, sorts and probes only the query hashes of its window -- 1/N of the batch's work.  A query's
// hit records then come from every rank; SearchResults.incr is a keyed sum (src/common.zig:121-129) and a hash's walk is
// independent of every other hash (src/FileSegment.zig:143-176), so they may be counted wherever they are brought together:
// rank r FINISHES the queries of its share of the batch's bins (bins of 8 queries, as on one GPU).
//   fpx_shard_probe   keys of the window -> k_probe_group<.., BINNED> drops the records into the batch's bins, [N x bpr][cell_cap]
//                     in the caller's send buffer (bpr = bins per rank), + the bins' fill counts
//   (the caller's all-to-all: bins [r bpr, (r + 1) bpr) travel to rank r -- fixed shapes, no sizes to agree on first)
//   fpx_shard_score   k_score_bin over the N pieces of each of the rank's bins + k_finish: the final results of its queries
// No table gather, no merge: a query's results are complete on the rank that owns it.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t SHARD_BQ = 3;           // queries per bin, as on one GPU: a rank receives ALL records of its bins
constexpr uint64_t SHARD_NEED_MARK = 0x40000000ull;     // a travelling count >= this: "my bins need (count & (mark - 1)) cells" (fpx.h, fpx_shard_score)

// per query: the hashes inside [win_lo, win_hi] -- later occurrences dropped (dedupSorted, src/Index.zig:489-499) -- as keys in the
// query's `stride` slots, their number in ko.qn[q], their counts per hash bucket added to ko.cnt (fpx_keyorder.hpp).
// QPW queries per workgroup: a wave each where the window is narrow (stride <= 1024: a rank of 2 or more), the workgroup
// for one otherwise.  Two phases, because only the window's share of the hashes needs the hash set: (1) all loads out, the hashes of
// the window compacted into an LDS list with ballots -- no atomics on a wave's own count; (2) the list through the hash set, the
// fresh ones to their slots.  (One pass that sent every loaded hash through the set and an LDS counter took 153 us for 16384
// queries at a rank of 2 -- 500 returning atomics on one address per query -- and, a wave per query with sixteen dependent
// rounds, 215 us for 65536 queries at a rank of 8.)
// QPW == 8: a workgroup of eight waves makes the keys of one GROUP of queries (KO_GROUP = 8), a wave per query: the group's bucket
// counts are summed in LDS and stored plainly -- no atomics on the count table, which needs no zeroing then.
// QPW == 1: a workgroup of four waves per query (wide windows: up to DEDUP_MAX hashes of the window), counts added atomically.
template <int QPW, uint32_t CAP>
__global__ __launch_bounds__(QPW == 8 ? 512 : 256) void k_make_keys_window(const uint32_t* __restrict__ hashes_base, const uint64_t* __restrict__ offsets,
                                                          uint32_t B, uint32_t qb, uint64_t* __restrict__ keys, uint32_t stride,
                                                          uint32_t win_lo, uint32_t win_hi, unsigned long long* counters, uint32_t* __restrict__ overflow,
                                                          KeyOrder ko)
{
    static_assert(QPW == 1 || QPW == 8, "a workgroup per query, or a wave per query of a group");
    constexpr uint32_t WG_T = QPW == 8 ? 512u : 256u;
    constexpr uint32_t TEAM = WG_T / QPW;                                   // threads per query: 64 or 256
    constexpr uint32_t UNR = QPW == 8 ? 16u : 4u;                           // loads a thread has in flight: 1024 hashes per round either way
    constexpr uint32_t LIST_CAP = CAP;                                      // hashes of the window a query may have
    constexpr uint32_t SLOTS = 2u * CAP;
    constexpr uint32_t SLOT_SHIFT = 32u - (CAP == 512u ? 10u : CAP == 1024u ? 11u : 12u);
    static_assert(CAP == 512u || CAP == 1024u || CAP == 2048u, "the hash set's size");
    __shared__ uint32_t s_list[QPW][LIST_CAP];
    __shared__ uint32_t s_tab[QPW][SLOTS];
    __shared__ uint32_t s_hist[KO_MAX_BUCKETS];                             // of the workgroup: one query, or one group of eight
    __shared__ uint32_t s_n[QPW], s_out[QPW], s_ones[QPW];
    const uint32_t tid = threadIdx.x, team = tid / TEAM, lt = tid % TEAM, lane = tid & 63u;
    const uint32_t q = blockIdx.x * QPW + team;
    if (blockIdx.x == 0 && tid < CTR_COUNT) counters[tid] = 0ull;
    const bool live = q < B;                                                 // (QPW == 8: the last group may be short; every wave reaches the barriers)
    for (uint32_t i = lt; i < SLOTS; i += TEAM) s_tab[team][i] = 0xFFFFFFFFu;
    if (tid < KO_MAX_BUCKETS) s_hist[tid] = 0u;
    if (lt == 0) { s_n[team] = 0u; s_out[team] = 0u; s_ones[team] = 0u; }
    __syncthreads();
    const uint64_t lo = live ? offsets[q] : 0ull, hi = live ? offsets[q + 1] : 0ull;
    const uint64_t below = (1ull << lane) - 1ull;
    // ---- phase 1: the window's hashes into the list
    uint32_t n = 0;                                                          // (QPW == 8: the wave's own running count)
    for (uint64_t i0 = lo; i0 < hi; i0 += TEAM * UNR) {
        uint32_t h[UNR]; bool in[UNR];
#pragma unroll
        for (uint32_t u = 0; u < UNR; ++u) {
            const uint64_t i = i0 + u * TEAM + lt;
            in[u] = i < hi;
            h[u] = in[u] ? hashes_base[i] : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < UNR; ++u) {
            in[u] = in[u] && h[u] >= win_lo && h[u] <= win_hi;
            const uint64_t m = __ballot(in[u]);
            if (m == 0ull) continue;
            uint32_t base = n;
            if constexpr (QPW == 1) {
                if (lane == (uint32_t)__builtin_ctzll(m)) base = atomicAdd(&s_n[team], (uint32_t)__popcll(m));
                base = __shfl(base, __builtin_ctzll(m));
            } else {
                n += (uint32_t)__popcll(m);
            }
            const uint32_t at = base + (uint32_t)__popcll(m & below);
            if (in[u] && at < LIST_CAP) s_list[team][at] = h[u];
        }
    }
    __syncthreads();
    if constexpr (QPW == 1) n = s_n[team];
    if (n > LIST_CAP) { if (lt == 0) *overflow = 1u; n = LIST_CAP; }
    // ---- phase 2: the list through the hash set; the first occurrence of a hash becomes a key
    uint64_t* mine = keys + (size_t)q * stride;
    uint32_t n_out = 0;
    for (uint32_t j0 = 0; j0 < n; j0 += TEAM) {
        const uint32_t j = j0 + lt;
        const bool have = j < n;
        const uint32_t h = have ? s_list[team][j] : 0u;
        bool fresh = false;
        if (have) {
            if (h == 0xFFFFFFFFu) {
                fresh = atomicExch(&s_ones[team], 1u) == 0u;            // (the table's empty mark is kept apart)
            } else {
                uint32_t slot = (h * 0x9E3779B1u) >> SLOT_SHIFT;
                for (;;) {
                    const uint32_t old = atomicCAS(&s_tab[team][slot], 0xFFFFFFFFu, h);
                    if (old == 0xFFFFFFFFu) { fresh = true; break; }
                    if (old == h) break;
                    slot = (slot + 1u) & (SLOTS - 1u);
                }
            }
        }
        const uint64_t m = __ballot(fresh);
        if (m == 0ull) continue;
        uint32_t base = n_out;
        if constexpr (QPW == 1) {
            if (lane == (uint32_t)__builtin_ctzll(m)) base = atomicAdd(&s_out[team], (uint32_t)__popcll(m));
            base = __shfl(base, __builtin_ctzll(m));
        } else {
            n_out += (uint32_t)__popcll(m);
        }
        const uint32_t at = base + (uint32_t)__popcll(m & below);
        if (fresh) {
            if (at < stride) {
                mine[at] = ((uint64_t)h << qb) | q;
                if (ko.nb) atomicAdd(&s_hist[(h >> ko.bshift) & (ko.nb - 1u)], 1u);
            } else {
                *overflow = 1u;
            }
        }
    }
    __syncthreads();
    if constexpr (QPW == 1) n_out = s_out[team];
    if (live && lt == 0 && ko.qn) ko.qn[q] = min(n_out, stride);
    if (ko.nb && tid < ko.nb) {
        const uint32_t G = (B + KO_GROUP - 1u) / KO_GROUP;
        if constexpr (QPW == 8) ko.cnt[(size_t)tid * G + blockIdx.x] = s_hist[tid];                       // (the group's cell: this workgroup's alone)
        else if (s_hist[tid] != 0u) atomicAdd(&ko.cnt[(size_t)tid * G + q / KO_GROUP], s_hist[tid]);
    }
}

// the bins' fill counts, compact (what travels with the bins), the fullest one and their sum
// (bit 31 of a travelling count: the bin's records are the 4-byte ones -- the receiving rank reads it per piece, ScoreBinArgs::rec_mode 2)
__global__ void k_cell_counts(const unsigned int* __restrict__ bin_count, uint32_t ncells, uint32_t* __restrict__ out, unsigned long long* __restrict__ counters,
                              uint32_t flag)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncells) return;
    const unsigned int v = bin_count[(size_t)c * BIN_STRIDE];
    out[c] = v | flag;
    atomicMax(&counters[CTR_TOTAL], (unsigned long long)v);
    atomicAdd(&counters[CTR_SLOTCANDS], (unsigned long long)v);
}

static unsigned log2_exact(uint32_t v) { unsigned b = 0; while ((1u << b) < v) ++b; return b; }

// hash bits the keys of a window are ordered by: with the window's own constant bits, the top 8 (as on one GPU)
static unsigned shard_sort_bits(unsigned win_bits) { return win_bits >= 8u ? 0u : 8u - win_bits; }

static_assert(SHARD_DEDUP_MAX == DEDUP_MAX, "fpx_sharded.hip routes longer queries to the record protocol");
static_assert(QS_SHARE_BQ == SHARD_BQ && QS_SHARE_STRIDE == BIN_STRIDE && DEDUP_MAX <= QS_MAX_HASHES, "k_search_window fills the protocol's bins");
static_assert(QS_PACK_MAX <= DEDUP_MAX, "k_search_packed takes the shorter queries of what k_search_window takes");
// Option shard_wg: would a step of the bin protocol on this snapshot WALK ITS WINDOW A QUERY PER WORKGROUP (k_search_window, fpx_qsearch.hpp)?
// ONE packed group with its hash window and nothing else -- or that plus memory segments behind their one table --, unfiltered (1) or
// filtered too (2).  (The caller has refused solo and block segments and memory segments without a table.)  The back-off after a
// hand-back, snap->qs_skip, is the caller's to look at: it counts calls.
bool shard_window_walk_ok(const Snapshot* snap)
{
    const int64_t shard_wg = ctx_opt(snap->ctx, OPT_SHARD_WG);
    if (shard_wg != 1 && shard_wg != 2) return false;
    if (snap->n_group != 1 || snap->n_solo != 0 || snap->n_file != 0 || !snap->groups[0]->packed) return false;
    if (snap->n_mem != 0 && snap->mem_items != 0 && !snap->d_memtab) return false;
    return shard_wg == 2 || !group_filtered(snap->h_group[0]);
}
// bins per rank: the batch's bins of 2^SHARD_BQ queries, dealt to the ranks in contiguous runs
int shard_bins_per_rank(uint32_t B, uint32_t world)
{
    const uint32_t nb = (B + (1u << SHARD_BQ) - 1u) >> SHARD_BQ;
    return (int)((nb + world - 1u) / world);
}

int shard_probe_impl(Snapshot* snap, const QueryBatch* qb, uint32_t world, uint32_t timeout_ms,
                     uint64_t* d_send, uint64_t cell_cap, uint32_t* d_send_counts, uint64_t* needed_cell_cap, fpx_stats* stats)
{
    if (qb->ctx != snap->ctx) { set_error("query batch and snapshot belong to different contexts"); return FPX_E_INVAL; }
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (needed_cell_cap) *needed_cell_cap = 0;
    const uint32_t B = qb->B;
    if (B == 0) return FPX_OK;
    // the bin protocol serves snapshots that are groups of direct-addressed segments with one hash window and nothing else;
    // anything else goes through fpx_probe_resident / fpx_score_partial (same results)
    // ... and memory segments behind the snapshot's ONE table (k_probe_memtab reads keys in any order; its records are binned with the
    // ones the group kernels could not place): a live index -- every Index.update publishes a memory segment, src/Index.zig:515-587
    if (snap->n_group == 0 || snap->n_solo != 0 || snap->n_file != 0 || (snap->n_mem != 0 && !snap->d_memtab && snap->mem_items != 0)) {
        set_error("fpx_shard_probe: the snapshot is not made of groups of direct-addressed segments (and memory segments behind their table) alone (use fpx_probe_resident)"); return FPX_E_INVAL;
    }
    uint32_t win_lo = snap->h_group[0].win_lo, win_hi = snap->h_group[0].win_hi;
    for (const GroupDesc& gd : snap->h_group)
        if (gd.win_lo != win_lo || gd.win_hi != win_hi) { set_error("fpx_shard_probe: the snapshot's groups have different hash windows"); return FPX_E_INVAL; }
    const uint64_t* offsets = qb->offsets.data();
    uint64_t max_len = 0;
    for (uint32_t q = 0; q < B; ++q) max_len = std::max<uint64_t>(max_len, offsets[q + 1] - offsets[q]);
    if (max_len > DEDUP_MAX) { set_error("fpx_shard_probe: queries of more than %u hashes (use fpx_probe_resident)", DEDUP_MAX); return FPX_E_INVAL; }
    // (a floor of 1 or 2 -- the legacy protocol's options, or a query of <= 40 hashes -- makes every counted doc a candidate: the
    // one-GPU path hands such batches to k_score's count-only round, run_batch's `binned`; here the record protocol takes them)
    for (uint32_t q = 0; q < B; ++q) {
        const fpx_opts& o = qb->opts[q];
        if (query_floor(o, offsets[q + 1] - offsets[q]) <= 2u) {
            set_error("fpx_shard_probe: query %u has a score floor of 1 or 2: this batch takes the record protocol (fpx_probe_resident)", q); return FPX_E_INVAL;
        }
    }
    if (max_len == 0) max_len = 1;
    const unsigned qbits = bits_for(B);
    if (qbits > 24u) { set_error("fpx_shard_probe: at most 2^24 queries"); return FPX_E_INVAL; }
    const uint32_t ncells = (uint32_t)shard_bins_per_rank(B, world) * world;
    if (ncells > (1u << 21)) { set_error("fpx_shard_probe: too many bins"); return FPX_E_INVAL; }
    // the window's share of the hash space (what fraction of a query's hashes to expect here)
    const double share = ((double)win_hi - (double)win_lo + 1.0) / 4294967296.0;
    const unsigned win_bits = log2_exact(std::max<uint32_t>(1u, (uint32_t)(1.0 / std::max(share, 1e-9) + 0.5)));      // the window's constant top hash bits
    FPX_HIP(hipSetDevice(snap->ctx->device));
    Workspace* ws = ws_acquire(snap->ctx);
    if (!ws) return FPX_E_NOMEM;
    auto body = [&]() -> int {
        int rc;
        hipStream_t st = ws->stream;
        const double t_start = now_ms();
        __atomic_store_n(ws->h_cancel, 0u, __ATOMIC_RELEASE);
        const uint32_t* cancel = timeout_ms ? ws->d_cancel : nullptr;
        // [bins' fill counters, a line each | LEAN_STAT_SETS x 8 u64 statistics slots | overflow flag]
        const size_t cell_words = (size_t)ncells * BIN_STRIDE, words = cell_words + LEAN_STAT_WORDS + 16;
        if (words > ws->cap_cells) {
            if (ws->d_cells) (void)hipFree(ws->d_cells);
            if (ws->h_cells) (void)hipHostFree(ws->h_cells);
            ws->d_cells = nullptr; ws->h_cells = nullptr; ws->cap_cells = 0;
            FPX_HIP(dmalloc(&ws->d_cells, words * sizeof(uint32_t)));
            FPX_HIP(hipHostMalloc(reinterpret_cast<void**>(&ws->h_cells), (LEAN_STAT_WORDS + 16) * sizeof(uint32_t)));
            ws->cap_cells = words;
        }
        uint32_t* d_stats32 = ws->d_cells + cell_words;
        uint32_t* d_overflow = d_stats32 + LEAN_STAT_WORDS;
        if (ws->cap_hits == 0 && (rc = grow_pair(ws->d_hits, &ws->cap_hits, (size_t)1 << 22))) return rc;
        // a query's share of its hashes + slack; a query that needs more has the whole query's length on the second attempt
        uint32_t stride = (uint32_t)std::min<uint64_t>(max_len, (uint64_t)((double)max_len * share * 1.25) + 48);
        const bool rec32_enabled = ctx_opt(snap->ctx, OPT_REC32) != 0;
        uint64_t rec_cap = cell_cap;                           // records a bin's cells hold
        // option shard_wg: the window walked a query per workgroup (k_search_window) -- no keys, one launch.  After a hand-back the
        // snapshot's next 32 calls do not try (qs_skip, as on one GPU)
        // option shard_pack: the walk by k_search_packed -- the window's probes packed before the rounds -- for a batch whose longest query
        // its hash registers hold whole; a longer one keeps the batch on k_search_window
        bool walk = shard_window_walk_ok(snap), walked = false, packed = false;
        const bool pack = ctx_opt(snap->ctx, OPT_SHARD_PACK) == 1 && max_len <= QS_PACK_MAX;
        if (walk) {
            const uint32_t skip = __atomic_load_n(&snap->qs_skip, __ATOMIC_RELAXED);
            if (skip != 0u) { __atomic_store_n(&snap->qs_skip, skip - 1u, __ATOMIC_RELAXED); walk = false; }
        }
        for (int attempt = 0;; ++attempt) {
            // 4-byte records (two per 8-byte cell) where the doc ids leave room for the query's three bits inside its bin
            const uint32_t rec32 = rec32_enabled && !__atomic_load_n(&snap->rec32_refused, __ATOMIC_RELAXED) &&
                                   snap->max_doc_declared < (0xFFFFFFFFu >> SHARD_BQ) ? 1u : 0u;
            rec_cap = cell_cap << rec32;
            if (walk) {
                FPX_HIP(hipMemsetAsync(ws->d_cells, 0, words * sizeof(uint32_t), st));
                FPX_HIP(hipMemsetAsync(ws->d_counters, 0, CTR_COUNT * sizeof(unsigned long long), st));
                QSearchArgs qa{};
                qa.hashes_base = qb->d_hashes; qa.offsets = qb->d_offsets; qa.opts = qb->d_opts; qa.q_begin = 0u; qa.q_end = B; qa.sb = 32u - qbits;
                qa.counters = ws->d_counters; qa.stat_sets = reinterpret_cast<unsigned long long*>(d_stats32); qa.qstats = nullptr; qa.cancel = cancel;
                if (snap->n_mem != 0 && snap->mem_items != 0) { qa.mem_tab = snap->d_memtab; qa.mem_bucket = snap->d_membucket; qa.mem_bits = snap->d_membits; }
                // (the step's bins: no candidates, no slots, no redo list -- QSearchArgs)
                qa.bins = d_send; qa.bin_cap = rec_cap; qa.bin_fill = ws->d_cells; qa.bin_rec32 = rec32;
                // (the launch's queue of queries: a word behind the overflow flag, zeroed with the cells)
                qa.next_q = FPX_QS_DYN ? d_overflow + 4 : nullptr; qa.stagger = 0u;
                const GroupArgs gargs{snap->h_group[0], snap->d_direct};
                const dim3 grid(std::min<uint32_t>(B, (uint32_t)device_cus(snap->ctx) * QS_WGS_PER_CU));
                FPX_HIP(hipEventRecord(ws->ev_probe0, st));
                const bool ns8 = snap->groups[0]->ns == 8u, mem = qa.mem_tab != nullptr, filt = group_filtered(snap->h_group[0]);
                if (pack) FPX_LAUNCH_QS(k_search_packed, grid, st, qa, gargs, ns8, mem, filt);
                else FPX_LAUNCH_QS(k_search_window, grid, st, qa, gargs, ns8, mem, filt);
                FPX_HIP(hipEventRecord(ws->ev_probe1, st));
                hipLaunchKernelGGL(k_cell_counts, dim3((ncells + 255) / 256), dim3(256), 0, st, (const unsigned int*)ws->d_cells, ncells, d_send_counts, ws->d_counters,
                                   rec32 << 31);
                FPX_HIP(hipGetLastError());
                FPX_HIP(hipMemcpyAsync(ws->h_counters, ws->d_counters, CTR_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
                FPX_HIP(hipMemcpyAsync(ws->h_cells, d_stats32, (LEAN_STAT_WORDS + 16) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                FPX_SYNC(ws);
                if (ws->h_counters[CTR_BINFAIL] == 3 && attempt < 3) {            // a doc id beyond the segments' declared range: wide records
                    __atomic_store_n(&snap->rec32_refused, 1u, __ATOMIC_RELAXED);
                    continue;
                }
                if (ws->h_counters[CTR_BINFAIL] != 0) {
                    // a query's records outgrew the workgroup's array (or its task queue): the pipeline below answers this call, and the
                    // snapshot's next 32 too
                    __atomic_store_n(&snap->qs_skip, 32u, __ATOMIC_RELAXED);
                    walk = false; attempt = -1;
                    continue;
                }
                walked = true; packed = pack;
                break;
            }
            const uint64_t P = (uint64_t)B * stride;
            if ((rc = grow_pair(ws->d_keys, &ws->cap_keys, (size_t)P + 1))) return rc;
            FPX_HIP(hipMemsetAsync(ws->d_cells, 0, words * sizeof(uint32_t), st));
            // the window's keys, compacted into (hash bucket, query) order -- buckets over the hash bits that, with the window's own,
            // make up the top 8: as wide as on one GPU, the same reach in the tables, and a round's 256 keys still belong to a
            // handful of neighbouring bins.  The count of keys stays on the device (ProbeArgs::P_dev); P is their capacity.
            KeyOrder ko{};
            unsigned long long* d_P = nullptr;
            if ((rc = key_order_setup(ws, B, win_bits, shard_sort_bits(win_bits), &ko, &d_P, st))) return rc;
            static_assert(KO_GROUP == 8, "k_make_keys_window<8> makes the keys of one group per workgroup");
            if (stride <= 512u)
                hipLaunchKernelGGL((k_make_keys_window<8, 512>), dim3((B + 7u) / 8u), dim3(512), 0, st, (const uint32_t*)qb->d_hashes, (const uint64_t*)qb->d_offsets, B, qbits,
                                   ws->d_keys[0], stride, win_lo, win_hi, ws->d_counters, d_overflow, ko);
            else if (stride <= 1024u)       // (a rank of 2: 96 KB of LDS, one workgroup per CU -- still half the time of a workgroup per query)
                hipLaunchKernelGGL((k_make_keys_window<8, 1024>), dim3((B + 7u) / 8u), dim3(512), 0, st, (const uint32_t*)qb->d_hashes, (const uint64_t*)qb->d_offsets, B, qbits,
                                   ws->d_keys[0], stride, win_lo, win_hi, ws->d_counters, d_overflow, ko);
            else
                hipLaunchKernelGGL((k_make_keys_window<1, DEDUP_MAX>), dim3(B), dim3(256), 0, st, (const uint32_t*)qb->d_hashes, (const uint64_t*)qb->d_offsets, B, qbits,
                                   ws->d_keys[0], stride, win_lo, win_hi, ws->d_counters, d_overflow, ko);
            hipLaunchKernelGGL(k_bucket_scan, dim3(ko.nb), dim3(256), 0, st, ko, (B + KO_GROUP - 1u) / KO_GROUP);
            hipLaunchKernelGGL(k_scatter_keys, dim3((B + KO_GROUP - 1u) / KO_GROUP), dim3(256), 0, st, ko, (const uint64_t*)ws->d_keys[0], (const uint64_t*)qb->d_offsets, 0ull, stride, B, qbits,
                               ws->d_keys[1], d_P);
            FPX_HIP(hipGetLastError());
            const int kcur = 1;
            ProbeArgs a;
            a.segs = snap->d_direct; a.pairs = ws->d_keys[kcur]; a.P = P; a.qb = qbits; a.ppw = 16u; a.bsp = 0u;
            a.hits = ws->d_hits[1]; a.hit_cap = ws->cap_hits; a.counters = ws->d_counters;
            a.def_list = nullptr; a.def_count = nullptr; a.def_cap = 0; a.ctr_off = 0; a.cancel = cancel;
            a.lean_stats = reinterpret_cast<unsigned long long*>(d_stats32);
            a.key_skip = KEY_SKIP_FLAGGED; a.P_dev = d_P;
            a.bins = d_send; a.bin_cap = rec_cap; a.bin_count = ws->d_cells; a.bin_shift = SHARD_BQ; a.rec32 = rec32;
            const uint64_t wgs = (P + FK_WG - 1) / FK_WG;
            a.rounds = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(4, wgs / 8192));
            const uint64_t per_wg = (uint64_t)FK_WG * a.rounds;
            FPX_HIP(hipEventRecord(ws->ev_probe0, st));
            for (const GroupDesc& gd : snap->h_group) {
                const GroupArgs gargs{gd, snap->d_direct};
                const dim3 grid((uint32_t)((P + per_wg - 1) / per_wg));
                const Group* grp = snap->groups[&gd - snap->h_group.data()].get();
                launch_probe_group(grp->packed, grp->ns == 8u, true, false, grid, st, a, gargs);
            }
            // the memory segments' table: the window's keys looked up there too, the records into the misc buffer (k_bin bins them)
            if (snap->n_mem && snap->d_memtab)
                hipLaunchKernelGGL(k_probe_memtab, dim3(memtab_grid(P)), dim3(WG), 0, st, (const uint64_t*)snap->d_memtab, (const uint32_t*)snap->d_membucket,
                                   (const uint64_t*)ws->d_keys[kcur], P, qbits, KEY_SKIP_FLAGGED, ws->d_hits[1], (uint64_t)ws->cap_hits, ws->d_counters, (const unsigned long long*)d_P, 0ull, (const uint32_t*)snap->d_membits);
            FPX_HIP(hipEventRecord(ws->ev_probe1, st));
            // what the kernel could not place itself (a clash of two bins on one slot of a round, a full stage): k_bin
            BinArgs hb{};
            hb.bins = d_send; hb.bin_cap = rec_cap; hb.bin_count = ws->d_cells; hb.shift = SHARD_BQ; hb.nbins = std::min<uint32_t>(ncells, MAX_SBINS);
            hb.rec32 = rec32; hb.counters = ws->d_counters;
            if (ncells <= MAX_SBINS)
                hipLaunchKernelGGL(k_bin, dim3(64), dim3(256), 0, st, hb, (const uint64_t*)ws->d_hits[1], (const unsigned long long*)&ws->d_counters[CTR_HITS], (uint64_t)ws->cap_hits);
            else
                hipLaunchKernelGGL(k_bin_each, dim3(64), dim3(256), 0, st, hb, (const uint64_t*)ws->d_hits[1], (const unsigned long long*)&ws->d_counters[CTR_HITS], (uint64_t)ws->cap_hits);
            hipLaunchKernelGGL(k_cell_counts, dim3((ncells + 255) / 256), dim3(256), 0, st, (const unsigned int*)ws->d_cells, ncells, d_send_counts, ws->d_counters,
                               rec32 << 31);
            FPX_HIP(hipGetLastError());
            FPX_HIP(hipMemcpyAsync(ws->h_counters, ws->d_counters, CTR_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            FPX_HIP(hipMemcpyAsync(ws->h_cells, d_stats32, (LEAN_STAT_WORDS + 16) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            FPX_SYNC(ws);
            if (ws->h_cells[LEAN_STAT_WORDS] != 0u && attempt == 0 && stride < max_len) { stride = (uint32_t)max_len; continue; }
            if (ws->h_counters[CTR_BINFAIL] == 3 && attempt < 3) {            // a doc id beyond the segments' declared range: wide records
                __atomic_store_n(&snap->rec32_refused, 1u, __ATOMIC_RELAXED);
                continue;
            }
            if (ws->h_counters[CTR_HITS] > ws->cap_hits) {              // the misc buffer itself was too small
                if (attempt >= 3) { set_error("fpx_shard_probe: misc buffer overflow persists"); return FPX_E_DEVICE; }
                if ((rc = grow_pair(ws->d_hits, &ws->cap_hits, (size_t)ws->h_counters[CTR_HITS] + 1024))) return rc;
                continue;
            }
            break;
        }
        if (ws->h_counters[CTR_TOTAL] > rec_cap) {
            const uint64_t per_cell = rec_cap / std::max<uint64_t>(cell_cap, 1);          // (1 or 2)
            if (needed_cell_cap) *needed_cell_cap = (ws->h_counters[CTR_TOTAL] * 17 / 16 + 128 + per_cell - 1) / std::max<uint64_t>(per_cell, 1);      // (the bins of a batch differ by a few per cent)
            set_error("fpx_shard_probe: a bin holds %llu records, the send buffer has room for %llu per bin", (unsigned long long)ws->h_counters[CTR_TOTAL],
                      (unsigned long long)rec_cap);
            return FPX_E_AGAIN;
        }
        {   // the window's probes join the context's running scan histograms (a step the ranks redo for larger buffers is observed again)
            const unsigned long long* ls = reinterpret_cast<const unsigned long long*>(ws->h_cells);
            uint64_t hist[HIST_SLOTS + 1];
            gather_hist(hist, ws->h_counters, ls, sum_stat_sets(ls).probes);
            ctx_hist_add(snap->ctx, hist, hist[HIST_SLOTS]);
        }
        if (stats) {
            const StatSums s = sum_stat_sets(reinterpret_cast<const unsigned long long*>(ws->h_cells));
            const unsigned long long blocks = s.blocks, docs = s.docs, probes = s.probes, dreads = s.dreads, bytes_off = s.bytes_off;
            const unsigned long long pads = ws->h_counters[CTR_PADS] + s.pads;
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ws->ev_probe0, ws->ev_probe1);
            stats->probes = probes; stats->scanned_blocks = blocks; stats->scanned_docs = docs; stats->hits = ws->h_counters[CTR_SLOTCANDS] - std::min<unsigned long long>(pads, ws->h_counters[CTR_SLOTCANDS]);
            stats->algorithmic_bytes = blocks * 512ull + bytes_off; stats->probe_kernel_bytes = blocks * 512ull + bytes_off;
            stats->probe_kernel_fetched_bytes = dreads * 64ull; stats->probe_kernel_ms = ms; stats->total_gpu_ms = ms; stats->probe_launches = 1;
            stats->path_flags = 1u | 4u | 8u | 16u;
            if (walked) {       // (k_search_window's sets, read the way finish_wg_path reads k_search_query's; bit 14: fpx.h)
                stats->hits = s.records;
                stats->probe_kernel_fetched_bytes = (dreads + 1) / 2 * 128ull;
                stats->path_flags |= 64u | 16384u;
                if (packed) stats->path_flags |= 32768u;      // (bit 15: k_search_packed answered the call)
            }
        }
        return FPX_OK;
    };
    const int rc = body();
    if (rc != FPX_OK) (void)hipStreamSynchronize(ws->stream);
    ws_release(snap->ctx, ws);
    return rc;
}

// ---- the same protocol with the KEYS routed instead of the hashes replicated ----------------------------------------
// fpx_shard_probe wants the whole batch's hashes on every rank: at N ranks every query hash crosses a link N - 1 times and every
// rank reads all of them.  Routed: rank r uploads only ITS share of the batch -- the queries of the bins it will finish --, makes
// their keys (dedupSorted where the keys are made, query numbers of the global batch) and orders them by (hash bucket, query) with
// the counting sort of fpx_keyorder.hpp, whose top buckets ARE the ranks' windows: window w's keys leave for rank w's slot
// [w][key_cap] of the send buffer.  One all-to-all of the slots (+ their counts), and rank w probes the N slots it received -- the
// keys of ITS window from every source, a launch per source.  A query hash crosses one link once (as an 8-byte key), whatever N.
int shard_keys_impl(Ctx* ctx, const QueryBatch* qb, uint32_t world, uint32_t rank, uint32_t B_global,
                    uint64_t* d_keys_send, uint64_t key_cap, unsigned long long* d_key_counts, uint64_t* needed_key_cap)
{
    if (needed_key_cap) *needed_key_cap = 0;
    if (qb->ctx != ctx) { set_error("query batch belongs to a different context"); return FPX_E_INVAL; }
    if (world == 0 || world > KO_MAX_BUCKETS || (world & (world - 1u)) != 0u) { set_error("fpx_shard_keys: the number of ranks must be a power of two <= %u", KO_MAX_BUCKETS); return FPX_E_INVAL; }
    const uint32_t bpr = (uint32_t)shard_bins_per_rank(B_global, world);
    const uint32_t q_lo = std::min<uint64_t>(B_global, (uint64_t)rank * bpr << SHARD_BQ), q_hi = std::min<uint64_t>(B_global, (uint64_t)(rank + 1u) * bpr << SHARD_BQ);
    const uint32_t B = qb->B;
    if (B != q_hi - q_lo) { set_error("fpx_shard_keys: rank %u of %u finishes queries [%u, %u) of the batch of %u: its share must hold exactly those %u (got %u)", rank, world, q_lo, q_hi, B_global, q_hi - q_lo, B); return FPX_E_INVAL; }
    const unsigned qbits = bits_for(B_global);
    if (qbits > 24u) { set_error("fpx_shard_keys: at most 2^24 queries"); return FPX_E_INVAL; }
    FPX_HIP(hipSetDevice(ctx->device));
    if (B == 0) { FPX_HIP(hipMemset(d_key_counts, 0, (size_t)world * sizeof(unsigned long long))); return FPX_OK; }
    const uint64_t* offsets = qb->offsets.data();
    for (uint32_t q = 0; q < B; ++q) {
        const uint64_t len = offsets[q + 1] - offsets[q];
        if (len > DEDUP_MAX) { set_error("fpx_shard_keys: queries of more than %u hashes (use fpx_probe_resident)", DEDUP_MAX); return FPX_E_INVAL; }
        const fpx_opts& o = qb->opts[q];
        if (query_floor(o, len) <= 2u) {
            set_error("fpx_shard_keys: query %u has a score floor of 1 or 2: this batch takes the record protocol (fpx_probe_resident)", q_lo + q); return FPX_E_INVAL;
        }
    }
    Workspace* ws = ws_acquire(ctx);
    if (!ws) return FPX_E_NOMEM;
    auto body = [&]() -> int {
        int rc;
        hipStream_t st = ws->stream;
        const uint64_t P = offsets[B];
        if ((rc = grow_pair(ws->d_keys, &ws->cap_keys, (size_t)P + 1))) return rc;
        KeyOrder ko{};
        if ((rc = key_order_setup(ws, B, 0u, 8u, &ko, nullptr, st, B >= KO_ROWS_MIN_B))) return rc;
        if (ko.nb < world) { set_error("fpx_shard_keys: the batch is too large for %u ranks", world); return FPX_E_INVAL; }
        hipLaunchKernelGGL(k_make_keys_dedup, dim3(B), dim3(256), 0, st, (const uint32_t*)qb->d_hashes, (const uint64_t*)qb->d_offsets, B, qbits, 0ull, ws->d_keys[0],
                           (unsigned long long*)nullptr, (unsigned int*)nullptr, 0u, ko, q_lo);
        if (ko.qrows) hipLaunchKernelGGL(k_group_hist, dim3((B + KO_GROUP - 1u) / KO_GROUP), dim3(256), 0, st, ko, B);
        hipLaunchKernelGGL(k_bucket_scan, dim3(ko.nb), dim3(256), 0, st, ko, (B + KO_GROUP - 1u) / KO_GROUP);
        hipLaunchKernelGGL(k_scatter_keys, dim3((B + KO_GROUP - 1u) / KO_GROUP), dim3(256), 0, st, ko, (const uint64_t*)ws->d_keys[0], (const uint64_t*)qb->d_offsets, 0ull, 0u, B, qbits,
                           d_keys_send, (unsigned long long*)nullptr, ko.nb / world, key_cap, d_key_counts);
        FPX_HIP(hipGetLastError());
        std::vector<unsigned long long> hc(world);
        FPX_HIP(hipMemcpyAsync(hc.data(), d_key_counts, (size_t)world * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        FPX_HIP(hipStreamSynchronize(st));
        unsigned long long worst = 0;
        for (unsigned long long c : hc) worst = std::max(worst, c);
        if (worst > key_cap) {
            if (needed_key_cap) *needed_key_cap = worst * 17 / 16 + 256;
            set_error("fpx_shard_keys: a window takes %llu keys, the send buffer has room for %llu per window", worst, (unsigned long long)key_cap);
            return FPX_E_AGAIN;
        }
        return FPX_OK;
    };
    const int rc = body();
    if (rc != FPX_OK) (void)hipStreamSynchronize(ws->stream);
    ws_release(ctx, ws);
    return rc;
}

// the N key slots a rank received (slot s = the keys of this rank's window from source s, d_key_counts[s] of them) -> the batch's bins
int shard_probe_keys_impl(Snapshot* snap, const uint64_t* d_keys_recv, uint64_t key_cap, const unsigned long long* d_key_counts, uint32_t world, uint32_t B_global,
                          uint32_t timeout_ms, uint64_t* d_send, uint64_t cell_cap, uint32_t* d_send_counts, uint64_t* needed_cell_cap, fpx_stats* stats)
{
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (needed_cell_cap) *needed_cell_cap = 0;
    const uint32_t B = B_global;
    if (B == 0) return FPX_OK;
    if (snap->n_group == 0 || snap->n_solo != 0 || snap->n_file != 0 || (snap->n_mem != 0 && !snap->d_memtab && snap->mem_items != 0)) {
        set_error("fpx_shard_probe_keys: the snapshot is not made of groups of direct-addressed segments (and memory segments behind their table) alone (use fpx_probe_resident)"); return FPX_E_INVAL;
    }
    const unsigned qbits = bits_for(B);
    if (qbits > 24u) { set_error("fpx_shard_probe_keys: at most 2^24 queries"); return FPX_E_INVAL; }
    const uint32_t ncells = (uint32_t)shard_bins_per_rank(B, world) * world;
    if (ncells > (1u << 21)) { set_error("fpx_shard_probe_keys: too many bins"); return FPX_E_INVAL; }
    FPX_HIP(hipSetDevice(snap->ctx->device));
    Workspace* ws = ws_acquire(snap->ctx);
    if (!ws) return FPX_E_NOMEM;
    auto body = [&]() -> int {
        int rc;
        hipStream_t st = ws->stream;
        const double t_start = now_ms();
        __atomic_store_n(ws->h_cancel, 0u, __ATOMIC_RELEASE);
        const uint32_t* cancel = timeout_ms ? ws->d_cancel : nullptr;
        const size_t cell_words = (size_t)ncells * BIN_STRIDE, words = cell_words + LEAN_STAT_WORDS + 16;
        if (words > ws->cap_cells) {
            if (ws->d_cells) (void)hipFree(ws->d_cells);
            if (ws->h_cells) (void)hipHostFree(ws->h_cells);
            ws->d_cells = nullptr; ws->h_cells = nullptr; ws->cap_cells = 0;
            FPX_HIP(dmalloc(&ws->d_cells, words * sizeof(uint32_t)));
            FPX_HIP(hipHostMalloc(reinterpret_cast<void**>(&ws->h_cells), (LEAN_STAT_WORDS + 16) * sizeof(uint32_t)));
            ws->cap_cells = words;
        }
        uint32_t* d_stats32 = ws->d_cells + cell_words;
        if (ws->cap_hits == 0 && (rc = grow_pair(ws->d_hits, &ws->cap_hits, (size_t)1 << 22))) return rc;
        const bool rec32_enabled = ctx_opt(snap->ctx, OPT_REC32) != 0;
        uint64_t rec_cap = cell_cap;
        for (int attempt = 0;; ++attempt) {
            const uint32_t rec32 = rec32_enabled && !__atomic_load_n(&snap->rec32_refused, __ATOMIC_RELAXED) &&
                                   snap->max_doc_declared < (0xFFFFFFFFu >> SHARD_BQ) ? 1u : 0u;
            rec_cap = cell_cap << rec32;
            FPX_HIP(hipMemsetAsync(ws->d_cells, 0, words * sizeof(uint32_t), st));
            FPX_HIP(hipMemsetAsync(ws->d_counters, 0, CTR_COUNT * sizeof(unsigned long long), st));
            ProbeArgs a;
            a.segs = snap->d_direct; a.P = key_cap; a.qb = qbits; a.ppw = 16u; a.bsp = 0u;
            a.hits = ws->d_hits[1]; a.hit_cap = ws->cap_hits; a.counters = ws->d_counters;
            a.def_list = nullptr; a.def_count = nullptr; a.def_cap = 0; a.ctr_off = 0; a.cancel = cancel;
            a.lean_stats = reinterpret_cast<unsigned long long*>(d_stats32);
            a.key_skip = KEY_SKIP_FLAGGED;
            a.bins = d_send; a.bin_cap = rec_cap; a.bin_count = ws->d_cells; a.bin_shift = SHARD_BQ; a.rec32 = rec32;
            const uint64_t wgs = (key_cap + FK_WG - 1) / FK_WG;
            a.rounds = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(4, wgs * world / 8192));
            const uint64_t per_wg = (uint64_t)FK_WG * a.rounds;
            FPX_HIP(hipEventRecord(ws->ev_probe0, st));
            // ONE launch over the N slots (blockIdx.y = the source): every slot's fill level lives on the device
            a.pairs = d_keys_recv; a.slot_stride = key_cap; a.P_dev = d_key_counts;
            for (const GroupDesc& gd : snap->h_group) {
                const GroupArgs gargs{gd, snap->d_direct};
                const dim3 grid((uint32_t)((key_cap + per_wg - 1) / per_wg), world);
                const Group* grp = snap->groups[&gd - snap->h_group.data()].get();
                launch_probe_group(grp->packed, grp->ns == 8u, true, false, grid, st, a, gargs);
            }
            // the memory segments' table (replicated on every rank: a rank only receives the keys of its window)
            if (snap->n_mem && snap->d_memtab)
                hipLaunchKernelGGL(k_probe_memtab, dim3(memtab_grid(key_cap), world), dim3(WG), 0, st, (const uint64_t*)snap->d_memtab, (const uint32_t*)snap->d_membucket,
                                   d_keys_recv, key_cap, qbits, KEY_SKIP_FLAGGED, ws->d_hits[1], (uint64_t)ws->cap_hits, ws->d_counters, d_key_counts, key_cap, (const uint32_t*)snap->d_membits);
            FPX_HIP(hipEventRecord(ws->ev_probe1, st));
            BinArgs hb{};
            hb.bins = d_send; hb.bin_cap = rec_cap; hb.bin_count = ws->d_cells; hb.shift = SHARD_BQ; hb.nbins = std::min<uint32_t>(ncells, MAX_SBINS);
            hb.rec32 = rec32; hb.counters = ws->d_counters;
            if (ncells <= MAX_SBINS)
                hipLaunchKernelGGL(k_bin, dim3(64), dim3(256), 0, st, hb, (const uint64_t*)ws->d_hits[1], (const unsigned long long*)&ws->d_counters[CTR_HITS], (uint64_t)ws->cap_hits);
            else
                hipLaunchKernelGGL(k_bin_each, dim3(64), dim3(256), 0, st, hb, (const uint64_t*)ws->d_hits[1], (const unsigned long long*)&ws->d_counters[CTR_HITS], (uint64_t)ws->cap_hits);
            hipLaunchKernelGGL(k_cell_counts, dim3((ncells + 255) / 256), dim3(256), 0, st, (const unsigned int*)ws->d_cells, ncells, d_send_counts, ws->d_counters,
                               rec32 << 31);
            FPX_HIP(hipGetLastError());
            FPX_HIP(hipMemcpyAsync(ws->h_counters, ws->d_counters, CTR_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            FPX_HIP(hipMemcpyAsync(ws->h_cells, d_stats32, (LEAN_STAT_WORDS + 16) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            FPX_SYNC(ws);
            if (ws->h_counters[CTR_BINFAIL] == 3 && attempt < 3) { __atomic_store_n(&snap->rec32_refused, 1u, __ATOMIC_RELAXED); continue; }
            if (ws->h_counters[CTR_HITS] > ws->cap_hits) {
                if (attempt >= 3) { set_error("fpx_shard_probe_keys: misc buffer overflow persists"); return FPX_E_DEVICE; }
                if ((rc = grow_pair(ws->d_hits, &ws->cap_hits, (size_t)ws->h_counters[CTR_HITS] + 1024))) return rc;
                continue;
            }
            break;
        }
        if (ws->h_counters[CTR_TOTAL] > rec_cap) {
            const uint64_t per_cell = rec_cap / std::max<uint64_t>(cell_cap, 1);
            if (needed_cell_cap) *needed_cell_cap = (ws->h_counters[CTR_TOTAL] * 17 / 16 + 128 + per_cell - 1) / std::max<uint64_t>(per_cell, 1);
            set_error("fpx_shard_probe_keys: a bin holds %llu records, the send buffer has room for %llu per bin", (unsigned long long)ws->h_counters[CTR_TOTAL],
                      (unsigned long long)rec_cap);
            return FPX_E_AGAIN;
        }
        {   // the window's probes join the context's running scan histograms (a step the ranks redo for larger buffers is observed again)
            const unsigned long long* ls = reinterpret_cast<const unsigned long long*>(ws->h_cells);
            uint64_t hist[HIST_SLOTS + 1];
            gather_hist(hist, ws->h_counters, ls, sum_stat_sets(ls).probes);
            ctx_hist_add(snap->ctx, hist, hist[HIST_SLOTS]);
        }
        if (stats) {
            const StatSums s = sum_stat_sets(reinterpret_cast<const unsigned long long*>(ws->h_cells));
            const unsigned long long blocks = s.blocks, docs = s.docs, probes = s.probes, dreads = s.dreads, bytes_off = s.bytes_off;
            const unsigned long long pads = ws->h_counters[CTR_PADS] + s.pads;
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ws->ev_probe0, ws->ev_probe1);
            stats->probes = probes; stats->scanned_blocks = blocks; stats->scanned_docs = docs; stats->hits = ws->h_counters[CTR_SLOTCANDS] - std::min<unsigned long long>(pads, ws->h_counters[CTR_SLOTCANDS]);
            stats->algorithmic_bytes = blocks * 512ull + bytes_off; stats->probe_kernel_bytes = blocks * 512ull + bytes_off;
            stats->probe_kernel_fetched_bytes = dreads * 64ull; stats->probe_kernel_ms = ms; stats->total_gpu_ms = ms; stats->probe_launches = 1;
            stats->path_flags = 1u | 4u | 8u | 16u;
        }
        return FPX_OK;
    };
    const int rc = body();
    if (rc != FPX_OK) (void)hipStreamSynchronize(ws->stream);
    ws_release(snap->ctx, ws);
    return rc;
}

int shard_score_impl(Ctx* ctx, const QueryBatch* qb, uint32_t world, uint32_t rank, const uint64_t* d_recv, uint64_t cell_cap, const uint32_t* d_recv_counts,
                     uint32_t timeout_ms, fpx_result* out, uint32_t out_cap, uint32_t* out_n, uint32_t* first_query, uint32_t* num_queries,
                     uint64_t* needed_cell_cap, uint32_t B_global)
{
    // B_global != 0: `qb` is this rank's SHARE of the batch of B_global queries -- exactly the queries it finishes (fpx_shard_keys)
    if (needed_cell_cap) *needed_cell_cap = 0;
    if (qb->ctx != ctx) { set_error("query batch belongs to a different context"); return FPX_E_INVAL; }
    const uint32_t B = B_global ? B_global : qb->B;
    const uint32_t bpr = (uint32_t)shard_bins_per_rank(B, world);
    const uint32_t q_lo = std::min<uint64_t>(B, (uint64_t)rank * bpr << SHARD_BQ), q_hi = std::min<uint64_t>(B, (uint64_t)(rank + 1u) * bpr << SHARD_BQ);
    if (first_query) *first_query = q_lo;
    if (num_queries) *num_queries = q_hi - q_lo;
    if (B_global && qb->B != q_hi - q_lo) { set_error("fpx_shard_score_share: the share holds %u queries, rank %u of %u finishes %u", qb->B, rank, world, q_hi - q_lo); return FPX_E_INVAL; }
    if (q_hi == q_lo) {
        // A rank that finishes no query of the batch (fewer bins than ranks: B = 1 or 72 at a world of 8) still takes part in the step's
        // exchanges, and a sender whose bins outgrew the step's size marked EVERY count it sent: this rank must see the mark and return
        // FPX_E_AGAIN with the others (they re-enter the collectives of the redo -- fpx.h, fpx_shard_score).
        const size_t ncounts = (size_t)world * bpr;
        if (d_recv_counts && ncounts) {
            FPX_HIP(hipSetDevice(ctx->device));
            std::vector<uint32_t> h(ncounts);
            FPX_HIP(hipMemcpy(h.data(), d_recv_counts, ncounts * sizeof(uint32_t), hipMemcpyDeviceToHost));
            uint64_t need = 0;
            for (uint32_t c : h) if (((uint64_t)c & 0x7FFFFFFFull) >= SHARD_NEED_MARK) need = std::max<uint64_t>(need, (uint64_t)c & (SHARD_NEED_MARK - 1u));
            if (need) {
                if (needed_cell_cap) *needed_cell_cap = need;
                set_error("fpx_shard_score: a sender's bins need %llu cells, the exchange ran with %llu: redo the step", (unsigned long long)need, (unsigned long long)cell_cap);
                return FPX_E_AGAIN;
            }
        }
        return FPX_OK;
    }
    // the options by BATCH query number (the kernels index them so): a share's array starts at the rank's first query
    const uint32_t* d_opts_b = B_global ? qb->d_opts - (size_t)q_lo * 4 : qb->d_opts;
    const uint32_t nq = q_hi - q_lo;
    const unsigned qbits = bits_for(B);
    FPX_HIP(hipSetDevice(ctx->device));
    Workspace* ws = ws_acquire(ctx);
    if (!ws) return FPX_E_NOMEM;
    auto body = [&]() -> int {
        int rc;
        hipStream_t st = ws->stream;
        const double t_start = now_ms();
        __atomic_store_n(ws->h_cancel, 0u, __ATOMIC_RELEASE);
        const uint32_t* cancel = timeout_ms ? ws->d_cancel : nullptr;
        // candidate slots, counts and results are indexed by the batch's query numbers; only [q_lo, q_hi) are this rank's
        if ((rc = ensure_queries(ws, B))) return rc;
        if ((rc = grow(&ws->d_out, &ws->cap_out, (size_t)B * out_cap + 1))) return rc;
        if ((rc = grow(&ws->d_qcand, &ws->cap_qcand, (size_t)B * QCAND_SLOTS + 2 * ((size_t)B / 2 + 1) + bpr))) return rc;
        uint64_t* d_qcand = ws->d_qcand;
        uint32_t* d_qcand_n = reinterpret_cast<uint32_t*>(ws->d_qcand + (size_t)B * QCAND_SLOTS);
        uint32_t* d_bin_n = reinterpret_cast<uint32_t*>(ws->d_qcand + (size_t)B * QCAND_SLOTS + (size_t)B / 2 + 1);
        const size_t cand_guess = std::max<size_t>(1u << 16, (size_t)nq * 64);
        if (ws->cap_cands < cand_guess && (rc = grow_pair(ws->d_cands, &ws->cap_cands, cand_guess))) return rc;
        const uint32_t sbf = 32u - qbits;
        // (k_finish walks the batch's queries from q_lo on: the view's first query is q_lo)
        auto finish = [&](const uint64_t* cands, uint64_t C) {
            hipLaunchKernelGGL(k_finish, dim3((nq + 127) / 128), dim3(128), 0, st, cands, C, (const uint32_t*)d_opts_b, nq, sbf, 0,
                               ws->d_out, out_cap, ws->d_out_n, (const uint64_t*)(d_qcand + (size_t)q_lo * QCAND_SLOTS), (const uint32_t*)(d_qcand_n + q_lo),
                               (unsigned long long*)nullptr, q_lo);
        };
        bool staged = false;
        for (int attempt = 0;; ++attempt) {
        FPX_HIP(hipMemsetAsync(ws->d_counters, 0, CTR_COUNT * sizeof(unsigned long long), st));
        FPX_HIP(hipMemsetAsync(d_qcand_n, 0, (size_t)B * sizeof(uint32_t), st));
        ScoreBinArgs sa{};
        sa.bins = d_recv; sa.bin_cap = cell_cap; sa.rec_mode = 2u; sa.bin_count = d_recv_counts; sa.nsrc = world; sa.src_stride = (uint64_t)bpr * cell_cap;
        sa.count_stride = bpr; sa.count_step = 1u; sa.bq = SHARD_BQ; sa.bin_base = rank * bpr; sa.B = B;
        sa.opts = d_opts_b; sa.sb = sbf; sa.cands = ws->d_cands[0]; sa.cand_cap = ws->cap_cands; sa.counters = ws->d_counters;
        sa.qcand = d_qcand; sa.qcand_n = d_qcand_n; sa.bin_n = d_bin_n; sa.cancel = cancel;
        const size_t sb_lds = ((size_t)8u << SB_TABLE_LOG2) + ((size_t)2u << SB_FILTER_LOG2) + ((size_t)SB_CAND << SHARD_BQ) * 8u;
        const uint32_t my_bins = (nq + (1u << SHARD_BQ) - 1u) >> SHARD_BQ;
        hipLaunchKernelGGL(k_score_bin<false>, dim3(my_bins), dim3(SB_WG), sb_lds, st, sa);
        finish(ws->d_cands[0], 0);
        FPX_HIP(hipGetLastError());
        if ((rc = stage_results(ws, nq, out_cap, st, &staged))) return rc;
        FPX_HIP(hipMemcpyAsync(ws->h_counters, ws->d_counters, CTR_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        FPX_SYNC(ws);
        // A sender whose bins outgrew the agreed cell_cap marks EVERY count it sends with SHARD_NEED_MARK | the cells it needs
        // (HashShardedReader / fpx_sharded_search_batch): every rank receives a piece from every sender, so all of them learn the
        // same maximum from the one exchange and redo the step with it -- no extra collective to agree on a size
        if (ws->h_counters[CTR_BINFAIL] == 2 && (ws->h_counters[CTR_TOTAL] & SHARD_NEED_MARK) != 0) {
            if (needed_cell_cap) *needed_cell_cap = ws->h_counters[CTR_TOTAL] & (SHARD_NEED_MARK - 1u);
            set_error("fpx_shard_score: a sender's bins need %llu cells, the exchange ran with %llu: redo the step", (unsigned long long)(ws->h_counters[CTR_TOTAL] & (SHARD_NEED_MARK - 1u)),
                      (unsigned long long)cell_cap);
            return FPX_E_AGAIN;
        }
        if (ws->h_counters[CTR_CANDS] > ws->cap_cands && attempt < 3) {          // the shared candidate list was too short: again with room
            if ((rc = grow_pair(ws->d_cands, &ws->cap_cands, (size_t)ws->h_counters[CTR_CANDS] + 1024))) return rc;
            continue;
        }
        if (ws->h_counters[CTR_BINFAIL] != 0 || ws->h_counters[CTR_MAXSCORE] != 0 || ws->h_counters[CTR_CANDS] > ws->cap_cands) {
            set_error("fpx_shard_score: a bin could not be scored in place (%s): use smaller batches or the record protocol (fpx_score_partial)",
                      ws->h_counters[CTR_BINFAIL] == 2 ? "a received bin overflowed" : ws->h_counters[CTR_MAXSCORE] ? "a score does not fit the candidate key" : "too many candidates");
            return FPX_E_INVAL;
        }
        break;
        }       // (attempts)
        if (ws->h_counters[CTR_CANDS] != 0) {             // queries with more candidates than slots: sort the shared list, finish again
            const uint64_t Cf = ws->h_counters[CTR_CANDS];
            int ccur = 0;
            if ((rc = sort_keys(ws, ws->d_cands, Cf, 0, 64, st, &ccur))) return rc;
            finish(ws->d_cands[ccur], Cf);
            FPX_HIP(hipGetLastError());
            if ((rc = stage_results(ws, nq, out_cap, st, &staged))) return rc;
            FPX_SYNC(ws);
        }
        return deliver_results(ws, nq, out_cap, staged, out, out_n, st);
    };
    const int rc = body();
    if (rc != FPX_OK) (void)hipStreamSynchronize(ws->stream);
    ws_release(ctx, ws);
    return rc;
}

// ------------------------------------------------------------------------------------------------
// bandwidth probes (denominators for the roofline report)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bw_stream(const uint4* __restrict__ src, size_t n16, unsigned long long* sink)
{
    uint32_t acc = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) {
        uint4 v = src[i];
        acc ^= v.x ^ v.y ^ v.z ^ v.w;
    }
    if (acc == 0x9e3779b9u) atomicAdd(sink, 1ull);
}

// every half-wave reads one random block_size-byte block per step (the access pattern of k_probe)
__global__ __launch_bounds__(256) void k_bw_random(const uint8_t* __restrict__ src, uint64_t nblocks, uint32_t block_size,
                                                   uint32_t steps, unsigned long long* sink)
{
    const uint32_t lane = threadIdx.x & 31u;
    const uint64_t hw = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 5;
    uint32_t acc = 0;
    uint64_t x = hw * 0x9E3779B97F4A7C15ull + 12345;
    for (uint32_t s = 0; s < steps; ++s) {
        x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
        const uint64_t b = x % nblocks;
        for (uint32_t o = lane * 16u; o < block_size; o += 512u) {
            uint4 v = *reinterpret_cast<const uint4*>(src + b * block_size + o);
            acc ^= v.x ^ v.y ^ v.z ^ v.w;
        }
    }
    if (acc == 0x9e3779b9u) atomicAdd(sink, 1ull);
}

// Calibration of the memory-side counters on k_probe_group's OWN access mix (VERDICT r3 #2a): `lanes` threads, each reading
//   MODE 0  one whole 128-byte line, as eight 16-byte loads (a directory line)
//   MODE 1  one 16-byte piece at a 4-byte-aligned address (a hash's words: 3 of 16 alignments straddle a 64-byte sector, 3 of
//           32 a 128-byte line)
//   MODE 2  one aligned 64-byte half line, as four 16-byte loads
//   MODE 3  a line AND two pieces (the kernel's mix)
// at addresses that are a PERMUTATION of the buffer's lines / words (index x odd constant mod a power of two): every line is
// touched once, nothing is served twice from a cache, so the requests the memory side must see are known exactly.
template <int MODE>
__global__ __launch_bounds__(256) void k_bw_pattern(const uint8_t* __restrict__ buf, uint64_t nlines_log2, uint64_t lanes, unsigned long long* sink)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= lanes) return;
    // MODE 3: the lines come from the buffer's lower half, the pieces from its upper half (no line is both)
    const uint64_t nl = MODE == 3 ? nlines_log2 - 1 : nlines_log2;
    const uint64_t lmask = (1ull << nl) - 1ull, wmask = (1ull << (nl + 5)) - 1ull;
    uint32_t acc = 0;
    if (MODE == 0 || MODE == 2 || MODE == 3) {
        const uint8_t* line = buf + ((i * 0x9E3779B97F4A7C15ull) & lmask) * 128ull + (MODE == 2 ? ((i & 1ull) * 64ull) : 0ull);
#pragma unroll
        for (int k = 0; k < (MODE == 2 ? 4 : 8); ++k) { const uint4 v = gload_u4(line + 16 * k); acc ^= v.x ^ v.y ^ v.z ^ v.w; }
    }
    if (MODE == 4) {            // the same 64 lines per wave, read COOPERATIVELY: eight lanes per line, eight lines per instruction
        const uint64_t wave0 = i & ~63ull, sub = i & 7ull, grp = (i & 63ull) >> 3;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint64_t j = wave0 + (uint64_t)k * 8ull + grp;
            const uint4 v = gload_u4(buf + ((j * 0x9E3779B97F4A7C15ull) & lmask) * 128ull + sub * 16ull);
            acc ^= v.x ^ v.y ^ v.z ^ v.w;
        }
    }
    if (MODE == 5) {            // mode 0 with non-temporal loads
        const u32x4_t* line = reinterpret_cast<const u32x4_t*>(buf + ((i * 0x9E3779B97F4A7C15ull) & lmask) * 128ull);
#pragma unroll
        for (int k = 0; k < 8; ++k) { const u32x4_t v = __builtin_nontemporal_load((const FPX_GLOBAL u32x4_t*)(line + k)); acc ^= v.x ^ v.y ^ v.z ^ v.w; }
    }
    if (MODE == 6) {            // mode 0, the first 16 bytes of the line only (what does a line cost when one piece of it is asked for?)
        const uint4 v = gload_u4(buf + ((i * 0x9E3779B97F4A7C15ull) & lmask) * 128ull);
        acc ^= v.x ^ v.y ^ v.z ^ v.w;
    }
    if (MODE == 1 || MODE == 3) {
        const uint32_t* words = reinterpret_cast<const uint32_t*>(buf) + (MODE == 3 ? (wmask + 1ull) : 0ull);
#pragma unroll
        for (int k = 0; k < (MODE == 3 ? 2 : 1); ++k) {
            const uint64_t j = MODE == 3 ? 2ull * i + (uint64_t)k : i;
            const uint64_t w = (j * 0xD1B54A32D192ED03ull) & wmask;           // (a permutation of the words: every alignment equally often)
            const uint4 v = gload_u4_a4(words + w);                            // (the buffer has 64 bytes of slack behind its last word)
            acc ^= v.x ^ v.y ^ v.z ^ v.w;
        }
    }
    if (acc == 0x9e3779b9u) atomicAdd(sink, 1ull);
}

int measure_access_impl(Ctx* ctx, size_t bytes, int mode, uint64_t lanes, double* ms_out)
{
    FPX_HIP(hipSetDevice(ctx->device));
    uint64_t nlines_log2 = 0;
    while ((128ull << (nlines_log2 + 1)) <= bytes) ++nlines_log2;
    if (nlines_log2 < 16 || mode < 0 || mode > 6) { set_error("fpx_measure_access: buffer too small or unknown mode"); return FPX_E_INVAL; }
    if (lanes > (1ull << nlines_log2) / (mode == 3 ? 2 : 1)) { set_error("fpx_measure_access: more lanes than lines"); return FPX_E_INVAL; }
    uint8_t* buf = nullptr; unsigned long long* sk = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto body = [&]() -> int {
        FPX_HIP(dmalloc(&buf, (128ull << nlines_log2) + 64));
        FPX_HIP(dmalloc(&sk, 8));
        FPX_HIP(hipMemset(buf, 0x5a, (128ull << nlines_log2) + 64));
        FPX_HIP(hipMemset(sk, 0, 8));
        FPX_HIP(hipEventCreate(&e0)); FPX_HIP(hipEventCreate(&e1));
        const dim3 grid((uint32_t)((lanes + 255) / 256));
        const uint8_t* b = buf;
        FPX_HIP(hipDeviceSynchronize());
        float ms = 0.f;
        for (int rep = 0; rep < 2; ++rep) {              // (the first launch also loads the kernel)
            FPX_HIP(hipEventRecord(e0, 0));
            switch (mode) {
                case 0: hipLaunchKernelGGL(k_bw_pattern<0>, grid, dim3(256), 0, 0, b, nlines_log2, lanes, sk); break;
                case 1: hipLaunchKernelGGL(k_bw_pattern<1>, grid, dim3(256), 0, 0, b, nlines_log2, lanes, sk); break;
                case 2: hipLaunchKernelGGL(k_bw_pattern<2>, grid, dim3(256), 0, 0, b, nlines_log2, lanes, sk); break;
                case 3: hipLaunchKernelGGL(k_bw_pattern<3>, grid, dim3(256), 0, 0, b, nlines_log2, lanes, sk); break;
                case 4: hipLaunchKernelGGL(k_bw_pattern<4>, grid, dim3(256), 0, 0, b, nlines_log2, lanes, sk); break;
                case 5: hipLaunchKernelGGL(k_bw_pattern<5>, grid, dim3(256), 0, 0, b, nlines_log2, lanes, sk); break;
                default: hipLaunchKernelGGL(k_bw_pattern<6>, grid, dim3(256), 0, 0, b, nlines_log2, lanes, sk); break;
            }
            FPX_HIP(hipGetLastError());
            FPX_HIP(hipEventRecord(e1, 0));
            FPX_HIP(hipEventSynchronize(e1));
            FPX_HIP(hipEventElapsedTime(&ms, e0, e1));
        }
        if (ms_out) *ms_out = ms;
        return FPX_OK;
    };
    const int rc = body();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (buf) (void)hipFree(buf);
    if (sk) (void)hipFree(sk);
    return rc;
}

int measure_bandwidth_impl(Ctx* ctx, size_t bytes, uint32_t block_size, double* stream_gbs, double* random_gbs)
{
    FPX_HIP(hipSetDevice(ctx->device));
    if (block_size < 64 || (block_size & 15u)) { set_error("block_size must be a multiple of 16"); return FPX_E_INVAL; }
    bytes = bytes / 4096 * 4096;
    if (bytes < (1u << 20)) { set_error("buffer too small"); return FPX_E_INVAL; }
    uint8_t* buf = nullptr; unsigned long long* sink = nullptr;
    FPX_HIP(dmalloc(&buf, bytes));
    FPX_HIP(dmalloc(&sink, 8));
    FPX_HIP(hipMemset(buf, 0x5a, bytes));
    FPX_HIP(hipMemset(sink, 0, 8));
    hipEvent_t e0, e1;
    FPX_HIP(hipEventCreate(&e0)); FPX_HIP(hipEventCreate(&e1));
    float ms = 0.f;
    for (int rep = 0; rep < 2; ++rep) {      // first pass warms up
        FPX_HIP(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(k_bw_stream, dim3(256 * 8), dim3(256), 0, 0, (const uint4*)buf, bytes / 16, sink);
        FPX_HIP(hipEventRecord(e1, 0));
        FPX_HIP(hipEventSynchronize(e1));
        FPX_HIP(hipEventElapsedTime(&ms, e0, e1));
    }
    if (stream_gbs) *stream_gbs = (double)bytes / (ms * 1e-3) / 1e9;
    const uint64_t nblocks = bytes / block_size;
    const uint32_t steps = 64;
    const uint32_t grid = 256 * 16;
    const double rbytes = (double)grid * (256 / 32) * steps * block_size;
    for (int rep = 0; rep < 2; ++rep) {
        FPX_HIP(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(k_bw_random, dim3(grid), dim3(256), 0, 0, (const uint8_t*)buf, nblocks, block_size, steps, sink);
        FPX_HIP(hipEventRecord(e1, 0));
        FPX_HIP(hipEventSynchronize(e1));
        FPX_HIP(hipEventElapsedTime(&ms, e0, e1));
    }
    if (random_gbs) *random_gbs = rbytes / (ms * 1e-3) / 1e9;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(buf); (void)hipFree(sink);
    return FPX_OK;
}

}  // namespace fpx
