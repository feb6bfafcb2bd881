// isx_compare_pool.hip -- SNV pooling over a comparison set (`inStrain compare --bams`).
//
// Replaces, for every scaffold of the set at once,
//   PoolController.__init__                 inStrain/polymorpher.py:39-75   (the own rows: not cryptic, highest mm)
//   extract_SNV_positions                   polymorpher.py:318-375          (the sites of a scaffold, what a sample pulls)
//   extract_SNVS_from_bam                   polymorpher.py:275-316          (the pulled counts: every level of the filtered reads)
//   genreate_pooled_SNV_table               polymorpher.py:397-448          (DSTdb)
//   generate_pooled_SNV_summary_table       polymorpher.py:471-551          (PMdb)
// Three passes over the set's word-aligned position space (isx_compare_set.hip):
//   sites    every own row ORs its bit into the site plane; popcounts + one exclusive scan rank the sites, so the sites of a
//            scaffold are a contiguous rank range; the own rows are scattered into counts[sample][rank] / meta[sample][rank]
//   pull     a batch of the sample again: its count table read at the sites, or its entry table walked and added at the ranks; or, for
//            a sample that came from a stored profile, pileup observations of its BAM added at the ranks (k_pull_obs)
//   summary  one thread per site over the samples
// Integers only; the atomics are integer adds and ORs, so a call's bytes do not depend on timing.
#include <algorithm>
#include <cstring>
#include <vector>
#include <rocprim/rocprim.hpp>

#include "isx_compare_set.h"

using namespace isxset;

namespace {

enum : uint8_t { META_HAS = 1, META_OWN = 2 };      // then cls << 2, con_base << 5

struct PullJob {                        // one batch scaffold whose sites the call reads from the count table
    int64_t t0;                         // first thread (ascending; a sentinel entry closes the list)
    int64_t src0, spos0;                // the scaffold's first position in the batch and in the set
    uint32_t rank0, pad;                // its first site
};

__device__ __forceinline__ uint32_t rank_of(const uint64_t *plane, const uint32_t *word_rank, uint32_t gpos)
{
    const uint64_t w = plane[gpos >> 6];
    return word_rank[gpos >> 6] + (uint32_t)__popcll(w & ((1ull << (gpos & 63)) - 1ull));
}

// one thread per own row: the site plane.  Rows on scaffolds that are not pooled, or that the sample does not have, make no site
__global__ void k_pool_mark(const PoolRow *rows, uint32_t n, const int64_t *spos, int n_scaf, const uint8_t *pooled, const uint8_t *has,
                            unsigned long long *plane, int64_t n_words)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = rows[i].gpos;
    const int sc = seg_of(spos, n_scaf, g);
    if ((int64_t)g >= spos[sc + 1] || !pooled[sc] || !has[sc] || (int64_t)(g >> 6) >= n_words) return;
    atomicOr(&plane[g >> 6], 1ull << (g & 63));
}

__global__ void k_pool_popc(const uint64_t *plane, int64_t n_words, uint32_t *pop)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w <= n_words) pop[w] = w < n_words ? (uint32_t)__popcll(plane[w]) : 0u;       // [n_words]: the scan's total lands there
}

// the sorted site list: a thread writes the positions of its word at the word's rank
__global__ void k_pool_expand(const uint64_t *plane, const uint32_t *word_rank, int64_t n_words, uint32_t *site_gpos, uint32_t n_sites)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    uint64_t bits = plane[w];
    uint32_t r = word_rank[w];
    while (bits && r < n_sites) {
        const int b = __ffsll((unsigned long long)bits) - 1;
        site_gpos[r++] = (uint32_t)(w * 64 + b);
        bits &= bits - 1;
    }
}

__global__ void k_scaffold_ranks(const uint32_t *word_rank, const int64_t *woff, int n_scaf, uint32_t *srank)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n_scaf) srank[i] = word_rank[woff[i]];
}

// meta[sample][site] = the sample has the site's scaffold
__global__ void k_pool_meta(const uint32_t *site_gpos, uint32_t n_sites, const int64_t *spos, int n_scaf, const uint8_t *has, int n_samples,
                            uint8_t *meta)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_sites) return;
    const int sc = seg_of(spos, n_scaf, site_gpos[r]);
    for (int s = 0; s < n_samples; s++) meta[(size_t)s * n_sites + r] = has[(size_t)s * n_scaf + sc] ? META_HAS : 0;
}

// one thread per own row of ONE sample: its counts, class and con_base at the site's rank; own[scaffold] counts the sample's own sites
__global__ void k_pool_scatter(const PoolRow *rows, uint32_t n, const int64_t *spos, int n_scaf, const uint8_t *pooled, const uint8_t *has,
                               const uint64_t *plane, const uint32_t *word_rank, int64_t n_words, uint32_t n_sites, uint4 *counts,
                               uint8_t *meta, uint8_t *site_ref, uint32_t *own)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PoolRow x = rows[i];
    const int sc = seg_of(spos, n_scaf, x.gpos);
    if ((int64_t)x.gpos >= spos[sc + 1] || !pooled[sc] || !has[sc] || (int64_t)(x.gpos >> 6) >= n_words) return;
    const uint32_t r = rank_of(plane, word_rank, x.gpos);
    if (r >= n_sites) return;
    counts[r] = make_uint4(x.cnt[0], x.cnt[1], x.cnt[2], x.cnt[3]);
    meta[r] = (uint8_t)(META_HAS | META_OWN | ((x.cls & 7) << 2) | ((x.con_base & 3) << 5));
    site_ref[r] = x.ref_base;           // (every sample's rows of a site name the same reference base)
    atomicAdd(&own[sc], 1u);
}

// pull, count-table path: one thread per site of the call's scaffolds
__global__ void k_pull_counts(const PullJob *jobs, int n_jobs, int64_t n_threads, const uint4 *table, uint32_t n_pos, const uint32_t *site_gpos,
                              uint32_t n_sites, const uint8_t *meta, uint4 *counts)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_threads) return;
    int lo = 0, hi = n_jobs;            // jobs[lo].t0 <= t < jobs[hi].t0
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (jobs[mid].t0 <= t) lo = mid; else hi = mid;
    }
    const PullJob j = jobs[lo];
    const uint64_t r = (uint64_t)j.rank0 + (uint64_t)(t - j.t0);
    if (r >= n_sites || (meta[r] & META_OWN)) return;
    const int64_t src = j.src0 + ((int64_t)site_gpos[r] - j.spos0);
    if (src < 0 || src >= (int64_t)n_pos) return;
    counts[r] = table[src];
}

// pull, entry path: one thread per entry slot (window slabs + overflow, or the flat table: SummaryIn); every level of a site adds up
__global__ void k_pull_entries(const isx_entry *entries, const uint32_t *win_nent, uint32_t slab, uint64_t ovf0, uint32_t n_ovf,
                               const int64_t *bbounds, int n_bscaf, const int64_t *set_pos0, const uint64_t *plane,
                               const uint32_t *word_rank, int64_t n_words, uint32_t n_sites, const uint8_t *meta, uint4 *counts)
{
    const uint64_t total = ovf0 + n_ovf;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        if (i < ovf0) {
            const uint32_t w = (uint32_t)(i / slab);
            if ((uint32_t)(i - (uint64_t)w * slab) >= win_nent[w]) continue;
        }
        const isx_entry e = entries[i];
        const int64_t g = e.gpos;
        const int sc = seg_of(bbounds, n_bscaf, g);
        const int64_t p0 = set_pos0[sc];
        if (p0 < 0 || g < bbounds[sc] || g >= bbounds[sc + 1]) continue;
        const uint32_t sp = (uint32_t)(p0 + (g - bbounds[sc]));
        if ((int64_t)(sp >> 6) >= n_words || !(plane[sp >> 6] >> (sp & 63) & 1ull)) continue;
        const uint32_t r = rank_of(plane, word_rank, sp);
        if (r >= n_sites || (meta[r] & META_OWN)) continue;
        uint32_t *c = reinterpret_cast<uint32_t *>(&counts[r]);
        for (int k = 0; k < 4; k++)
            if (e.cnt[k]) atomicAdd(&c[k], e.cnt[k]);
    }
}

// pull, observation path (isx_cmpset_pool_add_obs): one lane per pileup observation, grid-stride.  The region of an observation is found
// in the call's offsets (roff[lo] <= i < roff[lo + 1]; empty regions share an offset and the search lands behind them); rbase[region] is
// the set position of the region's gpos 0, OBS_SKIP for a region the call leaves out.  Observations come column by column, so the
// lanes of a wave mostly hit one (site, base) word: every run of equal (rank, base) keys in the wave -- found by comparing with the
// lane below, the run heads collected by ballot -- makes ONE atomic add of the run's length.  Any order of observations is correct (a
// run is whatever happens to be adjacent); -DISX_PULL_OBS_PLAIN builds the variant with one atomic per observation for the A/B.
constexpr int64_t OBS_SKIP = INT64_MIN;
constexpr int PULL_OBS_BLOCK = 256, PULL_OBS_MAX_BLOCKS = 2048;

__global__ void __launch_bounds__(PULL_OBS_BLOCK) k_pull_obs(const isx_obs *obs, int64_t n_obs, const int64_t *roff, const int64_t *rbase,
                                                             int n_regions, const uint64_t *plane, const uint32_t *word_rank, int64_t n_words,
                                                             uint32_t n_sites, const uint8_t *meta, uint32_t *counts)
{
    constexpr unsigned long long NONE = ~0ull;
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); i0 < n_obs; i0 += stride) {       // (wave-uniform)
        const int64_t i = i0 + lane;
        unsigned long long key = NONE;                  // rank * 4 + base of the word this observation counts in
        if (i < n_obs) {
            const isx_obs o = obs[i];
            int lo = 0, hi = n_regions;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (roff[mid] <= i) lo = mid; else hi = mid;
            }
            const int64_t p0 = rbase[lo];
            const int64_t sp = p0 + (int64_t)o.gpos;
            if (o.base < 4 && p0 != OBS_SKIP && sp >= 0 && (sp >> 6) < n_words && (plane[sp >> 6] >> (sp & 63) & 1ull)) {
                const uint32_t r = rank_of(plane, word_rank, (uint32_t)sp);
                if (r < n_sites && !(meta[r] & META_OWN)) key = (unsigned long long)r * 4 + o.base;
            }
        }
#ifdef ISX_PULL_OBS_PLAIN
        if (key != NONE) atomicAdd(&counts[key], 1u);
#else
        const unsigned long long below = __shfl_up(key, 1);
        const bool head = lane == 0 || below != key;
        const unsigned long long heads = __ballot(head);
        if (head && key != NONE) {
            const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);          // the next head ends the run
            atomicAdd(&counts[key], (uint32_t)(above ? __ffsll(above) : 64 - lane));
        }
#endif
    }
}

// PMdb: one thread per site, the samples in insertion order; the columns are [sample][site], so a wave reads runs of both
__global__ void __launch_bounds__(256) k_pool_summary(const uint32_t *site_gpos, const uint8_t *site_ref, const uint4 *counts, const uint8_t *meta,
                                                      uint32_t n_sites, int n_samples, isx_pool_site *out)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_sites) return;
    isx_pool_site o;
    memset(&o, 0, sizeof(o));
    o.gpos = site_gpos[r];
    o.ref_base = site_ref[r];
    uint32_t seen = 0;
    for (int s = 0; s < n_samples; s++) {
        const uint8_t m = meta[(size_t)s * n_sites + r];
        if (!(m & META_HAS)) continue;
        const uint4 c = counts[(size_t)s * n_sites + r];
        o.cnt[0] += c.x; o.cnt[1] += c.y; o.cnt[2] += c.z; o.cnt[3] += c.w;
        if (c.x | c.y | c.z | c.w) o.n_detect++;
        if ((uint64_t)c.x + c.y + c.z + c.w >= 5) o.n_detect_5x++;
        if (!(m & META_OWN)) continue;
        const uint32_t cls = (m >> 2) & 7, con = (m >> 5) & 3;
        if (cls >= 1 && cls <= 5) o.cls_count[cls - 1]++;
        if (!(seen >> con & 1u)) {
            seen |= 1u << con;
            o.con_bases |= (uint8_t)(con << (2 * o.n_con_bases));
            o.n_con_bases++;
        }
    }
    int con = 0;
    for (int k = 1; k < 4; k++) if (o.cnt[k] > o.cnt[con]) con = k;
    uint64_t rest[4] = {o.cnt[0], o.cnt[1], o.cnt[2], o.cnt[3]};
    rest[con] = 0;
    int var = 0;                        // the first index that holds the maximum: 'A' when nothing else was seen, also when con is 'A'
    for (int k = 1; k < 4; k++) if (rest[k] > rest[var]) var = k;
    o.con_base = (uint8_t)con; o.var_base = (uint8_t)var;
    out[r] = o;
}

bool sample_has(const Sample &sm, int32_t sc)
{
    if (sm.mm.empty() || !sm.have[(size_t)sc]) return false;
    const size_t L = sm.mm.size();
    for (size_t k = 0; k < L; k++) if (sm.present[(size_t)sc * L + k]) return true;
    return false;
}

}  // namespace

namespace isxset {

void cmpset_pool_drop(isx_cmpset *st)
{
    st->site_plane.drop(); st->word_rank.drop(); st->word_pop.drop(); st->site_gpos.drop(); st->site_ref.drop(); st->p_counts.drop();
    st->p_meta.drop(); st->d_phas.drop(); st->d_ppooled.drop(); st->d_pspos.drop(); st->d_pwoff.drop(); st->d_srank.drop(); st->d_own.drop();
    st->d_psum.drop();
    st->pooled = false; st->n_sites = 0;
}

}  // namespace isxset

#define POOL_ON(st, who)                                                                                                   \
    do {                                                                                                                   \
        if (!(st)) { isx_set_error(std::string(who) + ": bad argument"); return ISX_ERR_ARG; }                            \
        if (!(st)->pool_on) { isx_set_error(std::string(who) + ": the set keeps no pool rows (isx_cmpset_pool_enable before the first add)"); return ISX_ERR_STATE; } \
    } while (0)
#define POOL_SITES(st, who)                                                                                                \
    do {                                                                                                                   \
        POOL_ON(st, who);                                                                                                  \
        if (!(st)->pooled) { isx_set_error(std::string(who) + ": call isx_cmpset_pool_sites first (and again after an add)"); return ISX_ERR_STATE; } \
    } while (0)

extern "C" {

int isx_cmpset_pool_enable(isx_cmpset *st)
{
    if (!st) { isx_set_error("isx_cmpset_pool_enable: bad argument"); return ISX_ERR_ARG; }
    if (!st->samples.empty()) { isx_set_error("isx_cmpset_pool_enable: call it before the first isx_cmpset_add"); return ISX_ERR_STATE; }
    st->pool_on = true;
    return ISX_OK;
}

int isx_cmpset_pool_sites(isx_cmpset *st, int64_t *n_sites)
{
    POOL_ON(st, "isx_cmpset_pool_sites");
    if (!n_sites) { isx_set_error("isx_cmpset_pool_sites: bad argument"); return ISX_ERR_ARG; }
    *n_sites = 0;
    st->pooled = false;
    const int32_t S = (int32_t)st->samples.size(), n_scaf = st->n_scaf;
    const int64_t n_words = st->n_words;
    // membership (host): which sample has which scaffold, which scaffolds are pooled
    st->p_has.assign((size_t)std::max(S, 1) * n_scaf, 0);
    st->p_pooled.assign((size_t)n_scaf, 0);
    for (int32_t sc = 0; sc < n_scaf; sc++) {
        int n = 0;
        for (int32_t i = 0; i < S; i++)
            if (sample_has(st->samples[(size_t)i], sc)) { st->p_has[(size_t)i * n_scaf + sc] = 1; n++; }
        st->p_pooled[(size_t)sc] = n >= 2;
    }
    HIP_TRY(hipSetDevice(st->ctx->device));
    hipStream_t s = st->ctx->stream;
    for (Sample &sm : st->samples) {
        const int rc = cmpset_sort_pool_rows(st, sm);
        if (rc) return rc;
    }
    HIP_TRY(st->d_phas.put(st->p_has, s)); HIP_TRY(st->d_ppooled.put(st->p_pooled, s));
    HIP_TRY(st->d_pspos.put(st->spos, s)); HIP_TRY(st->d_pwoff.put(st->woff, s));
    HIP_TRY(st->site_plane.fit((size_t)n_words)); HIP_TRY(st->word_pop.fit((size_t)n_words + 1)); HIP_TRY(st->word_rank.fit((size_t)n_words + 1));
    HIP_TRY(st->d_srank.fit((size_t)n_scaf + 1)); HIP_TRY(st->d_own.fit((size_t)std::max(S, 1) * n_scaf));
    size_t t_scan = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, t_scan, st->word_pop.p, st->word_rank.p, 0u, (size_t)n_words + 1, rocprim::plus<uint32_t>(), s));
    int rc = cmpset_grow_temp(st, t_scan);
    if (rc) return rc;
    const dim3 blk(256);
    const dim3 wgrid((unsigned)((n_words + 1 + 255) / 256));
    // 1. the site plane
    HIP_TRY(hipMemsetAsync(st->site_plane.p, 0, (size_t)n_words * 8, s));
    for (int32_t i = 0; i < S; i++) {
        const Sample &sm = st->samples[(size_t)i];
        if (!sm.n_prows) continue;
        hipLaunchKernelGGL(k_pool_mark, dim3((unsigned)((sm.n_prows + 255) / 256)), blk, 0, s, sm.prows, (uint32_t)sm.n_prows, st->d_pspos.p,
                           n_scaf, st->d_ppooled.p, st->d_phas.p + (size_t)i * n_scaf, reinterpret_cast<unsigned long long *>(st->site_plane.p),
                           n_words);
    }
    // 2. ranks: sites before every word; the last element is the number of sites
    hipLaunchKernelGGL(k_pool_popc, wgrid, blk, 0, s, st->site_plane.p, n_words, st->word_pop.p);
    size_t tb = st->temp.cap;
    HIP_TRY(rocprim::exclusive_scan(st->temp.p, tb, st->word_pop.p, st->word_rank.p, 0u, (size_t)n_words + 1, rocprim::plus<uint32_t>(), s));
    hipLaunchKernelGGL(k_scaffold_ranks, dim3((unsigned)((n_scaf + 1 + 255) / 256)), blk, 0, s, st->word_rank.p, st->d_pwoff.p, n_scaf, st->d_srank.p);
    st->p_srank.assign((size_t)n_scaf + 1, 0);
    HIP_TRY(hipMemcpyAsync(st->p_srank.data(), st->d_srank.p, ((size_t)n_scaf + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(isx_wait_stream(s));
    HIP_TRY(hipGetLastError());
    const uint32_t n = st->p_srank[(size_t)n_scaf];
    // 3. the site list, the samples' columns, the own rows in them
    HIP_TRY(st->site_gpos.fit(n)); HIP_TRY(st->site_ref.fit(n));
    HIP_TRY(st->p_counts.fit((size_t)std::max(S, 1) * n)); HIP_TRY(st->p_meta.fit((size_t)std::max(S, 1) * n));
    HIP_TRY(hipMemsetAsync(st->d_own.p, 0, (size_t)std::max(S, 1) * n_scaf * 4, s));
    std::vector<uint32_t> own((size_t)std::max(S, 1) * n_scaf, 0);
    if (n) {
        HIP_TRY(hipMemsetAsync(st->p_counts.p, 0, (size_t)S * n * sizeof(uint4), s));
        HIP_TRY(hipMemsetAsync(st->site_ref.p, 4, n, s));
        hipLaunchKernelGGL(k_pool_expand, wgrid, blk, 0, s, st->site_plane.p, st->word_rank.p, n_words, st->site_gpos.p, n);
        hipLaunchKernelGGL(k_pool_meta, dim3((n + 255) / 256), blk, 0, s, st->site_gpos.p, n, st->d_pspos.p, n_scaf, st->d_phas.p, S, st->p_meta.p);
        for (int32_t i = 0; i < S; i++) {
            const Sample &sm = st->samples[(size_t)i];
            if (!sm.n_prows) continue;
            hipLaunchKernelGGL(k_pool_scatter, dim3((unsigned)((sm.n_prows + 255) / 256)), blk, 0, s, sm.prows, (uint32_t)sm.n_prows,
                               st->d_pspos.p, n_scaf, st->d_ppooled.p, st->d_phas.p + (size_t)i * n_scaf, st->site_plane.p, st->word_rank.p,
                               n_words, n, st->p_counts.p + (size_t)i * n, st->p_meta.p + (size_t)i * n, st->site_ref.p,
                               st->d_own.p + (size_t)i * n_scaf);
        }
        HIP_TRY(hipMemcpyAsync(own.data(), st->d_own.p, own.size() * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(isx_wait_stream(s));
        HIP_TRY(hipGetLastError());
    }
    // 4. what every (sample, scaffold) still has to pull
    for (int32_t i = 0; i < S; i++) {
        Sample &sm = st->samples[(size_t)i];
        sm.pulled.assign((size_t)n_scaf, 0);
        sm.to_pull.assign((size_t)n_scaf, 0);
        for (int32_t sc = 0; sc < n_scaf; sc++)
            if (st->p_has[(size_t)i * n_scaf + sc] && st->p_pooled[(size_t)sc])
                sm.to_pull[(size_t)sc] = (int64_t)(st->p_srank[(size_t)sc + 1] - st->p_srank[(size_t)sc]) - own[(size_t)i * n_scaf + sc];
    }
    st->n_sites = n;
    st->pooled = true;
    *n_sites = n;
    return ISX_OK;
}

int isx_cmpset_pool_fetch_sites(isx_cmpset *st, uint32_t *gpos)
{
    POOL_SITES(st, "isx_cmpset_pool_fetch_sites");
    if (!st->n_sites) return ISX_OK;
    if (!gpos) { isx_set_error("isx_cmpset_pool_fetch_sites: bad argument"); return ISX_ERR_ARG; }
    HIP_TRY(hipSetDevice(st->ctx->device));
    HIP_TRY(isx_wait_stream(st->ctx->stream));
    HIP_TRY(hipMemcpy(gpos, st->site_gpos.p, (size_t)st->n_sites * 4, hipMemcpyDeviceToHost));
    return ISX_OK;
}

int isx_cmpset_pool_add(isx_cmpset *st, int32_t sample, isx_batch *b, int32_t n_bscaf, const int64_t *bb, const int32_t *ids)
{
    const int rc_args = cmpset_check_batch("isx_cmpset_pool_add", st, sample, b, n_bscaf, bb, ids);
    if (rc_args) return rc_args;
    POOL_SITES(st, "isx_cmpset_pool_add");
    if ((size_t)sample >= st->samples.size() || st->samples[(size_t)sample].mm.empty()) {
        isx_set_error("isx_cmpset_pool_add: sample " + std::to_string(sample) + " was never added");
        return ISX_ERR_ARG;
    }
    Sample &sm = st->samples[(size_t)sample];
    const bool by_table = b->M == 1;
    if (by_table ? !b->d_counts : (b->lean || !b->d_entries)) {
        isx_set_error(by_table ? "isx_cmpset_pool_add: this pipe slot keeps no per-base count table: create the pipe with want_counts (isx_pipe_params.want_counts)"
                               : "isx_cmpset_pool_add: a lean pipe slot (isx_pipe_params.lean_output) keeps no level table to pull counts from; with one mm bin create the pipe with want_counts");
        return ISX_ERR_STATE;
    }
    const int32_t n_scaf = st->n_scaf;
    std::vector<uint8_t> seen((size_t)n_scaf, 0);
    std::vector<int64_t> set_pos0((size_t)n_bscaf, -1);
    std::vector<PullJob> jobs;
    std::vector<int32_t> taken;
    int64_t t = 0;
    for (int i = 0; i < n_bscaf; i++) {
        const int32_t sid = ids[i];
        if (sid == -1) continue;
        if (sid < 0 || sid >= n_scaf) { isx_set_error("isx_cmpset_pool_add: set_scaffold_ids[" + std::to_string(i) + "] outside the set"); return ISX_ERR_ARG; }
        if (bb[i + 1] - bb[i] != st->len[(size_t)sid]) {
            isx_set_error("isx_cmpset_pool_add: batch scaffold " + std::to_string(i) + " has not the length of set scaffold " + std::to_string(sid));
            return ISX_ERR_ARG;
        }
        if (!st->p_has[(size_t)sample * n_scaf + sid] || !st->p_pooled[(size_t)sid]) continue;
        if (seen[(size_t)sid] || sm.pulled[(size_t)sid]) {
            isx_set_error("isx_cmpset_pool_add: scaffold " + std::to_string(sid) + " of sample " + std::to_string(sample) +
                          (sm.pulled[(size_t)sid] == PULL_OBS ? " has observations of isx_cmpset_pool_add_obs under way" : " was pulled before"));
            return ISX_ERR_STATE;
        }
        seen[(size_t)sid] = 1;
        taken.push_back(sid);
        const uint32_t r0 = st->p_srank[(size_t)sid], r1 = st->p_srank[(size_t)sid + 1];
        set_pos0[(size_t)i] = st->spos[(size_t)sid];
        if (r1 > r0) {
            jobs.push_back({t, bb[i], st->spos[(size_t)sid], r0, 0});
            t += r1 - r0;
        }
    }
    const uint32_t n = (uint32_t)st->n_sites;
    if (!jobs.empty()) {
        const int n_jobs = (int)jobs.size();
        jobs.push_back({t, 0, 0, 0, 0});
        HIP_TRY(hipSetDevice(st->ctx->device));
        hipStream_t s = st->ctx->stream;
        uint4 *counts = st->p_counts.p + (size_t)sample * n;
        const uint8_t *meta = st->p_meta.p + (size_t)sample * n;
        SetBuf<PullJob> d_jobs;
        auto done = [&](int r) { d_jobs.drop(); return r; };
#define PA_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { isx_set_error(std::string("isx_cmpset_pool_add: ") + #expr + ": " + hipGetErrorString(_e)); isx_read_drop(); return done(ISX_ERR_HIP); } } while (0)
        if (by_table) {
            PA_TRY(d_jobs.put(jobs, s));
            hipLaunchKernelGGL(k_pull_counts, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, s, d_jobs.p, n_jobs, t, b->d_counts,
                               (uint32_t)b->n_pos, st->site_gpos.p, n, meta, counts);
        } else {
            const std::vector<int64_t> h_bounds(bb, bb + n_bscaf + 1);
            PA_TRY(st->bbounds.put(h_bounds, s));
            PA_TRY(st->set_pos0.put(set_pos0, s));
            SummaryIn in{};
            fill_summary_in(b, n_bscaf, bb, in);
            if (in.ovf0 + in.n_ovf)
                hipLaunchKernelGGL(k_pull_entries, dim3(2048), dim3(256), 0, s, in.entries, in.win_nent, in.slab, in.ovf0, in.n_ovf, st->bbounds.p,
                                   n_bscaf, st->set_pos0.p, st->site_plane.p, st->word_rank.p, st->n_words, n, meta, counts);
        }
        PA_TRY(isx_wait_stream(s));
        PA_TRY(hipGetLastError());
#undef PA_TRY
        d_jobs.drop();
    }
    for (int32_t sid : taken) sm.pulled[(size_t)sid] = PULL_DONE;
    return ISX_OK;
}

int isx_cmpset_pool_add_obs(isx_cmpset *st, int32_t sample, int32_t n_regions, const int32_t *ids, const int64_t *gpos0, const int64_t *off,
                            int64_t n_obs, const isx_obs *obs, float *device_ms)
{
    const std::string who("isx_cmpset_pool_add_obs: ");
    if (device_ms) *device_ms = 0.f;
    POOL_SITES(st, "isx_cmpset_pool_add_obs");
    if (sample < 0 || n_regions < 0 || n_regions > (1 << 24) || n_obs < 0 || !off || (n_regions && (!ids || !gpos0)) || (n_obs && !obs)) {
        isx_set_error(who + "bad argument");
        return ISX_ERR_ARG;
    }
    if ((size_t)sample >= st->samples.size() || st->samples[(size_t)sample].mm.empty()) {
        isx_set_error(who + "sample " + std::to_string(sample) + " was never added");
        return ISX_ERR_ARG;
    }
    Sample &sm = st->samples[(size_t)sample];
    const int32_t n_scaf = st->n_scaf;
    if (off[0] != 0 || off[n_regions] != n_obs) { isx_set_error(who + "obs_offsets must start at 0 and end at n_obs"); return ISX_ERR_ARG; }
    for (int i = 0; i < n_regions; i++)
        if (off[i + 1] < off[i]) { isx_set_error(who + "obs_offsets must not descend"); return ISX_ERR_ARG; }
    std::vector<int64_t> rbase((size_t)n_regions, OBS_SKIP);
    std::vector<int32_t> taken;
    for (int i = 0; i < n_regions; i++) {
        const int32_t sid = ids[i];
        if (sid < -1 || sid >= n_scaf) { isx_set_error(who + "set_scaffold_ids[" + std::to_string(i) + "] outside the set"); return ISX_ERR_ARG; }
        const int64_t len = sid < 0 ? 0 : st->len[(size_t)sid];
        for (int64_t k = off[i]; k < off[i + 1]; k++) {
            const int64_t p = (int64_t)obs[k].gpos - gpos0[i];
            if (obs[k].base > 4 || (sid >= 0 && (p < 0 || p >= len))) {
                isx_set_error(who + "observation " + std::to_string(k) + " of region " + std::to_string(i) +
                              (obs[k].base > 4 ? ": base code above 4" : ": position outside the scaffold"));
                return ISX_ERR_ARG;
            }
        }
        if (sid < 0 || !st->p_has[(size_t)sample * n_scaf + sid] || !st->p_pooled[(size_t)sid]) continue;
        if (sm.pulled[(size_t)sid] == PULL_DONE) {
            isx_set_error(who + "scaffold " + std::to_string(sid) + " of sample " + std::to_string(sample) + " was pulled before");
            return ISX_ERR_STATE;
        }
        rbase[(size_t)i] = st->spos[(size_t)sid] - gpos0[i];
        taken.push_back(sid);
    }
    const uint32_t n = (uint32_t)st->n_sites;
    if (n_obs && n && !taken.empty()) {
        HIP_TRY(hipSetDevice(st->ctx->device));
        hipStream_t s = st->ctx->stream;
        const std::vector<int64_t> h_off(off, off + n_regions + 1);
        HIP_TRY(st->obs_stage.fit((size_t)n_obs));
        HIP_TRY(st->obs_roff.put(h_off, s)); HIP_TRY(st->obs_rbase.put(rbase, s));
        HIP_TRY(hipMemcpyAsync(st->obs_stage.p, obs, (size_t)n_obs * sizeof(isx_obs), hipMemcpyHostToDevice, s));
        const unsigned blocks = (unsigned)std::min<int64_t>((n_obs + PULL_OBS_BLOCK - 1) / PULL_OBS_BLOCK, PULL_OBS_MAX_BLOCKS);
        HIP_TRY(hipEventRecord(st->ev[0], s));
        hipLaunchKernelGGL(k_pull_obs, dim3(blocks), dim3(PULL_OBS_BLOCK), 0, s, st->obs_stage.p, n_obs, st->obs_roff.p, st->obs_rbase.p, n_regions,
                           st->site_plane.p, st->word_rank.p, st->n_words, n, st->p_meta.p + (size_t)sample * n,
                           reinterpret_cast<uint32_t *>(st->p_counts.p + (size_t)sample * n));
        HIP_TRY(hipEventRecord(st->ev[1], s));
        HIP_TRY(isx_wait_stream(s));
        HIP_TRY(hipGetLastError());
        if (device_ms) (void)hipEventElapsedTime(device_ms, st->ev[0], st->ev[1]);
    }
    for (int32_t sid : taken) sm.pulled[(size_t)sid] = PULL_OBS;
    return ISX_OK;
}

int isx_cmpset_pool_obs_done(isx_cmpset *st, int32_t sample, int32_t n_ids, const int32_t *ids)
{
    const std::string who("isx_cmpset_pool_obs_done: ");
    POOL_SITES(st, "isx_cmpset_pool_obs_done");
    if (sample < 0 || n_ids < 0 || (n_ids && !ids)) { isx_set_error(who + "bad argument"); return ISX_ERR_ARG; }
    if ((size_t)sample >= st->samples.size() || st->samples[(size_t)sample].mm.empty()) {
        isx_set_error(who + "sample " + std::to_string(sample) + " was never added");
        return ISX_ERR_ARG;
    }
    Sample &sm = st->samples[(size_t)sample];
    const int32_t n_scaf = st->n_scaf;
    std::vector<uint8_t> seen((size_t)n_scaf, 0);
    std::vector<int32_t> taken;
    for (int i = 0; i < n_ids; i++) {
        const int32_t sid = ids[i];
        if (sid < -1 || sid >= n_scaf) { isx_set_error(who + "set_scaffold_ids[" + std::to_string(i) + "] outside the set"); return ISX_ERR_ARG; }
        if (sid < 0 || !st->p_has[(size_t)sample * n_scaf + sid] || !st->p_pooled[(size_t)sid]) continue;
        if (seen[(size_t)sid] || sm.pulled[(size_t)sid] == PULL_DONE) {
            isx_set_error(who + "scaffold " + std::to_string(sid) + " of sample " + std::to_string(sample) + " was pulled before");
            return ISX_ERR_STATE;
        }
        seen[(size_t)sid] = 1;
        taken.push_back(sid);
    }
    for (int32_t sid : taken) sm.pulled[(size_t)sid] = PULL_DONE;      // (a scaffold without any observation: its counts are the zeros of pool_sites)
    return ISX_OK;
}

int isx_cmpset_pool_summary(isx_cmpset *st, int64_t cap_sites, isx_pool_site *out, float *device_ms)
{
    POOL_SITES(st, "isx_cmpset_pool_summary");
    if (cap_sites < st->n_sites || (!out && st->n_sites)) { isx_set_error("isx_cmpset_pool_summary: out holds fewer rows than the set has sites"); return ISX_ERR_ARG; }
    if (device_ms) *device_ms = 0.f;
    const int32_t S = (int32_t)st->samples.size();
    for (int32_t i = 0; i < S; i++)
        for (int32_t sc = 0; sc < st->n_scaf; sc++)
            if (st->samples[(size_t)i].to_pull[(size_t)sc] > 0 && st->samples[(size_t)i].pulled[(size_t)sc] != PULL_DONE) {
                isx_set_error("isx_cmpset_pool_summary: sample " + std::to_string(i) + " has " + std::to_string(st->samples[(size_t)i].to_pull[(size_t)sc]) +
                              " sites to pull on scaffold " + std::to_string(sc) +
                              (st->samples[(size_t)i].pulled[(size_t)sc] == PULL_OBS ? " and its observations were never closed by isx_cmpset_pool_obs_done"
                                                                                     : " and was never handed to isx_cmpset_pool_add there"));
                return ISX_ERR_STATE;
            }
    const uint32_t n = (uint32_t)st->n_sites;
    if (!n) return ISX_OK;
    HIP_TRY(hipSetDevice(st->ctx->device));
    hipStream_t s = st->ctx->stream;
    HIP_TRY(st->d_psum.fit(n));
    HIP_TRY(hipEventRecord(st->ev[0], s));
    hipLaunchKernelGGL(k_pool_summary, dim3((n + 255) / 256), dim3(256), 0, s, st->site_gpos.p, st->site_ref.p, st->p_counts.p, st->p_meta.p, n, S,
                       st->d_psum.p);
    HIP_TRY(hipEventRecord(st->ev[1], s));
    HIP_TRY(hipMemcpyAsync(out, st->d_psum.p, (size_t)n * sizeof(isx_pool_site), hipMemcpyDeviceToHost, s));
    HIP_TRY(isx_wait_stream(s));
    HIP_TRY(hipGetLastError());
    if (device_ms) (void)hipEventElapsedTime(device_ms, st->ev[0], st->ev[1]);
    return ISX_OK;
}

int isx_cmpset_pool_fetch_sample(isx_cmpset *st, int32_t sample, uint32_t *counts, uint8_t *meta)
{
    POOL_SITES(st, "isx_cmpset_pool_fetch_sample");
    if (sample < 0 || (size_t)sample >= st->samples.size() || ((!counts || !meta) && st->n_sites)) {
        isx_set_error("isx_cmpset_pool_fetch_sample: bad argument");
        return ISX_ERR_ARG;
    }
    const size_t n = (size_t)st->n_sites;
    if (!n) return ISX_OK;
    HIP_TRY(hipSetDevice(st->ctx->device));
    HIP_TRY(isx_wait_stream(st->ctx->stream));
    HIP_TRY(hipMemcpy(counts, st->p_counts.p + (size_t)sample * n, n * sizeof(uint4), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(meta, st->p_meta.p + (size_t)sample * n, n, hipMemcpyDeviceToHost));
    return ISX_OK;
}

}  // extern "C"
