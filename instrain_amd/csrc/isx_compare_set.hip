// isx_compare_set.hip -- `inStrain compare` over a whole sample set from per-sample sketches.
//
// Replaces, for every pair of every scaffold at once,
//   compare_scaffold                 inStrain/readComparer.py:35-143   (the i < j loop, :80-121)
//   calc_mm2overlap                  readComparer.py:145-191
//   _calc_SNP_count_alternate        readComparer.py:205-290
//   _update_overlap_table            readComparer.py:437-502
//   ScaffoldComparison.add_profile   compare_controller.py (which profiles a scaffold is compared among: cur_names)
// The per-pair body on two resident batches stays in isx_summary.hip (run_compare); this file keeps of each sample only
//   planes[level][word]   one bit per set position: coverage cumulated over levels <= level reaches min_cov
//   present[scaffold][level]   the level is a key of the sample's covT on the scaffold (Acc.present of run_compare)
//   rows[]                the highest-mm SNV row of every position, in set-position order
//   prows[]               (after isx_cmpset_pool_enable) the highest-mm row that is not cryptic: SNV pooling, isx_compare_pool.hip
// so a batch can go as soon as it has been added.  A sample's STORED profile (covT, cumulative_snv_table: compare_controller.py:520-577)
// leaves the same three through isx_cmpset_add_profile: k_profile_planes turns the sparse covT series into the planes without a dense
// coverage array, the SNV tail (reserve_snv_tail / launch_rows) is shared with isx_cmpset_add.  The set's position space starts every scaffold on a 64-position word
// (cmpset_layout.cpp): no word belongs to two scaffolds, `both` of a pair is popcount(a & b) word by word.
// Everything counted here is an integer; sums go through 64-bit integer atomics, so a call's bytes do not depend on timing.
#include <algorithm>
#include <cstring>
#include <string.h>
#include <vector>
#include <rocprim/rocprim.hpp>

#include "isx_compare_set.h"
#include "isx_snp_rules.h"

using namespace isxset;

namespace {

struct CovItem { uint16_t ra, rb; uint32_t out; };      // two staged rows and the output row their count goes to (ra == rb: one sample's own count)

struct SnpPair { int32_t i, j; uint32_t out; uint32_t pad; };

constexpr int SAMPLE_BLOCK = 64;        // samples whose tile words one workgroup stages per side
constexpr int TILE_WORDS = 64;          // a tile: at most 4096 positions of one scaffold (fewer when two sample blocks are staged)
constexpr int LDS_WORDS = 6144;         // 48 KiB of staged words: three workgroups a CU

// cov >= min_cov of 64 consecutive positions of one scaffold -> one word of the set's plane.  One wave per destination word;
// source position = (word - scaffold's first word) * 64 + lane + the scaffold's first position in the batch.
__global__ void __launch_bounds__(256) k_pack_plane(const uint32_t *cov, uint32_t n_pos, uint32_t min_cov, const PackJob *jobs, int n_jobs,
                                                    int64_t n_job_words, uint64_t *plane, int64_t n_words)
{
    const int64_t jw = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;       // wave-uniform
    const int lane = threadIdx.x & 63;
    if (jw >= n_job_words) return;
    int lo = 0, hi = n_jobs;            // jobs[lo].jw0 <= jw < jobs[hi].jw0
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (jobs[mid].jw0 <= jw) lo = mid; else hi = mid;
    }
    const PackJob j = jobs[lo];
    const int64_t local = (jw - j.jw0) * 64 + lane, src = j.src0 + local;
    const bool bit = local < j.len && src >= 0 && src < (int64_t)n_pos && cov[src] >= min_cov;
    const unsigned long long mask = __ballot(bit);
    const int64_t dw = j.dst_w0 + (jw - j.jw0);
    if (lane == 0 && dw >= 0 && dw < n_words) plane[dw] = mask;
}

// (set position, mm) keys of a batch's SNV rows; rows of scaffolds the set does not name get the all-ones key (sorted last).
// POOL: the pooling keys (polymorpher.py:65-68) -- the same, with cryptic rows keyed out as well
template <bool POOL>
__global__ void k_set_keys(const isx_snv *snv, uint32_t n, const int64_t *bbounds, int n_bscaf, const int64_t *set_pos0, uint64_t *keys,
                           uint32_t *idx)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t g = snv[i].gpos;
    const int sc = seg_of(bbounds, n_bscaf, g);
    const int64_t p0 = set_pos0[sc];
    const bool in = p0 >= 0 && g >= bbounds[sc] && g < bbounds[sc + 1] && !(POOL && snv[i].cryptic);
    keys[i] = in ? ((uint64_t)(p0 + (g - bbounds[sc])) << 16) | snv[i].mm : ~0ull;
    idx[i] = i;
}

// the same keys for the rows of a stored cumulative_snv_table: the scaffold is named, not found (the host has checked every field).
// A stored row has no class / cryptic fields, they come beside it (snv_flags: bits 0..2 class, bit 3 cryptic; NULL unless POOL)
template <bool POOL>
__global__ void k_profile_keys(const isx_profile_snv *snv, const uint8_t *snv_flags, uint32_t n, const int64_t *set_pos0, int n_cscaf,
                               uint64_t *keys, uint32_t *idx)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t sc = snv[i].scaffold;
    const int64_t p0 = sc >= 0 && sc < n_cscaf && !(POOL && (snv_flags[i] & 8)) ? set_pos0[sc] : -1;
    keys[i] = p0 >= 0 ? ((uint64_t)(p0 + snv[i].position) << 16) | (uint32_t)(snv[i].mm & 0xFFFF) : ~0ull;
    idx[i] = i;
}

// Stored covT -> the sample's planes, with no dense coverage array in global memory.  One workgroup per tile (ProfTile: at most 64
// words = 4096 positions of one scaffold of the call) keeps the tile's coverage in 16 KiB of LDS counters, zeroed once.  Per level,
// ascending: its slice of the (scaffold, level) series -- two binary searches on the ascending positions -- is added into the counters
// (positions are unique within a level: one lane owns a counter, no atomics; the add is clamped at min_cov, which keeps `>= min_cov`
// exact and cannot wrap), then every wave turns 64 counters at a time into a word by ballot and one lane stores it.  A level that is
// no key of the scaffold has an empty series: its plane is the carried one.  Bits beyond the scaffold's length stay zero.
constexpr int PROF_TILE_WORDS = 64;
constexpr int PROF_TILE_POS = PROF_TILE_WORDS * 64;

__device__ __forceinline__ int64_t first_at_least(const uint32_t *pos, int64_t lo, int64_t hi, uint64_t want)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)pos[mid] < want) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) k_profile_planes(const ProfTile *tiles, const int64_t *entry_off, int n_levels,
                                                        const uint32_t *positions, const uint32_t *values, uint32_t min_cov,
                                                        uint64_t *planes, int64_t n_words)
{
    __shared__ uint32_t cov[PROF_TILE_POS];
    const ProfTile t = tiles[blockIdx.x];
    const int tw = min(t.n_words, PROF_TILE_WORDS);
    if (tw <= 0 || t.scaf < 0 || t.word0 < 0 || t.word0 + tw > n_words) return;                         // (block-uniform)
    const uint32_t n_tile = (uint32_t)tw * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    for (uint32_t p = threadIdx.x; p < n_tile; p += blockDim.x) cov[p] = 0;
    for (int lv = 0; lv < n_levels; lv++) {
        __syncthreads();                    // the counters are zeroed / the words of the level before have been read
        const int64_t b = entry_off[(int64_t)t.scaf * n_levels + lv], e = entry_off[(int64_t)t.scaf * n_levels + lv + 1];
        const int64_t k0 = first_at_least(positions, b, e, t.pos0), k1 = first_at_least(positions, k0, e, (uint64_t)t.pos0 + n_tile);
        for (int64_t k = k0 + threadIdx.x; k < k1; k += blockDim.x) {
            const uint32_t p = positions[k] - t.pos0, v = values[k];
            if (p >= n_tile) continue;                                                                  // (the host's checks rule it out)
            const uint32_t c = cov[p];                                                                  // c <= min_cov
            cov[p] = c + min(v, min_cov - min(c, min_cov));
        }
        __syncthreads();
        uint64_t *plane = planes + (int64_t)lv * n_words + t.word0;
        for (int w = wave; w < tw; w += n_waves) {                                                      // wave-uniform
            const uint32_t p = (uint32_t)w * 64 + lane;
            const unsigned long long mask = __ballot(cov[p] >= min_cov && (uint64_t)t.pos0 + p < t.len);
            if (lane == 0) plane[w] = mask;
        }
    }
}

__global__ void k_last_flags(const uint64_t *keys, uint32_t n, uint32_t *flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flags[i] = keys[i] != ~0ull && (i + 1 == n || (keys[i + 1] >> 16) != (keys[i] >> 16)) ? 1u : 0u;
}

__device__ __forceinline__ uint8_t class_of(const isx_snv &x, const uint8_t *, uint32_t) { return x.cls; }
__device__ __forceinline__ uint8_t class_of(const isx_profile_snv &, const uint8_t *snv_flags, uint32_t i) { return snv_flags[i] & 7; }

// what a compare row / a pool row keeps of source row i besides its position and counts
template <class Src>
__device__ __forceinline__ void fill_row(CsRow &r, const Src &x, const uint8_t *, uint32_t)
{
    r.con_base = x.con_base; r.ref_base = x.ref_base; r.var_base = x.var_base; r.allele_count = x.allele_count;
}
template <class Src>
__device__ __forceinline__ void fill_row(PoolRow &r, const Src &x, const uint8_t *snv_flags, uint32_t i)
{
    r.con_base = x.con_base; r.ref_base = x.ref_base; r.cls = class_of(x, snv_flags, i); r.pad = 0;
}

// the flagged rows, in key order, behind the sample's earlier rows; total[0] = how many.  Src: isx_snv (a resident batch; snv_flags
// unused) or isx_profile_snv (a stored cumulative_snv_table; its snv_flags when Row is PoolRow) -- both name the payload fields alike
template <class Src, class Row>
__global__ void k_gather_last(const uint64_t *keys, const uint32_t *idx, const uint32_t *flags, const uint32_t *pos, uint32_t n,
                              const Src *snv, const uint8_t *snv_flags, Row *out, uint32_t cap, uint32_t *total)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i + 1 == n) total[0] = pos[i] + flags[i];
    if (!flags[i] || pos[i] >= cap) return;
    const Src x = snv[idx[i]];
    Row r;
    r.gpos = (uint32_t)(keys[i] >> 16);
    fill_row(r, x, snv_flags, idx[i]);
    for (int k = 0; k < 4; k++) r.cnt[k] = x.cnt[k];
    out[pos[i]] = r;
}

template <class Row>
__global__ void k_row_keys(const Row *rows, uint32_t n, uint32_t *keys, uint32_t *idx)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { keys[i] = rows[i].gpos; idx[i] = i; }
}

template <class Row>
__global__ void k_gather_rows(const Row *rows, const uint32_t *idx, uint32_t n, Row *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && idx[i] < n) out[i] = rows[idx[i]];
}

// Coverage half.  One workgroup per tile (a run of words of ONE scaffold).  Per axis level the tile's words of the staged samples go
// to LDS (a sample's plane at an axis level = its own highest level <= it, zero when it has none), then every item -- a pair of staged
// rows, or a row with itself for the sample's own count -- sums popcount(a & b) over the tile.  A wave takes `np` items at a time
// (np = a power of two <= 64): lane = (item, word slice), the 64 / np slices of an item are added by xor shuffles, one lane per
// item adds the tile's count to cnt[out][scaffold][level].
__global__ void __launch_bounds__(256) k_cmpset_cov(const uint64_t *const *planes, const int16_t *lmap, int A, int64_t n_words,
                                                    const int32_t *rows, int n_rows, const CovItem *items, int n_items, int np,
                                                    const isx_cmpset_tile *tiles, int tile_words, int n_scaf, unsigned long long *cnt,
                                                    uint32_t n_out)
{
    extern __shared__ uint64_t lds[];
    const isx_cmpset_tile t = tiles[blockIdx.x];
    const int tw = min(t.n_words, tile_words), stride = tile_words + 1;
    if (t.scaffold < 0 || t.scaffold >= n_scaf || t.word0 < 0 || t.word0 + tw > n_words) return;     // (block-uniform)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const int pl = lane & (np - 1), sl = lane / np, ns = 64 / np;
    for (int a = 0; a < A; a++) {
        __syncthreads();
        for (int e = threadIdx.x; e < n_rows * tw; e += blockDim.x) {
            const int r = e / tw, w = e - r * tw;
            const int s = rows[r], lv = lmap[s * A + a];
            lds[r * stride + w] = lv < 0 ? 0ull : planes[s][(int64_t)lv * n_words + t.word0 + w];
        }
        __syncthreads();
        for (int g = wave; g * np < n_items; g += n_waves) {                    // wave-uniform
            const int it = g * np + pl;
            const bool have = it < n_items;
            CovItem x = {0, 0, 0};
            if (have) x = items[it];
            unsigned long long acc = 0;
            if (have && x.ra < n_rows && x.rb < n_rows)
                for (int w = sl; w < tw; w += ns) acc += __popcll(lds[x.ra * stride + w] & lds[x.rb * stride + w]);
            for (int off = np; off < 64; off <<= 1) acc += __shfl_xor(acc, off);
            if (have && sl == 0 && acc && x.out < n_out) atomicAdd(&cnt[((size_t)x.out * n_scaf + t.scaffold) * A + a], acc);
        }
    }
}

// row of `gpos` in a sample's table (ascending set positions), or -1
__device__ __forceinline__ int64_t row_of(const CsRow *rows, uint32_t n, uint32_t gpos)
{
    uint32_t lo = 0, up = n;            // first index with position >= gpos
    while (lo < up) {
        const uint32_t mid = (lo + up) >> 1;
        if (rows[mid].gpos < gpos) lo = mid + 1; else up = mid;
    }
    return lo < n && rows[lo].gpos == gpos ? (int64_t)lo : -1;
}

struct SnpArgs {
    const CsRow *const *rows;           // [S] last-row tables
    const uint32_t *n_rows;             // [S]
    const SnpPair *pairs;               // the launch's pairs
    const uint64_t *cand_off;           // [n_pairs + 1]: prefix of n_rows[i] + n_rows[j]
    int n_pairs;
    isxsnp::NullModel nm;
    const uint64_t *const *planes;
    const int16_t *lmap;
    int A;
    int64_t n_words;
    const int64_t *spos;                // [n_scaf + 1] first set position of every scaffold, then the end of the space
    int n_scaf;
    const uint8_t *pres;                // [S][n_scaf][A] the axis level is a covT key of the sample on the scaffold
    unsigned long long *n_con, *n_pop;  // [n_out][n_scaf][A]
    uint32_t *failed;                   // [n_out][n_scaf]
    uint32_t n_out;
    const int32_t *axis_mm;
    isx_compare_snp *out_rows;          // NULL: counts only
    uint32_t *cursor, cap_rows;
};

// SNP half, one thread per (pair, row of either sample): the verdict of isx_snp_rules.h on the two samples' last-row tables, then
// per axis level the two planes' bits at the position
__global__ void __launch_bounds__(256) k_cmpset_snp(const SnpArgs a)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.cand_off[a.n_pairs]) return;
    int lo = 0, hi = a.n_pairs;         // cand_off[lo] <= t < cand_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.cand_off[mid] <= t) lo = mid; else hi = mid;
    }
    const SnpPair pr = a.pairs[lo];
    if (pr.out >= a.n_out) return;
    const uint32_t n_a = a.n_rows[pr.i], n_b = a.n_rows[pr.j], local = (uint32_t)(t - a.cand_off[lo]);
    if (local >= n_a + n_b) return;
    const bool from_a = local < n_a;
    const CsRow *ra = a.rows[pr.i], *rb = a.rows[pr.j];
    const CsRow x = from_a ? ra[local] : rb[local - n_a];
    const int64_t j = from_a ? row_of(rb, n_b, x.gpos) : row_of(ra, n_a, x.gpos);
    if (!from_a && j >= 0) return;                                          // shared rows are judged from the lower-indexed sample's side
    const int sc = seg_of(a.spos, a.n_scaf, x.gpos);
    if ((int64_t)x.gpos >= a.spos[sc + 1]) return;
    const uint8_t *pa = a.pres + ((size_t)pr.i * a.n_scaf + sc) * a.A, *pb = a.pres + ((size_t)pr.j * a.n_scaf + sc) * a.A;
    bool has_a = false, has_b = false;
    for (int k = 0; k < a.A; k++) { has_a |= pa[k] != 0; has_b |= pb[k] != 0; }
    if (!has_a || !has_b) return;                                           // the pair is not compared on this scaffold (cur_names)
    CsRow y = x;                        // the other sample's row when both have one
    uint32_t verdict;
    if (j < 0) {                        // the row exists in one sample only (the other's columns are NaN)
        verdict = isxsnp::snp_verdict(x, (const CsRow *)nullptr, a.nm);
        if (verdict == isxsnp::SNP_REF_FAILS) {
            atomicOr(&a.failed[(size_t)pr.out * a.n_scaf + sc], 1u);
            return;
        }
    } else {
        y = rb[j];                      // (from_a holds here)
        verdict = isxsnp::snp_verdict(x, &y, a.nm);
    }
    if (!verdict) return;                                                   // "Only keep SNPs" :281
    const bool con = verdict & isxsnp::SNP_CON, pop = verdict & isxsnp::SNP_POP;
    const int64_t word = x.gpos >> 6;
    if (word >= a.n_words) return;
    const uint64_t bit = 1ull << (x.gpos & 63);
    for (int k = 0; k < a.A; k++) {
        if (!pa[k] && !pb[k]) continue;                                     // not a key of either covT: the pair has no such mm
        const int la = a.lmap[pr.i * a.A + k], lb = a.lmap[pr.j * a.A + k];
        if (la < 0 || lb < 0) continue;
        if (!(a.planes[pr.i][(int64_t)la * a.n_words + word] & bit) || !(a.planes[pr.j][(int64_t)lb * a.n_words + word] & bit)) continue;
        const size_t o = ((size_t)pr.out * a.n_scaf + sc) * a.A + k;
        if (con) atomicAdd(&a.n_con[o], 1ull);
        if (pop) atomicAdd(&a.n_pop[o], 1ull);
        if (!a.out_rows) continue;
        const uint32_t at = atomicAdd(a.cursor, 1u);
        if (at >= a.cap_rows) continue;
        isx_compare_snp r;
        memset(&r, 0, sizeof(r));
        r.gpos = x.gpos; r.mm = (uint16_t)a.axis_mm[k];
        r.consensus_snp = con ? 1 : 0; r.population_snp = pop ? 1 : 0;
        const bool row_a = from_a, row_b = !from_a || j >= 0;
        const CsRow &xa = x, &xb = from_a ? y : x;
        if (row_a) isxsnp::snp_fill_side<false>(r, xa);
        if (row_b) isxsnp::snp_fill_side<true>(r, xb);
        a.out_rows[at] = r;
    }
}

}  // namespace

namespace isxset {

int cmpset_grow_temp(isx_cmpset *st, size_t bytes)
{
    if (st->temp.cap < bytes + 256) HIP_TRY(st->temp.fit(bytes + 256));
    return ISX_OK;
}

}  // namespace isxset

namespace {

int grow_temp(isx_cmpset *st, size_t bytes) { return cmpset_grow_temp(st, bytes); }

// the sample's real mm values and the set's level axis
int level_axis(const isx_cmpset *st, std::vector<int32_t> &axis, int32_t *n_axis, std::vector<int32_t> &map)
{
    const int32_t S = (int32_t)st->samples.size();
    std::vector<int32_t> n_levels, all;
    for (const Sample &s : st->samples) {
        n_levels.push_back((int32_t)s.mm.size());
        all.insert(all.end(), s.mm.begin(), s.mm.end());
    }
    axis.assign(ISX_CMPSET_MAX_LEVELS, 0);
    map.assign((size_t)std::max(S, 1) * ISX_CMPSET_MAX_LEVELS, -1);
    return isx_cmpset_level_map(S, n_levels.data(), all.data(), ISX_CMPSET_MAX_LEVELS, axis.data(), n_axis, map.data());
}

// one of a sample's two row tables -- compare rows (CsRow), pool rows (PoolRow) -- as the SNV tail and the re-sort see it
template <class Row>
struct RowTable { Row *&rows; size_t &n, &cap; bool &sorted; };

RowTable<CsRow> own_rows(Sample &sm) { return {sm.rows, sm.n_rows, sm.cap_rows, sm.sorted}; }
RowTable<PoolRow> pool_rows(Sample &sm) { return {sm.prows, sm.n_prows, sm.cap_prows, sm.psorted}; }

// room for n_snv new rows behind the table's (a call adds at most one row per SNV row)
template <class Row>
int reserve_rows(isx_cmpset *st, RowTable<Row> t, uint32_t n_snv)
{
    hipStream_t s = st->ctx->stream;
    if (t.cap >= t.n + n_snv) return ISX_OK;
    const size_t want = std::max(t.n + n_snv, t.cap * 2);
    Row *grown = nullptr;
    HIP_TRY(isx_raw_dev_malloc(&grown, want * sizeof(Row)));
    if (t.n) HIP_TRY(hipMemcpyAsync(grown, t.rows, t.n * sizeof(Row), hipMemcpyDeviceToDevice, s));
    HIP_TRY(isx_wait_stream(s));
    if (t.rows) isx_dev_free(t.rows);
    t.rows = grown; t.cap = want;
    return ISX_OK;
}

// The SNV tail both entry points share.  reserve_snv_tail: every scratch array of n_snv rows -- one set, which the pool rows' pass
// uses after the compare rows' -- and room in the sample's table(s), all before anything is launched.
int reserve_snv_tail(isx_cmpset *st, Sample &sm, uint32_t n_snv, bool pool)
{
    if (!n_snv) return ISX_OK;
    hipStream_t s = st->ctx->stream;
    HIP_TRY(st->keys.fit(n_snv)); HIP_TRY(st->keys_in.fit(n_snv)); HIP_TRY(st->idx.fit(n_snv)); HIP_TRY(st->idx_in.fit(n_snv));
    HIP_TRY(st->flags.fit(n_snv)); HIP_TRY(st->pos.fit((size_t)n_snv + 1));
    size_t t_sort = 0, t_scan = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, t_sort, st->keys_in.p, st->keys.p, st->idx_in.p, st->idx.p, n_snv, 0, 64, s));
    HIP_TRY(rocprim::exclusive_scan(nullptr, t_scan, st->flags.p, st->pos.p, 0u, n_snv, rocprim::plus<uint32_t>(), s));
    int rc = grow_temp(st, std::max(t_sort, t_scan));
    if (!rc) rc = reserve_rows(st, own_rows(sm), n_snv);
    if (!rc && pool) rc = reserve_rows(st, pool_rows(sm), n_snv);
    return rc;
}

// launch_rows: st->keys_in / idx_in hold the (set position, mm) keys of the source rows (the pooling keys for the pool rows); sort,
// flag the last row of every position, scan, gather them behind the table's rows; *n_new = how many, once the stream has drained
template <class Src, class Row>
int launch_rows(isx_cmpset *st, RowTable<Row> t, uint32_t n_snv, const Src *d_snv, const uint8_t *d_snv_flags, uint32_t *n_new)
{
    hipStream_t s = st->ctx->stream;
    const dim3 blk(256), grid((n_snv + 255) / 256);
    size_t tb = st->temp.cap;
    HIP_TRY(rocprim::radix_sort_pairs(st->temp.p, tb, st->keys_in.p, st->keys.p, st->idx_in.p, st->idx.p, n_snv, 0, 64, s));
    hipLaunchKernelGGL(k_last_flags, grid, blk, 0, s, st->keys.p, n_snv, st->flags.p);
    tb = st->temp.cap;
    HIP_TRY(rocprim::exclusive_scan(st->temp.p, tb, st->flags.p, st->pos.p, 0u, n_snv, rocprim::plus<uint32_t>(), s));
    hipLaunchKernelGGL((k_gather_last<Src, Row>), grid, blk, 0, s, st->keys.p, st->idx.p, st->flags.p, st->pos.p, n_snv, d_snv, d_snv_flags,
                       t.rows + t.n, (uint32_t)(t.cap - t.n), st->pos.p + n_snv);
    HIP_TRY(hipMemcpyAsync(n_new, st->pos.p + n_snv, 4, hipMemcpyDeviceToHost, s));
    return ISX_OK;
}

// the call's n_new rows are the table's; out_of_order: the call brought a scaffold below one the sample already had
template <class Row>
void commit_rows(RowTable<Row> t, uint32_t n_new, bool out_of_order)
{
    if (n_new && t.n && out_of_order) t.sorted = false;
    t.n += std::min<size_t>(n_new, t.cap - t.n);
}

// rows (compare rows or pool rows) of a sample whose batches did not arrive in set order: one sort by position
template <class Row>
int sort_rows_of(isx_cmpset *st, RowTable<Row> t)
{
    if (t.sorted || t.n < 2) { t.sorted = true; return ISX_OK; }
    hipStream_t s = st->ctx->stream;
    const uint32_t n = (uint32_t)t.n;
    SetBuf<uint32_t> k_in, k_out;
    Row *fresh = nullptr;
    auto done = [&](int rc) { k_in.drop(); k_out.drop(); if (fresh) isx_dev_free(fresh); return rc; };
    if (k_in.fit(n) != hipSuccess || k_out.fit(n) != hipSuccess || st->idx_in.fit(n) != hipSuccess || st->idx.fit(n) != hipSuccess ||
        isx_raw_dev_malloc(&fresh, t.cap * sizeof(Row)) != hipSuccess) {
        isx_set_error("isx_cmpset_compare: out of device memory while ordering a sample's SNV rows");
        return done(ISX_ERR_HIP);
    }
    size_t tb = 0;
    if (rocprim::radix_sort_pairs(nullptr, tb, k_in.p, k_out.p, st->idx_in.p, st->idx.p, n, 0, 32, s) != hipSuccess) return done(ISX_ERR_HIP);
    int rc = grow_temp(st, tb);
    if (rc) return done(rc);
    const dim3 blk(256), grid((n + 255) / 256);
    hipLaunchKernelGGL(k_row_keys<Row>, grid, blk, 0, s, t.rows, n, k_in.p, st->idx_in.p);
    tb = st->temp.cap;
    if (rocprim::radix_sort_pairs(st->temp.p, tb, k_in.p, k_out.p, st->idx_in.p, st->idx.p, n, 0, 32, s) != hipSuccess) {
        isx_set_error("isx_cmpset_compare: radix sort of a sample's SNV rows failed");
        return done(ISX_ERR_HIP);
    }
    hipLaunchKernelGGL(k_gather_rows<Row>, grid, blk, 0, s, t.rows, st->idx.p, n, fresh);
    if (isx_wait_stream(s) != hipSuccess) { isx_set_error("isx_cmpset_compare: ordering a sample's SNV rows failed"); return done(ISX_ERR_HIP); }
    std::swap(t.rows, fresh);
    t.sorted = true;
    return done(ISX_OK);
}

int sort_rows(isx_cmpset *st, Sample &sm) { return sort_rows_of(st, own_rows(sm)); }

int pow2_ceil(int n) { int p = 1; while (p < n) p <<= 1; return p; }

// ---- what isx_cmpset_add and the stored-profile entry points do alike around their own passes ----
struct Caller {
    std::string who;                    // heads every error text: "isx_cmpset_add: "
    const char *unit, *units;           // what the entry point's texts call one call and several: "batch" / "batches"
};

// the call's level values ascend strictly within 0..65535 and are those of the sample's earlier calls; *fresh: it has had none
int check_levels(const Caller &c, const isx_cmpset *st, int32_t sample, const std::vector<int32_t> &mmv, bool *fresh)
{
    for (size_t k = 0; k < mmv.size(); k++)
        if (mmv[k] < 0 || mmv[k] > 65535 || (k && mmv[k] <= mmv[k - 1])) {
            isx_set_error(c.who + "level_mm_values must ascend strictly within 0..65535");
            return ISX_ERR_ARG;
        }
    *fresh = (size_t)sample >= st->samples.size() || st->samples[(size_t)sample].mm.empty();
    if (!*fresh && st->samples[(size_t)sample].mm != mmv) {
        isx_set_error(c.who + "this " + c.unit + "'s level_mm_values differ from those of the sample's earlier " + c.units);
        return ISX_ERR_ARG;
    }
    return ISX_OK;
}

struct Claim {
    std::vector<int64_t> set_pos0;      // per scaffold of the call: its first set position, -1 when the set does not name it
    std::vector<int32_t> named;         // the call's scaffolds the set names
    int32_t min_sid, max_sid;           // the lowest and highest set scaffold among them
};

// the call's scaffolds, ids[i] = scaffold of the set or -1: each within the set, of the set's length where the call has lengths of its
// own (bounds: n + 1 ascending bounds, or NULL), and new to the sample
int claim_scaffolds(const Caller &c, const isx_cmpset *st, int32_t sample, bool fresh, int32_t n, const int32_t *ids, const int64_t *bounds,
                    Claim &out)
{
    std::vector<uint8_t> seen((size_t)st->n_scaf, 0);
    out.set_pos0.assign((size_t)n, -1);
    out.named.clear();
    out.min_sid = st->n_scaf; out.max_sid = -1;
    for (int i = 0; i < n; i++) {
        const int32_t sid = ids[i];
        if (sid == -1) continue;
        if (sid < 0 || sid >= st->n_scaf) { isx_set_error(c.who + "set_scaffold_ids[" + std::to_string(i) + "] outside the set"); return ISX_ERR_ARG; }
        if (bounds && bounds[i + 1] - bounds[i] != st->len[(size_t)sid]) {
            isx_set_error(c.who + "batch scaffold " + std::to_string(i) + " has not the length of set scaffold " + std::to_string(sid));
            return ISX_ERR_ARG;
        }
        if (seen[(size_t)sid] || (!fresh && st->samples[(size_t)sample].have[(size_t)sid])) {
            isx_set_error(c.who + "scaffold " + std::to_string(sid) + " of sample " + std::to_string(sample) + " was added before");
            return ISX_ERR_STATE;
        }
        seen[(size_t)sid] = 1;
        out.set_pos0[(size_t)i] = st->spos[(size_t)sid];
        out.named.push_back(i);
        out.min_sid = std::min(out.min_sid, sid); out.max_sid = std::max(out.max_sid, sid);
    }
    return ISX_OK;
}

// the sample's slot; its first call fixes its levels and gives it zeroed planes.  Whatever was derived from the set as it was -- the
// pair counters, the clustering, the sites, ranks and pulled counts of isx_cmpset_pool_sites -- no longer holds.
int open_sample(isx_cmpset *st, int32_t sample, int n_levels, Sample **out)
{
    if ((size_t)sample >= st->samples.size()) st->samples.resize((size_t)sample + 1);
    Sample &sm = st->samples[(size_t)sample];
    if (sm.mm.empty()) {
        if (sm.planes) isx_dev_free(sm.planes);
        sm.planes = nullptr;
        HIP_TRY(isx_raw_dev_malloc(&sm.planes, (size_t)n_levels * (size_t)st->n_words * 8));
        HIP_TRY(hipMemsetAsync(sm.planes, 0, (size_t)n_levels * (size_t)st->n_words * 8, st->ctx->stream));
        sm.have.assign((size_t)st->n_scaf, 0);
        sm.present.assign((size_t)st->n_scaf * n_levels, 0);
    }
    st->compared = false;
    st->clustered = false;
    st->pooled = false;
    *out = &sm;
    return ISX_OK;
}

// only now is the call part of the sample.  present_at(i, k): level k is a key of the covT of the call's scaffold i
template <class PresentAt>
void commit_call(Sample &sm, const std::vector<int32_t> &mmv, const int32_t *ids, const Claim &cl, PresentAt present_at, uint32_t n_new,
                 uint32_t n_new_pool)
{
    const size_t L = mmv.size();
    if (sm.mm.empty()) sm.mm = mmv;
    for (const int32_t i : cl.named) {
        sm.have[(size_t)ids[i]] = 1;
        for (size_t k = 0; k < L; k++) sm.present[(size_t)ids[i] * L + k] = present_at(i, (int)k) ? 1 : 0;
    }
    const bool out_of_order = cl.min_sid < sm.max_sid;
    commit_rows(own_rows(sm), n_new, out_of_order);
    commit_rows(pool_rows(sm), n_new_pool, out_of_order);
    sm.max_sid = std::max(sm.max_sid, cl.max_sid);
}

}  // namespace

namespace isxset {

int cmpset_sort_pool_rows(isx_cmpset *st, Sample &sm) { return sort_rows_of(st, pool_rows(sm)); }

int cmpset_check_batch(const char *who, const isx_cmpset *st, int32_t sample, const isx_batch *b, int32_t n_bscaf, const int64_t *bb,
                       const int32_t *ids)
{
    const std::string w(who);
    if (!st || !b || !bb || !ids || n_bscaf <= 0 || sample < 0 || sample >= ISX_CMPSET_MAX_SAMPLES) {
        isx_set_error(w + ": bad argument");
        return ISX_ERR_ARG;
    }
    if (!b->ran) { isx_set_error(w + ": run the batch first"); return ISX_ERR_STATE; }
    if (b->ctx != st->ctx) { isx_set_error(w + ": the batch belongs to another ctx than the set"); return ISX_ERR_ARG; }
    if (bb[0] != 0 || bb[n_bscaf] != b->n_pos) { isx_set_error(w + ": batch_scaffold_bounds must span [0, n_pos]"); return ISX_ERR_ARG; }
    for (int i = 0; i < n_bscaf; i++)
        if (bb[i + 1] <= bb[i]) { isx_set_error(w + ": batch_scaffold_bounds must be strictly ascending"); return ISX_ERR_ARG; }
    if (b->n_pos > (int64_t)0xFFFFFFFFll) { isx_set_error(w + ": flat space beyond 2^32 positions"); return ISX_ERR_ARG; }
    return ISX_OK;
}

}  // namespace isxset

extern "C" {

int isx_cmpset_create(isx_ctx *ctx, int32_t n_scaffolds, const int64_t *scaffold_lengths, int32_t min_cov, isx_cmpset **out)
{
    if (!ctx || !out || n_scaffolds <= 0 || !scaffold_lengths || min_cov < 0) { isx_set_error("isx_cmpset_create: bad argument"); return ISX_ERR_ARG; }
    *out = nullptr;
    std::vector<int64_t> woff((size_t)n_scaffolds + 1);
    const int rc = isx_cmpset_layout(n_scaffolds, scaffold_lengths, woff.data());
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    isx_cmpset *st = new isx_cmpset();
    st->ctx = ctx; st->min_cov = min_cov; st->n_scaf = n_scaffolds;
    st->len.assign(scaffold_lengths, scaffold_lengths + n_scaffolds);
    st->woff = woff;
    st->n_words = woff.back();
    for (int64_t w : woff) st->spos.push_back(w * 64);
    hipError_t e = hipEventCreate(&st->ev[0]);
    if (e == hipSuccess) e = hipEventCreate(&st->ev[1]);
    if (e != hipSuccess) {
        isx_set_error(std::string("isx_cmpset_create: ") + hipGetErrorString(e));
        isx_cmpset_destroy(st);
        return ISX_ERR_HIP;
    }
    *out = st;
    return ISX_OK;
}

void isx_cmpset_destroy(isx_cmpset *st)
{
    if (!st) return;
    (void)hipSetDevice(st->ctx->device);
    (void)isx_wait_stream(st->ctx->stream);
    for (Sample &s : st->samples) {
        if (s.planes) isx_dev_free(s.planes);
        if (s.rows) isx_dev_free(s.rows);
        if (s.prows) isx_dev_free(s.prows);
    }
    cmpset_pool_drop(st);
    cmpset_cluster_drop(st);
    st->cov.drop(); st->present.drop(); st->idx.drop(); st->idx_in.drop(); st->flags.drop(); st->pos.drop(); st->scratch_f.drop();
    st->bbounds.drop(); st->set_pos0.drop(); st->acc.drop(); st->temp.drop(); st->jobs.drop(); st->keys.drop(); st->keys_in.drop();
    st->d_planes.drop(); st->d_rows.drop(); st->d_n_rows.drop(); st->d_failed.drop(); st->d_cursor.drop(); st->d_lmap.drop();
    st->d_pres.drop(); st->d_spos.drop(); st->d_axis.drop(); st->d_cnt.drop(); st->d_snp.drop(); st->snp_rows.drop();
    st->pf_off.drop(); st->pf_pos.drop(); st->pf_val.drop(); st->pf_tiles.drop(); st->pf_snv.drop(); st->pf_flags.drop();
    st->obs_stage.drop(); st->obs_roff.drop(); st->obs_rbase.drop();
    for (hipEvent_t e : st->ev) if (e) (void)hipEventDestroy(e);
    delete st;
}

int isx_cmpset_add(isx_cmpset *st, int32_t sample, isx_batch *b, int32_t n_bscaf, const int64_t *bb, const int32_t *ids,
                   const int32_t *level_mm_values)
{
    const int rc_args = cmpset_check_batch("isx_cmpset_add", st, sample, b, n_bscaf, bb, ids);
    if (rc_args) return rc_args;
    if (b->lean && !b->d_counts) { isx_set_error("a batch of a lean pipe slot (isx_pipe_params.lean_output) keeps no dense coverage / clonality arrays"); return ISX_ERR_STATE; }
    const int M = b->M;
    if (M <= 0 || M > ISX_CMPSET_MAX_LEVELS) {
        isx_set_error("isx_cmpset_add: a batch of " + std::to_string(M) + " levels; a set compares at most " + std::to_string(ISX_CMPSET_MAX_LEVELS));
        return ISX_ERR_CAPACITY;
    }
    const Caller who{"isx_cmpset_add: ", "batch", "batches"};
    std::vector<int32_t> mmv((size_t)M);
    for (int k = 0; k < M; k++) mmv[(size_t)k] = level_mm_values ? level_mm_values[k] : k;
    bool fresh = false;
    Claim cl;
    int rc = check_levels(who, st, sample, mmv, &fresh);
    if (!rc) rc = claim_scaffolds(who, st, sample, fresh, n_bscaf, ids, bb, cl);
    if (rc) return rc;
    if (cl.named.empty()) return ISX_OK;            // nothing of this batch is in the set
    std::vector<PackJob> jobs;
    int64_t jw = 0;
    for (const int32_t i : cl.named) {
        const size_t sid = (size_t)ids[i];
        jobs.push_back({jw, st->woff[sid], bb[i], st->len[sid]});
        jw += st->woff[sid + 1] - st->woff[sid];
    }
    const int n_jobs = (int)jobs.size();
    jobs.push_back({jw, 0, 0, 0});
    const uint32_t n_snv = (uint32_t)b->sizes.n_snv, n_pos = (uint32_t)b->n_pos;

    HIP_TRY(hipSetDevice(st->ctx->device));
    hipStream_t s = st->ctx->stream;
    Sample *opened = nullptr;
    if ((rc = open_sample(st, sample, M, &opened))) return rc;
    Sample &sm = *opened;
    // scratch, all sized before anything is launched
    HIP_TRY(st->cov.fit(n_pos)); HIP_TRY(st->scratch_f.fit((size_t)n_pos * 2));
    HIP_TRY(st->acc.fit(level_acc_bytes(n_bscaf))); HIP_TRY(st->present.fit((size_t)n_bscaf * M));
    const std::vector<int64_t> h_bounds(bb, bb + n_bscaf + 1);
    HIP_TRY(st->bbounds.put(h_bounds, s));
    HIP_TRY(st->set_pos0.put(cl.set_pos0, s));
    HIP_TRY(st->jobs.put(jobs, s));
    if ((rc = reserve_snv_tail(st, sm, n_snv, st->pool_on))) return rc;
    SummaryIn in{};
    fill_summary_in(b, n_bscaf, bb, in);
    in.stream = s;
    const dim3 blk(256);
    // coverage: the levels cumulated as run_compare does, each packed into the sample's plane of that level
    HIP_TRY(hipMemsetAsync(st->cov.p, 0, (size_t)n_pos * 4, s));
    for (int mm = 0; mm < M; mm++) {
        launch_level_cumulate(in, mm, st->cov.p, st->scratch_f.p, st->scratch_f.p + n_pos, st->bbounds.p, st->acc.p,
                              st->present.p + (size_t)mm * n_bscaf);
        hipLaunchKernelGGL(k_pack_plane, dim3((unsigned)((jw * 64 + 255) / 256)), blk, 0, s, st->cov.p, n_pos, (uint32_t)st->min_cov,
                           st->jobs.p, n_jobs, jw, sm.planes + (size_t)mm * (size_t)st->n_words, st->n_words);
    }
    std::vector<uint32_t> present((size_t)n_bscaf * M);
    HIP_TRY(hipMemcpyAsync(present.data(), st->present.p, present.size() * 4, hipMemcpyDeviceToHost, s));
    // SNV rows: (set position, mm) keys, sorted; the last row of every position, in order, behind the sample's rows
    uint32_t n_new = 0;
    if (n_snv) {
        const dim3 grid((n_snv + 255) / 256);
        hipLaunchKernelGGL(k_set_keys<false>, grid, blk, 0, s, b->d_snv, n_snv, st->bbounds.p, n_bscaf, st->set_pos0.p, st->keys_in.p, st->idx_in.p);
        if ((rc = launch_rows(st, own_rows(sm), n_snv, b->d_snv, (const uint8_t *)nullptr, &n_new))) return rc;
    }
    // pool rows: the same scheme on keys that leave the cryptic rows out, so a position's last row is its highest-mm row that counts
    uint32_t n_new_pool = 0;
    if (n_snv && st->pool_on) {
        const dim3 grid((n_snv + 255) / 256);
        hipLaunchKernelGGL(k_set_keys<true>, grid, blk, 0, s, b->d_snv, n_snv, st->bbounds.p, n_bscaf, st->set_pos0.p, st->keys_in.p, st->idx_in.p);
        if ((rc = launch_rows(st, pool_rows(sm), n_snv, b->d_snv, (const uint8_t *)nullptr, &n_new_pool))) return rc;
    }
    HIP_TRY(isx_wait_stream(s));
    HIP_TRY(hipGetLastError());
    commit_call(sm, mmv, ids, cl, [&](int i, int mm) { return present[(size_t)mm * n_bscaf + i] != 0; }, n_new, n_new_pool);
    return ISX_OK;
}

// both stored-profile entry points.  pool: isx_cmpset_add_profile_pool, snv_flags beside the rows; otherwise isx_cmpset_add_profile
static int add_profile(bool pool, isx_cmpset *st, int32_t sample, int32_t n_cscaf, const int32_t *ids, int32_t L, const int32_t *level_mm_values,
                       const uint8_t *present, const int64_t *off, const uint32_t *positions, const uint32_t *values, int64_t n_snv_in,
                       const isx_profile_snv *snv, const uint8_t *snv_flags, float *device_ms)
{
    const Caller caller{pool ? "isx_cmpset_add_profile_pool: " : "isx_cmpset_add_profile: ", "call", "calls"};
    const std::string &who = caller.who;
    if (device_ms) *device_ms = 0.f;
    if (!st || sample < 0 || sample >= ISX_CMPSET_MAX_SAMPLES || n_cscaf <= 0 || !ids || L <= 0 || !level_mm_values || !present || !off ||
        n_snv_in < 0 || (n_snv_in && (!snv || (pool && !snv_flags)))) {
        isx_set_error(who + "bad argument");
        return ISX_ERR_ARG;
    }
    if (st->pool_on && !pool) {
        isx_set_error(who + "the own rows of a set with pooling enabled need the class / cryptic columns: isx_cmpset_add_profile_pool takes them");
        return ISX_ERR_STATE;
    }
    if (pool && !st->pool_on) {
        isx_set_error(who + "the set keeps no pool rows (isx_cmpset_pool_enable before the first add); isx_cmpset_add_profile is its call");
        return ISX_ERR_STATE;
    }
    if (L > ISX_CMPSET_MAX_LEVELS) {
        isx_set_error(who + "a profile of " + std::to_string(L) + " levels; a set compares at most " + std::to_string(ISX_CMPSET_MAX_LEVELS));
        return ISX_ERR_CAPACITY;
    }
    if (n_snv_in > (int64_t)0x7FFFFFFFll) { isx_set_error(who + "more SNV rows than one call holds"); return ISX_ERR_CAPACITY; }
    const std::vector<int32_t> mmv(level_mm_values, level_mm_values + L);
    bool fresh = false;
    Claim cl;
    int rc = check_levels(caller, st, sample, mmv, &fresh);
    if (!rc) rc = claim_scaffolds(caller, st, sample, fresh, n_cscaf, ids, nullptr, cl);
    if (rc) return rc;
    const std::vector<int32_t> &sub_scaf = cl.named;
    std::vector<int64_t> sub_len;
    for (const int32_t i : sub_scaf) sub_len.push_back(st->len[(size_t)ids[i]]);
    // the covT series
    const int64_t n_series = (int64_t)n_cscaf * L;
    if (off[0] != 0) { isx_set_error(who + "entry_offsets must start at 0"); return ISX_ERR_ARG; }
    for (int64_t q = 0; q < n_series; q++)
        if (off[q + 1] < off[q]) { isx_set_error(who + "entry_offsets must not descend"); return ISX_ERR_ARG; }
    const int64_t n_entries = off[n_series];
    if (n_entries && (!positions || !values)) { isx_set_error(who + "bad argument"); return ISX_ERR_ARG; }
    for (int i = 0; i < n_cscaf; i++)
        for (int k = 0; k < L; k++) {
            const int64_t q = (int64_t)i * L + k, b = off[q], e = off[q + 1];
            if (!present[q] && e != b) {
                isx_set_error(who + "scaffold " + std::to_string(i) + " has entries at a level that is no key of its covT");
                return ISX_ERR_ARG;
            }
            if (ids[i] < 0) continue;
            const int64_t len = st->len[(size_t)ids[i]];
            for (int64_t x = b; x < e; x++)
                if ((int64_t)positions[x] >= len || (x > b && positions[x] <= positions[x - 1])) {
                    isx_set_error(who + "the positions of scaffold " + std::to_string(i) + ", level " + std::to_string(k) +
                                  " must ascend strictly below the scaffold's length");
                    return ISX_ERR_ARG;
                }
        }
    // the SNV rows
    const uint32_t n_snv = (uint32_t)n_snv_in;
    for (uint32_t r = 0; r < n_snv; r++) {
        const isx_profile_snv &x = snv[r];
        const bool ok = x.scaffold >= 0 && x.scaffold < n_cscaf && x.mm >= 0 && x.mm <= 65535 && x.con_base <= 3 && x.var_base <= 3 &&
                        x.ref_base <= 4 && (ids[x.scaffold] < 0 || (int64_t)x.position < st->len[(size_t)ids[x.scaffold]]);
        if (!ok) {
            isx_set_error(who + "SNV row " + std::to_string(r) + ": scaffold index, position, mm or a base code out of range");
            return ISX_ERR_ARG;
        }
        if (pool && ((snv_flags[r] & 7) > 5 || (snv_flags[r] & ~15))) {
            isx_set_error(who + "snv_flags[" + std::to_string(r) + "]: a class code above 5 or a bit above 3");
            return ISX_ERR_ARG;
        }
    }
    if (sub_scaf.empty()) return ISX_OK;            // nothing of this call is in the set
    // the tiles: the set's tile geometry over the call's scaffolds only
    const int64_t n_tiles = isx_cmpset_tiles((int32_t)sub_len.size(), sub_len.data(), PROF_TILE_WORDS, nullptr);
    if (n_tiles < 0) return (int)n_tiles;
    if (n_tiles > 0x7FFFFFFFll) { isx_set_error(who + "too many tiles for one launch"); return ISX_ERR_CAPACITY; }
    std::vector<isx_cmpset_tile> sub_tiles((size_t)n_tiles);
    (void)isx_cmpset_tiles((int32_t)sub_len.size(), sub_len.data(), PROF_TILE_WORDS, sub_tiles.data());
    std::vector<int64_t> sub_off(sub_len.size() + 1);
    (void)isx_cmpset_layout((int32_t)sub_len.size(), sub_len.data(), sub_off.data());
    std::vector<ProfTile> tiles((size_t)n_tiles);
    for (int64_t q = 0; q < n_tiles; q++) {
        const isx_cmpset_tile &u = sub_tiles[(size_t)q];
        const int32_t i = sub_scaf[(size_t)u.scaffold], sid = ids[i];
        const int64_t w_in = u.word0 - sub_off[(size_t)u.scaffold];
        tiles[(size_t)q] = {st->woff[(size_t)sid] + w_in, u.n_words, i, (uint32_t)(w_in * 64), (uint32_t)st->len[(size_t)sid]};
    }

    HIP_TRY(hipSetDevice(st->ctx->device));
    hipStream_t s = st->ctx->stream;
    Sample *opened = nullptr;
    if ((rc = open_sample(st, sample, L, &opened))) return rc;
    Sample &sm = *opened;
    // scratch and uploads, all sized before anything is launched
    HIP_TRY(st->pf_off.fit((size_t)n_series + 1)); HIP_TRY(st->pf_pos.fit((size_t)n_entries)); HIP_TRY(st->pf_val.fit((size_t)n_entries));
    HIP_TRY(st->pf_snv.fit(n_snv));
    if (pool) HIP_TRY(st->pf_flags.fit(n_snv));
    if ((rc = reserve_snv_tail(st, sm, n_snv, pool))) return rc;
    HIP_TRY(hipMemcpyAsync(st->pf_off.p, off, ((size_t)n_series + 1) * 8, hipMemcpyHostToDevice, s));
    if (n_entries) {
        HIP_TRY(hipMemcpyAsync(st->pf_pos.p, positions, (size_t)n_entries * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(st->pf_val.p, values, (size_t)n_entries * 4, hipMemcpyHostToDevice, s));
    }
    if (n_snv) HIP_TRY(hipMemcpyAsync(st->pf_snv.p, snv, (size_t)n_snv * sizeof(isx_profile_snv), hipMemcpyHostToDevice, s));
    if (n_snv && pool) HIP_TRY(hipMemcpyAsync(st->pf_flags.p, snv_flags, n_snv, hipMemcpyHostToDevice, s));
    HIP_TRY(st->pf_tiles.put(tiles, s));
    HIP_TRY(st->set_pos0.put(cl.set_pos0, s));
    HIP_TRY(hipEventRecord(st->ev[0], s));
    hipLaunchKernelGGL(k_profile_planes, dim3((unsigned)n_tiles), dim3(256), 0, s, st->pf_tiles.p, st->pf_off.p, (int)L, st->pf_pos.p,
                       st->pf_val.p, (uint32_t)st->min_cov, sm.planes, st->n_words);
    uint32_t n_new = 0;
    if (n_snv) {
        hipLaunchKernelGGL(k_profile_keys<false>, dim3((n_snv + 255) / 256), dim3(256), 0, s, st->pf_snv.p, (const uint8_t *)nullptr, n_snv,
                           st->set_pos0.p, (int)n_cscaf, st->keys_in.p, st->idx_in.p);
        if ((rc = launch_rows(st, own_rows(sm), n_snv, st->pf_snv.p, (const uint8_t *)nullptr, &n_new))) return rc;
    }
    uint32_t n_new_pool = 0;                        // pool rows: as isx_cmpset_add makes them, the cryptic rows keyed out
    if (n_snv && pool) {
        hipLaunchKernelGGL(k_profile_keys<true>, dim3((n_snv + 255) / 256), dim3(256), 0, s, st->pf_snv.p, st->pf_flags.p, n_snv,
                           st->set_pos0.p, (int)n_cscaf, st->keys_in.p, st->idx_in.p);
        if ((rc = launch_rows(st, pool_rows(sm), n_snv, st->pf_snv.p, st->pf_flags.p, &n_new_pool))) return rc;
    }
    HIP_TRY(hipEventRecord(st->ev[1], s));
    HIP_TRY(isx_wait_stream(s));
    HIP_TRY(hipGetLastError());
    if (device_ms) (void)hipEventElapsedTime(device_ms, st->ev[0], st->ev[1]);
    commit_call(sm, mmv, ids, cl, [&](int i, int k) { return present[(size_t)i * L + k] != 0; }, n_new, n_new_pool);
    return ISX_OK;
}

int isx_cmpset_add_profile(isx_cmpset *st, int32_t sample, int32_t n_cscaf, const int32_t *ids, int32_t L, const int32_t *level_mm_values,
                           const uint8_t *present, const int64_t *off, const uint32_t *positions, const uint32_t *values, int64_t n_snv,
                           const isx_profile_snv *snv, float *device_ms)
{
    return add_profile(false, st, sample, n_cscaf, ids, L, level_mm_values, present, off, positions, values, n_snv, snv, nullptr, device_ms);
}

int isx_cmpset_add_profile_pool(isx_cmpset *st, int32_t sample, int32_t n_cscaf, const int32_t *ids, int32_t L, const int32_t *level_mm_values,
                                const uint8_t *present, const int64_t *off, const uint32_t *positions, const uint32_t *values, int64_t n_snv,
                                const isx_profile_snv *snv, const uint8_t *snv_flags, float *device_ms)
{
    return add_profile(true, st, sample, n_cscaf, ids, L, level_mm_values, present, off, positions, values, n_snv, snv, snv_flags, device_ms);
}

int isx_cmpset_axis(isx_cmpset *st, int32_t *n_samples, int32_t *n_levels, int32_t *axis_mm)
{
    if (!st || !n_samples || !n_levels) { isx_set_error("isx_cmpset_axis: bad argument"); return ISX_ERR_ARG; }
    std::vector<int32_t> axis, map;
    int32_t A = 0;
    const int rc = level_axis(st, axis, &A, map);
    if (rc) return rc;
    *n_samples = (int32_t)st->samples.size();
    *n_levels = A;
    if (axis_mm) std::copy(axis.begin(), axis.begin() + A, axis_mm);
    return ISX_OK;
}

int isx_cmpset_compare(isx_cmpset *st, double min_freq, int64_t cap_rows, isx_compare_level *out, float *device_ms)
{
    if (!st || (!out && cap_rows > 0) || cap_rows < 0) { isx_set_error("isx_cmpset_compare: bad argument"); return ISX_ERR_ARG; }
    if (!st->ctx->d_lut) { isx_set_error("isx_cmpset_compare: set the null model first"); return ISX_ERR_STATE; }
    const int32_t S = (int32_t)st->samples.size(), n_scaf = st->n_scaf;
    std::vector<int32_t> axis, map;
    int32_t A = 0;
    int rc = level_axis(st, axis, &A, map);
    if (rc) return rc;
    const int64_t n_pairs = (int64_t)S * (S - 1) / 2, n_out = n_pairs + S;
    if (n_pairs * n_scaf * A > cap_rows) { isx_set_error("isx_cmpset_compare: out holds fewer than pairs x scaffolds x levels rows"); return ISX_ERR_ARG; }
    if (device_ms) *device_ms = 0.f;
    st->compared = false;
    st->clustered = false;
    if (n_pairs == 0 || A == 0) return ISX_OK;
    HIP_TRY(hipSetDevice(st->ctx->device));
    hipStream_t s = st->ctx->stream;
    for (Sample &sm : st->samples)
        if ((rc = sort_rows(st, sm))) return rc;

    // the samples as the kernels see them
    std::vector<const uint64_t *> planes((size_t)S);
    std::vector<const CsRow *> rows((size_t)S);
    std::vector<uint32_t> n_rows((size_t)S);
    std::vector<int16_t> lmap((size_t)S * A);
    std::vector<uint8_t> pres((size_t)S * n_scaf * A, 0);
    for (int32_t i = 0; i < S; i++) {
        const Sample &sm = st->samples[(size_t)i];
        planes[(size_t)i] = sm.planes; rows[(size_t)i] = sm.rows; n_rows[(size_t)i] = (uint32_t)sm.n_rows;
        const int L = (int)sm.mm.size();
        for (int a = 0; a < A; a++) {
            const int32_t lv = sm.planes ? map[(size_t)i * ISX_CMPSET_MAX_LEVELS + a] : -1;
            lmap[(size_t)i * A + a] = (int16_t)lv;
            if (lv < 0 || sm.mm[(size_t)lv] != axis[(size_t)a]) continue;       // not one of the sample's own values
            for (int32_t sc = 0; sc < n_scaf; sc++)
                if (sm.have[(size_t)sc]) pres[((size_t)i * n_scaf + sc) * A + a] = sm.present[(size_t)sc * L + lv];
        }
    }
    axis.resize((size_t)A);
    HIP_TRY(st->d_planes.put(planes, s)); HIP_TRY(st->d_rows.put(rows, s)); HIP_TRY(st->d_n_rows.put(n_rows, s));
    HIP_TRY(st->d_lmap.put(lmap, s)); HIP_TRY(st->d_pres.put(pres, s)); HIP_TRY(st->d_spos.put(st->spos, s)); HIP_TRY(st->d_axis.put(axis, s));
    const size_t n_cnt = (size_t)n_out * n_scaf * A, n_snp = (size_t)n_pairs * n_scaf * A;
    HIP_TRY(st->d_cnt.fit(n_cnt)); HIP_TRY(st->d_snp.fit(n_snp * 2)); HIP_TRY(st->d_failed.fit((size_t)n_pairs * n_scaf)); HIP_TRY(st->d_cursor.fit(1));
    HIP_TRY(hipMemsetAsync(st->d_cnt.p, 0, n_cnt * 8, s));
    HIP_TRY(hipMemsetAsync(st->d_snp.p, 0, n_snp * 16, s));
    HIP_TRY(hipMemsetAsync(st->d_failed.p, 0, (size_t)n_pairs * n_scaf * 4, s));
    auto pair_index = [S](int64_t i, int64_t j) { return (uint32_t)(i * (2 * (int64_t)S - i - 1) / 2 + (j - i - 1)); };

    // coverage half: sample blocks I <= J; a diagonal launch also makes its samples' own counts
    const int n_blocks = (S + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK;
    const int rows_max = n_blocks == 1 ? S : 2 * SAMPLE_BLOCK;
    const int tile_words = std::max(1, std::min(TILE_WORDS, LDS_WORDS / rows_max - 1));
    const int64_t n_tiles = isx_cmpset_tiles(n_scaf, st->len.data(), tile_words, nullptr);
    if (n_tiles < 0) return (int)n_tiles;
    if (n_tiles > 0x7FFFFFFFll) { isx_set_error("isx_cmpset_compare: too many tiles for one launch"); return ISX_ERR_CAPACITY; }
    std::vector<isx_cmpset_tile> tiles((size_t)n_tiles);
    (void)isx_cmpset_tiles(n_scaf, st->len.data(), tile_words, tiles.data());
    SetBuf<isx_cmpset_tile> d_tiles;
    SetBuf<int32_t> d_stage;
    SetBuf<CovItem> d_items;
    SetBuf<SnpPair> d_pairs;
    SetBuf<uint64_t> d_cand;
    auto done = [&](int r) { d_tiles.drop(); d_stage.drop(); d_items.drop(); d_pairs.drop(); d_cand.drop(); return r; };
#define CMP_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { isx_set_error(std::string("isx_cmpset_compare: ") + #expr + ": " + hipGetErrorString(_e)); isx_read_drop(); return done(ISX_ERR_HIP); } } while (0)
    CMP_TRY(d_tiles.put(tiles, s));
    // every launch's staged samples and items, uploaded once
    struct Launch { size_t stage0, item0; int n_stage, n_items; };
    std::vector<Launch> launches;
    std::vector<int32_t> stage;
    std::vector<CovItem> items;
    for (int I = 0; I < n_blocks; I++)
        for (int J = I; J < n_blocks; J++) {
            Launch L{stage.size(), items.size(), 0, 0};
            const int a0 = I * SAMPLE_BLOCK, a1 = std::min(S, a0 + SAMPLE_BLOCK), b0 = J * SAMPLE_BLOCK, b1 = std::min(S, b0 + SAMPLE_BLOCK);
            for (int i = a0; i < a1; i++) stage.push_back(i);
            if (J != I) for (int j = b0; j < b1; j++) stage.push_back(j);
            if (I == J) {
                for (int i = a0; i < a1; i++) {
                    items.push_back({(uint16_t)(i - a0), (uint16_t)(i - a0), (uint32_t)(n_pairs + i)});
                    for (int j = i + 1; j < a1; j++) items.push_back({(uint16_t)(i - a0), (uint16_t)(j - a0), pair_index(i, j)});
                }
            } else {
                for (int i = a0; i < a1; i++)
                    for (int j = b0; j < b1; j++) items.push_back({(uint16_t)(i - a0), (uint16_t)(a1 - a0 + j - b0), pair_index(i, j)});
            }
            L.n_stage = (int)(stage.size() - L.stage0); L.n_items = (int)(items.size() - L.item0);
            launches.push_back(L);
        }
    CMP_TRY(d_stage.put(stage, s));
    CMP_TRY(d_items.put(items, s));
    // SNP half: every pair's candidates = the rows of both samples
    std::vector<SnpPair> pairs;
    std::vector<uint64_t> cand_off(1, 0);
    for (int32_t i = 0; i < S; i++)
        for (int32_t j = i + 1; j < S; j++) {
            pairs.push_back({i, j, pair_index(i, j), 0});
            cand_off.push_back(cand_off.back() + n_rows[(size_t)i] + n_rows[(size_t)j]);
        }
    if ((cand_off.back() + 255) / 256 > 0x7FFFFFFFull) { isx_set_error("isx_cmpset_compare: too many SNV rows x pairs for one launch"); return done(ISX_ERR_CAPACITY); }
    CMP_TRY(d_pairs.put(pairs, s));
    CMP_TRY(d_cand.put(cand_off, s));

    CMP_TRY(hipEventRecord(st->ev[0], s));
    for (const Launch &L : launches) {
        const int np = std::min(64, pow2_ceil(L.n_items));
        const size_t lds = (size_t)L.n_stage * (tile_words + 1) * 8;
        hipLaunchKernelGGL(k_cmpset_cov, dim3((unsigned)n_tiles), dim3(256), lds, s, st->d_planes.p, st->d_lmap.p, A, st->n_words,
                           d_stage.p + L.stage0, L.n_stage, d_items.p + L.item0, L.n_items, np, d_tiles.p, tile_words, n_scaf,
                           st->d_cnt.p, (uint32_t)n_out);
    }
    SnpArgs sa{};
    sa.rows = st->d_rows.p; sa.n_rows = st->d_n_rows.p; sa.pairs = d_pairs.p; sa.cand_off = d_cand.p; sa.n_pairs = (int)pairs.size();
    sa.nm = {st->ctx->d_lut, st->ctx->lut_n, st->ctx->fallback, min_freq};
    sa.planes = st->d_planes.p; sa.lmap = st->d_lmap.p; sa.A = A; sa.n_words = st->n_words; sa.spos = st->d_spos.p; sa.n_scaf = n_scaf;
    sa.pres = st->d_pres.p; sa.n_con = st->d_snp.p; sa.n_pop = st->d_snp.p + n_snp; sa.failed = st->d_failed.p; sa.n_out = (uint32_t)n_pairs;
    sa.axis_mm = st->d_axis.p; sa.out_rows = nullptr; sa.cursor = st->d_cursor.p; sa.cap_rows = 0;
    if (cand_off.back())
        hipLaunchKernelGGL(k_cmpset_snp, dim3((unsigned)((cand_off.back() + 255) / 256)), dim3(256), 0, s, sa);
    CMP_TRY(hipEventRecord(st->ev[1], s));
    std::vector<unsigned long long> cnt(n_cnt), snp(n_snp * 2);
    std::vector<uint32_t> failed((size_t)n_pairs * n_scaf);
    CMP_TRY(hipMemcpyAsync(cnt.data(), st->d_cnt.p, n_cnt * 8, hipMemcpyDeviceToHost, s));
    CMP_TRY(hipMemcpyAsync(snp.data(), st->d_snp.p, n_snp * 16, hipMemcpyDeviceToHost, s));
    CMP_TRY(hipMemcpyAsync(failed.data(), st->d_failed.p, failed.size() * 4, hipMemcpyDeviceToHost, s));
    CMP_TRY(isx_wait_stream(s));
    CMP_TRY(hipGetLastError());
#undef CMP_TRY
    if (device_ms) (void)hipEventElapsedTime(device_ms, st->ev[0], st->ev[1]);

    for (const SnpPair &p : pairs)
        for (int32_t sc = 0; sc < n_scaf; sc++) {
            const uint8_t *pa = &pres[((size_t)p.i * n_scaf + sc) * A], *pb = &pres[((size_t)p.j * n_scaf + sc) * A];
            const bool both_have = std::any_of(pa, pa + A, [](uint8_t v) { return v != 0; }) && std::any_of(pb, pb + A, [](uint8_t v) { return v != 0; });
            const bool bad = failed[(size_t)p.out * n_scaf + sc] != 0;
            for (int a = 0; a < A; a++) {
                const size_t o = ((size_t)p.out * n_scaf + sc) * A + a;
                isx_compare_level r;
                memset(&r, 0, sizeof(r));
                r.mm = axis[(size_t)a];
                if (both_have) {
                    const int64_t na = (int64_t)cnt[((size_t)(n_pairs + p.i) * n_scaf + sc) * A + a], nb = (int64_t)cnt[((size_t)(n_pairs + p.j) * n_scaf + sc) * A + a];
                    r.both = (int64_t)cnt[o]; r.either = na + nb - r.both;
                    r.present_a = pa[a]; r.present_b = pb[a];
                    r.consensus_snps = bad ? -2 : (int64_t)snp[o];
                    r.population_snps = bad ? -2 : (int64_t)snp[n_snp + o];
                }
                out[o] = r;
            }
        }
    st->compared = true; st->min_freq = min_freq; st->A = A;
    return done(ISX_OK);
}

int isx_cmpset_pair_snps(isx_cmpset *st, int32_t i, int32_t j, int64_t *n_rows)
{
    if (!st || !n_rows) { isx_set_error("isx_cmpset_pair_snps: bad argument"); return ISX_ERR_ARG; }
    *n_rows = 0;
    st->n_snp_rows = 0;
    if (!st->compared) { isx_set_error("isx_cmpset_pair_snps: call isx_cmpset_compare first (and again after an add)"); return ISX_ERR_STATE; }
    const int32_t S = (int32_t)st->samples.size();
    if (i < 0 || j <= i || j >= S) { isx_set_error("isx_cmpset_pair_snps: a pair is 0 <= i < j < n_samples"); return ISX_ERR_ARG; }
    const uint64_t n_ab = (uint64_t)st->samples[(size_t)i].n_rows + st->samples[(size_t)j].n_rows, cap = n_ab * (uint64_t)st->A;
    if (!n_ab) return ISX_OK;
    if (cap > 0xFFFFFFFFull) { isx_set_error("isx_cmpset_pair_snps: more candidate rows than one call holds"); return ISX_ERR_CAPACITY; }
    HIP_TRY(hipSetDevice(st->ctx->device));
    hipStream_t s = st->ctx->stream;
    const int n_scaf = st->n_scaf, A = st->A;
    SetBuf<SnpPair> d_pair;
    SetBuf<uint64_t> d_cand;
    SetBuf<unsigned long long> d_cnt;
    SetBuf<uint32_t> d_failed;
    const std::vector<SnpPair> h_pair(1, SnpPair{i, j, 0, 0});
    const std::vector<uint64_t> h_cand{0, n_ab};
    auto done = [&](int r) { d_pair.drop(); d_cand.drop(); d_cnt.drop(); d_failed.drop(); return r; };
#define PS_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { isx_set_error(std::string("isx_cmpset_pair_snps: ") + #expr + ": " + hipGetErrorString(_e)); isx_read_drop(); return done(ISX_ERR_HIP); } } while (0)
    PS_TRY(st->snp_rows.fit((size_t)cap));
    PS_TRY(d_pair.put(h_pair, s));
    PS_TRY(d_cand.put(h_cand, s));
    PS_TRY(d_cnt.fit((size_t)n_scaf * A * 2));
    PS_TRY(d_failed.fit((size_t)n_scaf));
    PS_TRY(hipMemsetAsync(d_cnt.p, 0, (size_t)n_scaf * A * 16, s));
    PS_TRY(hipMemsetAsync(d_failed.p, 0, (size_t)n_scaf * 4, s));
    PS_TRY(hipMemsetAsync(st->d_cursor.p, 0, 4, s));
    SnpArgs sa{};
    sa.rows = st->d_rows.p; sa.n_rows = st->d_n_rows.p; sa.pairs = d_pair.p; sa.cand_off = d_cand.p; sa.n_pairs = 1;
    sa.nm = {st->ctx->d_lut, st->ctx->lut_n, st->ctx->fallback, st->min_freq};
    sa.planes = st->d_planes.p; sa.lmap = st->d_lmap.p; sa.A = A; sa.n_words = st->n_words; sa.spos = st->d_spos.p; sa.n_scaf = n_scaf;
    sa.pres = st->d_pres.p; sa.n_con = d_cnt.p; sa.n_pop = d_cnt.p + (size_t)n_scaf * A; sa.failed = d_failed.p; sa.n_out = 1;
    sa.axis_mm = st->d_axis.p; sa.out_rows = st->snp_rows.p; sa.cursor = st->d_cursor.p; sa.cap_rows = (uint32_t)cap;
    hipLaunchKernelGGL(k_cmpset_snp, dim3((unsigned)((n_ab + 255) / 256)), dim3(256), 0, s, sa);
    uint32_t n = 0;
    PS_TRY(hipMemcpyAsync(&n, st->d_cursor.p, 4, hipMemcpyDeviceToHost, s));
    PS_TRY(isx_wait_stream(s));
    PS_TRY(hipGetLastError());
#undef PS_TRY
    st->n_snp_rows = (uint32_t)std::min<uint64_t>(n, cap);
    *n_rows = st->n_snp_rows;
    return done(ISX_OK);
}

int isx_cmpset_fetch_snps(isx_cmpset *st, isx_compare_snp *out)
{
    if (!st || !out) { isx_set_error("isx_cmpset_fetch_snps: bad argument"); return ISX_ERR_ARG; }
    const size_t n = st->n_snp_rows;
    if (!n) return ISX_OK;
    HIP_TRY(hipSetDevice(st->ctx->device));
    HIP_TRY(hipMemcpy(out, st->snp_rows.p, n * sizeof(isx_compare_snp), hipMemcpyDeviceToHost));
    std::sort(out, out + n, [](const isx_compare_snp &x, const isx_compare_snp &y) {
        return x.mm != y.mm ? x.mm < y.mm : x.gpos < y.gpos;
    });
    return ISX_OK;
}

}  // extern "C"
