// isx_compare_set.h -- the comparison set behind isx_cmpset_*, shared by isx_compare_set.hip (sketches, the pair pass) and
// isx_compare_pool.hip (SNV pooling over the same position space)
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "isx_batch.h"

namespace isxset {

struct CsRow {                          // what the SNP half reads of an isx_snv
    uint32_t gpos;                      // set position
    uint8_t con_base, ref_base, var_base, allele_count;
    uint32_t cnt[4];
};

struct PoolRow {                        // what pooling reads of an isx_snv: the highest-mm row of a position that is not cryptic
    uint32_t gpos;                      // set position
    uint8_t con_base, ref_base, cls, pad;
    uint32_t cnt[4];
};
static_assert(sizeof(PoolRow) == 24, "PoolRow is 24 bytes");
enum : uint8_t { PULL_NONE = 0, PULL_DONE = 1, PULL_OBS = 2 };     // Sample::pulled

struct PackJob {                        // one batch scaffold that the set names: its words as a run of the call's job words
    int64_t jw0;                        // first job word (ascending; a sentinel entry closes the list)
    int64_t dst_w0, src0, len;          // first word in the set, first position in the batch, positions
};

struct ProfTile {                       // one workgroup of k_profile_planes: at most 64 words = 4096 positions of ONE scaffold of the call
    int64_t word0;                      // first word in the set
    int32_t n_words, scaf;              // words of the tile; the scaffold's index in the call
    uint32_t pos0, len;                 // first position of the tile on the scaffold; the scaffold's length
};

struct Sample {
    std::vector<int32_t> mm;            // real mm of every own level (fixed by the first batch)
    uint64_t *planes = nullptr;         // [levels][n_words]
    std::vector<uint8_t> have;          // [n_scaf] the scaffold has been added
    std::vector<uint8_t> present;       // [n_scaf][levels]
    CsRow *rows = nullptr;
    size_t n_rows = 0, cap_rows = 0;
    bool sorted = true;                 // rows ascend (every batch so far brought higher scaffolds than the ones before)
    int32_t max_sid = -1;
    // pooling (isx_cmpset_pool_enable)
    PoolRow *prows = nullptr;
    size_t n_prows = 0, cap_prows = 0;
    bool psorted = true;
    std::vector<uint8_t> pulled;        // [n_scaf] since the last isx_cmpset_pool_sites: PULL_DONE isx_cmpset_pool_add has brought the scaffold /
                                        // isx_cmpset_pool_obs_done has closed it, PULL_OBS isx_cmpset_pool_add_obs has brought observations of it
    std::vector<int64_t> to_pull;       // [n_scaf] sites of the scaffold the sample does not own
};

template <class T>
struct SetBuf {                         // a device array that lives as long as its owner says
    T *p = nullptr;
    size_t cap = 0;
    hipError_t fit(size_t n)
    {
        if (p && cap >= n) return hipSuccess;
        drop();
        const hipError_t e = isx_raw_dev_malloc(&p, std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) cap = std::max<size_t>(n, 1);
        return e;
    }
    hipError_t put(const std::vector<T> &h, hipStream_t s)
    {
        hipError_t e = fit(h.size());
        if (e == hipSuccess && !h.empty()) e = hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s);
        return e;
    }
    void drop() { if (p) isx_dev_free(p); p = nullptr; cap = 0; }
};

// bounds[lo] <= g < bounds[hi]
__device__ __forceinline__ int seg_of(const int64_t *bounds, int n_seg, int64_t g)
{
    int lo = 0, hi = n_seg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (bounds[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace isxset

struct isx_cmpset {
    isx_ctx *ctx = nullptr;
    int32_t min_cov = 5, n_scaf = 0;
    std::vector<int64_t> len, woff, spos;   // lengths; first word of every scaffold + total; the same in positions
    int64_t n_words = 0;
    std::vector<isxset::Sample> samples;
    hipEvent_t ev[2] = {nullptr, nullptr};
    // scratch of isx_cmpset_add
    isxset::SetBuf<uint32_t> cov, present, idx, idx_in, flags, pos;
    isxset::SetBuf<float> scratch_f;
    isxset::SetBuf<int64_t> bbounds, set_pos0;
    isxset::SetBuf<uint8_t> acc, temp;
    isxset::SetBuf<isxset::PackJob> jobs;
    isxset::SetBuf<uint64_t> keys, keys_in;
    // scratch of isx_cmpset_add_profile: the call's covT series (CSR offsets, index, value), its tiles and its SNV rows
    isxset::SetBuf<int64_t> pf_off;
    isxset::SetBuf<uint32_t> pf_pos, pf_val;
    isxset::SetBuf<isxset::ProfTile> pf_tiles;
    isxset::SetBuf<isx_profile_snv> pf_snv;
    isxset::SetBuf<uint8_t> pf_flags;               // isx_cmpset_add_profile_pool: class / cryptic of every row of pf_snv
    // what the last isx_cmpset_compare left for isx_cmpset_pair_snps
    bool compared = false;
    double min_freq = 0.05;
    int32_t A = 0;
    isxset::SetBuf<const uint64_t *> d_planes;
    isxset::SetBuf<const isxset::CsRow *> d_rows;
    isxset::SetBuf<uint32_t> d_n_rows, d_failed, d_cursor;
    isxset::SetBuf<int16_t> d_lmap;
    isxset::SetBuf<uint8_t> d_pres;
    isxset::SetBuf<int64_t> d_spos;
    isxset::SetBuf<int32_t> d_axis;
    isxset::SetBuf<unsigned long long> d_cnt, d_snp;
    isxset::SetBuf<isx_compare_snp> snp_rows;
    uint32_t n_snp_rows = 0;
    // SNV pooling (isx_compare_pool.hip).  pool_on: isx_cmpset_add keeps pool rows; pooled: isx_cmpset_pool_sites has run since the last add
    bool pool_on = false, pooled = false;
    int64_t n_sites = 0;
    std::vector<uint8_t> p_has, p_pooled;           // [samples][n_scaf] the sample has the scaffold; [n_scaf] >= 2 samples have it
    std::vector<uint32_t> p_srank;                  // [n_scaf + 1] rank of every scaffold's first site, then n_sites
    isxset::SetBuf<uint64_t> site_plane;            // [n_words] one bit per set position: a site
    isxset::SetBuf<uint32_t> word_rank, word_pop;   // [n_words + 1] sites before the word; the scan's input
    isxset::SetBuf<uint32_t> site_gpos;             // [n_sites] ascending
    isxset::SetBuf<uint8_t> site_ref;               // [n_sites] ref_base of the own rows
    isxset::SetBuf<uint4> p_counts;                 // [samples][n_sites] A C T G
    isxset::SetBuf<uint8_t> p_meta;                 // [samples][n_sites] bit 0 has the scaffold, 1 owns the site, 2..4 cls, 5..6 con_base
    isxset::SetBuf<uint8_t> d_phas, d_ppooled;
    isxset::SetBuf<int64_t> d_pspos;                // [n_scaf + 1]
    isxset::SetBuf<int64_t> d_pwoff;                // [n_scaf + 1]
    isxset::SetBuf<uint32_t> d_srank, d_own;        // [n_scaf + 1]; [samples][n_scaf] own rows
    isxset::SetBuf<isx_pool_site> d_psum;
    isxset::SetBuf<isx_obs> obs_stage;              // scratch of isx_cmpset_pool_add_obs: the call's observations, its regions' offsets
    isxset::SetBuf<int64_t> obs_roff, obs_rbase;    // [n_regions + 1]; [n_regions] set position of the region's gpos 0 (OBS_SKIP: skipped)
    // strain clustering (isx_cluster.hip).  clustered: isx_cmpset_cluster has run since the last add / compare
    bool clustered = false;
    int64_t cl_P = 0;
    std::vector<isx_cluster_status> cl_status;      // [genomes of the call]
    isxset::SetBuf<isx_genome_pair> d_gpairs;       // [genomes][pairs] the roll-up
    isxset::SetBuf<double> d_clZ;                   // [genomes][samples - 1][4]
};

// isx_compare_set.hip, for isx_compare_pool.hip
namespace isxset {
// the host-side checks of a batch handed to the set (`who` heads the error text): ISX_OK or the code, text set
int cmpset_check_batch(const char *who, const isx_cmpset *st, int32_t sample, const isx_batch *b, int32_t n_bscaf, const int64_t *bb,
                       const int32_t *ids);
int cmpset_grow_temp(isx_cmpset *st, size_t bytes);
void cmpset_pool_drop(isx_cmpset *st);          // isx_compare_pool.hip: frees every pooling array of the set (not the samples' pool rows)
int cmpset_sort_pool_rows(isx_cmpset *st, Sample &sm);
void cmpset_cluster_drop(isx_cmpset *st);       // isx_cluster.hip: frees what the last isx_cmpset_cluster left
}
