// isx_summary.h -- host-side interface of the per-scaffold summary pass (isx_summary.hip)
#pragma once
#include <functional>
#include <vector>

#include "isx_internal.h"

struct SummaryBuffers {
    uint32_t *cov = nullptr;        // cumulative coverage over levels <= mm, per flat position
    float *cv = nullptr, *cr = nullptr;     // clonality / rarefied clonality of the highest level <= mm
    uint32_t *k_u32 = nullptr;
    float *k_f32 = nullptr;
    uint32_t *seg_off = nullptr, *seg_be = nullptr;
    int64_t *bounds = nullptr;
    void *acc = nullptr;
    double *med = nullptr;
    isx_scaffold_level *rows = nullptr;
    void *temp = nullptr;
    size_t temp_bytes = 0;
    int n_seg = -1;
    size_t cap_pos = 0;             // positions the position-sized arrays hold (a pipe slot sees batches of different sizes)
    void release();
    void fit_positions(size_t n_pos);
};

// sparse source (isx_stored.hip): a stored profile's covT / clonT / clonTR as level-major CSRs on the device, one (flat position,
// value) pair per entry -- coverage as uint32, clonalities as float bits -- so that a lane loads an entry with one 8-byte read.
// Table t (0 covT, 1 clonT, 2 clonTR) has the entries [off[t][mm], off[t][mm + 1]) at level mm, ordered by flat position.
struct SparseLevels {
    const uint2 *pairs[3];          // device; NULL: the profile has no such table
    const int64_t *off[3];          // host, [M + 1]
    const uint8_t *cov_present;     // device, [n_scaffolds][M]: the level is a key of the scaffold's covT
};

struct SummaryIn {
    hipStream_t stream;
    hipEvent_t *ev;                 // 2 events
    uint32_t n_pos;
    int n_scaffolds, M;
    const int64_t *scaffold_bounds; // host, [n_scaffolds + 1]
    // dense path
    const uint4 *counts;            // NULL: a pipe slot without a count table -> cov16 + the exact values of saturated positions
    const uint16_t *cov16;
    const uint2 *sat;
    uint32_t n_sat;
    const float *clon, *clon_r;
    // mm path
    const isx_entry *entries;
    const uint32_t *win_nent;
    uint32_t slab, n_win, n_ovf;
    uint64_t ovf0;
    // sparse path (not NULL: the source, whatever M is)
    const SparseLevels *sparse;
};

// (position, value) pairs ordered by position: a 32-bit radix sort of the 8-byte entries on their low word; *temp grows on demand
int sort_pairs_by_position(hipStream_t s, const uint2 *in, uint2 *out, size_t n, void **temp, size_t *temp_bytes);

int run_summary(const SummaryIn &in, SummaryBuffers &B, isx_scaffold_level *host_out, float *ms);
int run_genome_summary(const SummaryIn &in, SummaryBuffers &B, int n_genomes, const int32_t *genome_first, int mask_edges,
                       isx_genome_level *host_out, float *ms);

struct CompareBuffers {
    uint32_t *cov_a = nullptr, *cov_b = nullptr;
    float *scratch_f = nullptr;
    int64_t *bounds = nullptr;
    void *acc_a = nullptr, *acc_b = nullptr;
    unsigned long long *both = nullptr;     // [4 * n_seg]: both, either, consensus SNPs, population SNPs
    isx_compare_level *rows = nullptr;
    // SNP-table half (readComparer.py:205-290)
    uint64_t *keys = nullptr;               // [4 * cap_snv]: sorted A, sorted B, 2 x sort input
    uint32_t *idx = nullptr;                // same layout
    void *cand = nullptr;                   // candidate rows (mm independent verdicts)
    isx_compare_snp *snp_rows = nullptr;    // emitted (position, mm) rows
    uint32_t *cursors = nullptr;            // [0] n_cand, [1] n_snp_rows, [2..2+n_seg) scaffold failed
    void *temp = nullptr;
    size_t temp_bytes = 0;
    size_t cap_pos = 0, cap_seg = 0, cap_rows = 0, cap_snv = 0, cap_snp_rows = 0;
    uint32_t n_snp_rows = 0;                // rows of the last isx_compare_scaffolds
    void release();
};

struct CompareSnpIn {                       // nullptr lut = coverage half only
    const uint8_t *lut = nullptr;           // 255 = coverage not in the null model -> fallback
    int32_t lut_n = 0, fallback = 0;
    double min_freq = 0.05;
    const isx_snv *snv_a = nullptr, *snv_b = nullptr;
    uint32_t n_a = 0, n_b = 0;
};

int run_compare(const SummaryIn &a, const SummaryIn &b, uint32_t min_cov, const CompareSnpIn &snp, CompareBuffers &B,
                isx_compare_level *host_out, float *ms);

// One level of what run_compare materialises, for the comparison set (isx_compare_set.hip): level `mm` of `in` applied onto cov[n_pos]
// (zeroed by the caller before level 0; f0 / f1: 2 x n_pos floats of scratch), the level's Acc.present of every scaffold of
// in.scaffold_bounds (on the device: d_bounds) into present_out[n_scaffolds].  acc_scratch: level_acc_bytes(n_scaffolds) device bytes.
size_t level_acc_bytes(int n_seg);
void launch_level_cumulate(const SummaryIn &in, int mm, uint32_t *cov, float *f0, float *f1, const int64_t *d_bounds, void *acc_scratch,
                           uint32_t *present_out);

// the mm path's entry table (window slabs + overflow) compacted and ordered by (gpos, mm) on the device, then brought to
// host_out: by one hipMemcpyAsync, or by `copier` (device source, host destination, bytes, stream) when the caller has a
// faster way to pageable memory (a pipe's pinned staging + its host threads)
typedef std::function<int(const void *, void *, size_t, hipStream_t)> EntryCopier;
// soa != NULL: the shrunk hand-back instead (isx_pipe_fetch_entries_shrunk): four host columns of n_entries 4-byte values
struct EntrySoa { uint32_t *gpos, *mm_cov; float *clon, *clon_rarefied; };
int fetch_entries_sorted(hipStream_t s, const isx_entry *entries, const uint32_t *win_nent, uint32_t slab, uint32_t n_win,
                         uint32_t n_ovf, uint64_t n_entries, isx_entry *host_out, const EntryCopier *copier = nullptr,
                         const EntrySoa *soa = nullptr);

// ---- gene profiling (isx_genes.hip; GeneProfile.py:304-707) ----
struct isx_genes {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    std::vector<isx_gene> h;            // the set as the caller gave it
    isx_gene *d = nullptr;
    uint8_t *d_seq = nullptr;           // the letters as codes 0..4 (A C G T N), gene orientation
    int64_t seq_bytes = 0;
};

// one gene of a call: its interval in the call's flat space, clipped to its scaffold (fe < fs: nothing of it lies inside)
struct GeneWork {
    uint32_t fs, fe;                    // inclusive
    int32_t gene;                       // index in the set
    int32_t scaf;                       // index among the call's scaffolds
};

// the call's genes in call order (scaffold by scaffold, set order inside one), with the checks every gene entry point makes
int genes_build_work(const isx_genes *g, int32_t n_scaffolds, const int64_t *bounds, const int32_t *first, const int32_t *last,
                     std::vector<GeneWork> &work);
// one level of the coverage half: rows[w * M + mm] for every call gene w (isx_genes.hip)
void launch_gene_cov(hipStream_t s, const GeneWork *work, uint32_t n_work, const uint32_t *cov, const float *cv, int M, int mm,
                     isx_gene_cov *rows);
// ISX_GENE_COV_ANY / ISX_GENE_CLON_ANY of every scaffold for the current level into flags[n_seg] (zeroed by the caller)
void launch_scaffold_any(hipStream_t s, const uint32_t *cov, const float *cv, uint32_t n_pos, const int64_t *bounds, int n_seg,
                         uint32_t *flags);
int run_gene_cov(const SummaryIn &in, SummaryBuffers &B, const std::vector<GeneWork> &work, isx_gene_cov *host_out,
                 uint8_t *flags_out, float *ms);
int run_gene_snvs(isx_genes *g, int32_t n_scaffolds, const int64_t *bounds, const std::vector<GeneWork> &work, int64_t n_snv,
                  const isx_snv *snv, int32_t n_levels, isx_gene_mutation *mut_out, isx_gene_snv_count *cnt_out, float *ms);
int run_gene_sites(isx_genes *g, double *sites, float *ms);

// ---- genome_info roll-ups (isx_genomes.hip; genomeUtilities.py:145-269) ----
// one level of the masked coverage distribution: acc / hist point at that level of genome 0, consecutive genomes lie acc_stride rows /
// hist_stride words apart (both zeroed by the caller)
void launch_genome_hist(hipStream_t s, const uint32_t *cov, uint32_t n_pos, const int64_t *sbounds, const int32_t *sgen, int n_scaf,
                        int mask_edges, int hist_bins, isx_genome_cov *acc, size_t acc_stride, uint32_t *hist, size_t hist_stride);
int run_genome_cov(const SummaryIn &in, SummaryBuffers &B, const int32_t *scaffold_genome, int n_genomes, int mask_edges, int hist_bins,
                   isx_genome_cov *acc_out, uint32_t *hist_out, float *ms);
int run_snv_levels(int device, hipStream_t s, int32_t n_scaffolds, const int64_t *scaffold_bounds, int64_t n_snv, const isx_snv *snv,
                   int32_t n_levels, isx_snv_level *out, float *device_ms);
// iRep's block sums of one batch (isx_irep_add): the coverage cumulated up to `level` (materialised as run_genome_cov does; -1: no
// coverage, G+C counts only) and the batch's resident reference, added into the set's block arrays.  scaffold_base[n_scaffolds] (host):
// where every batch scaffold's first unmasked position lies in the block space, -1 = adds nothing
struct IrepAdd {
    const int64_t *scaffold_base;
    int level, mask_edges;
    const uint8_t *ref, *ref_n;
    int ref_packed;
    uint64_t *block_cov;
    uint32_t *block_gc;
};
void launch_irep_blocks(hipStream_t s, const uint32_t *cov, uint32_t n_pos, const int64_t *sbounds, const int64_t *sbase, int n_scaf,
                        int mask_edges, const uint8_t *ref, int ref_packed, const uint8_t *ref_n, uint64_t *block_cov, uint32_t *block_gc);
int run_irep_add(const SummaryIn &in, SummaryBuffers &B, const IrepAdd &a, float *ms);
// ---- a stored profile's level series resident on the device (isx_stored.hip): the third source of the passes above ----
struct isx_stored {
    isx_ctx *ctx = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    int32_t n_scaf = 0, M = 0;
    std::vector<int64_t> bounds;        // [n_scaf + 1]
    std::vector<int64_t> off[3];        // covT, clonT, clonTR: [M + 1], empty = no such table
    uint2 *d_pairs[3] = {nullptr, nullptr, nullptr};
    uint8_t *d_present = nullptr;       // cov_present
    uint8_t *d_ref = nullptr;           // base codes 0..4 per flat position, or NULL
    SparseLevels view{};
    SummaryBuffers S;
};
void stored_summary_in(isx_stored *st, SummaryIn &in);

int run_ld_levels(int device, hipStream_t s, int32_t n_scaffolds, const int64_t *scaffold_bounds, int64_t n_ld, const isx_ld *ld,
                  int32_t n_levels, isx_ld_level *out, float *device_ms);
