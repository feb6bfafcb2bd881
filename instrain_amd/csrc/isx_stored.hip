// isx_stored.hip -- a stored profile's covT / clonT / clonTR on the device (include/instrain_amd.h isx_stored_*).
//
// The reference reads these tables back from raw_data/*.hd5 for
//   calculate_gene_metrics          inStrain/GeneProfile.py:304-422   (profile_genes -i IS)
//   genomeLevel_from_IS             inStrain/genomeUtilities.py:145-269 (genome_wide -i IS)
// one pandas Series per (scaffold, mm).  Here the series of a chunk of scaffolds lie level-major over one flat space, and every
// position-sized pass is the one a live batch runs (isx_summary.hip run_summary / run_gene_cov / run_genome_cov / run_irep_add) with
// its third source, k_level_sparse.  This file is the host side: the checks, the upload, the entry points.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "isx_batch.h"

namespace {

constexpr int MAX_LEVELS = 128;

int bad(const std::string &msg, int code = ISX_ERR_ARG)
{
    isx_set_error("isx_stored_create: " + msg);
    return code;
}

// one table of the pack: offsets ascend from 0; inside a level positions ascend strictly below n_pos and lie on scaffolds that have the key
int check_table(const char *name, int32_t n_scaf, const int64_t *bounds, int32_t M, const uint8_t *present, const int64_t *off,
                const uint32_t *gpos, bool have_values)
{
    const std::string nm(name);
    if (off[0] != 0) return bad(nm + "_offsets must start at 0");
    for (int k = 0; k < M; k++)
        if (off[k + 1] < off[k]) return bad(nm + "_offsets must ascend (level " + std::to_string(k) + ")");
    if (off[M] > 0 && (!gpos || !have_values)) return bad(nm + "_gpos / " + nm + "_values are NULL with " + std::to_string(off[M]) + " entries");
    const int64_t n_pos = bounds[n_scaf];
    for (int k = 0; k < M; k++) {
        int s = 0;
        for (int64_t i = off[k]; i < off[k + 1]; i++) {
            const int64_t g = gpos[i];
            if (g >= n_pos) return bad(nm + "_gpos[" + std::to_string(i) + "] = " + std::to_string(g) + " lies beyond the flat space (" + std::to_string(n_pos) + " positions)");
            if (i > off[k] && g <= (int64_t)gpos[i - 1])
                return bad(nm + "_gpos must ascend strictly inside a level (entry " + std::to_string(i) + " of level " + std::to_string(k) + ")");
            while (bounds[s + 1] <= g) s++;
            if (present && !present[(size_t)s * M + k])
                return bad(nm + "_gpos[" + std::to_string(i) + "]: scaffold " + std::to_string(s) + " has a series at level " + std::to_string(k) +
                           " but " + nm + "_present says the level is no key of it");
        }
    }
    return ISX_OK;
}

int check_clonalities(const char *name, const float *v, int64_t n)
{
    for (int64_t i = 0; i < n; i++)
        if (!(std::isfinite(v[i]) && v[i] > 0.0f && v[i] <= 1.0f))
            return bad(std::string(name) + "_values[" + std::to_string(i) + "] is not a finite clonality in (0, 1]");
    return ISX_OK;
}

}  // namespace

void stored_summary_in(isx_stored *st, SummaryIn &in)
{
    in.stream = st->stream; in.ev = st->ev;
    in.n_pos = (uint32_t)st->bounds.back(); in.n_scaffolds = st->n_scaf; in.M = st->M;
    in.scaffold_bounds = st->bounds.data();
    in.sparse = &st->view;
}

extern "C" {

int isx_stored_create(isx_ctx *ctx, int32_t n_scaf, const int64_t *bounds, int32_t M, const uint8_t *cov_present, const uint8_t *clon_present,
                      const int64_t *cov_off, const uint32_t *cov_gpos, const uint32_t *cov_val,
                      const int64_t *clon_off, const uint32_t *clon_gpos, const float *clon_val,
                      const int64_t *clonr_off, const uint32_t *clonr_gpos, const float *clonr_val,
                      const uint8_t *ref_codes, isx_stored **out)
{
    if (!out) return bad("out is NULL");
    *out = nullptr;
    if (!ctx) return bad("ctx is NULL (a context needs a gfx950 device: there is no CPU path)");
    if (n_scaf <= 0 || !bounds || bounds[0] != 0) return bad("scaffold_bounds must span [0, n_pos]");
    for (int i = 0; i < n_scaf; i++)
        if (bounds[i + 1] <= bounds[i]) return bad("scaffold_bounds must be strictly ascending");
    if (bounds[n_scaf] > (int64_t)0xFFFFFFFFll) return bad("scaffold_bounds: flat space beyond 2^32 positions");
    if (M < 1) return bad("n_levels must be at least 1");
    if (M > MAX_LEVELS) return bad("n_levels = " + std::to_string(M) + ", at most " + std::to_string(MAX_LEVELS) + " levels fit one object", ISX_ERR_CAPACITY);
    if (!cov_present) return bad("cov_present is NULL");
    if (!cov_off) return bad("cov_offsets is NULL");
    if (clon_off && !clon_present) return bad("clon_present is NULL with a clonT");
    int rc;
    if ((rc = check_table("cov", n_scaf, bounds, M, cov_present, cov_off, cov_gpos, cov_val != nullptr))) return rc;
    if (clon_off && ((rc = check_table("clon", n_scaf, bounds, M, clon_present, clon_off, clon_gpos, clon_val != nullptr)) ||
                     (rc = check_clonalities("clon", clon_val, clon_off[M])))) return rc;
    if (clonr_off && ((rc = check_table("clonr", n_scaf, bounds, M, nullptr, clonr_off, clonr_gpos, clonr_val != nullptr)) ||
                      (rc = check_clonalities("clonr", clonr_val, clonr_off[M])))) return rc;
    const int64_t n_pos = bounds[n_scaf];
    if (ref_codes)
        for (int64_t p = 0; p < n_pos; p++)
            if (ref_codes[p] > 4) return bad("ref_codes[" + std::to_string(p) + "] is no base code 0..4");

    // (position, value) pairs: what a lane of k_level_sparse loads in one piece
    const int64_t *offs[3] = {cov_off, clon_off, clonr_off};
    const uint32_t *gp[3] = {cov_gpos, clon_gpos, clonr_gpos};
    const void *vals[3] = {cov_val, clon_val, clonr_val};
    HIP_TRY(hipSetDevice(ctx->device));
    isx_stored *st = new isx_stored();
    st->ctx = ctx; st->device = ctx->device; st->n_scaf = n_scaf; st->M = M;
    st->bounds.assign(bounds, bounds + n_scaf + 1);
    hipError_t e = hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&st->ev[0]);
    if (e == hipSuccess) e = hipEventCreate(&st->ev[1]);
    std::vector<uint2> host[3];
    for (int t = 0; t < 3 && e == hipSuccess; t++) {
        if (!offs[t]) continue;
        st->off[t].assign(offs[t], offs[t] + M + 1);
        const size_t n = (size_t)offs[t][M];
        host[t].resize(n);
        const uint32_t *v = static_cast<const uint32_t *>(vals[t]);     // float bits travel as they are
        for (size_t i = 0; i < n; i++) host[t][i] = make_uint2(gp[t][i], v[i]);
        e = isx_raw_dev_malloc(&st->d_pairs[t], std::max<size_t>(n, 1) * sizeof(uint2));
        if (e == hipSuccess && n) e = hipMemcpyAsync(st->d_pairs[t], host[t].data(), n * sizeof(uint2), hipMemcpyHostToDevice, st->stream);
    }
    if (e == hipSuccess) e = isx_raw_dev_malloc(&st->d_present, (size_t)n_scaf * M);
    if (e == hipSuccess) e = hipMemcpyAsync(st->d_present, cov_present, (size_t)n_scaf * M, hipMemcpyHostToDevice, st->stream);
    if (e == hipSuccess && ref_codes) {
        e = isx_raw_dev_malloc(&st->d_ref, (size_t)n_pos);
        if (e == hipSuccess) e = hipMemcpyAsync(st->d_ref, ref_codes, (size_t)n_pos, hipMemcpyHostToDevice, st->stream);
    }
    if (e == hipSuccess) e = isx_wait_stream(st->stream);
    if (e != hipSuccess) {
        isx_set_error(std::string("isx_stored_create: ") + hipGetErrorString(e));
        isx_stored_destroy(st);
        return ISX_ERR_HIP;
    }
    for (int t = 0; t < 3; t++) {
        st->view.pairs[t] = st->d_pairs[t];
        st->view.off[t] = st->off[t].empty() ? nullptr : st->off[t].data();
    }
    st->view.cov_present = st->d_present;
    *out = st;
    return ISX_OK;
}

void isx_stored_destroy(isx_stored *st)
{
    if (!st) return;
    (void)hipSetDevice(st->device);
    if (st->stream) (void)isx_wait_stream(st->stream);
    st->S.release();
    for (uint2 *p : st->d_pairs) if (p) isx_dev_free(p);
    if (st->d_present) isx_dev_free(st->d_present);
    if (st->d_ref) isx_dev_free(st->d_ref);
    for (hipEvent_t e : st->ev) if (e) (void)hipEventDestroy(e);
    if (st->stream) (void)hipStreamDestroy(st->stream);
    delete st;
}

int isx_stored_summarize(isx_stored *st, isx_scaffold_level *out, float *device_ms)
{
    if (!st || !out) { isx_set_error("isx_stored_summarize: bad argument"); return ISX_ERR_ARG; }
    HIP_TRY(hipSetDevice(st->device));
    SummaryIn in{};
    stored_summary_in(st, in);
    return run_summary(in, st->S, out, device_ms);
}

int isx_stored_genome_coverage(isx_stored *st, const int32_t *scaffold_genome, int32_t n_genomes, int32_t mask_edges, int32_t hist_bins,
                               isx_genome_cov *acc, uint32_t *hist, float *device_ms)
{
    if (!st || !acc || !hist || !scaffold_genome || n_genomes <= 0 || mask_edges < 0 || hist_bins < 2) {
        isx_set_error("isx_stored_genome_coverage: n_genomes > 0, mask_edges >= 0, hist_bins >= 2");
        return ISX_ERR_ARG;
    }
    for (int i = 0; i < st->n_scaf; i++)
        if (scaffold_genome[i] < -1 || scaffold_genome[i] >= n_genomes) {
            isx_set_error("isx_stored_genome_coverage: genome of scaffold " + std::to_string(i) + " outside [-1, n_genomes)");
            return ISX_ERR_ARG;
        }
    HIP_TRY(hipSetDevice(st->device));
    SummaryIn in{};
    stored_summary_in(st, in);
    return run_genome_cov(in, st->S, scaffold_genome, n_genomes, mask_edges, hist_bins, acc, hist, device_ms);
}

int isx_stored_profile_genes(isx_stored *st, isx_genes *g, const int32_t *gene_first, const int32_t *gene_last, isx_gene_cov *cov_out,
                             uint8_t *scaffold_flags, float *device_ms)
{
    if (!st || !scaffold_flags) { isx_set_error("isx_stored_profile_genes: bad argument"); return ISX_ERR_ARG; }
    if (!g || g->device != st->device) { isx_set_error("isx_stored_profile_genes: the gene set belongs to another device"); return ISX_ERR_ARG; }
    std::vector<GeneWork> work;
    const int rc = genes_build_work(g, st->n_scaf, st->bounds.data(), gene_first, gene_last, work);
    if (rc) return rc;
    if (!work.empty() && !cov_out) { isx_set_error("isx_stored_profile_genes: bad argument"); return ISX_ERR_ARG; }
    HIP_TRY(hipSetDevice(st->device));
    SummaryIn in{};
    stored_summary_in(st, in);
    return run_gene_cov(in, st->S, work, cov_out, scaffold_flags, device_ms);
}

}  // extern "C"
