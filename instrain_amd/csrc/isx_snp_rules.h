// isx_snp_rules.h -- the SNP rules of `inStrain compare` (readComparer.py:292-367), said once for every kernel that judges a
// position: k_snp_candidates / k_snp_apply on two resident batches (isx_summary.hip) and k_cmpset_snp on the sample set's last-row
// tables (isx_compare_set.hip).  Device-inline and without state.  Row: isx_snv or isxset::CsRow -- any type with con_base, ref_base,
// var_base, allele_count and cnt[4] (A C T G).
#pragma once
#include "isx_internal.h"

namespace isxsnp {

struct NullModel {                      // the ctx's null model and compare's --min_freq, as is_present reads them
    const uint8_t *lut;
    int32_t lut_n, fallback;
    double min_freq;
};

enum : uint32_t {
    SNP_CON = 1u,                       // consensus_SNP
    SNP_POP = 2u,                       // population_SNP
    SNP_REF_FAILS = 4u                  // a one-sided row with reference base N: the reference fails on the whole scaffold
};

// readComparer.py:306-315 is_present
__device__ __forceinline__ bool is_present(uint32_t count, uint32_t total, const NullModel &nm)
{
    int32_t min_bases = nm.fallback;
    if (total < (uint32_t)nm.lut_n && nm.lut[total] != 255) min_bases = nm.lut[total];
    return (int64_t)count >= (int64_t)min_bases && ((double)count / (double)total) >= nm.min_freq;
}

// The verdict on one position: x is the highest-mm row of one sample, y that of the other sample or NULL when it has none (its
// columns are NaN in the reference).  -> SNP_CON | SNP_POP, 0 when the position is no SNP ("Only keep SNPs" :281 is the caller's),
// or SNP_REF_FAILS.
template <class Row>
__device__ __forceinline__ uint32_t snp_verdict(const Row &x, const Row *y, const NullModel &nm)
{
    bool con, pop;
    const uint32_t tx = x.cnt[0] + x.cnt[1] + x.cnt[2] + x.cnt[3];
    if (!y) {                           // the row exists in one sample only
        con = x.con_base != x.ref_base;                                     // call_con_snps :296-301
        if (x.ref_base > 3) return SNP_REF_FAILS;                           // '{ref_base}_2' with ref_base N: the reference raises KeyError
        pop = !is_present(x.cnt[x.ref_base], tx, nm);                       // call_pop_snps :329-344
    } else {
        con = x.con_base != y->con_base;                                    // :304
        const uint32_t ty = y->cnt[0] + y->cnt[1] + y->cnt[2] + y->cnt[3];
        if (!con) pop = false;                                                                          // :325
        else if (is_present(y->cnt[x.con_base & 3], ty, nm)) pop = false;                               // :349-355
        else if (is_present(x.cnt[y->con_base & 3], tx, nm)) pop = false;                               // :358-361
        else if (x.allele_count > 1 && y->allele_count > 1 && x.var_base == y->var_base) pop = false;   // :364-367
        else pop = true;
    }
    return (con ? SNP_CON : 0u) | (pop ? SNP_POP : 0u);
}

// one sample's columns of a mismatch row (readComparer.py:221-225 OUT_COLUMNS): SIDE_B false = has_a / con_a / ..., true = the _b twin
template <bool SIDE_B, class Row>
__device__ __forceinline__ void snp_fill_side(isx_compare_snp &r, const Row &x)
{
    (SIDE_B ? r.has_b : r.has_a) = 1;
    (SIDE_B ? r.con_b : r.con_a) = x.con_base;
    (SIDE_B ? r.ref_b : r.ref_a) = x.ref_base;
    (SIDE_B ? r.var_b : r.var_a) = x.var_base;
    uint32_t *cnt = SIDE_B ? r.cnt_b : r.cnt_a;
    for (int k = 0; k < 4; k++) cnt[k] = x.cnt[k];
}

}  // namespace isxsnp
