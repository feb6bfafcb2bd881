// irep_layout.cpp -- the iRep accumulator's host-side geometry (include/instrain_amd.h isx_irep_layout): every genome's scaffold
// order, its masked concatenated length, its blocks and windows, and where every scaffold's first unmasked position lies in its
// genome's array (genomeUtilities.py:312-313, 932-981).  Plain host code: callable without a device.
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/instrain_amd.h"

void isx_set_error(const std::string &msg);

// the block scheme: a window is a whole number of blocks
static_assert(ISX_IREP_WINDOW % ISX_IREP_SLIDE == 0, "iRep's slide must divide its window");

extern "C" {

int isx_irep_layout(int32_t n_scaffolds, const int64_t *scaffold_lengths, const int32_t *scaffold_genome, int32_t n_genomes,
                    int32_t mask_edges, isx_irep_genome *genomes, int32_t *order, int64_t *scaffold_offset)
{
    if (n_scaffolds <= 0 || !scaffold_lengths || !scaffold_genome || n_genomes <= 0 || mask_edges < 0 || !genomes || !order || !scaffold_offset) {
        isx_set_error("isx_irep_layout: bad argument");
        return ISX_ERR_ARG;
    }
    for (int32_t i = 0; i < n_scaffolds; i++) {
        if (scaffold_lengths[i] <= 0 || scaffold_lengths[i] > (int64_t)0xFFFFFFFFll) {
            isx_set_error("isx_irep_layout: scaffold " + std::to_string(i) + " has no positions / too many");
            return ISX_ERR_ARG;
        }
        if (scaffold_genome[i] < -1 || scaffold_genome[i] >= n_genomes) {
            isx_set_error("isx_irep_layout: genome of scaffold " + std::to_string(i) + " outside [-1, n_genomes)");
            return ISX_ERR_ARG;
        }
    }
    // genome by genome (no genome last), longest first, ties in the caller's order
    std::vector<int32_t> idx((size_t)n_scaffolds);
    std::iota(idx.begin(), idx.end(), 0);
    auto key = [&](int32_t i) { return scaffold_genome[i] < 0 ? n_genomes : scaffold_genome[i]; };
    std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) {
        if (key(a) != key(b)) return key(a) < key(b);
        return key(a) < n_genomes && scaffold_lengths[a] > scaffold_lengths[b];
    });
    std::copy(idx.begin(), idx.end(), order);
    size_t at = 0;
    int64_t block = 0, window = 0;
    for (int32_t g = 0; g < n_genomes; g++) {
        isx_irep_genome &G = genomes[g];
        G.first_scaffold = (int32_t)at;
        G.num_contigs = 0;
        G.L = 0;
        for (; at < idx.size() && scaffold_genome[idx[at]] == g; at++) {
            const int32_t s = idx[at];
            G.num_contigs++;
            if (scaffold_lengths[s] >= 2 * (int64_t)mask_edges) {
                scaffold_offset[s] = G.L;
                G.L += scaffold_lengths[s] - 2 * (int64_t)mask_edges;
            } else scaffold_offset[s] = -1;
        }
        G.n_blocks = (G.L + ISX_IREP_SLIDE - 1) / ISX_IREP_SLIDE;
        G.n_windows = G.L >= ISX_IREP_WINDOW ? (G.L - ISX_IREP_WINDOW) / ISX_IREP_SLIDE + 1 : 0;
        G.first_block = block;
        G.first_window = window;
        block += G.n_blocks;
        window += G.n_windows;
    }
    for (; at < idx.size(); at++) scaffold_offset[idx[at]] = -1;
    if (block > (int64_t)0x7FFFFFFFll) { isx_set_error("isx_irep_layout: more than 2^31 blocks"); return ISX_ERR_ARG; }
    return ISX_OK;
}

}  // extern "C"
