// cmpset_layout.cpp -- the comparison set's host-side geometry (include/instrain_amd.h isx_cmpset_*): the word-aligned
// position space, the pair kernel's tile directory and the level axis.  Plain host code: callable without a device.
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/instrain_amd.h"

void isx_set_error(const std::string &msg);

extern "C" {

int isx_cmpset_layout(int32_t n_scaffolds, const int64_t *scaffold_lengths, int64_t *word_offsets)
{
    if (n_scaffolds <= 0 || !scaffold_lengths || !word_offsets) { isx_set_error("isx_cmpset_layout: bad argument"); return ISX_ERR_ARG; }
    int64_t w = 0;
    for (int32_t i = 0; i < n_scaffolds; i++) {
        if (scaffold_lengths[i] <= 0 || scaffold_lengths[i] > (int64_t)0xFFFFFFFFll) {
            isx_set_error("isx_cmpset_layout: scaffold " + std::to_string(i) + " has no positions / too many");
            return ISX_ERR_ARG;
        }
        word_offsets[i] = w;
        w += (scaffold_lengths[i] + 63) / 64;
        if (w * 64 > (int64_t)0xFFFFFFFFll) { isx_set_error("isx_cmpset_layout: set space beyond 2^32 positions"); return ISX_ERR_ARG; }
    }
    word_offsets[n_scaffolds] = w;
    return ISX_OK;
}

int64_t isx_cmpset_tiles(int32_t n_scaffolds, const int64_t *scaffold_lengths, int32_t tile_words, isx_cmpset_tile *tiles)
{
    if (n_scaffolds <= 0 || !scaffold_lengths || tile_words <= 0) { isx_set_error("isx_cmpset_tiles: bad argument"); return ISX_ERR_ARG; }
    std::vector<int64_t> off((size_t)n_scaffolds + 1);
    const int rc = isx_cmpset_layout(n_scaffolds, scaffold_lengths, off.data());
    if (rc) return rc;
    int64_t n = 0;
    for (int32_t i = 0; i < n_scaffolds; i++)
        for (int64_t w = off[(size_t)i]; w < off[(size_t)i + 1]; w += tile_words, n++)
            if (tiles) {
                tiles[n].word0 = w;
                tiles[n].n_words = (int32_t)std::min<int64_t>(tile_words, off[(size_t)i + 1] - w);
                tiles[n].scaffold = i;
            }
    return n;
}

int isx_cmpset_level_map(int32_t n_samples, const int32_t *n_levels, const int32_t *level_mm, int32_t cap_axis, int32_t *axis,
                         int32_t *n_axis, int32_t *map)
{
    if (n_samples < 0 || (n_samples && (!n_levels || !map)) || cap_axis <= 0 || !axis || !n_axis) {
        isx_set_error("isx_cmpset_level_map: bad argument");
        return ISX_ERR_ARG;
    }
    std::vector<int32_t> all;
    size_t at = 0;
    for (int32_t s = 0; s < n_samples; s++) {
        if (n_levels[s] < 0 || (n_levels[s] && !level_mm)) { isx_set_error("isx_cmpset_level_map: bad argument"); return ISX_ERR_ARG; }
        for (int32_t k = 0; k < n_levels[s]; k++, at++) {
            const int32_t v = level_mm[at];
            if (v < 0 || v > 65535 || (k && v <= level_mm[at - 1])) {
                isx_set_error("isx_cmpset_level_map: the mm values of sample " + std::to_string(s) + " must ascend strictly within 0..65535");
                return ISX_ERR_ARG;
            }
            all.push_back(v);
        }
    }
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    if ((int64_t)all.size() > cap_axis) {
        isx_set_error("the samples' mm values make " + std::to_string(all.size()) + " axis levels, more than " + std::to_string(cap_axis));
        return ISX_ERR_CAPACITY;
    }
    *n_axis = (int32_t)all.size();
    std::copy(all.begin(), all.end(), axis);
    at = 0;
    for (int32_t s = 0; s < n_samples; s++) {
        int32_t k = -1;                 // own highest level with value <= axis[a]
        for (int32_t a = 0; a < cap_axis; a++) {
            if (a < *n_axis)
                while (k + 1 < n_levels[s] && level_mm[at + (size_t)k + 1] <= all[(size_t)a]) k++;
            map[(size_t)s * cap_axis + a] = a < *n_axis ? k : -1;
        }
        at += (size_t)n_levels[s];
    }
    return ISX_OK;
}

}  // extern "C"
