// isx_genomes.hip -- the device passes behind genome_info (`inStrain profile --stb`, `inStrain genome_wide`).
//
// Replaces the per-genome pandas / numpy work of
//   genomeLevel_coverage_info on generate_genome_coverage_array   inStrain/genomeUtilities.py (v1.9.1):297-365, 932-981
//   calc_snps, once per scaffold and level                        profile/snv_utilities.py:249-272
//   _genome_wide_linkage                                          genomeUtilities.py:636-659
// with three passes whose results are additive over scaffolds and batches (the host adds them: profile/genome_utilities.py).
//
// Coverage: one pass over the positions per level.  A workgroup walks the scaffold pieces of its tile, keeps a coverage histogram in
// LDS and adds it to its genome's when the tile moves on to another genome -- the median becomes a sum instead of a sort.
// SNV rows: one lane per row, integer atomics into every (scaffold, level) the row is current at.  LD rows: one wave per
// (scaffold, level) over the scaffold's rows, partials combined in a fixed shuffle tree (identical bytes run to run).
#include <algorithm>
#include <string>
#include <vector>

#include "isx_internal.h"
#include "isx_summary.h"

namespace {

constexpr uint32_t GH_TILE = 4096;          // positions per workgroup
constexpr int GH_LDS_BINS = 8192;           // histograms up to this many bins live in LDS (32 KiB), longer ones take global atomics

__device__ __forceinline__ int scaf_of(const int64_t *bounds, int n_seg, int64_t g)
{
    int lo = 0, hi = n_seg;                 // bounds[lo] <= g < bounds[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (bounds[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// acc / hist point at level mm of genome 0; consecutive genomes lie acc_stride rows / hist_stride words apart
__global__ void __launch_bounds__(256) k_genome_hist(const uint32_t *cov, uint32_t n_pos, const int64_t *sbounds, const int32_t *sgen,
                                                     int n_scaf, int64_t mask, int bins, int use_lds, isx_genome_cov *acc,
                                                     size_t acc_stride, uint32_t *hist, size_t hist_stride)
{
    extern __shared__ uint32_t s_hist[];    // [bins] when use_lds
    __shared__ uint32_t s_top;              // highest bin touched since the last flush
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t t0 = (int64_t)blockIdx.x * GH_TILE;
    const int64_t t1 = min((int64_t)n_pos, t0 + (int64_t)GH_TILE);
    if (use_lds) for (int i = tid; i < bins; i += 256) s_hist[i] = 0;
    if (tid == 0) s_top = 0;
    __syncthreads();
    unsigned long long n = 0, sum = 0, sq = 0;
    uint32_t mx = 0;
    int cur = -1;                           // the genome the partials belong to
    // everything that decides the control flow below depends on the tile alone: the workgroup stays together
    auto flush = [&]() {
        if (cur < 0) return;
        for (int o = 32; o > 0; o >>= 1) {
            n += (unsigned long long)__shfl_xor((long long)n, o);
            sum += (unsigned long long)__shfl_xor((long long)sum, o);
            sq += (unsigned long long)__shfl_xor((long long)sq, o);
            mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
        }
        if (lane == 0 && n) {
            isx_genome_cov *a = acc + (size_t)cur * acc_stride;
            atomicAdd(reinterpret_cast<unsigned long long *>(&a->n), n);
            atomicAdd(reinterpret_cast<unsigned long long *>(&a->sum_cov), sum);
            atomicAdd(reinterpret_cast<unsigned long long *>(&a->sumsq_cov), sq);
            atomicMax(&a->max_cov, mx);
        }
        n = sum = sq = 0; mx = 0;
        if (use_lds) {
            __syncthreads();
            const int top = (int)s_top;
            uint32_t *h = hist + (size_t)cur * hist_stride;
            for (int i = tid; i <= top; i += 256) {
                const uint32_t v = s_hist[i];
                if (v) { atomicAdd(&h[i], v); s_hist[i] = 0; }
            }
            __syncthreads();
            if (tid == 0) s_top = 0;
            __syncthreads();
        }
    };
    int sc = scaf_of(sbounds, n_scaf, t0);
    for (; sc < n_scaf; sc++) {
        const int64_t s0 = sbounds[sc], s1 = sbounds[sc + 1];
        if (s0 >= t1) break;
        const int g = sgen[sc];
        if (g < 0 || s1 - s0 < 2 * mask) continue;
        const int64_t lo = max(t0, s0 + mask), hi = min(t1, s1 - mask);
        if (lo >= hi) continue;
        if (g != cur) { flush(); cur = g; }
        uint32_t *h = use_lds ? s_hist : hist + (size_t)g * hist_stride;
        uint32_t top = 0;
        for (int64_t p = lo + tid; p < hi; p += 256) {
            const uint32_t c = cov[p];
            const uint32_t bin = min(c, (uint32_t)(bins - 1));
            atomicAdd(&h[bin], 1u);
            top = max(top, bin);
            n++; sum += c; sq += (unsigned long long)c * c; mx = max(mx, c);
        }
        if (use_lds && top) atomicMax(&s_top, top);
    }
    flush();
}

// iRep's block sums (include/instrain_amd.h isx_irep_add): the tiles of k_genome_hist; sbase[sc] = where the scaffold's first unmasked
// position lies in the set's block space (its genome's first block * ISX_IREP_SLIDE + its offset in the genome's array), -1 = the scaffold
// adds nothing.  A wave's 64 consecutive positions touch at most two blocks (64 <= ISX_IREP_SLIDE): both partial sums are reduced inside
// the wave and lane 0 issues at most two integer atomics per array.  cov == NULL: the G+C counts alone.
static_assert(ISX_IREP_SLIDE >= 64, "a wave must not span more than two blocks");
__global__ void __launch_bounds__(256) k_irep_blocks(const uint32_t *cov, uint32_t n_pos, const int64_t *sbounds, const int64_t *sbase,
                                                     int n_scaf, int64_t mask, const uint8_t *ref, int ref_packed, const uint8_t *ref_n,
                                                     unsigned long long *bcov, uint32_t *bgc)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t t0 = (int64_t)blockIdx.x * GH_TILE;
    const int64_t t1 = min((int64_t)n_pos, t0 + (int64_t)GH_TILE);
    // the loops below depend on the tile alone: whole waves stay together through the shuffles
    for (int sc = scaf_of(sbounds, n_scaf, t0); sc < n_scaf; sc++) {
        const int64_t s0 = sbounds[sc], s1 = sbounds[sc + 1];
        if (s0 >= t1) break;
        const int64_t base = sbase[sc];
        if (base < 0 || s1 - s0 < 2 * mask) continue;
        const int64_t lo = max(t0, s0 + mask), hi = min(t1, s1 - mask);
        const int64_t shift = base - s0 - mask;                     // flat position -> position in the block space
        for (int64_t w0 = lo + (tid - lane); w0 < hi; w0 += 256) {  // w0: the wave's first position
            const int64_t p = w0 + lane;
            const bool on = p < hi;
            const int64_t q0 = (w0 + shift) / ISX_IREP_SLIDE;
            const bool second = on && (p + shift) / ISX_IREP_SLIDE != q0;
            unsigned long long c0 = 0, c1 = 0;
            bool gc = false;
            if (on) {
                const unsigned long long c = cov ? cov[p] : 0u;
                if (second) c1 = c; else c0 = c;
                uint32_t code;
                if (ref_packed == 2) code = (ref_n && ((ref_n[p >> 3] >> (p & 7)) & 1u)) ? 4u : (uint32_t)((ref[p >> 2] >> ((p & 3) << 1)) & 3u);
                else code = ref[p];
                gc = code == 1u || code == 3u;                      // codes: A C T G, anything else is no base
            }
            const uint32_t g0 = (uint32_t)__popcll(__ballot(gc && !second)), g1 = (uint32_t)__popcll(__ballot(gc && second));
            if (cov)
                for (int o = 32; o > 0; o >>= 1) {
                    c0 += (unsigned long long)__shfl_xor((long long)c0, o);
                    c1 += (unsigned long long)__shfl_xor((long long)c1, o);
                }
            if (lane == 0) {
                if (c0) atomicAdd(&bcov[q0], c0);
                if (c1) atomicAdd(&bcov[q0 + 1], c1);
                if (g0) atomicAdd(&bgc[q0], g0);
                if (g1) atomicAdd(&bgc[q0 + 1], g1);
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_snv_levels(const isx_snv *snv, uint32_t n, const int64_t *bounds, int n_seg, int n_levels,
                                                    uint32_t *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const isx_snv r = snv[i];
    const int next = (i + 1 < n && snv[i + 1].gpos == r.gpos) ? (int)snv[i + 1].mm : n_levels;
    const int s = scaf_of(bounds, n_seg, (int64_t)r.gpos);
    const bool sns = r.allele_count == 1, snvv = r.allele_count > 1;
    const bool con = r.cls == 2 || r.cls == 4 || r.cls == 5, pop = r.cls == 2 || r.cls == 5;
    for (int lv = r.mm; lv < next; lv++) {
        uint32_t *c = out + ((size_t)s * n_levels + lv) * 5;
        atomicAdd(&c[0], 1u);
        if (sns) atomicAdd(&c[1], 1u);
        if (snvv) atomicAdd(&c[2], 1u);
        if (con) atomicAdd(&c[3], 1u);
        if (pop) atomicAdd(&c[4], 1u);
    }
}

// one wave per (scaffold, level): lane l takes rows first + l, first + l + 64, ... of the scaffold
__global__ void __launch_bounds__(256) k_ld_levels(const isx_ld *ld, const int64_t *row_off, int n_seg, int n_levels, isx_ld_level *out)
{
    const int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= (int64_t)n_seg * n_levels) return;                 // whole waves leave together
    const int s = (int)(w / n_levels), lv = (int)(w % n_levels);
    const int64_t r0 = row_off[s], r1 = row_off[s + 1];
    long long n = 0, n_r2 = 0, n_dp = 0, dist = 0;
    double s_r2 = 0.0, s_dp = 0.0;
    for (int64_t i = r0 + lane; i < r1; i += 64) {
        const isx_ld *r = ld + i;
        const int mm = r->mm;
        if (mm > lv) continue;
        const uint32_t a = r->gpos_a, b = r->gpos_b;
        if (i + 1 < r1 && ld[i + 1].gpos_a == a && ld[i + 1].gpos_b == b && (int)ld[i + 1].mm <= lv) continue;     // a later row replaces it
        n++;
        dist += (long long)b - (long long)a;
        const double r2 = r->r2, dp = r->d_prime;
        if (r2 == r2) { n_r2++; s_r2 += r2; }
        if (dp == dp) { n_dp++; s_dp += dp; }
    }
    for (int o = 32; o > 0; o >>= 1) {                          // fixed tree: identical bytes run to run
        n += __shfl_xor(n, o);
        n_r2 += __shfl_xor(n_r2, o);
        n_dp += __shfl_xor(n_dp, o);
        dist += __shfl_xor(dist, o);
        s_r2 += __shfl_xor(s_r2, o);
        s_dp += __shfl_xor(s_dp, o);
    }
    if (lane == 0) {
        isx_ld_level r;
        r.n = n; r.n_r2 = n_r2; r.n_dprime = n_dp; r.sum_distance = dist; r.sum_r2 = s_r2; r.sum_dprime = s_dp;
        out[w] = r;
    }
}

template <class T>
hipError_t dmalloc(T **p, size_t n) { return isx_raw_dev_malloc(p, std::max<size_t>(n, 1) * sizeof(T)); }

struct Events {
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t create() { hipError_t e = hipEventCreate(&ev[0]); return e == hipSuccess ? hipEventCreate(&ev[1]) : e; }
    ~Events() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

}  // namespace

void launch_genome_hist(hipStream_t s, const uint32_t *cov, uint32_t n_pos, const int64_t *sbounds, const int32_t *sgen, int n_scaf,
                        int mask_edges, int hist_bins, isx_genome_cov *acc, size_t acc_stride, uint32_t *hist, size_t hist_stride)
{
    if (!n_pos) return;
    const int use_lds = hist_bins <= GH_LDS_BINS;
    const uint32_t tiles = (n_pos + GH_TILE - 1) / GH_TILE;
    hipLaunchKernelGGL(k_genome_hist, dim3(tiles), dim3(256), use_lds ? (size_t)hist_bins * 4 : 0, s, cov, n_pos, sbounds, sgen, n_scaf,
                       (int64_t)mask_edges, hist_bins, use_lds, acc, acc_stride, hist, hist_stride);
}

void launch_irep_blocks(hipStream_t s, const uint32_t *cov, uint32_t n_pos, const int64_t *sbounds, const int64_t *sbase, int n_scaf,
                        int mask_edges, const uint8_t *ref, int ref_packed, const uint8_t *ref_n, uint64_t *block_cov, uint32_t *block_gc)
{
    if (!n_pos) return;
    const uint32_t tiles = (n_pos + GH_TILE - 1) / GH_TILE;
    hipLaunchKernelGGL(k_irep_blocks, dim3(tiles), dim3(256), 0, s, cov, n_pos, sbounds, sbase, n_scaf, (int64_t)mask_edges, ref, ref_packed,
                       ref_n, reinterpret_cast<unsigned long long *>(block_cov), block_gc);
}

int run_snv_levels(int device, hipStream_t s, int32_t n_scaffolds, const int64_t *scaffold_bounds, int64_t n_snv, const isx_snv *snv,
                   int32_t n_levels, isx_snv_level *out, float *device_ms)
{
    static_assert(sizeof(isx_snv_level) == 5 * sizeof(uint32_t), "counter rows are 5 words");
    // host side: rows in (gpos, mm) order inside the flat space, levels in range
    for (int64_t i = 0; i < n_snv; i++) {
        if ((int64_t)snv[i].gpos >= scaffold_bounds[n_scaffolds]) { isx_set_error("isx_snv_level_counts: SNV row outside the flat space"); return ISX_ERR_ARG; }
        if (snv[i].mm >= n_levels) { isx_set_error("isx_snv_level_counts: SNV row with mm >= n_levels"); return ISX_ERR_ARG; }
        if (i && (snv[i - 1].gpos > snv[i].gpos || (snv[i - 1].gpos == snv[i].gpos && snv[i - 1].mm >= snv[i].mm))) {
            isx_set_error("isx_snv_level_counts: SNV rows must be in (gpos, mm) order, one row per (gpos, mm)");
            return ISX_ERR_ARG;
        }
    }
    const size_t n_out = (size_t)n_scaffolds * n_levels;
    isx_snv *d_snv = nullptr;
    int64_t *d_b = nullptr;
    uint32_t *d_out = nullptr;
    Events E;
    auto done = [&](int code) {
        void *ps[] = {d_snv, d_b, d_out};
        for (void *p : ps) if (p) isx_dev_free(p);
        return code;
    };
#define GN_TRY(expr) do { if ((expr) != hipSuccess) { isx_set_error(std::string("HIP error in isx_snv_level_counts: ") + #expr); return done(ISX_ERR_HIP); } } while (0)
    GN_TRY(hipSetDevice(device));
    GN_TRY(E.create());
    GN_TRY(dmalloc(&d_snv, (size_t)n_snv));
    GN_TRY(dmalloc(&d_b, (size_t)n_scaffolds + 1));
    GN_TRY(dmalloc(&d_out, n_out * 5));
    if (n_snv) GN_TRY(hipMemcpyAsync(d_snv, snv, (size_t)n_snv * sizeof(isx_snv), hipMemcpyHostToDevice, s));
    GN_TRY(hipMemcpyAsync(d_b, scaffold_bounds, ((size_t)n_scaffolds + 1) * 8, hipMemcpyHostToDevice, s));
    GN_TRY(hipMemsetAsync(d_out, 0, n_out * 5 * 4, s));
    GN_TRY(hipEventRecord(E.ev[0], s));
    if (n_snv) {
        hipLaunchKernelGGL(k_snv_levels, dim3((uint32_t)((n_snv + 255) / 256)), dim3(256), 0, s, d_snv, (uint32_t)n_snv, d_b, (int)n_scaffolds,
                           (int)n_levels, d_out);
        GN_TRY(hipGetLastError());
    }
    GN_TRY(hipEventRecord(E.ev[1], s));
    GN_TRY(hipMemcpyAsync(out, d_out, n_out * sizeof(isx_snv_level), hipMemcpyDeviceToHost, s));
    GN_TRY(isx_wait_stream(s));
#undef GN_TRY
    if (device_ms) { float v = 0.f; (void)hipEventElapsedTime(&v, E.ev[0], E.ev[1]); *device_ms = v; }
    return done(ISX_OK);
}

int run_ld_levels(int device, hipStream_t s, int32_t n_scaffolds, const int64_t *scaffold_bounds, int64_t n_ld, const isx_ld *ld,
                  int32_t n_levels, isx_ld_level *out, float *device_ms)
{
    // rows in (gpos_a, gpos_b, mm) order inside the flat space, levels in range; where every scaffold's rows begin
    std::vector<int64_t> row_off((size_t)n_scaffolds + 1, 0);
    int sc = 0;
    for (int64_t i = 0; i < n_ld; i++) {
        const isx_ld &r = ld[i];
        if ((int64_t)r.gpos_a >= scaffold_bounds[n_scaffolds]) { isx_set_error("isx_ld_level_sums: LD row outside the flat space"); return ISX_ERR_ARG; }
        if (r.mm >= n_levels) { isx_set_error("isx_ld_level_sums: LD row with mm >= n_levels"); return ISX_ERR_ARG; }
        if (i) {
            const isx_ld &q = ld[i - 1];
            const bool ordered = q.gpos_a != r.gpos_a ? q.gpos_a < r.gpos_a : q.gpos_b != r.gpos_b ? q.gpos_b < r.gpos_b : q.mm < r.mm;
            if (!ordered) {
                isx_set_error("isx_ld_level_sums: LD rows must be in (gpos_a, gpos_b, mm) order, one row per (gpos_a, gpos_b, mm)");
                return ISX_ERR_ARG;
            }
        }
        while ((int64_t)r.gpos_a >= scaffold_bounds[sc + 1]) row_off[(size_t)++sc] = i;
    }
    while (sc < n_scaffolds) row_off[(size_t)++sc] = n_ld;
    const size_t n_out = (size_t)n_scaffolds * n_levels;
    isx_ld *d_ld = nullptr;
    int64_t *d_off = nullptr;
    isx_ld_level *d_out = nullptr;
    Events E;
    auto done = [&](int code) {
        void *ps[] = {d_ld, d_off, d_out};
        for (void *p : ps) if (p) isx_dev_free(p);
        return code;
    };
#define GN_TRY(expr) do { if ((expr) != hipSuccess) { isx_set_error(std::string("HIP error in isx_ld_level_sums: ") + #expr); return done(ISX_ERR_HIP); } } while (0)
    GN_TRY(hipSetDevice(device));
    GN_TRY(E.create());
    GN_TRY(dmalloc(&d_ld, (size_t)n_ld));
    GN_TRY(dmalloc(&d_off, (size_t)n_scaffolds + 1));
    GN_TRY(dmalloc(&d_out, n_out));
    if (n_ld) GN_TRY(hipMemcpyAsync(d_ld, ld, (size_t)n_ld * sizeof(isx_ld), hipMemcpyHostToDevice, s));
    GN_TRY(hipMemcpyAsync(d_off, row_off.data(), row_off.size() * 8, hipMemcpyHostToDevice, s));
    GN_TRY(hipEventRecord(E.ev[0], s));
    hipLaunchKernelGGL(k_ld_levels, dim3((uint32_t)((n_out + 3) / 4)), dim3(256), 0, s, d_ld, d_off, (int)n_scaffolds, (int)n_levels, d_out);
    GN_TRY(hipGetLastError());
    GN_TRY(hipEventRecord(E.ev[1], s));
    GN_TRY(hipMemcpyAsync(out, d_out, n_out * sizeof(isx_ld_level), hipMemcpyDeviceToHost, s));
    GN_TRY(isx_wait_stream(s));
#undef GN_TRY
    if (device_ms) { float v = 0.f; (void)hipEventElapsedTime(&v, E.ev[0], E.ev[1]); *device_ms = v; }
    return done(ISX_OK);
}
