// isx_irep.hip -- iRep on the device (include/instrain_amd.h isx_irep_*).
//
// Replaces, per genome,
//   calculate_iRep_from_coverage_array      inStrain/irep_utilities.py (v1.9.1):22-81 with _iRep_windows :136-149, _iRep_filter_windows
//                                           :151-164, _calc_iRep :186-206, trim_data :208-221, fit_coverage :223-249
// on the array generate_genome_coverage_array(mask_edges=100) builds (genomeUtilities.py:932-981).  The position-sized part is one
// additive pass per batch (isx_genomes.hip k_irep_blocks through isx_summary.hip run_irep_add): sums over blocks of ISX_IREP_SLIDE
// positions.  The tail works on L / ISX_IREP_SLIDE windows per genome: integer window sums, one rocPRIM segmented sort, and one
// workgroup per genome for the median, the kept range and the trimmed least-squares line -- the exact value the reference's FFT windows
// and iterative solver approximate -- and the same again on the GC-corrected coverage (_iRep_gc_bias :268-294).  fp64 sums go through one fixed tree: identical bytes call to call.
#include <algorithm>
#include <cstring>
#include <string.h>
#include <string>
#include <vector>
#include <rocprim/rocprim.hpp>

#include "isx_batch.h"

namespace {

constexpr int WIN_BLOCKS = ISX_IREP_WINDOW / ISX_IREP_SLIDE;

// the genome of window w: the last one whose first_window <= w (a genome without windows shares its first_window with the next)
__device__ __forceinline__ int genome_of_window(const isx_irep_genome *gen, int n_gen, int64_t w)
{
    int lo = 0, hi = n_gen;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (gen[mid].first_window <= w) lo = mid; else hi = mid;
    }
    return lo;
}

// one lane per window: S[w] = the sum of its WIN_BLOCKS blocks, and the same of the G+C counts
__global__ void __launch_bounds__(256) k_irep_windows(const isx_irep_genome *gen, int n_gen, int64_t n_windows, const unsigned long long *bcov,
                                                      const uint32_t *bgc, unsigned long long *keys, uint32_t *gcw)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= n_windows) return;
    const isx_irep_genome g = gen[genome_of_window(gen, n_gen, w)];
    const int64_t b0 = g.first_block + (w - g.first_window);
    unsigned long long s = 0;
    uint32_t c = 0;
    for (int k = 0; k < WIN_BLOCKS; k++) { s += bcov[b0 + k]; c += bgc[b0 + k]; }
    keys[w] = s;
    gcw[w] = c;
}

// what the GC stage takes over from the raw fit, and its own line
struct GcState {
    unsigned long long med2;            // the doubled median of the window sums
    long long n_kept;
    double m, b, r2;                    // the current line coverage = m * gc + b
    double av;                          // mean coverage of the kept windows
};

__device__ __forceinline__ double block_sum(double v, double *sh)
{
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {         // fixed tree
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// The trimmed fit (irep_utilities.py:186-249 _calc_iRep, trim_data, fit_coverage) by the whole workgroup: X_i = int(i * (L / n)) + 1,
// Y_i = yf(i) for the n sorted kept windows, int(n * 0.05) points trimmed at either end, the least-squares line in the centred two-pass
// form, r2 = 1 - var(residual) / var(Y).  Y[n]: scratch.  -> 2 ** (m L), NaN (and *r2 NaN) with fewer than three points
template <class YF>
__device__ double trimmed_fit(int64_t n, double Ld, YF yf, double *Y, double *sh, double *r2)
{
    const int tid = threadIdx.x;
    const int64_t trim = (int64_t)((double)n * 0.05);
    const int64_t cnt = n - 2 * trim;
    *r2 = __builtin_nan("");
    if (cnt < 3) return __builtin_nan("");
    const double dif = Ld / (double)n, dc = (double)cnt;
    double sx = 0.0, sy = 0.0;
    for (int64_t i = trim + tid; i < n - trim; i += 256) {
        const double y = yf(i);
        Y[i] = y;
        sx += (double)((long long)((double)i * dif)) + 1.0;
        sy += y;
    }
    const double mx = block_sum(sx, sh) / dc, my = block_sum(sy, sh) / dc;
    double sxx = 0.0, sxy = 0.0, syy = 0.0;
    for (int64_t i = trim + tid; i < n - trim; i += 256) {
        const double dx = (double)((long long)((double)i * dif)) + 1.0 - mx, dy = Y[i] - my;
        sxx += dx * dx; sxy += dx * dy; syy += dy * dy;
    }
    sxx = block_sum(sxx, sh); sxy = block_sum(sxy, sh); syy = block_sum(syy, sh);
    const double m = sxy / sxx, b = my - m * mx;
    double sr = 0.0;
    for (int64_t i = trim + tid; i < n - trim; i += 256)
        sr += (m * ((double)((long long)((double)i * dif)) + 1.0) + b) - Y[i];
    const double mr = block_sum(sr, sh) / dc;
    double srr = 0.0;
    for (int64_t i = trim + tid; i < n - trim; i += 256) {
        const double d = (m * ((double)((long long)((double)i * dif)) + 1.0) + b) - Y[i] - mr;
        srr += d * d;
    }
    srr = block_sum(srr, sh);
    *r2 = 1.0 - (srr / dc) / (syy / dc);
    return exp2(m * Ld);
}

// one workgroup per genome, on its sorted window sums
__global__ void __launch_bounds__(256) k_irep_fit(const isx_irep_genome *gen, const unsigned long long *bcov, const unsigned long long *sorted,
                                                  double *ys, isx_irep_row *out, GcState *state)
{
    __shared__ double sh[256];
    __shared__ unsigned long long sh_u[256];
    __shared__ long long s_lo, s_hi;
    __shared__ unsigned long long s_med2;
    const int tid = threadIdx.x;
    const isx_irep_genome g = gen[blockIdx.x];
    const double nan = __builtin_nan("");
    // the exact coverage sum
    unsigned long long part = 0;
    for (int64_t i = tid; i < g.n_blocks; i += 256) part += bcov[g.first_block + i];
    sh_u[tid] = part;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sh_u[tid] += sh_u[tid + o];
        __syncthreads();
    }
    const unsigned long long sum_cov = sh_u[0];
    const unsigned long long *S = sorted + g.first_window;
    const int64_t W = g.n_windows;
    if (tid == 0) {
        long long lo = 0, hi = 0;
        unsigned long long med2 = 0;
        if (W > 0) {
            // the doubled median, then the kept run: S > 0, med2 > 0, max / min <= 8 on both sides
            med2 = (W & 1) ? 2 * S[W / 2] : S[W / 2 - 1] + S[W / 2];
            if (med2 > 0) {
                int64_t a = 0, b = W;               // first index with S > 0 and 16 S >= med2
                while (a < b) { const int64_t m = (a + b) >> 1; if (S[m] > 0 && 16 * S[m] >= med2) b = m; else a = m + 1; }
                lo = a;
                a = lo; b = W;                      // first index with 2 S > 8 med2
                while (a < b) { const int64_t m = (a + b) >> 1; if (2 * S[m] > 8 * med2) b = m; else a = m + 1; }
                hi = a;
            }
        }
        s_lo = lo; s_hi = hi; s_med2 = med2;
    }
    __syncthreads();
    const int64_t lo = s_lo, n_kept = s_hi - s_lo;
    const double Ld = (double)g.L;
    double r2 = nan;
    uint32_t flags = 0;
    const double raw = trimmed_fit(n_kept, Ld, [&](int64_t i) { return log2((double)S[lo + i] / (double)ISX_IREP_WINDOW); },
                                   ys + g.first_window, sh, &r2);
    if (raw != raw) flags |= ISX_IREP_NO_FIT;
    if (tid == 0) {
        GcState st;
        st.med2 = s_med2; st.n_kept = n_kept; st.m = st.b = st.r2 = 0.0; st.av = nan;
        state[blockIdx.x] = st;
        isx_irep_row r;
        r.L = g.L; r.n_windows = W; r.n_kept = n_kept; r.sum_cov = sum_cov; r.num_contigs = g.num_contigs;
        r.gc_irep = nan;
        if (g.L == 0) {
            r.avg_cov = r.fragMbp = r.kept_windows = r.r2 = r.raw_irep = r.irep = nan;
            r.flags = ISX_IREP_EMPTY | ISX_IREP_NO_FIT;
        } else {
            r.avg_cov = (double)sum_cov / Ld;
            r.fragMbp = (double)g.num_contigs / (Ld / 1000000.0);
            r.kept_windows = W > 0 ? (double)n_kept / (double)W : nan;
            r.r2 = r2; r.raw_irep = raw;
            if (r.kept_windows < 0.98) flags |= ISX_IREP_FAIL_KEPT;
            if (r.avg_cov < 5.0) flags |= ISX_IREP_FAIL_COV;
            if (r2 < 0.9) flags |= ISX_IREP_FAIL_R2;
            if (r.fragMbp > 175.0) flags |= ISX_IREP_FAIL_FRAG;
            r.flags = flags;
            r.irep = flags ? nan : raw;
        }
        out[blockIdx.x] = r;
    }
}

__device__ __forceinline__ bool window_kept(unsigned long long S, unsigned long long med2)
{
    return S > 0 && med2 > 0 && 16 * S >= med2 && 2 * S <= 8 * med2;
}

// _iRep_gc_bias (irep_utilities.py:268-294), one workgroup per genome over its windows in window order; the line-fit kernel, run twice.
// stage 0: the line coverage = m * gc + b through every kept window; val[w] = |coverage - line| (not kept: -inf, sorts first).
// stage 1: sorted = val in ascending order; the cutoff is the int(n * 0.01)-th largest error, the line is fitted again without the
// windows whose error reaches it, and val[w] = the corrected coverage, coverage + (mean - line) (not kept: +inf, sorts last).  A fit of
// two points or fewer leaves m = b = r2 = 0 as the reference's `False`s do; r2 < 0 corrects nothing.
__global__ void __launch_bounds__(256) k_irep_gc_line(const isx_irep_genome *gen, const unsigned long long *keys, const uint32_t *gcw,
                                                      const double *sorted, double *val, GcState *state, int stage)
{
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const isx_irep_genome g = gen[blockIdx.x];
    GcState st = state[blockIdx.x];
    const int64_t W = g.n_windows, n = st.n_kept;
    if (n <= 0) return;                                             // whole workgroups leave together
    const unsigned long long *S = keys + g.first_window;
    const uint32_t *G = gcw + g.first_window;
    double *V = val + g.first_window;
    const double inf = __builtin_inf();
    double cutoff = inf;
    if (stage == 1) cutoff = sorted[g.first_window + W - 1 - (int64_t)((double)n * 0.01)];
    auto used = [&](int64_t w) { return window_kept(S[w], st.med2) && (stage == 0 || !(V[w] >= cutoff)); };
    double cn = 0.0, sx = 0.0, sy = 0.0;
    for (int64_t w = tid; w < W; w += 256)
        if (used(w)) { cn += 1.0; sx += (double)G[w] / (double)ISX_IREP_WINDOW; sy += (double)S[w] / (double)ISX_IREP_WINDOW; }
    cn = block_sum(cn, sh); sx = block_sum(sx, sh); sy = block_sum(sy, sh);
    double m = 0.0, b = 0.0, r2 = 0.0;
    if (cn > 2.0) {
        const double mx = sx / cn, my = sy / cn;
        double sxx = 0.0, sxy = 0.0, syy = 0.0;
        for (int64_t w = tid; w < W; w += 256)
            if (used(w)) {
                const double dx = (double)G[w] / (double)ISX_IREP_WINDOW - mx, dy = (double)S[w] / (double)ISX_IREP_WINDOW - my;
                sxx += dx * dx; sxy += dx * dy; syy += dy * dy;
            }
        sxx = block_sum(sxx, sh); sxy = block_sum(sxy, sh); syy = block_sum(syy, sh);
        m = sxy / sxx; b = my - m * mx;
        double sr = 0.0;
        for (int64_t w = tid; w < W; w += 256)
            if (used(w)) sr += (m * ((double)G[w] / (double)ISX_IREP_WINDOW) + b) - (double)S[w] / (double)ISX_IREP_WINDOW;
        const double mr = block_sum(sr, sh) / cn;
        double srr = 0.0;
        for (int64_t w = tid; w < W; w += 256)
            if (used(w)) {
                const double d = (m * ((double)G[w] / (double)ISX_IREP_WINDOW) + b) - (double)S[w] / (double)ISX_IREP_WINDOW - mr;
                srr += d * d;
            }
        srr = block_sum(srr, sh);
        r2 = 1.0 - (srr / cn) / (syy / cn);
    }
    const double av = stage == 0 ? sy / cn : st.av;                 // every kept window is used at stage 0
    __syncthreads();                                                // every read of V above is done before it is overwritten
    for (int64_t w = tid; w < W; w += 256) {
        const double cov = (double)S[w] / (double)ISX_IREP_WINDOW, line = m * ((double)G[w] / (double)ISX_IREP_WINDOW) + b;
        if (!window_kept(S[w], st.med2)) V[w] = stage == 0 ? -inf : inf;
        else if (stage == 0) V[w] = fabs(cov - line);
        else V[w] = r2 < 0.0 ? cov : cov + (av - line);
    }
    if (tid == 0) {
        st.m = m; st.b = b; st.r2 = r2; st.av = av;
        state[blockIdx.x] = st;
    }
}

// the trimmed fit on the sorted corrected coverage (kept windows first) -> unfiltered_iRep
__global__ void __launch_bounds__(256) k_irep_gc_fit(const isx_irep_genome *gen, const double *sorted, const GcState *state, double *ys,
                                                     isx_irep_row *out)
{
    __shared__ double sh[256];
    const isx_irep_genome g = gen[blockIdx.x];
    const int64_t n = state[blockIdx.x].n_kept;
    if (n <= 0) return;
    const double *C = sorted + g.first_window;
    double r2;
    // _iRep_log_transform: anything below 1e-50 counts as 1e-50
    const double v = trimmed_fit(n, (double)g.L, [&](int64_t i) { return log2(C[i] < 1e-50 ? 1e-50 : C[i]); }, ys + g.first_window, sh, &r2);
    if (threadIdx.x == 0) out[blockIdx.x].gc_irep = v;
}

__global__ void k_irep_add_blocks(const unsigned long long *cov, const uint32_t *gc, int64_t n, unsigned long long *bcov, uint32_t *bgc)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bcov[i] += cov[i];
    bgc[i] += gc[i];
}

}  // namespace

struct isx_irep {
    isx_ctx *ctx = nullptr;
    int32_t n_scaf = 0, n_gen = 0, mask = 0;
    int64_t n_blocks = 0, n_windows = 0;
    std::vector<int64_t> len, base;         // per scaffold: length; first unmasked position in the block space or -1
    std::vector<uint8_t> seen;              // host mirror of d_seen
    std::vector<isx_irep_genome> gen;
    hipEvent_t ev[2] = {nullptr, nullptr};
    isx_irep_genome *d_gen = nullptr;
    uint64_t *d_cov = nullptr, *d_keys = nullptr, *d_sorted = nullptr;
    uint32_t *d_gc = nullptr, *d_seg = nullptr;
    uint8_t *d_seen = nullptr;
    double *d_y = nullptr, *d_val = nullptr, *d_val_sorted = nullptr;  // the fits' Y scratch; the GC stage's errors / corrected coverage
    uint32_t *d_gcw = nullptr;              // G+C count of every window
    GcState *d_state = nullptr;
    isx_irep_row *d_rows = nullptr;
    void *d_temp = nullptr;
    size_t temp_bytes = 0;
};

extern "C" {

int isx_irep_create(isx_ctx *ctx, int32_t n_scaffolds, const int64_t *scaffold_lengths, const int32_t *scaffold_genome, int32_t n_genomes,
                    int32_t mask_edges, isx_irep **out)
{
    if (!ctx || !out) { isx_set_error("isx_irep_create: bad argument"); return ISX_ERR_ARG; }
    *out = nullptr;
    std::vector<isx_irep_genome> gen((size_t)std::max(n_genomes, 1));
    std::vector<int32_t> order((size_t)std::max(n_scaffolds, 1));
    std::vector<int64_t> off((size_t)std::max(n_scaffolds, 1));
    const int rc = isx_irep_layout(n_scaffolds, scaffold_lengths, scaffold_genome, n_genomes, mask_edges, gen.data(), order.data(), off.data());
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    isx_irep *st = new isx_irep();
    st->ctx = ctx; st->n_scaf = n_scaffolds; st->n_gen = n_genomes; st->mask = mask_edges;
    st->len.assign(scaffold_lengths, scaffold_lengths + n_scaffolds);
    st->gen = gen;
    st->base.assign((size_t)n_scaffolds, -1);
    for (int32_t i = 0; i < n_scaffolds; i++)
        if (off[(size_t)i] >= 0) st->base[(size_t)i] = gen[(size_t)scaffold_genome[i]].first_block * ISX_IREP_SLIDE + off[(size_t)i];
    st->seen.assign((size_t)n_scaffolds, 0);
    st->n_blocks = gen.back().first_block + gen.back().n_blocks;
    st->n_windows = gen.back().first_window + gen.back().n_windows;
    std::vector<uint32_t> seg((size_t)n_genomes + 1);
    for (int32_t g = 0; g < n_genomes; g++) seg[(size_t)g] = (uint32_t)gen[(size_t)g].first_window;
    seg[(size_t)n_genomes] = (uint32_t)st->n_windows;
    const size_t nb = (size_t)std::max<int64_t>(st->n_blocks, 1), nw = (size_t)std::max<int64_t>(st->n_windows, 1);
    hipStream_t s = ctx->stream;
    hipError_t e = hipEventCreate(&st->ev[0]);
    if (e == hipSuccess) e = hipEventCreate(&st->ev[1]);
    if (e == hipSuccess) e = isx_raw_dev_malloc(&st->d_gen, gen.size() * sizeof(isx_irep_genome));
    if (e == hipSuccess) e = isx_raw_dev_malloc(&st->d_cov, nb * 8);
    if (e == hipSuccess) e = isx_raw_dev_malloc(&st->d_gc, nb * 4);
    if (e == hipSuccess) e = isx_raw_dev_malloc(&st->d_seen, (size_t)n_scaffolds);
    if (e == hipSuccess) e = isx_raw_dev_malloc(&st->d_keys, nw * 8);
    if (e == hipSuccess) e = isx_raw_dev_malloc(&st->d_sorted, nw * 8);
    if (e == hipSuccess) e = isx_raw_dev_malloc(&st->d_y, nw * 8);
    if (e == hipSuccess) e = isx_raw_dev_malloc(&st->d_val, nw * 8);
    if (e == hipSuccess) e = isx_raw_dev_malloc(&st->d_val_sorted, nw * 8);
    if (e == hipSuccess) e = isx_raw_dev_malloc(&st->d_gcw, nw * 4);
    if (e == hipSuccess) e = isx_raw_dev_malloc(&st->d_state, gen.size() * sizeof(GcState));
    if (e == hipSuccess) e = isx_raw_dev_malloc(&st->d_seg, seg.size() * 4);
    if (e == hipSuccess) e = isx_raw_dev_malloc(&st->d_rows, gen.size() * sizeof(isx_irep_row));
    if (e == hipSuccess && st->n_windows) e = rocprim::segmented_radix_sort_keys(nullptr, st->temp_bytes, st->d_keys, st->d_sorted, (unsigned)st->n_windows,
                                                                (unsigned)n_genomes, st->d_seg, st->d_seg + 1, 0, 64, s);
    size_t tb2 = 0;
    if (e == hipSuccess && st->n_windows) e = rocprim::segmented_radix_sort_keys(nullptr, tb2, st->d_val, st->d_val_sorted, (unsigned)st->n_windows,
                                                                                 (unsigned)n_genomes, st->d_seg, st->d_seg + 1, 0, 64, s);
    st->temp_bytes = std::max(st->temp_bytes, tb2);
    if (e == hipSuccess) e = isx_raw_dev_malloc(&st->d_temp, st->temp_bytes + 256);
    if (e == hipSuccess) e = hipMemcpyAsync(st->d_gen, gen.data(), gen.size() * sizeof(isx_irep_genome), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(st->d_seg, seg.data(), seg.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(st->d_cov, 0, nb * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(st->d_gc, 0, nb * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(st->d_seen, 0, (size_t)n_scaffolds, s);
    if (e == hipSuccess) e = isx_wait_stream(s);
    if (e != hipSuccess) {
        isx_set_error(std::string("isx_irep_create: ") + hipGetErrorString(e));
        isx_irep_destroy(st);
        return ISX_ERR_HIP;
    }
    *out = st;
    return ISX_OK;
}

void isx_irep_destroy(isx_irep *st)
{
    if (!st) return;
    (void)hipSetDevice(st->ctx->device);
    (void)isx_wait_stream(st->ctx->stream);
    void *ps[] = {st->d_gen, st->d_cov, st->d_gc, st->d_seen, st->d_keys, st->d_sorted, st->d_y, st->d_val, st->d_val_sorted, st->d_gcw,
                  st->d_state, st->d_seg, st->d_rows, st->d_temp};
    for (void *p : ps) if (p) isx_dev_free(p);
    for (hipEvent_t e : st->ev) if (e) (void)hipEventDestroy(e);
    delete st;
}

int isx_irep_sizes(isx_irep *st, int64_t *n_blocks, int32_t *n_scaffolds, int32_t *n_genomes)
{
    if (!st) { isx_set_error("isx_irep_sizes: bad argument"); return ISX_ERR_ARG; }
    if (n_blocks) *n_blocks = st->n_blocks;
    if (n_scaffolds) *n_scaffolds = st->n_scaf;
    if (n_genomes) *n_genomes = st->n_gen;
    return ISX_OK;
}

int isx_irep_add(isx_irep *st, isx_batch *b, int32_t n_bscaf, const int64_t *bb, const int32_t *set_index, int32_t level, float *device_ms)
{
    if (!st || !b || !bb || !set_index || n_bscaf <= 0) { isx_set_error("isx_irep_add: bad argument"); return ISX_ERR_ARG; }
    if (!b->ran) { isx_set_error("isx_irep_add: run the batch first"); return ISX_ERR_STATE; }
    if (b->ctx != st->ctx) { isx_set_error("isx_irep_add: the batch belongs to another ctx than the accumulator"); return ISX_ERR_ARG; }
    if (bb[0] != 0 || bb[n_bscaf] != b->n_pos) { isx_set_error("isx_irep_add: scaffold_bounds must span [0, n_pos]"); return ISX_ERR_ARG; }
    for (int32_t i = 0; i < n_bscaf; i++)
        if (bb[i + 1] <= bb[i]) { isx_set_error("isx_irep_add: scaffold_bounds must be strictly ascending"); return ISX_ERR_ARG; }
    if (b->n_pos > (int64_t)0xFFFFFFFFll) { isx_set_error("isx_irep_add: flat space beyond 2^32 positions"); return ISX_ERR_ARG; }
    if (level < -1 || level >= b->M) {
        isx_set_error("isx_irep_add: level " + std::to_string(level) + " outside [-1, " + std::to_string(b->M) + ")");
        return ISX_ERR_ARG;
    }
    std::vector<int64_t> base((size_t)n_bscaf, -1);
    std::vector<uint8_t> mine((size_t)st->n_scaf, 0);
    for (int32_t i = 0; i < n_bscaf; i++) {
        const int32_t sid = set_index[i];
        if (sid == -1) continue;
        if (sid < 0 || sid >= st->n_scaf) { isx_set_error("isx_irep_add: set_index[" + std::to_string(i) + "] outside the set"); return ISX_ERR_ARG; }
        if (bb[i + 1] - bb[i] != st->len[(size_t)sid]) {
            isx_set_error("isx_irep_add: batch scaffold " + std::to_string(i) + " has not the length of set scaffold " + std::to_string(sid));
            return ISX_ERR_ARG;
        }
        if (st->seen[(size_t)sid] || mine[(size_t)sid]) {
            isx_set_error("isx_irep_add: scaffold " + std::to_string(sid) + " was added before");
            return ISX_ERR_STATE;
        }
        mine[(size_t)sid] = 1;
        base[(size_t)i] = st->base[(size_t)sid];
    }
    if (b->lean && !b->d_counts && !b->d_entries) { isx_set_error("this batch lives in a lean pipe slot (isx_pipe_params.lean_output): its dense coverage / clonality arrays were not written"); return ISX_ERR_STATE; }
    if (!b->d_ref) { isx_set_error("isx_irep_add: the batch keeps no reference on the device"); return ISX_ERR_STATE; }
    HIP_TRY(hipSetDevice(st->ctx->device));
    SummaryIn in{};
    fill_summary_in(b, n_bscaf, bb, in);
    IrepAdd a{};
    a.scaffold_base = base.data(); a.level = level; a.mask_edges = st->mask;
    a.ref = b->d_ref; a.ref_n = b->d_ref_n; a.ref_packed = b->ref_packed;
    a.block_cov = st->d_cov; a.block_gc = st->d_gc;
    const int rc = run_irep_add(in, b->S, a, device_ms);
    if (rc) return rc;
    for (int32_t i = 0; i < st->n_scaf; i++) st->seen[(size_t)i] |= mine[(size_t)i];
    HIP_TRY(hipMemcpyAsync(st->d_seen, st->seen.data(), (size_t)st->n_scaf, hipMemcpyHostToDevice, st->ctx->stream));
    HIP_TRY(isx_wait_stream(st->ctx->stream));
    return ISX_OK;
}

int isx_irep_add_stored(isx_irep *st, isx_stored *sp, const int32_t *set_index, int32_t level, float *device_ms)
{
    if (!st || !sp || !set_index) { isx_set_error("isx_irep_add_stored: bad argument"); return ISX_ERR_ARG; }
    if (sp->ctx != st->ctx) { isx_set_error("isx_irep_add_stored: the stored profile belongs to another ctx than the accumulator"); return ISX_ERR_ARG; }
    if (level < -1 || level >= sp->M) {
        isx_set_error("isx_irep_add_stored: level " + std::to_string(level) + " outside [-1, " + std::to_string(sp->M) + ")");
        return ISX_ERR_ARG;
    }
    const int32_t n_bscaf = sp->n_scaf;
    const int64_t *bb = sp->bounds.data();
    std::vector<int64_t> base((size_t)n_bscaf, -1);
    std::vector<uint8_t> mine((size_t)st->n_scaf, 0);
    for (int32_t i = 0; i < n_bscaf; i++) {
        const int32_t sid = set_index[i];
        if (sid == -1) continue;
        if (sid < 0 || sid >= st->n_scaf) { isx_set_error("isx_irep_add_stored: set_index[" + std::to_string(i) + "] outside the set"); return ISX_ERR_ARG; }
        if (bb[i + 1] - bb[i] != st->len[(size_t)sid]) {
            isx_set_error("isx_irep_add_stored: scaffold " + std::to_string(i) + " has not the length of set scaffold " + std::to_string(sid));
            return ISX_ERR_ARG;
        }
        if (st->seen[(size_t)sid] || mine[(size_t)sid]) {
            isx_set_error("isx_irep_add_stored: scaffold " + std::to_string(sid) + " was added before");
            return ISX_ERR_STATE;
        }
        mine[(size_t)sid] = 1;
        base[(size_t)i] = st->base[(size_t)sid];
    }
    if (!sp->d_ref) { isx_set_error("isx_irep_add_stored: the stored profile was created without ref_codes"); return ISX_ERR_STATE; }
    HIP_TRY(hipSetDevice(st->ctx->device));
    SummaryIn in{};
    stored_summary_in(sp, in);
    IrepAdd a{};
    a.scaffold_base = base.data(); a.level = level; a.mask_edges = st->mask;
    a.ref = sp->d_ref; a.ref_n = nullptr; a.ref_packed = 0;
    a.block_cov = st->d_cov; a.block_gc = st->d_gc;
    const int rc = run_irep_add(in, sp->S, a, device_ms);
    if (rc) return rc;
    for (int32_t i = 0; i < st->n_scaf; i++) st->seen[(size_t)i] |= mine[(size_t)i];
    HIP_TRY(hipMemcpyAsync(st->d_seen, st->seen.data(), (size_t)st->n_scaf, hipMemcpyHostToDevice, st->ctx->stream));
    HIP_TRY(isx_wait_stream(st->ctx->stream));
    return ISX_OK;
}

int isx_irep_blocks_fetch(isx_irep *st, uint64_t *cov, uint32_t *gc, uint8_t *seen)
{
    if (!st || !cov || !gc || !seen) { isx_set_error("isx_irep_blocks_fetch: bad argument"); return ISX_ERR_ARG; }
    HIP_TRY(hipSetDevice(st->ctx->device));
    hipStream_t s = st->ctx->stream;
    if (st->n_blocks) {
        HIP_TRY(hipMemcpyAsync(cov, st->d_cov, (size_t)st->n_blocks * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(gc, st->d_gc, (size_t)st->n_blocks * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipMemcpyAsync(seen, st->d_seen, (size_t)st->n_scaf, hipMemcpyDeviceToHost, s));
    HIP_TRY(isx_wait_stream(s));
    return ISX_OK;
}

int isx_irep_blocks_add(isx_irep *st, const uint64_t *cov, const uint32_t *gc, const uint8_t *seen)
{
    if (!st || !cov || !gc || !seen) { isx_set_error("isx_irep_blocks_add: bad argument"); return ISX_ERR_ARG; }
    for (int32_t i = 0; i < st->n_scaf; i++)
        if (seen[i] && st->seen[(size_t)i]) {
            isx_set_error("isx_irep_blocks_add: scaffold " + std::to_string(i) + " was added on both sides");
            return ISX_ERR_STATE;
        }
    HIP_TRY(hipSetDevice(st->ctx->device));
    hipStream_t s = st->ctx->stream;
    if (st->n_blocks) {
        uint64_t *d_c = nullptr;
        uint32_t *d_g = nullptr;
        auto done = [&](int code) { if (d_c) isx_dev_free(d_c); if (d_g) isx_dev_free(d_g); return code; };
#define IB_TRY(expr) do { if ((expr) != hipSuccess) { isx_set_error(std::string("HIP error in isx_irep_blocks_add: ") + #expr); return done(ISX_ERR_HIP); } } while (0)
        IB_TRY(isx_raw_dev_malloc(&d_c, (size_t)st->n_blocks * 8));
        IB_TRY(isx_raw_dev_malloc(&d_g, (size_t)st->n_blocks * 4));
        IB_TRY(hipMemcpyAsync(d_c, cov, (size_t)st->n_blocks * 8, hipMemcpyHostToDevice, s));
        IB_TRY(hipMemcpyAsync(d_g, gc, (size_t)st->n_blocks * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_irep_add_blocks, dim3((uint32_t)((st->n_blocks + 255) / 256)), dim3(256), 0, s,
                           reinterpret_cast<const unsigned long long *>(d_c), d_g, st->n_blocks,
                           reinterpret_cast<unsigned long long *>(st->d_cov), st->d_gc);
        IB_TRY(hipGetLastError());
        IB_TRY(isx_wait_stream(s));
#undef IB_TRY
        done(ISX_OK);
    }
    for (int32_t i = 0; i < st->n_scaf; i++) st->seen[(size_t)i] |= seen[i] ? 1 : 0;
    HIP_TRY(hipMemcpyAsync(st->d_seen, st->seen.data(), (size_t)st->n_scaf, hipMemcpyHostToDevice, s));
    HIP_TRY(isx_wait_stream(s));
    return ISX_OK;
}

int isx_irep_finish(isx_irep *st, isx_irep_row *out, float *device_ms)
{
    if (!st || !out) { isx_set_error("isx_irep_finish: bad argument"); return ISX_ERR_ARG; }
    HIP_TRY(hipSetDevice(st->ctx->device));
    hipStream_t s = st->ctx->stream;
    HIP_TRY(hipEventRecord(st->ev[0], s));
    if (st->n_windows) {
        hipLaunchKernelGGL(k_irep_windows, dim3((uint32_t)((st->n_windows + 255) / 256)), dim3(256), 0, s, st->d_gen, (int)st->n_gen,
                           st->n_windows, reinterpret_cast<const unsigned long long *>(st->d_cov), st->d_gc,
                           reinterpret_cast<unsigned long long *>(st->d_keys), st->d_gcw);
        HIP_TRY(hipGetLastError());
        size_t tb = st->temp_bytes + 256;
        HIP_TRY(rocprim::segmented_radix_sort_keys(st->d_temp, tb, st->d_keys, st->d_sorted, (unsigned)st->n_windows, (unsigned)st->n_gen,
                                                   st->d_seg, st->d_seg + 1, 0, 64, s));
    }
    hipLaunchKernelGGL(k_irep_fit, dim3((uint32_t)st->n_gen), dim3(256), 0, s, st->d_gen,
                       reinterpret_cast<const unsigned long long *>(st->d_cov), reinterpret_cast<const unsigned long long *>(st->d_sorted),
                       st->d_y, st->d_rows, st->d_state);
    HIP_TRY(hipGetLastError());
    if (st->n_windows) {
        // the GC stage: line, sort of the errors, line again without the largest, sort of the corrected coverage, the trimmed fit
        const dim3 grid((uint32_t)st->n_gen), blk(256);
        const unsigned long long *keys = reinterpret_cast<const unsigned long long *>(st->d_keys);
        for (int stage = 0; stage < 2; stage++) {
            hipLaunchKernelGGL(k_irep_gc_line, grid, blk, 0, s, st->d_gen, keys, st->d_gcw, st->d_val_sorted, st->d_val, st->d_state, stage);
            HIP_TRY(hipGetLastError());
            size_t tb = st->temp_bytes + 256;
            HIP_TRY(rocprim::segmented_radix_sort_keys(st->d_temp, tb, st->d_val, st->d_val_sorted, (unsigned)st->n_windows, (unsigned)st->n_gen,
                                                       st->d_seg, st->d_seg + 1, 0, 64, s));
        }
        hipLaunchKernelGGL(k_irep_gc_fit, grid, blk, 0, s, st->d_gen, st->d_val_sorted, st->d_state, st->d_y, st->d_rows);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(st->ev[1], s));
    HIP_TRY(hipMemcpyAsync(out, st->d_rows, (size_t)st->n_gen * sizeof(isx_irep_row), hipMemcpyDeviceToHost, s));
    HIP_TRY(isx_wait_stream(s));
    if (device_ms) { float v = 0.f; (void)hipEventElapsedTime(&v, st->ev[0], st->ev[1]); *device_ms = v; }
    return ISX_OK;
}

}  // extern "C"
