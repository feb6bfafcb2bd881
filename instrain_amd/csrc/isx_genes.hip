// isx_genes.hip -- gene profiling on the device (`inStrain profile -g genes.fna`).
//
// Replaces the per-gene pandas slices of
//   calc_gene_coverage / calc_gene_clonality   inStrain/GeneProfile.py (v1.9.1):352-422
//   count_sites                                GeneProfile.py:428-486
//   calc_gene_snp_counts                       GeneProfile.py:495-598
//   characterize_SNPs                          GeneProfile.py:600-707
// that the reference runs in its merge workers, one scaffold at a time (profile_utilities.py:385-396).
//
// Coverage half: one wave per gene and level over the per-position arrays the summary pass materialises (isx_summary.hip
// run_gene_cov); partials combine in a fixed shuffle tree, no float atomics.  SNV half: one lane per SNV row on rows in
// (gpos, mm) order -- a position's highest-mm row is classified by one codon lookup, every row is counted into each
// (covering gene, level) it is current for with integer atomics.  Sites: one lane per gene walks its codons in order.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "isx_internal.h"
#include "isx_summary.h"

namespace {

// gene letters as codes: A 0, C 1, G 2, T 3, N 4
struct CodeTables {
    uint8_t aa[128];        // [a * 25 + b * 5 + c] over codes 0..4: Biopython's Standard table with its ambiguity rule (ASCII)
    uint8_t s_cnt[64];      // [a * 16 + b * 4 + c] over codes 0..3: synonymous neighbours of the codon (count_sites, k = 1)
    uint8_t n_cnt[64];      //   non-synonymous neighbours (a stop neighbour counts as N)
    uint8_t stop[64];       //   the codon is a stop codon (count_sites skips it)
};

// standard genetic code, first / second / third base in T C A G order
const char *STD_CODE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";

char std_aa(int a, int b, int c)
{
    static const int tcag[4] = {2, 1, 3, 0};        // code (A C G T) -> index in T C A G order
    return STD_CODE[tcag[a] * 16 + tcag[b] * 4 + tcag[c]];
}

// Bio.Seq.translate on one codon of A/C/G/T/N letters (CodonTable.ambiguous_generic_by_name["Standard"] + _translate_str):
// every expansion of N codes the same amino acid -> that one; only stops -> '*'; stops and amino acids -> 'X' (pos_stop);
// several amino acids -> the smallest ambiguous letter holding all of them (B = D/N, Z = E/Q, J = I/L), else 'X'
char translate_codon(int a, int b, int c)
{
    std::string set;
    bool stop = false;
    for (int x = 0; x < 4; x++) {
        if (a != 4 && x != a) continue;
        for (int y = 0; y < 4; y++) {
            if (b != 4 && y != b) continue;
            for (int z = 0; z < 4; z++) {
                if (c != 4 && z != c) continue;
                const char aa = std_aa(x, y, z);
                if (aa == '*') stop = true;
                else if (set.find(aa) == std::string::npos) set.push_back(aa);
            }
        }
    }
    if (stop) return set.empty() ? '*' : 'X';
    if (set.size() == 1) return set[0];
    auto within = [&](const char *letters) {
        for (char x : set) if (!strchr(letters, x)) return false;
        return true;
    };
    if (within("DN")) return 'B';
    if (within("EQ")) return 'Z';
    if (within("IL")) return 'J';
    return 'X';
}

CodeTables make_tables()
{
    CodeTables t;
    memset(&t, 0, sizeof(t));
    for (int a = 0; a < 5; a++)
        for (int b = 0; b < 5; b++)
            for (int c = 0; c < 5; c++) t.aa[a * 25 + b * 5 + c] = (uint8_t)translate_codon(a, b, c);
    for (int i = 0; i < 64; i++) {
        const int cod[3] = {i >> 4, (i >> 2) & 3, i & 3};
        const char aa = std_aa(cod[0], cod[1], cod[2]);
        t.stop[i] = aa == '*';
        for (int p = 0; p < 3; p++)
            for (int x = 0; x < 4; x++) {
                if (x == cod[p]) continue;
                int nb[3] = {cod[0], cod[1], cod[2]};
                nb[p] = x;
                const char na = std_aa(nb[0], nb[1], nb[2]);
                if (na != '*' && na == aa) t.s_cnt[i]++;
                else t.n_cnt[i]++;
            }
    }
    return t;
}

const CodeTables &tables()
{
    static const CodeTables t = make_tables();
    return t;
}

__device__ __forceinline__ uint8_t comp_code(uint8_t x) { return x < 4 ? (uint8_t)(3 - x) : (uint8_t)4; }

// isx_snv base codes (0 A, 1 C, 2 T, 3 G, 4 other) -> gene letter codes
__device__ __forceinline__ uint8_t snv_to_code(uint8_t b)
{
    return b == 0 ? 0 : b == 1 ? 1 : b == 2 ? 3 : b == 3 ? 2 : 4;
}

__device__ __forceinline__ int seg_of(const int64_t *bounds, int n_seg, uint32_t g)
{
    int lo = 0, hi = n_seg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (bounds[mid] <= (int64_t)g) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- coverage half: one wave per call gene, this level ----
__global__ void __launch_bounds__(256) k_gene_cov(const GeneWork *work, uint32_t n_work, const uint32_t *cov, const float *cv,
                                                  int M, int mm, isx_gene_cov *rows)
{
    const uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= n_work) return;                                    // whole waves leave together
    const GeneWork g = work[w];
    unsigned long long sum = 0;
    uint32_t nz = 0, cnt = 0;
    double sc = 0.0;
    if (g.fe >= g.fs) {
        for (uint64_t p = (uint64_t)g.fs + lane; p <= g.fe; p += 64) {
            const uint32_t c = cov[p];
            sum += c;
            nz += c ? 1u : 0u;
            const float v = cv[p];
            if (v == v) { cnt++; sc += (double)v; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {                          // fixed tree: identical bytes run to run
        sum += (unsigned long long)__shfl_xor((long long)sum, o);
        nz += (uint32_t)__shfl_xor((int)nz, o);
        cnt += (uint32_t)__shfl_xor((int)cnt, o);
        sc += __shfl_xor(sc, o);
    }
    if (lane == 0) {
        isx_gene_cov r;
        r.sum_cov = sum; r.nonzero = nz; r.counted = cnt; r.sum_clon = sc;
        rows[(size_t)w * M + mm] = r;
    }
}

// every scaffold: does it have cumulative coverage / a clonality anywhere.  A wave takes 64 x 64 positions, lane l every 64th from
// l (coalesced loads), keeps its bits while its scaffold stays the same and flushes them with one atomic when it changes
__global__ void __launch_bounds__(256) k_scaffold_any(const uint32_t *cov, const float *cv, uint32_t n_pos, const int64_t *bounds,
                                                      int n_seg, uint32_t *flags)
{
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t p0 = wave * 4096 + lane;
    if (p0 >= n_pos) return;
    const uint64_t p1 = min((uint64_t)n_pos, wave * 4096 + 4096);
    int seg = seg_of(bounds, n_seg, (uint32_t)p0);
    uint32_t f = 0;
    for (uint64_t p = p0; p < p1; p += 64) {
        if ((int64_t)p >= bounds[seg + 1]) {
            if (f) atomicOr(&flags[seg], f);
            f = 0;
            seg = seg_of(bounds, n_seg, (uint32_t)p);
        }
        if (cov[p]) f |= ISX_GENE_COV_ANY;
        const float v = cv[p];
        if (v == v) f |= ISX_GENE_CLON_ANY;
    }
    if (f) atomicOr(&flags[seg], f);
}

// ---- SNV half ----
struct SnvGenes {
    const uint32_t *fs, *fe;        // call genes with something inside their scaffold, ascending fs
    const uint32_t *w;              // ... their call index
    uint32_t n;
    const uint32_t *maxlen;         // [n_seg] longest clipped gene of the scaffold: how far a position looks back
    const int64_t *bounds;
    int n_seg;
};

// the covering genes of gpos: f(call index) for each, in descending fs order
template <class F>
__device__ __forceinline__ void for_covering(const SnvGenes &G, uint32_t gpos, F f)
{
    uint32_t lo = 0, hi = G.n;                                  // first index with fs > gpos
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (G.fs[mid] <= gpos) lo = mid + 1; else hi = mid;
    }
    const int s = seg_of(G.bounds, G.n_seg, gpos);
    const int64_t reach = (int64_t)gpos - (int64_t)G.maxlen[s];   // a gene starting at or before this cannot reach gpos
    const int64_t s0 = G.bounds[s];
    for (uint32_t j = lo; j-- > 0;) {
        const int64_t fs = G.fs[j];
        if (fs <= reach || fs < s0) break;
        if (G.fe[j] >= gpos) f(G.w[j]);
    }
}

__global__ void __launch_bounds__(256) k_snv_classify(const isx_snv *snv, uint32_t n, SnvGenes G, const GeneWork *work,
                                                      const isx_gene *genes, const uint8_t *seq, CodeTables T, isx_gene_mutation *mut)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const isx_snv r = snv[i];
    isx_gene_mutation m;
    m.gene = -1; m.k = 0; m.type = 0; m.aa_old = 0; m.aa_new = 0; m.n_genes = 0; m.pad = 0;
    const bool last = i + 1 == n || snv[i + 1].gpos != r.gpos;
    if (!last || r.allele_count < 1 || r.allele_count > 2) { mut[i] = m; return; }
    uint32_t c = 0, first = 0xFFFFFFFFu;
    for_covering(G, r.gpos, [&](uint32_t w) { c++; first = min(first, w); });
    m.n_genes = (uint8_t)min(c, 255u);
    if (c == 0) { m.type = 'I'; mut[i] = m; return; }
    const GeneWork gw = work[first];
    m.gene = gw.gene;
    if (c > 1) { m.type = 'M'; mut[i] = m; return; }
    const isx_gene g = genes[gw.gene];
    const int64_t L = g.end - g.start + 1;
    const int64_t k = (int64_t)r.gpos - (int64_t)gw.fs;        // genome orientation, also on strand -1
    m.k = (int32_t)k;
    const bool fwd = g.strand >= 0;
    const uint8_t *s = seq + g.seq_off;
    const int64_t j = fwd ? k : L - 1 - k;                      // the letter in gene orientation
    const uint8_t ob = fwd ? s[j] : comp_code(s[j]);            // the scaffold-orientation base there
    uint8_t nb = snv_to_code(r.con_base);
    if (nb == ob) nb = snv_to_code(r.var_base);
    const int64_t c0 = j - j % 3;
    if (c0 + 3 > L) { m.type = 'S'; mut[i] = m; return; }      // the trailing partial codon translates to nothing
    uint8_t o[3] = {s[c0], s[c0 + 1], s[c0 + 2]}, x[3] = {o[0], o[1], o[2]};
    x[j - c0] = fwd ? nb : comp_code(nb);
    const uint8_t ao = T.aa[o[0] * 25 + o[1] * 5 + o[2]], an = T.aa[x[0] * 25 + x[1] * 5 + x[2]];
    if (ao != an) { m.type = 'N'; m.aa_old = ao; m.aa_new = an; }
    else m.type = 'S';
    mut[i] = m;
}

__global__ void __launch_bounds__(256) k_snv_count(const isx_snv *snv, uint32_t n, SnvGenes G, const isx_gene_mutation *mut,
                                                   int n_levels, uint32_t *cnt)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const isx_snv r = snv[i];
    uint32_t j = i;                                             // the position's highest-mm row: its type counts for every level
    while (j + 1 < n && snv[j + 1].gpos == r.gpos) j++;
    const uint8_t t = mut[j].type;
    const int next = (i + 1 < n && snv[i + 1].gpos == r.gpos) ? (int)snv[i + 1].mm : n_levels;
    const int ac = r.allele_count;
    for_covering(G, r.gpos, [&](uint32_t w) {
        for (int lv = r.mm; lv < next; lv++) {
            uint32_t *c = cnt + ((size_t)w * n_levels + lv) * 7;
            atomicAdd(&c[0], 1u);
            if (ac == 1 || ac == 2) {
                uint32_t *d = c + (ac == 1 ? 1 : 4);
                atomicAdd(&d[0], 1u);
                if (t == 'N') atomicAdd(&d[1], 1u);
                if (t == 'S') atomicAdd(&d[2], 1u);
            }
        }
    });
}

// ---- sites: one lane per gene, codons in order (the reference's summation order) ----
__global__ void __launch_bounds__(256) k_gene_sites(const isx_gene *genes, uint32_t n, const uint8_t *seq, CodeTables T, double *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const isx_gene g = genes[i];
    const int64_t L = g.end - g.start + 1;
    const uint8_t *s = seq + g.seq_off;
    double S = 0.0, N = 0.0;
    for (int64_t c = 0; c + 3 <= L; c += 3) {
        const uint8_t a = s[c], b = s[c + 1], d = s[c + 2];
        if (a > 3 || b > 3 || d > 3) continue;                  // a codon with N
        const int x = a * 16 + b * 4 + d;
        if (T.stop[x]) continue;
        S += (double)T.s_cnt[x] / 3.0;                          // norm_const = (S + N) / 3 = 3
        N += (double)T.n_cnt[x] / 3.0;
    }
    out[2 * (size_t)i] = S;
    out[2 * (size_t)i + 1] = N;
}

template <class T>
hipError_t dmalloc(T **p, size_t n) { return isx_raw_dev_malloc(p, std::max<size_t>(n, 1) * sizeof(T)); }

}  // namespace

void launch_gene_cov(hipStream_t s, const GeneWork *work, uint32_t n_work, const uint32_t *cov, const float *cv, int M, int mm,
                     isx_gene_cov *rows)
{
    if (!n_work) return;
    hipLaunchKernelGGL(k_gene_cov, dim3((n_work + 3) / 4), dim3(256), 0, s, work, n_work, cov, cv, M, mm, rows);
}

void launch_scaffold_any(hipStream_t s, const uint32_t *cov, const float *cv, uint32_t n_pos, const int64_t *bounds, int n_seg,
                         uint32_t *flags)
{
    const uint32_t waves = (n_pos + 4095) / 4096;
    if (waves) hipLaunchKernelGGL(k_scaffold_any, dim3((waves + 3) / 4), dim3(256), 0, s, cov, cv, n_pos, bounds, n_seg, flags);
}

int genes_build_work(const isx_genes *g, int32_t n_scaffolds, const int64_t *bounds, const int32_t *first, const int32_t *last,
                     std::vector<GeneWork> &work)
{
    if (!g || n_scaffolds <= 0 || !bounds || !first || !last || bounds[0] != 0) {
        isx_set_error("gene profiling: bad arguments (scaffold_bounds must start at 0)");
        return ISX_ERR_ARG;
    }
    if (bounds[n_scaffolds] > (int64_t)0xFFFFFFFFll) { isx_set_error("gene profiling: flat space beyond 2^32 positions"); return ISX_ERR_ARG; }
    work.clear();
    const int64_t n_genes = (int64_t)g->h.size();
    for (int s = 0; s < n_scaffolds; s++) {
        if (bounds[s + 1] <= bounds[s]) { isx_set_error("gene profiling: scaffold_bounds must be strictly ascending"); return ISX_ERR_ARG; }
        if (first[s] < 0 || last[s] < first[s] || last[s] > n_genes) {
            isx_set_error("gene profiling: gene range of scaffold " + std::to_string(s) + " outside the gene set");
            return ISX_ERR_ARG;
        }
        const int64_t len = bounds[s + 1] - bounds[s];
        for (int32_t i = first[s]; i < last[s]; i++) {
            const isx_gene &x = g->h[(size_t)i];
            GeneWork w;
            w.gene = i; w.scaf = s;
            const int64_t a = std::max<int64_t>(x.start, 0), b = std::min<int64_t>(x.end, len - 1);
            if (a <= b) { w.fs = (uint32_t)(bounds[s] + a); w.fe = (uint32_t)(bounds[s] + b); }
            else { w.fs = 1; w.fe = 0; }
            work.push_back(w);
        }
    }
    if (work.size() > 0x7FFFFFFFu) { isx_set_error("gene profiling: too many genes in one call"); return ISX_ERR_ARG; }
    return ISX_OK;
}

int run_gene_snvs(isx_genes *g, int32_t n_scaffolds, const int64_t *bounds, const std::vector<GeneWork> &work, int64_t n_snv,
                  const isx_snv *snv, int32_t n_levels, isx_gene_mutation *mut_out, isx_gene_snv_count *cnt_out, float *ms)
{
    static_assert(sizeof(isx_gene_snv_count) == 7 * sizeof(uint32_t), "counter rows are 7 words");
    hipStream_t s = g->stream;
    const size_t n_work = work.size();
    // host side: rows in (gpos, mm) order inside the flat space, levels in range
    for (int64_t i = 0; i < n_snv; i++) {
        if ((int64_t)snv[i].gpos >= bounds[n_scaffolds]) { isx_set_error("isx_genes_profile_snvs: SNV row outside the flat space"); return ISX_ERR_ARG; }
        if (snv[i].mm >= n_levels) { isx_set_error("isx_genes_profile_snvs: SNV row with mm >= n_levels"); return ISX_ERR_ARG; }
        if (i && (snv[i - 1].gpos > snv[i].gpos || (snv[i - 1].gpos == snv[i].gpos && snv[i - 1].mm >= snv[i].mm))) {
            isx_set_error("isx_genes_profile_snvs: SNV rows must be in (gpos, mm) order, one row per (gpos, mm)");
            return ISX_ERR_ARG;
        }
    }
    // genes by flat start (the search table) and every scaffold's longest gene (the look-back)
    std::vector<uint32_t> order;
    for (uint32_t w = 0; w < (uint32_t)n_work; w++) if (work[w].fe >= work[w].fs) order.push_back(w);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return work[a].fs < work[b].fs; });
    std::vector<uint32_t> fs(order.size()), fe(order.size()), maxlen((size_t)n_scaffolds, 0);
    for (size_t i = 0; i < order.size(); i++) {
        const GeneWork &w = work[order[i]];
        fs[i] = w.fs; fe[i] = w.fe;
        maxlen[(size_t)w.scaf] = std::max(maxlen[(size_t)w.scaf], w.fe - w.fs + 1);
    }
    const size_t n_cnt = n_work * (size_t)n_levels;
    isx_snv *d_snv = nullptr;
    GeneWork *d_work = nullptr;
    uint32_t *d_fs = nullptr, *d_fe = nullptr, *d_ord = nullptr, *d_max = nullptr, *d_cnt = nullptr;
    int64_t *d_b = nullptr;
    isx_gene_mutation *d_mut = nullptr;
    auto done = [&](int code) {
        void *ps[] = {d_snv, d_work, d_fs, d_fe, d_ord, d_max, d_cnt, d_b, d_mut};
        for (void *p : ps) if (p) isx_dev_free(p);
        return code;
    };
#define GN_TRY(expr) do { if ((expr) != hipSuccess) { isx_set_error(std::string("HIP error in the gene pass: ") + #expr); return done(ISX_ERR_HIP); } } while (0)
    GN_TRY(hipSetDevice(g->device));
    GN_TRY(dmalloc(&d_snv, (size_t)n_snv));
    GN_TRY(dmalloc(&d_work, n_work));
    GN_TRY(dmalloc(&d_fs, fs.size()));
    GN_TRY(dmalloc(&d_fe, fe.size()));
    GN_TRY(dmalloc(&d_ord, order.size()));
    GN_TRY(dmalloc(&d_max, (size_t)n_scaffolds));
    GN_TRY(dmalloc(&d_cnt, n_cnt * 7));
    GN_TRY(dmalloc(&d_b, (size_t)n_scaffolds + 1));
    GN_TRY(dmalloc(&d_mut, (size_t)n_snv));
    if (n_snv) GN_TRY(hipMemcpyAsync(d_snv, snv, (size_t)n_snv * sizeof(isx_snv), hipMemcpyHostToDevice, s));
    if (n_work) GN_TRY(hipMemcpyAsync(d_work, work.data(), n_work * sizeof(GeneWork), hipMemcpyHostToDevice, s));
    if (!order.empty()) {
        GN_TRY(hipMemcpyAsync(d_fs, fs.data(), fs.size() * 4, hipMemcpyHostToDevice, s));
        GN_TRY(hipMemcpyAsync(d_fe, fe.data(), fe.size() * 4, hipMemcpyHostToDevice, s));
        GN_TRY(hipMemcpyAsync(d_ord, order.data(), order.size() * 4, hipMemcpyHostToDevice, s));
    }
    GN_TRY(hipMemcpyAsync(d_max, maxlen.data(), maxlen.size() * 4, hipMemcpyHostToDevice, s));
    GN_TRY(hipMemcpyAsync(d_b, bounds, ((size_t)n_scaffolds + 1) * 8, hipMemcpyHostToDevice, s));
    GN_TRY(hipMemsetAsync(d_cnt, 0, std::max<size_t>(n_cnt, 1) * 7 * 4, s));
    SnvGenes G;
    G.fs = d_fs; G.fe = d_fe; G.w = d_ord; G.n = (uint32_t)order.size(); G.maxlen = d_max; G.bounds = d_b; G.n_seg = n_scaffolds;
    GN_TRY(hipEventRecord(g->ev[0], s));
    if (n_snv) {
        const dim3 grid((uint32_t)((n_snv + 255) / 256));
        hipLaunchKernelGGL(k_snv_classify, grid, dim3(256), 0, s, d_snv, (uint32_t)n_snv, G, d_work, g->d, g->d_seq, tables(), d_mut);
        hipLaunchKernelGGL(k_snv_count, grid, dim3(256), 0, s, d_snv, (uint32_t)n_snv, G, d_mut, (int)n_levels, d_cnt);
        GN_TRY(hipGetLastError());
    }
    GN_TRY(hipEventRecord(g->ev[1], s));
    if (n_snv) GN_TRY(hipMemcpyAsync(mut_out, d_mut, (size_t)n_snv * sizeof(isx_gene_mutation), hipMemcpyDeviceToHost, s));
    if (n_cnt) GN_TRY(hipMemcpyAsync(cnt_out, d_cnt, n_cnt * sizeof(isx_gene_snv_count), hipMemcpyDeviceToHost, s));
    GN_TRY(isx_wait_stream(s));
#undef GN_TRY
    if (ms) { float v = 0.f; (void)hipEventElapsedTime(&v, g->ev[0], g->ev[1]); *ms = v; }
    return done(ISX_OK);
}

int run_gene_sites(isx_genes *g, double *sites, float *ms)
{
    hipStream_t s = g->stream;
    const size_t n = g->h.size();
    double *d_out = nullptr;
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(dmalloc(&d_out, 2 * n));
    HIP_TRY(hipEventRecord(g->ev[0], s));
    if (n) hipLaunchKernelGGL(k_gene_sites, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, g->d, (uint32_t)n, g->d_seq, tables(), d_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(g->ev[1], s);
    if (e == hipSuccess && n) e = hipMemcpyAsync(sites, d_out, 2 * n * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = isx_wait_stream(s);
    isx_dev_free(d_out);
    if (e != hipSuccess) { isx_set_error(std::string("HIP error in isx_genes_sites: ") + hipGetErrorString(e)); return ISX_ERR_HIP; }
    if (ms) { float v = 0.f; (void)hipEventElapsedTime(&v, g->ev[0], g->ev[1]); *ms = v; }
    return ISX_OK;
}
