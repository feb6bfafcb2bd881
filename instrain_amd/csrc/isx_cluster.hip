// isx_cluster.hip -- strain clustering per genome (`inStrain compare`'s strain_clusters.tsv), every genome of a call at once.
//
// Replaces
//   _genome_wide_readComparer (mm_level off)     inStrain/genomeUtilities.py:739-800   (k_cmpset_genome_pairs: the pair roll-up)
//   cluster_genome_strains, add_av_RC            inStrain/compare_utils.py:169-268     (membership, order, the skipped genomes, the matrix)
//   scipy.cluster.hierarchy.linkage              average / complete / weighted: the NN-chain, its stable sort, its relabel
//   scipy.cluster.hierarchy.fcluster             criterion='distance'
// One problem (genome) per workgroup: a single wave up to 64 points, 256 threads beyond; the condensed fp64 matrix lives in LDS up to
// ISX_CLUSTER_LDS_MAX_POINTS points and in a global workspace beyond.  The scans (nearest neighbour, row update, rank sort) are spread
// over the lanes; the relabel and the tree walk are O(n) on one lane.  Every float is an IEEE double made by one operation at a time
// (-ffp-contract=off) in the order of DESIGN section 15, so the bytes equal tests/cluster_ref.py's and scipy's.  Every loop is bounded:
// a merge that does not close within 2n scans, or a walk that outlives 4n steps, sets ISX_CLUSTER_ERROR and the workgroup leaves.
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "isx_compare_set.h"

using namespace isxset;

namespace {

enum : int32_t { M_AVERAGE = 0, M_COMPLETE = 1, M_WEIGHTED = 2 };
constexpr int WAVE_MAX = 64, LDS_MAX = ISX_CLUSTER_LDS_MAX_POINTS, N_MAX = ISX_CLUSTER_MAX_POINTS;
constexpr size_t WORKSPACE_BUDGET = (size_t)256 << 20;      // bytes of global matrices one launch of the largest variant may use

struct ClusterArgs {
    const int32_t *items;               // the launch's problems: workgroup b works on items[b]
    int32_t n_items, method;
    double cutoff;
    double *work;                       // the variant without an LDS matrix: workgroup b owns work[b * work_stride ...]
    int64_t work_stride;
    // table form (gpairs == NULL)
    const int32_t *n_points;
    const int64_t *val_off, *pt_off;    // first value / first point of every problem
    const double *values;
    // set form
    const isx_genome_pair *gpairs;      // [genome][pair]
    int32_t S;
    int64_t P;
    const int32_t *by_rank;             // [S] the samples in the order of their names
    const double *glen;
    double cov_thr;
    // out
    int32_t *labels;                    // table: [pt_off[p] + i]; set: [genome][S]
    double *Z;                          // table: rows from pt_off[p] - p (may be NULL); set: rows from genome * (S - 1)
    isx_cluster_status *status;
};

__host__ __device__ __forceinline__ int64_t cidx(int64_t n, int64_t i, int64_t j)      // i < j
{
    return n * i - i * (i + 1) / 2 + (j - i - 1);
}
__device__ __forceinline__ int64_t cidx_any(int n, int i, int j) { return i < j ? cidx(n, i, j) : cidx(n, j, i); }

template <int BLOCK>
__device__ __forceinline__ void bsync()
{
    if (BLOCK == 64) {                  // one wave: lockstep, only the compiler and the LDS queue have to be held in order
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

template <int BLOCK>
__device__ __forceinline__ bool bany(bool p)
{
    if (BLOCK == 64) return __any(p ? 1 : 0) != 0;
    return __syncthreads_or(p ? 1 : 0) != 0;
}

// the smallest key (distance, index) of the workgroup, left in every thread
template <int BLOCK>
__device__ __forceinline__ void bargmin(double &d, int &i, double *red_d, int *red_i)
{
    for (int off = 32; off; off >>= 1) {
        const double od = __shfl_xor(d, off);
        const int oi = __shfl_xor(i, off);
        if (od < d || (od == d && oi < i)) { d = od; i = oi; }
    }
    if (BLOCK > 64) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) { red_d[wave] = d; red_i[wave] = i; }
        __syncthreads();
        d = red_d[0]; i = red_i[0];
        for (int w = 1; w < BLOCK / 64; w++) {
            const double od = red_d[w];
            const int oi = red_i[w];
            if (od < d || (od == d && oi < i)) { d = od; i = oi; }
        }
        __syncthreads();                // (the next reduction writes red_* again)
    }
}

__device__ __forceinline__ double new_dist(int method, double d_xi, double d_yi, int nx, int ny)
{
    if (method == M_AVERAGE) return ((double)nx * d_xi + (double)ny * d_yi) / (double)(nx + ny);
    if (method == M_COMPLETE) return d_xi > d_yi ? d_xi : d_yi;
    return (d_xi + d_yi) / 2.0;
}

__device__ __forceinline__ int uf_find(int *parent, int v, int n)
{
    const int first = v;
    for (int it = 0; it < 2 * n && parent[v] != v; it++) v = parent[v];
    int p = first;
    for (int it = 0; it < 2 * n && p != v && parent[p] != v; it++) {
        const int up = parent[p];
        parent[p] = v;
        p = up;
    }
    return v;
}

// one thread per scaffold: some pair failed on it (SampleSet.compare leaves the whole scaffold out)
__global__ void k_cmpset_failed_any(const uint32_t *failed, int64_t P, int n_scaf, uint8_t *sc_failed)
{
    const int sc = blockIdx.x * blockDim.x + threadIdx.x;
    if (sc >= n_scaf) return;
    uint32_t any = 0;
    for (int64_t p = 0; p < P; p++) any |= failed[p * n_scaf + sc];
    sc_failed[sc] = any ? 1 : 0;
}

// rule 1.  One thread per (genome, pair): the genome's scaffolds in set order, of each the row at the highest axis level that is a key
// of either sample; integers and the sequential fp64 sum, no atomics
__global__ void __launch_bounds__(256) k_cmpset_genome_pairs(const int2 *pairs, int64_t P, int G, const int32_t *g_off, const int32_t *g_sc,
                                                             int n_scaf, int A, const uint8_t *pres, const unsigned long long *cnt,
                                                             const unsigned long long *pop, const uint8_t *sc_failed, isx_genome_pair *out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)G * P) return;
    const int g = (int)(t / P);
    const int64_t p = t - (int64_t)g * P;
    const int2 pr = pairs[p];
    int64_t tcb = 0;
    double w = 0.0;
    int rows = 0;
    for (int q = g_off[g]; q < g_off[g + 1]; q++) {
        const int sc = g_sc[q];
        if (sc < 0 || sc >= n_scaf || sc_failed[sc]) continue;
        const uint8_t *pa = pres + ((size_t)pr.x * n_scaf + sc) * A, *pb = pres + ((size_t)pr.y * n_scaf + sc) * A;
        bool has_a = false, has_b = false;
        int top = -1;
        for (int k = 0; k < A; k++) {
            has_a |= pa[k] != 0; has_b |= pb[k] != 0;
            if (pa[k] || pb[k]) top = k;
        }
        if (!has_a || !has_b) continue;
        const size_t o = ((size_t)p * n_scaf + sc) * A + top;
        const int64_t both = (int64_t)cnt[o], snps = (int64_t)pop[o];
        tcb += both;
        rows++;
        if (both > 0) w = w + ((double)(both - snps) / (double)both) * (double)both;
    }
    isx_genome_pair r;
    r.tcb = tcb; r.w = w; r.n_rows = rows; r.pad = 0;
    out[t] = r;
}

// rules 2-6 for one problem per workgroup.  BLOCK threads, at most NCAP points, the matrix in LDS (LDSM) or in the launch's workspace
template <int BLOCK, int NCAP, bool LDSM>
__global__ void __launch_bounds__(BLOCK) k_cluster_genomes(const ClusterArgs a)
{
    __shared__ double s_m[LDSM ? NCAP * (NCAP - 1) / 2 : 1];
    __shared__ double s_mh[NCAP], s_zh[NCAP], s_crit[NCAP], s_red_d[4];
    __shared__ int s_size[NCAP], s_chain[NCAP], s_ma[NCAP], s_mb[NCAP], s_zl[NCAP], s_zr[NCAP], s_pts[NCAP];
    __shared__ int s_parent[2 * NCAP], s_count[2 * NCAP], s_red_i[4], s_n, s_err;
    if ((int)blockIdx.x >= a.n_items) return;
    const int prob = a.items[blockIdx.x], tid = threadIdx.x;
    double *M = LDSM ? s_m : a.work + (int64_t)blockIdx.x * a.work_stride;
    const bool from_set = a.gpairs != nullptr;
    int n;
    int32_t *out_labels;
    double *out_Z;

    if (from_set) {
        // rule 2: the genome's samples, by name; rule 3: the genomes that are not clustered; rule 4: the matrix
        const int S = a.S;
        if (S > NCAP) {                                                         // (the host sends such a set to a larger variant)
            if (tid == 0) a.status[prob] = {ISX_CLUSTER_ERROR, 0};
            return;
        }
        const isx_genome_pair *gp = a.gpairs + (int64_t)prob * a.P;
        bool zero = false;
        for (int s = tid; s < S; s += BLOCK) {
            int member = 0;
            for (int t = 0; t < S; t++) {
                if (t == s) continue;
                const isx_genome_pair *v = gp + cidx_any(S, s, t);
                if (v->n_rows > 0) {
                    member = 1;
                    if (v->tcb == 0) zero = true;
                }
            }
            s_ma[s] = member;
        }
        zero = bany<BLOCK>(zero);
        bsync<BLOCK>();
        if (tid == 0) {
            int k = 0;
            for (int r = 0; r < S; r++) {
                const int s = a.by_rank[r];
                if (s >= 0 && s < S && s_ma[s] && k < NCAP) s_pts[k++] = s;
            }
            s_n = k;
        }
        bsync<BLOCK>();
        n = s_n;
        out_labels = a.labels + (int64_t)prob * S;
        out_Z = a.Z + (int64_t)prob * (S - 1) * 4;
        for (int s = tid; s < S; s += BLOCK) out_labels[s] = 0;
        bool missing = false;
        if (n >= 2 && !zero) {
            const double len = a.glen[prob];
            for (int i = 0; i + 1 < n; i++)
                for (int j = i + 1 + tid; j < n; j += BLOCK) {
                    const isx_genome_pair v = gp[cidx_any(S, s_pts[i], s_pts[j])];
                    double d = 0.0;
                    if (v.n_rows == 0) {
                        missing = true;
                    } else {
                        const double pc = (double)v.tcb / len;
                        d = pc < a.cov_thr ? 1.0 : 1.0 - v.w / (double)v.tcb;
                    }
                    M[cidx(n, i, j)] = d;
                }
        }
        missing = bany<BLOCK>(missing);
        const int status = n < 2 ? ISX_CLUSTER_EMPTY : zero ? ISX_CLUSTER_NO_OVERLAP : missing ? ISX_CLUSTER_MISSING_PAIR : ISX_CLUSTER_OK;
        if (status != ISX_CLUSTER_OK) {                                         // (workgroup-uniform)
            if (tid == 0) a.status[prob] = {status, n};
            return;
        }
    } else {
        n = a.n_points[prob];
        if (n < 2 || n > NCAP) {                                                // (the host has checked)
            if (tid == 0) a.status[prob] = {ISX_CLUSTER_ERROR, n};
            return;
        }
        const double *src = a.values + a.val_off[prob];
        for (int e = tid; e < n * (n - 1) / 2; e += BLOCK) M[e] = src[e];
        out_labels = a.labels + a.pt_off[prob];
        out_Z = a.Z ? a.Z + (a.pt_off[prob] - prob) * 4 : nullptr;
    }
    for (int i = tid; i < n; i += BLOCK) s_size[i] = 1;
    for (int v = tid; v < 2 * n - 1; v += BLOCK) { s_parent[v] = v; s_count[v] = 1; }
    if (tid == 0) s_err = 0;
    bsync<BLOCK>();

    // rule 5: the NN-chain.  chain_len, x, y, cur are the same in every thread; the chain itself is in LDS, written by thread 0
    const double INF = __longlong_as_double(0x7FF0000000000000ll);
    int chain_len = 0;
    bool bad = false;
    for (int k = 0; k < n - 1 && !bad; k++) {
        if (chain_len == 0) {
            double d = INF;
            int first = INT_MAX;
            for (int i = tid; i < n; i += BLOCK)
                if (s_size[i] > 0 && i < first) { d = 0.0; first = i; }
            bargmin<BLOCK>(d, first, s_red_d, s_red_i);
            if (first >= n) { bad = true; break; }
            if (tid == 0) s_chain[0] = first;
            chain_len = 1;
            bsync<BLOCK>();
        }
        int x = -1, y = -1;
        double cur = INF;
        bool closed = false;
        for (int scan = 0; scan < 2 * n; scan++) {
            x = s_chain[chain_len - 1];
            const int pred = chain_len > 1 ? s_chain[chain_len - 2] : -1;
            const double seed = pred >= 0 ? M[cidx_any(n, x, pred)] : INF;
            double bd = INF;
            int bi = INT_MAX;
            for (int i = tid; i < n; i += BLOCK) {
                if (s_size[i] == 0 || i == x) continue;
                const double d = M[cidx_any(n, x, i)];
                if (d < bd) { bd = d; bi = i; }
            }
            bargmin<BLOCK>(bd, bi, s_red_d, s_red_i);
            if (bd < seed && bi < n) { y = bi; cur = bd; } else { y = pred; cur = seed; }
            if (pred >= 0 && y == pred) { closed = true; break; }
            if (y < 0 || chain_len >= n) break;
            if (tid == 0) s_chain[chain_len] = y;
            chain_len++;
            bsync<BLOCK>();
        }
        if (!closed) { bad = true; break; }
        chain_len -= 2;
        if (x > y) { const int t = x; x = y; y = t; }
        const int nx = s_size[x], ny = s_size[y];
        bsync<BLOCK>();
        if (tid == 0) {
            s_ma[k] = x; s_mb[k] = y; s_mh[k] = cur;
            s_size[x] = 0; s_size[y] = nx + ny;
        }
        bsync<BLOCK>();
        for (int i = tid; i < n; i += BLOCK) {
            if (s_size[i] == 0 || i == y) continue;
            const int64_t iy = cidx_any(n, i, y);
            M[iy] = new_dist(a.method, M[cidx_any(n, i, x)], M[iy], nx, ny);
        }
        bsync<BLOCK>();
    }
    if (bad) {                                                                  // (workgroup-uniform)
        if (tid == 0) a.status[prob] = {ISX_CLUSTER_ERROR, n};
        return;
    }

    // the stable sort by height: every merge counts the merges that come before it
    for (int e = tid; e < n - 1; e += BLOCK) {
        const double he = s_mh[e];
        int r = 0;
        for (int j = 0; j < n - 1; j++) {
            const double hj = s_mh[j];
            r += (hj < he || (hj == he && j < e)) ? 1 : 0;
        }
        s_chain[r] = e;
    }
    bsync<BLOCK>();

    // the relabel (merge k becomes cluster n + k, the smaller id left), the criterion of rule 6 and the walk: one lane, O(n)
    if (tid == 0) {
        for (int k = 0; k < n - 1; k++) {
            const int o = s_chain[k];
            int l = uf_find(s_parent, s_ma[o], n), r = uf_find(s_parent, s_mb[o], n);
            if (l > r) { const int t = l; l = r; r = t; }
            s_parent[l] = n + k; s_parent[r] = n + k;
            s_count[n + k] = s_count[l] + s_count[r];
            s_zl[k] = l; s_zr[k] = r; s_zh[k] = s_mh[o];
            double m = s_mh[o];
            if (l >= n && s_crit[l - n] > m) m = s_crit[l - n];
            if (r >= n && s_crit[r - n] > m) m = s_crit[r - n];
            s_crit[k] = m;
        }
        int *stack = s_chain, *visited = s_size, *lab = s_ma;                   // (the chain, the sizes and the raw merges are done with)
        for (int i = 0; i < n; i++) { visited[i] = 0; lab[i] = 0; }
        int top = 0, leader = -1, n_cluster = 0, it = 0;
        stack[0] = n - 2;
        for (; it < 4 * n && top >= 0; it++) {
            const int root = stack[top], lc = s_zl[root], rc = s_zr[root];
            if (leader == -1 && s_crit[root] <= a.cutoff) { leader = root; n_cluster++; }
            if (lc >= n && !visited[lc - n] && top + 1 < n) { visited[lc - n] = 1; stack[++top] = lc - n; continue; }
            if (rc >= n && !visited[rc - n] && top + 1 < n) { visited[rc - n] = 1; stack[++top] = rc - n; continue; }
            if (lc < n) { if (leader == -1) n_cluster++; lab[lc] = n_cluster; }
            if (rc < n) { if (leader == -1) n_cluster++; lab[rc] = n_cluster; }
            if (leader == root) leader = -1;
            top--;
        }
        if (top >= 0) s_err = 1;
    }
    bsync<BLOCK>();
    if (s_err) {
        if (tid == 0) a.status[prob] = {ISX_CLUSTER_ERROR, n};
        return;
    }
    for (int i = tid; i < n; i += BLOCK) out_labels[from_set ? s_pts[i] : i] = s_ma[i];
    if (out_Z)
        for (int k = tid; k < n - 1; k += BLOCK) {
            out_Z[4 * (int64_t)k + 0] = (double)s_zl[k]; out_Z[4 * (int64_t)k + 1] = (double)s_zr[k];
            out_Z[4 * (int64_t)k + 2] = s_zh[k]; out_Z[4 * (int64_t)k + 3] = (double)s_count[n + k];
        }
    if (tid == 0) a.status[prob] = {ISX_CLUSTER_OK, n};
}

int method_of(const char *who, const char *name, int32_t *method)
{
    static const char *known[] = {"average", "complete", "weighted"};
    static const char *other[] = {"single", "centroid", "median", "ward"};
    if (name)
        for (int k = 0; k < 3; k++)
            if (!strcmp(name, known[k])) { *method = k; return ISX_OK; }
    std::string msg = std::string(who) + ": clustering method '" + (name ? name : "(null)") + "' is not supported";
    if (name)
        for (const char *o : other)
            if (!strcmp(name, o)) msg += " (scipy runs another algorithm for it than the NN-chain this library restates)";
    isx_set_error(msg + "; supported: average, complete, weighted");
    return ISX_ERR_ARG;
}

// the launches of one call: the problems by size class; glob_cap = the largest n among `glob` (the stride of its workspace)
struct Classes { std::vector<int32_t> wave, lds, glob; int glob_cap = 0; };

int launch_classes(const Classes &c, ClusterArgs a, SetBuf<int32_t> &d_items, SetBuf<double> &d_work, hipStream_t s)
{
    std::vector<int32_t> all(c.wave);
    all.insert(all.end(), c.lds.begin(), c.lds.end());
    all.insert(all.end(), c.glob.begin(), c.glob.end());
    if (all.empty()) return ISX_OK;
    HIP_TRY(d_items.put(all, s));
    if (!c.wave.empty()) {
        a.items = d_items.p; a.n_items = (int32_t)c.wave.size();
        hipLaunchKernelGGL((k_cluster_genomes<64, WAVE_MAX, true>), dim3((unsigned)c.wave.size()), dim3(64), 0, s, a);
    }
    if (!c.lds.empty()) {
        a.items = d_items.p + c.wave.size(); a.n_items = (int32_t)c.lds.size();
        hipLaunchKernelGGL((k_cluster_genomes<256, LDS_MAX, true>), dim3((unsigned)c.lds.size()), dim3(256), 0, s, a);
    }
    if (!c.glob.empty()) {
        const int64_t stride = std::max<int64_t>(1, (int64_t)c.glob_cap * (c.glob_cap - 1) / 2);
        const size_t chunk = std::max<size_t>(1, std::min<size_t>(c.glob.size(), WORKSPACE_BUDGET / ((size_t)stride * 8)));
        HIP_TRY(d_work.fit(chunk * (size_t)stride));
        a.work = d_work.p; a.work_stride = stride;
        for (size_t at = 0; at < c.glob.size(); at += chunk) {                  // (same stream: a chunk has the workspace to itself)
            const size_t m = std::min(chunk, c.glob.size() - at);
            a.items = d_items.p + c.wave.size() + c.lds.size() + at; a.n_items = (int32_t)m;
            hipLaunchKernelGGL((k_cluster_genomes<256, N_MAX, false>), dim3((unsigned)m), dim3(256), 0, s, a);
        }
    }
    return ISX_OK;
}

int report_errors(const char *who, const std::vector<isx_cluster_status> &status)
{
    for (size_t k = 0; k < status.size(); k++)
        if (status[k].status == ISX_CLUSTER_ERROR) {
            isx_set_error(std::string(who) + ": problem " + std::to_string(k) + " left its bounds (the neighbour chain did not close within 2n scans)");
            return ISX_ERR_HIP;
        }
    return ISX_OK;
}

}  // namespace

namespace isxset {

void cmpset_cluster_drop(isx_cmpset *st)
{
    st->d_gpairs.drop(); st->d_clZ.drop();
    st->clustered = false; st->cl_status.clear();
}

}  // namespace isxset

extern "C" {

int isx_cluster_linkage(isx_ctx *ctx, int32_t n_problems, const int32_t *n_points, const int64_t *offsets, const double *values,
                        int64_t n_values, const char *method, double cutoff, int32_t *labels, double *Z, float *device_ms)
{
    const char *who = "isx_cluster_linkage";
    if (!ctx || n_problems < 0 || (n_problems && (!n_points || !offsets || !values || !labels)) || n_values < 0 || cutoff != cutoff) {
        isx_set_error("isx_cluster_linkage: bad argument");
        return ISX_ERR_ARG;
    }
    int32_t m = 0;
    int rc = method_of(who, method, &m);
    if (rc) return rc;
    if (device_ms) *device_ms = 0.f;
    if (!n_problems) return ISX_OK;
    Classes c;
    std::vector<int64_t> pt_off((size_t)n_problems + 1, 0);
    for (int32_t p = 0; p < n_problems; p++) {
        const int64_t n = n_points[p];
        if (n < 2) { isx_set_error("isx_cluster_linkage: problem " + std::to_string(p) + " has fewer than two points"); return ISX_ERR_ARG; }
        if (n > N_MAX) {
            isx_set_error("isx_cluster_linkage: problem " + std::to_string(p) + " has " + std::to_string(n) + " points, more than ISX_CLUSTER_MAX_POINTS");
            return ISX_ERR_CAPACITY;
        }
        const int64_t len = n * (n - 1) / 2;
        if (offsets[p] < 0 || offsets[p] > n_values - len) {
            isx_set_error("isx_cluster_linkage: the condensed matrix of problem " + std::to_string(p) + " (" + std::to_string(len) +
                          " values from " + std::to_string(offsets[p]) + ") does not lie inside the " + std::to_string(n_values) + " values");
            return ISX_ERR_ARG;
        }
        for (int64_t e = 0; e < len; e++)
            if (!std::isfinite(values[offsets[p] + e])) {
                isx_set_error("isx_cluster_linkage: the condensed matrix of problem " + std::to_string(p) + " holds a value that is not finite");
                return ISX_ERR_ARG;
            }
        pt_off[(size_t)p + 1] = pt_off[(size_t)p] + n;
        if (n <= WAVE_MAX) c.wave.push_back(p);
        else if (n <= LDS_MAX) c.lds.push_back(p);
        else { c.glob.push_back(p); c.glob_cap = std::max(c.glob_cap, (int)n); }
    }
    const size_t n_pts = (size_t)pt_off[(size_t)n_problems], n_z = (n_pts - (size_t)n_problems) * 4;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    SetBuf<int32_t> d_np, d_items, d_labels;
    SetBuf<int64_t> d_voff, d_poff;
    SetBuf<double> d_values, d_Z, d_work;
    SetBuf<isx_cluster_status> d_status;
    hipEvent_t ev[2] = {nullptr, nullptr};
    auto done = [&](int r) {
        d_np.drop(); d_items.drop(); d_labels.drop(); d_voff.drop(); d_poff.drop(); d_values.drop(); d_Z.drop(); d_work.drop(); d_status.drop();
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        return r;
    };
#define CL_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { isx_set_error(std::string("isx_cluster_linkage: ") + #expr + ": " + hipGetErrorString(_e)); isx_read_drop(); return done(ISX_ERR_HIP); } } while (0)
    CL_TRY(hipEventCreate(&ev[0])); CL_TRY(hipEventCreate(&ev[1]));
    const std::vector<int32_t> h_np(n_points, n_points + n_problems);          // (alive until the stream has been waited for)
    const std::vector<int64_t> h_voff(offsets, offsets + n_problems);
    CL_TRY(d_np.put(h_np, s));
    CL_TRY(d_voff.put(h_voff, s));
    CL_TRY(d_poff.put(pt_off, s));
    CL_TRY(d_values.fit((size_t)n_values));
    if (n_values) CL_TRY(hipMemcpyAsync(d_values.p, values, (size_t)n_values * 8, hipMemcpyHostToDevice, s));
    CL_TRY(d_labels.fit(n_pts)); CL_TRY(d_Z.fit(n_z)); CL_TRY(d_status.fit((size_t)n_problems));
    CL_TRY(hipMemsetAsync(d_labels.p, 0, n_pts * 4, s));
    CL_TRY(hipMemsetAsync(d_status.p, 0xFF, (size_t)n_problems * sizeof(isx_cluster_status), s));
    ClusterArgs a{};
    a.method = m; a.cutoff = cutoff; a.n_points = d_np.p; a.val_off = d_voff.p; a.pt_off = d_poff.p; a.values = d_values.p;
    a.labels = d_labels.p; a.Z = d_Z.p; a.status = d_status.p;
    CL_TRY(hipEventRecord(ev[0], s));
    rc = launch_classes(c, a, d_items, d_work, s);
    if (rc) return done(rc);
    CL_TRY(hipEventRecord(ev[1], s));
    std::vector<isx_cluster_status> status((size_t)n_problems);
    CL_TRY(hipMemcpyAsync(status.data(), d_status.p, status.size() * sizeof(isx_cluster_status), hipMemcpyDeviceToHost, s));
    CL_TRY(hipMemcpyAsync(labels, d_labels.p, n_pts * 4, hipMemcpyDeviceToHost, s));
    if (Z && n_z) CL_TRY(hipMemcpyAsync(Z, d_Z.p, n_z * 8, hipMemcpyDeviceToHost, s));
    CL_TRY(isx_wait_stream(s));
    CL_TRY(hipGetLastError());
#undef CL_TRY
    if (device_ms) (void)hipEventElapsedTime(device_ms, ev[0], ev[1]);
    for (isx_cluster_status &x : status)
        if (x.status != ISX_CLUSTER_OK) x.status = ISX_CLUSTER_ERROR;          // (a problem no workgroup wrote counts as one that failed)
    return done(report_errors(who, status));
}

int isx_cmpset_cluster(isx_cmpset *st, int32_t n_genomes, const int32_t *scaffold_genome, const double *genome_lengths,
                       const int32_t *sample_rank, const char *method, double cutoff, double coverage_treshold, isx_cluster_status *status,
                       int32_t *labels, float *device_ms)
{
    const char *who = "isx_cmpset_cluster";
    if (!st || n_genomes <= 0 || !scaffold_genome || !genome_lengths || !sample_rank || !status || !labels || cutoff != cutoff ||
        coverage_treshold != coverage_treshold) {
        isx_set_error("isx_cmpset_cluster: bad argument");
        return ISX_ERR_ARG;
    }
    int32_t m = 0;
    int rc = method_of(who, method, &m);
    if (rc) return rc;
    if (device_ms) *device_ms = 0.f;
    if (!st->compared) { isx_set_error("isx_cmpset_cluster: call isx_cmpset_compare first (and again after an add)"); return ISX_ERR_STATE; }
    const int32_t S = (int32_t)st->samples.size(), n_scaf = st->n_scaf, A = st->A, G = n_genomes;
    if (S > N_MAX) {
        isx_set_error("isx_cmpset_cluster: the set has " + std::to_string(S) + " samples, more than ISX_CLUSTER_MAX_POINTS");
        return ISX_ERR_CAPACITY;
    }
    const int64_t P = (int64_t)S * (S - 1) / 2;
    if (S < 2 || A <= 0) { isx_set_error("isx_cmpset_cluster: the last compare had no pair"); return ISX_ERR_STATE; }
    std::vector<int32_t> by_rank((size_t)S, -1);
    for (int32_t i = 0; i < S; i++) {
        const int32_t r = sample_rank[i];
        if (r < 0 || r >= S || by_rank[(size_t)r] != -1) { isx_set_error("isx_cmpset_cluster: sample_rank must be a permutation of 0 .. n_samples - 1"); return ISX_ERR_ARG; }
        by_rank[(size_t)r] = i;
    }
    std::vector<int32_t> g_off((size_t)G + 1, 0), g_sc;
    for (int32_t sc = 0; sc < n_scaf; sc++) {
        const int32_t g = scaffold_genome[sc];
        if (g < -1 || g >= G) { isx_set_error("isx_cmpset_cluster: scaffold_genome[" + std::to_string(sc) + "] names no genome of the call"); return ISX_ERR_ARG; }
        if (g >= 0) g_off[(size_t)g + 1]++;
    }
    for (int32_t g = 0; g < G; g++) g_off[(size_t)g + 1] += g_off[(size_t)g];
    g_sc.assign((size_t)g_off[(size_t)G], 0);
    {
        std::vector<int32_t> at(g_off.begin(), g_off.end() - 1);
        for (int32_t sc = 0; sc < n_scaf; sc++)
            if (scaffold_genome[sc] >= 0) g_sc[(size_t)at[(size_t)scaffold_genome[sc]]++] = sc;       // (ascending: set order)
    }
    if (((int64_t)G * P + 255) / 256 > 0x7FFFFFFFll) { isx_set_error("isx_cmpset_cluster: too many genomes x pairs for one launch"); return ISX_ERR_CAPACITY; }
    std::vector<int2> pairs;
    pairs.reserve((size_t)P);
    for (int32_t i = 0; i < S; i++)
        for (int32_t j = i + 1; j < S; j++) pairs.push_back(make_int2(i, j));

    HIP_TRY(hipSetDevice(st->ctx->device));
    hipStream_t s = st->ctx->stream;
    cmpset_cluster_drop(st);
    SetBuf<int2> d_pairs;
    SetBuf<int32_t> d_goff, d_gsc, d_rank, d_items, d_labels;
    SetBuf<uint8_t> d_scfail;
    SetBuf<double> d_len, d_work;
    SetBuf<isx_cluster_status> d_status;
    auto done = [&](int r) {
        d_pairs.drop(); d_goff.drop(); d_gsc.drop(); d_rank.drop(); d_items.drop(); d_labels.drop(); d_scfail.drop(); d_len.drop(); d_work.drop();
        d_status.drop();
        if (r) cmpset_cluster_drop(st);
        return r;
    };
#define CS_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { isx_set_error(std::string("isx_cmpset_cluster: ") + #expr + ": " + hipGetErrorString(_e)); isx_read_drop(); return done(ISX_ERR_HIP); } } while (0)
    CS_TRY(d_pairs.put(pairs, s)); CS_TRY(d_goff.put(g_off, s)); CS_TRY(d_gsc.put(g_sc, s)); CS_TRY(d_rank.put(by_rank, s));
    const std::vector<double> h_len(genome_lengths, genome_lengths + G);
    CS_TRY(d_len.put(h_len, s));
    CS_TRY(d_scfail.fit((size_t)n_scaf)); CS_TRY(d_labels.fit((size_t)G * S)); CS_TRY(d_status.fit((size_t)G));
    CS_TRY(st->d_gpairs.fit((size_t)G * P)); CS_TRY(st->d_clZ.fit((size_t)G * (S - 1) * 4));
    CS_TRY(hipMemsetAsync(d_status.p, 0xFF, (size_t)G * sizeof(isx_cluster_status), s));
    CS_TRY(hipMemsetAsync(d_labels.p, 0, (size_t)G * S * 4, s));
    CS_TRY(hipMemsetAsync(st->d_clZ.p, 0, (size_t)G * (S - 1) * 32, s));
    Classes c;
    std::vector<int32_t> &cls = S <= WAVE_MAX ? c.wave : S <= LDS_MAX ? c.lds : c.glob;
    for (int32_t g = 0; g < G; g++) cls.push_back(g);
    c.glob_cap = S;
    ClusterArgs a{};
    a.method = m; a.cutoff = cutoff; a.gpairs = st->d_gpairs.p; a.S = S; a.P = P; a.by_rank = d_rank.p; a.glen = d_len.p;
    a.cov_thr = coverage_treshold; a.labels = d_labels.p; a.Z = st->d_clZ.p; a.status = d_status.p;
    const size_t n_snp = (size_t)P * n_scaf * A;
    CS_TRY(hipEventRecord(st->ev[0], s));
    hipLaunchKernelGGL(k_cmpset_failed_any, dim3((unsigned)((n_scaf + 255) / 256)), dim3(256), 0, s, st->d_failed.p, P, n_scaf, d_scfail.p);
    hipLaunchKernelGGL(k_cmpset_genome_pairs, dim3((unsigned)(((int64_t)G * P + 255) / 256)), dim3(256), 0, s, d_pairs.p, P, G, d_goff.p, d_gsc.p,
                       n_scaf, A, st->d_pres.p, st->d_cnt.p, st->d_snp.p + n_snp, d_scfail.p, st->d_gpairs.p);
    rc = launch_classes(c, a, d_items, d_work, s);
    if (rc) return done(rc);
    CS_TRY(hipEventRecord(st->ev[1], s));
    std::vector<isx_cluster_status> h_status((size_t)G);
    CS_TRY(hipMemcpyAsync(h_status.data(), d_status.p, (size_t)G * sizeof(isx_cluster_status), hipMemcpyDeviceToHost, s));
    CS_TRY(hipMemcpyAsync(labels, d_labels.p, (size_t)G * S * 4, hipMemcpyDeviceToHost, s));
    CS_TRY(isx_wait_stream(s));
    CS_TRY(hipGetLastError());
#undef CS_TRY
    if (device_ms) (void)hipEventElapsedTime(device_ms, st->ev[0], st->ev[1]);
    for (isx_cluster_status &x : h_status)
        if (x.status < ISX_CLUSTER_OK || x.status > ISX_CLUSTER_EMPTY) x.status = ISX_CLUSTER_ERROR;
    rc = report_errors(who, h_status);
    if (rc) return done(rc);
    std::copy(h_status.begin(), h_status.end(), status);
    st->cl_status = h_status;
    st->cl_P = P;
    st->clustered = true;
    return done(ISX_OK);
}

int isx_cmpset_cluster_fetch_pairs(isx_cmpset *st, isx_genome_pair *out)
{
    if (!st || !out) { isx_set_error("isx_cmpset_cluster_fetch_pairs: bad argument"); return ISX_ERR_ARG; }
    if (!st->compared || !st->clustered) { isx_set_error("isx_cmpset_cluster_fetch_pairs: call isx_cmpset_cluster first (and again after an add or a compare)"); return ISX_ERR_STATE; }
    HIP_TRY(hipSetDevice(st->ctx->device));
    HIP_TRY(isx_wait_stream(st->ctx->stream));
    HIP_TRY(hipMemcpy(out, st->d_gpairs.p, st->cl_status.size() * (size_t)st->cl_P * sizeof(isx_genome_pair), hipMemcpyDeviceToHost));
    return ISX_OK;
}

int isx_cmpset_cluster_fetch_linkage(isx_cmpset *st, int32_t genome, double *Z)
{
    if (!st || !Z) { isx_set_error("isx_cmpset_cluster_fetch_linkage: bad argument"); return ISX_ERR_ARG; }
    if (!st->compared || !st->clustered) { isx_set_error("isx_cmpset_cluster_fetch_linkage: call isx_cmpset_cluster first (and again after an add or a compare)"); return ISX_ERR_STATE; }
    if (genome < 0 || (size_t)genome >= st->cl_status.size() || st->cl_status[(size_t)genome].status != ISX_CLUSTER_OK) {
        isx_set_error("isx_cmpset_cluster_fetch_linkage: genome " + std::to_string(genome) + " was not clustered");
        return ISX_ERR_ARG;
    }
    const size_t S = st->samples.size(), n = (size_t)st->cl_status[(size_t)genome].n_points;
    HIP_TRY(hipSetDevice(st->ctx->device));
    HIP_TRY(isx_wait_stream(st->ctx->stream));
    HIP_TRY(hipMemcpy(Z, st->d_clZ.p + (size_t)genome * (S - 1) * 4, (n - 1) * 32, hipMemcpyDeviceToHost));
    return ISX_OK;
}

}  // extern "C"
