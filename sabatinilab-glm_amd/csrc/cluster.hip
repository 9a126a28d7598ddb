// Cluster-robust covariance (by trial or session): the meat M = sum_c g_c g_c^T of the sandwich
// A^-1 M A^-1, g_c = sum_{i in cluster c} m_i s_i x~_i (statsmodels cov_type='cluster', R
// sandwich::vcovCL).  sglm_cov_groups (infer.hip) reads M as its cov_type 2 meat.
//
//   sglm_infer_scores    the signed score residuals m dloss/deta of each fit, float64 from the
//                        f32 eta and y, in the overflow-free forms of sglm_infer_rows.
//   sglm_cluster_scores  S[q][r][j] = sum over the rows of run r (a maximal stretch of rows of
//                        one cluster) of bit_j(i) s[q][i], from the column bit-planes: one pass
//                        over the planes for every four fits, the s tiles in LDS.
//   sglm_cluster_meat    g_c = the sum of the runs of cluster c (skipped when every cluster is
//                        one run), then M = sum_c g_c g_c^T on v_mfma_f64_16x16x4_f64.
//
// Summation orders are fixed: ascending rows inside a run (add under the bit's mask, so the order
// does not depend on where the set bits are or on the launch), ascending runs inside a cluster,
// ascending clusters four at a time in the MFMA.  A repeated call returns the same bits, and a
// fit's result does not depend on the fits that share its launch.  No atomics.
#include <math.h>

#include <vector>

#include "common.h"

namespace sglm {
namespace {

constexpr int kColsBlk = 256;     // columns of a run-score workgroup, one per thread
constexpr int kTileW = 16;        // 32-row words of a staged tile (512 rows)
constexpr int kSeg = 1024;        // a workgroup owns the runs that start in one 1024-row segment
constexpr int kNQ = 4;            // fits that share one pass over the planes
constexpr int kT = 64;            // tile edge of M
constexpr int kKT = 32;           // clusters staged per step of the meat
constexpr int kLdT = 80;          // LDS row pitch (doubles): rows k, k + 1 fall in opposite bank halves
constexpr int kMaxP = 8192;       // as sglm_cov_groups

typedef double f64x4 __attribute__((ext_vector_type(4)));

// s = dloss/deta of one row in float64: the forms of fisher_row (infer.hip)
__device__ __forceinline__ double score_row_d(int family, double power, double y, double eta) {
    if (family == SGLM_FAM_NB2_LOG) {
        const double kappa = power, ik = 1.0 / kappa;
        if (eta + log(kappa) <= 0.0) {
            const double mu = exp(eta);
            return (mu - y) / (1.0 + kappa * mu);
        }
        const double e = exp(-eta) * ik;        // 1 / (kappa mu)
        return (ik - y * e) / (1.0 + e);
    }
    if (family == SGLM_FAM_SQUARED) return eta - y;
    if (family == SGLM_FAM_BINOMIAL_LOGIT) {
        const double e = exp(-fabs(eta));
        const double inv = 1.0 / (1.0 + e);
        return (eta >= 0.0 ? inv : e * inv) - y;
    }
    if (power == 1.0) return exp(eta) - y;
    if (power == 2.0) return 1.0 - y * exp(-eta);
    return exp((2.0 - power) * eta) - y * exp((1.0 - power) * eta);
}

__global__ void __launch_bounds__(256) infer_scores_kernel(
    int32_t family, float power, int64_t n, int64_t ld, const int32_t* __restrict__ slots,
    const float* __restrict__ eta, const float* __restrict__ Y, const uint8_t* __restrict__ M,
    const int32_t* __restrict__ fit_resp, const int32_t* __restrict__ fit_mask,
    double* __restrict__ s) {
    const int q = blockIdx.y;
    const int k = slots ? slots[q] : q;
    const float* e = eta + (int64_t)k * ld;
    const float* yv = Y + (int64_t)fit_resp[k] * ld;
    const uint8_t* m = M + (int64_t)fit_mask[k] * ld;
    double* sq = s + (int64_t)q * ld;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ld;
         i += (int64_t)gridDim.x * 256) {
        double v = 0.0;
        if (i < n) {
            const uint8_t mi = m[i];
            if (mi) v = (double)mi * score_row_d(family, (double)power, (double)yv[i], (double)e[i]);
        }
        sq[i] = v;
    }
}

// Workgroup (column block, row segment, four fits): thread t owns column c0 + t and walks the
// rows of the runs that START in its segment, from the first such run's first row to the last
// one's end (which may lie in a later segment), tile by tile.  Every thread sees the same rows,
// so the run boundaries are uniform branches; a boundary may fall anywhere in a word.
__global__ void __launch_bounds__(256) run_scores_kernel(
    const uint32_t* __restrict__ xbits, int64_t ld, int32_t P, const double* __restrict__ s,
    int32_t B, const int32_t* __restrict__ roff, int32_t R, double* __restrict__ S) {
    __shared__ uint32_t bw[kTileW][kColsBlk + 1];
    __shared__ double sv[kNQ][kTileW * 32];
    __shared__ int sh_r[2];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * kColsBlk;
    const int q0 = blockIdx.z * kNQ;
    if (tid < 2) {
        // the first run that starts at or after the segment's (tid 0) / the next one's first row
        const int64_t target = ((int64_t)blockIdx.y + tid) * kSeg;
        int lo = 0, hi = R;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (roff[mid] < target) lo = mid + 1;
            else hi = mid;
        }
        sh_r[tid] = lo;
    }
    __syncthreads();
    int r = sh_r[0];
    const int re = sh_r[1];
    if (r >= re) return;
    const int64_t row_end = roff[re];
    const int64_t nw = ld / 32;
    int64_t i = roff[r], next = roff[r + 1];
    double acc[kNQ];
#pragma unroll
    for (int q = 0; q < kNQ; ++q) acc[q] = 0.0;
    for (int64_t w0 = i / 32; w0 * 32 < row_end; w0 += kTileW) {
        __syncthreads();
        for (int e = tid; e < kTileW * kColsBlk; e += 256) {
            const int col = e / kTileW, w = e % kTileW;
            bw[w][col] = w0 + w < nw ? xbits[(int64_t)(c0 + col) * nw + w0 + w] : 0u;
        }
        for (int e = tid; e < kNQ * kTileW * 32; e += 256) {
            const int q = e / (kTileW * 32), x = e % (kTileW * 32);
            const int64_t row = w0 * 32 + x;
            sv[q][x] = (q0 + q < B && row < ld) ? s[(int64_t)(q0 + q) * ld + row] : 0.0;
        }
        __syncthreads();
        const int64_t tile_hi = (w0 + kTileW) * 32;
        const int64_t tile_end = row_end < tile_hi ? row_end : tile_hi;
        while (i < tile_end) {
            const int64_t stop = next < tile_end ? next : tile_end;
            for (; i < stop; ++i) {
                const int x = (int)(i - w0 * 32);
                const bool on = (bw[x >> 5][tid] >> (x & 31)) & 1u;
#pragma unroll
                for (int q = 0; q < kNQ; ++q) acc[q] += on ? sv[q][x] : 0.0;
            }
            if (i == next) {
#pragma unroll
                for (int q = 0; q < kNQ; ++q) {
                    if (q0 + q < B) S[((int64_t)(q0 + q) * R + r) * P + c0 + tid] = acc[q];
                    acc[q] = 0.0;
                }
                ++r;
                next = r < re ? roff[r + 1] : row_end;
            }
        }
    }
}

// g_c = the runs cruns[coff[c] .. coff[c + 1]) of cluster c added in that (ascending) order
__global__ void __launch_bounds__(256) cluster_merge_kernel(
    const double* __restrict__ S, int32_t R, int32_t P, const int32_t* __restrict__ coff,
    const int32_t* __restrict__ cruns, int32_t G, double* __restrict__ Gm) {
    const int q = blockIdx.z;
    const int j = blockIdx.x * 256 + threadIdx.x;
    for (int c = blockIdx.y; c < G; c += gridDim.y) {
        double a = 0.0;
        for (int e = coff[c]; e < coff[c + 1]; ++e) a += S[((int64_t)q * R + cruns[e]) * P + j];
        Gm[((int64_t)q * G + c) * P + j] = a;
    }
}

// M tile (bi <= bj) = sum_c g_c[rows of bi] g_c[cols of bj]^T, written with its mirror image.
// v_mfma_f64_16x16x4_f64: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15];
// its result register v is D[i = (l >> 4) + 4 v][j = l & 15] (not the f32 forms' C/D map).
// Wave w of the four owns rows 16 w .. 16 w + 15 of the tile and all four 16-column blocks.
__global__ void __launch_bounds__(256) cluster_meat_kernel(const double* __restrict__ Gs,
                                                           int32_t G, int32_t P,
                                                           double* __restrict__ Mout) {
    __shared__ double LA[kKT][kLdT];
    __shared__ double LB[kKT][kLdT];
    const int f = blockIdx.y;
    const int nb = P / kT;
    int t = blockIdx.x, bi = 0;
    {
        int rowlen = nb;
        while (t >= rowlen) { t -= rowlen; ++bi; --rowlen; }
    }
    const int bj = bi + t;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const double* Gf = Gs + (int64_t)f * G * P;
    double* Mf = Mout + (int64_t)f * P * P;
    f64x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < G; c0 += kKT) {
        __syncthreads();
        for (int e = tid; e < kKT * kT; e += 256) {
            const int r = e >> 6, x = e & 63;
            const bool in = c0 + r < G;         // clusters past the last enter as exact zeros
            LA[r][x] = in ? Gf[(int64_t)(c0 + r) * P + bi * kT + x] : 0.0;
            LB[r][x] = in ? Gf[(int64_t)(c0 + r) * P + bj * kT + x] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k0 = 0; k0 < kKT; k0 += 4) {
            const double a = LA[k0 + lk][16 * wave + li];
#pragma unroll
            for (int b = 0; b < 4; ++b)
                acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, LB[k0 + lk][16 * b + li], acc[b],
                                                              0, 0, 0);
        }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int row = 16 * wave + lk + 4 * v, col = 16 * b + li;
            if (bi < bj || row <= col) {
                const int64_t i = bi * kT + row, j = bj * kT + col;
                const double val = acc[b][v];
                Mf[i * P + j] = val;
                Mf[j * P + i] = val;
            }
        }
}

// the run offsets read back and validated on the host: 0 <= roff[0] < ... < roff[R] <= n
int read_runs(const char* who, const int32_t* roff, int32_t R, int64_t n, hipStream_t s) {
    std::vector<int32_t> off((size_t)R + 1);
    if (hipMemcpyAsync(off.data(), roff, off.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        set_error("%s: reading the run offsets failed", who);
        return SGLM_EHIP;
    }
    if (off[0] < 0 || (int64_t)off[R] > n) {
        set_error("%s: run offsets must lie in [0, n=%lld]", who, (long long)n);
        return SGLM_EINVAL;
    }
    for (int r = 0; r < R; ++r)
        if (off[r + 1] <= off[r]) {
            set_error("%s: run %d is empty or its offsets decrease", who, r);
            return SGLM_EINVAL;
        }
    return SGLM_OK;
}

// the runs-per-cluster CSR read back and validated: every run listed once, ascending in a cluster
int read_cluster_csr(const char* who, const int32_t* coff, const int32_t* cruns, int32_t G,
                     int32_t R, hipStream_t s) {
    std::vector<int32_t> off((size_t)G + 1), runs((size_t)R);
    if (hipMemcpyAsync(off.data(), coff, off.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        hipMemcpyAsync(runs.data(), cruns, runs.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                       s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        set_error("%s: reading the cluster lists failed", who);
        return SGLM_EHIP;
    }
    if (off[0] != 0 || off[G] != R) {
        set_error("%s: cluster offsets must run from 0 to R=%d", who, R);
        return SGLM_EINVAL;
    }
    std::vector<char> seen((size_t)R, 0);
    for (int c = 0; c < G; ++c) {
        if (off[c + 1] <= off[c] || off[c + 1] > R) {
            set_error("%s: cluster %d is empty or its offsets decrease", who, c);
            return SGLM_EINVAL;
        }
        for (int e = off[c]; e < off[c + 1]; ++e) {
            const int32_t r = runs[e];
            if (r < 0 || r >= R || seen[r] || (e > off[c] && r <= runs[e - 1])) {
                set_error("%s: cruns[%d]=%d is outside [0, %d), listed twice or not ascending",
                          who, e, r, R);
                return SGLM_EINVAL;
            }
            seen[r] = 1;
        }
    }
    return SGLM_OK;
}

}  // namespace
}  // namespace sglm

using namespace sglm;

extern "C" int sglm_infer_scores(int32_t family, float power, int64_t n, int64_t ld, int32_t B,
                                 const int32_t* slots, const float* eta, const float* Y,
                                 const uint8_t* M, const int32_t* fit_resp,
                                 const int32_t* fit_mask, double* s, sglm_stream_t stream) {
    if (B <= 0) return SGLM_OK;
    if (!eta || !Y || !M || !fit_resp || !fit_mask || !s || n < 0 || ld < n || ld < 1 ||
        B > 65535 || family < SGLM_FAM_SQUARED || family > SGLM_FAM_NB2_LOG ||
        (family == SGLM_FAM_NB2_LOG && !(power > 0.0f))) {
        set_error("sglm_infer_scores: bad args (family=%d B=%d)", family, B);
        return SGLM_EINVAL;
    }
    int64_t nblk = (ld + 255) / 256;
    if (nblk > 1024) nblk = 1024;
    infer_scores_kernel<<<dim3((unsigned)nblk, (unsigned)B), 256, 0, as_stream(stream)>>>(
        family, power, n, ld, slots, eta, Y, M, fit_resp, fit_mask, s);
    return check_launch("infer_scores_kernel");
}

extern "C" int sglm_cluster_scores(const uint32_t* xbits, int64_t ld, int32_t P, int64_t n,
                                   const double* s, int32_t B, const int32_t* roff, int32_t R,
                                   double* S, sglm_stream_t stream) {
    if (B <= 0 || R <= 0) return SGLM_OK;
    const int64_t nseg = (n + kSeg - 1) / kSeg;
    if (!xbits || !s || !roff || !S || n < 1 || ld < n || ld % 32 || ld >= ((int64_t)1 << 31) ||
        P < kColsBlk || P % kColsBlk || P > kMaxP || (int64_t)R > n || nseg > 65535 ||
        (B + kNQ - 1) / kNQ > 65535) {
        set_error("sglm_cluster_scores: bad args (P=%d, a multiple of %d up to %d; ld=%lld a "
                  "multiple of 32 below 2^31; n=%lld up to %d; R=%d B=%d)", P, kColsBlk, kMaxP,
                  (long long)ld, (long long)n, 65535 * kSeg, R, B);
        return SGLM_EINVAL;
    }
    hipStream_t st = as_stream(stream);
    const int rs = read_runs("sglm_cluster_scores", roff, R, n, st);
    if (rs) return rs;
    run_scores_kernel<<<dim3((unsigned)(P / kColsBlk), (unsigned)nseg,
                             (unsigned)((B + kNQ - 1) / kNQ)), 256, 0, st>>>(xbits, ld, P, s, B,
                                                                             roff, R, S);
    return check_launch("run_scores_kernel");
}

extern "C" size_t sglm_cluster_meat_work_bytes(int32_t P, int32_t B, int32_t G) {
    if (P < 1 || B < 1 || G < 1) return 0;
    return (size_t)B * G * P * sizeof(double);
}

extern "C" int sglm_cluster_meat(const double* S, int32_t P, int32_t B, int32_t R,
                                 const int32_t* coff, const int32_t* cruns, int32_t G,
                                 double* Mout, void* work, sglm_stream_t stream) {
    if (B <= 0) return SGLM_OK;
    const bool merge = coff != nullptr;
    if (!S || !Mout || P < kColsBlk || P % kColsBlk || P > kMaxP || B > 65535 || G < 1 || R < G ||
        (merge && (!cruns || !work)) || (!merge && R != G)) {
        set_error("sglm_cluster_meat: bad args (P=%d B=%d R=%d G=%d; without the cluster lists "
                  "R must equal G)", P, B, R, G);
        return SGLM_EINVAL;
    }
    hipStream_t st = as_stream(stream);
    const double* Gs = S;
    if (merge) {
        const int rs = read_cluster_csr("sglm_cluster_meat", coff, cruns, G, R, st);
        if (rs) return rs;
        cluster_merge_kernel<<<dim3((unsigned)(P / 256), (unsigned)(G < 65535 ? G : 65535),
                                    (unsigned)B), 256, 0, st>>>(S, R, P, coff, cruns, G,
                                                                (double*)work);
        const int ms = check_launch("cluster_merge_kernel");
        if (ms) return ms;
        Gs = (const double*)work;
    }
    const int nt = P / kT;
    cluster_meat_kernel<<<dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)B), 256, 0, st>>>(Gs, G, P,
                                                                                         Mout);
    return check_launch("cluster_meat_kernel");
}
