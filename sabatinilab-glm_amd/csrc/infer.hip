// Inference on fitted models: standard errors, covariance blocks and per-group Wald statistics
// (statsmodels GLM.fit().cov_params() / R vcov, in the engine's sum scaling).
//
//   sglm_infer_rows      one pass over the rows of each fit: the expected (Fisher) weights
//                        m v(eta), or the squared score residuals m s^2 (HC0's meat), as three
//                        bf16-exact f32 planes whose sum is the f32 weight bit for bit -- the
//                        operands of three bf16 MFMA Grams that together lose nothing of it --
//                        and the float64 Pearson sums.
//   sglm_chol64_inverse  Ainv = (U^T U)^-1 in float64 from the factor of sglm_chol64_factor:
//                        diagonal tile inverses, the blocked triangular inverse T = U^-1 one
//                        tile diagonal per launch, then T T^T.
//   sglm_cov_groups      variances, per-group blocks C_gg of the chosen covariance, their
//                        Cholesky factor in LDS and the Wald statistic; optionally all of C.
//
// Float64 arithmetic is plain v_fma_f64 throughout.  On gfx950 the float64 MFMA
// (v_mfma_f64_16x16x4_f64) has the same peak as the vector FMA, its C/D layout differs from
// every other MFMA's, and these products are P^3 / 3 flop once per model (P <= 4096: under
// 2.3e10), far from any rate; the FMA form keeps one summation order per entry, which is what
// makes Ainv bitwise symmetric and a repeated call bitwise equal.
#include <math.h>

#include "common.h"

namespace sglm {

// gcd.hip: the group CSR read back and validated on the host
int read_groups(const char* who, int32_t p, const int32_t* goff, const int32_t* gcols, int32_t ng,
                hipStream_t s, int32_t* kmax);

namespace {

constexpr int kT = 64;            // tile edge of the float64 kernels
constexpr int kMaxP = 8192;       // as sglm_chol64_factor
constexpr int kCovK = 64;         // columns of a group sglm_cov_groups factors in LDS
constexpr int kRowBlocks = 128;   // partial Pearson sums per fit (fixed: the reduction order)
constexpr float kTinyW = 0x1p-100f;
enum : uint8_t { ST_KEPT = 0 };

// ------------------------------------------------------------------------------ row pass
// v = the Fisher weight, s = dloss/deta of one row, single precision, in the overflow-free forms
// of half_loss / nb2_loss (common.h) with expf for every exponential.
struct RowOut { float v, s; };

__device__ __forceinline__ RowOut fisher_row(int family, float power, float y, float eta) {
    RowOut o;
    if (family == SGLM_FAM_NB2_LOG) {
        const float kappa = power, ik = 1.0f / kappa;
        const float z = eta + logf(kappa);
        if (z <= 0.0f) {
            const float mu = expf(eta);
            const float inv = 1.0f / (1.0f + kappa * mu);
            o.v = mu * inv;                     // mu / (1 + kappa mu)
            o.s = (mu - y) * inv;
        } else {
            const float e = expf(-eta) * ik;    // 1 / (kappa mu)
            const float inv = 1.0f / (1.0f + e);
            o.v = ik * inv;
            o.s = (ik - y * e) * inv;
        }
    } else if (family == SGLM_FAM_SQUARED) {
        o.v = 1.0f;
        o.s = eta - y;
    } else if (family == SGLM_FAM_BINOMIAL_LOGIT) {
        const float e = expf(-fabsf(eta));
        const float inv = 1.0f / (1.0f + e);
        o.v = e * inv * inv;
        o.s = (eta >= 0.0f ? inv : e * inv) - y;
    } else if (power == 1.0f) {
        const float mu = expf(eta);
        o.v = mu;
        o.s = mu - y;
    } else if (power == 2.0f) {
        o.v = 1.0f;
        o.s = 1.0f - y * expf(-eta);
    } else {
        const float a = expf((2.0f - power) * eta);
        o.v = a;
        o.s = a - y * expf((1.0f - power) * eta);
    }
    return o;
}

// (y - mu)^2 / V(mu) of one row in float64
__device__ __forceinline__ double pearson_row(int family, double power, double y, double eta) {
    double mu, V;
    if (family == SGLM_FAM_SQUARED) {
        mu = eta;
        V = 1.0;
    } else if (family == SGLM_FAM_BINOMIAL_LOGIT) {
        const double e = exp(-fabs(eta));
        const double inv = 1.0 / (1.0 + e);
        mu = eta >= 0.0 ? inv : e * inv;
        V = e * inv * inv;
    } else {
        mu = exp(eta);
        if (family == SGLM_FAM_NB2_LOG) V = mu + power * mu * mu;
        else V = power == 1.0 ? mu : power == 2.0 ? mu * mu : exp(power * eta);
    }
    const double r = y - mu;
    return r * r / V;
}

__device__ __forceinline__ float top8(float x) {
    return __uint_as_float(__float_as_uint(x) & 0xffff0000u);
}

__global__ void __launch_bounds__(256) infer_rows_kernel(
    int32_t family, float power, int32_t mode, int64_t n, int64_t ld, int32_t B,
    const int32_t* __restrict__ slots, const float* __restrict__ eta, const float* __restrict__ Y,
    const uint8_t* __restrict__ M, const int32_t* __restrict__ fit_resp,
    const int32_t* __restrict__ fit_mask, float* __restrict__ Wp, double* __restrict__ part) {
    const int q = blockIdx.y;
    const int k = slots ? slots[q] : q;
    const float* e = eta + (int64_t)k * ld;
    const float* yv = Y + (int64_t)fit_resp[k] * ld;
    const uint8_t* m = M + (int64_t)fit_mask[k] * ld;
    float* w0 = Wp + (int64_t)q * ld;
    const int64_t plane = (int64_t)B * ld;
    double sp = 0.0, sm = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ld;
         i += (int64_t)gridDim.x * 256) {
        float wi = 0.0f;
        if (i < n) {
            const float mi = (float)m[i];
            if (mi != 0.0f) {
                const float yi = yv[i], ei = e[i];
                const RowOut o = fisher_row(family, power, yi, ei);
                wi = mi * (mode ? o.s * o.s : o.v);
                if (wi < kTinyW) wi = 0.0f;
                if (part) {
                    sp += (double)mi * pearson_row(family, (double)power, (double)yi, (double)ei);
                    sm += (double)mi;
                }
            }
        }
        // truncation split: the top 8 significand bits, the next 8 and the rest; each
        // subtraction is exact
        const float p0 = top8(wi);
        const float r1 = wi - p0;
        const float p1 = top8(r1);
        w0[i] = p0;
        w0[plane + i] = p1;
        w0[2 * plane + i] = r1 - p1;
    }
    if (part) {
        __shared__ double ls[4][2];
        sp = wave_sum_d(sp);
        sm = wave_sum_d(sm);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) { ls[wave][0] = sp; ls[wave][1] = sm; }
        __syncthreads();
        if (threadIdx.x < 2) {
            const int c = threadIdx.x;
            part[((int64_t)q * gridDim.x + blockIdx.x) * 2 + c] =
                ((ls[0][c] + ls[1][c]) + ls[2][c]) + ls[3][c];
        }
    }
}

// sums[q] = the nblk block partials of launch row q in a fixed order: one wave per row
__global__ void __launch_bounds__(64) infer_rows_sum_kernel(const double* __restrict__ part,
                                                            int32_t nblk,
                                                            double* __restrict__ sums) {
    const int q = blockIdx.x, l = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int j = l; j < nblk; j += 64) {
        a += part[((int64_t)q * nblk + j) * 2];
        b += part[((int64_t)q * nblk + j) * 2 + 1];
    }
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    if (l == 0) {
        sums[2 * q] = a;
        sums[2 * q + 1] = b;
    }
}

int rows_blocks(int64_t ld) {
    const int64_t nb = (ld + 255) / 256;
    return (int)(nb < kRowBlocks ? (nb < 1 ? 1 : nb) : kRowBlocks);
}

// ------------------------------------------------------------------------------ inverse
// The factor with its coordinates that are not kept replaced by identity rows / columns (a
// dependent coordinate's column above the diagonal, which the factor keeps, is dropped).
//
// Diagonal tile kb of factor f: T_kk = U_kk^-1 by back substitution, lane c owns column c
// (X[.][c] is read and written by that lane alone).
__global__ void __launch_bounds__(64) inv_diag_kernel(const double* __restrict__ U, int32_t P,
                                                      const uint8_t* __restrict__ state,
                                                      double* __restrict__ T) {
    extern __shared__ double inv_lds[];
    double* A = inv_lds;                   // [kT][kT]
    double* X = inv_lds + kT * kT;         // [kT][kT]
    uint8_t* st = reinterpret_cast<uint8_t*>(X + kT * kT);
    const int kb = blockIdx.x, f = blockIdx.y, c = threadIdx.x;
    const int k0 = kb * kT;
    const double* Uf = U + (int64_t)f * P * P;
    double* Tf = T + (int64_t)f * P * P;
    st[c] = state[(int64_t)f * P + k0 + c];
    __syncthreads();
    const bool kc = st[c] == ST_KEPT;
    for (int r = 0; r < kT; ++r) {
        double v = 0.0;
        if (r == c) v = kc ? Uf[(int64_t)(k0 + r) * P + k0 + c] : 1.0;
        else if (r < c && kc && st[r] == ST_KEPT) v = Uf[(int64_t)(k0 + r) * P + k0 + c];
        A[r * kT + c] = v;
    }
    __syncthreads();
    for (int i = kT - 1; i >= 0; --i) {
        double s = i == c ? 1.0 : 0.0;
        for (int k = i + 1; k < kT; ++k) s = fma(-A[i * kT + k], X[k * kT + c], s);
        X[i * kT + c] = i <= c ? s / A[i * kT + i] : 0.0;
    }
    for (int r = 0; r < kT; ++r) Tf[(int64_t)(k0 + r) * P + k0 + c] = X[r * kT + c];
}

// acc[x][y] += sum_kk SA[kk][4 tr + x] SB[kk][4 tc + y]
__device__ __forceinline__ void tile_fma(double (*SA)[kT + 1], double (*SB)[kT + 1],
                                         int tr, int tc, double acc[4][4]) {
    for (int kk = 0; kk < kT; ++kk) {
        double a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a[q] = SA[kk][tr * 4 + q];
            b[q] = SB[kk][tc * 4 + q];
        }
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) acc[x][y] = fma(a[x], b[y], acc[x][y]);
    }
}

// Tile diagonal d >= 1: T[bi][bj] = -T[bi][bi] sum_{k = bi+1 .. bj} U[bi][k] T[k][bj], bj = bi + d
// (the T tiles read lie on the diagonals < d, written by the launches before this one).
__global__ void __launch_bounds__(256) inv_off_kernel(const double* __restrict__ U, int32_t P,
                                                      const uint8_t* __restrict__ state, int32_t d,
                                                      double* __restrict__ T) {
    __shared__ double SA[kT][kT + 1];
    __shared__ double SB[kT][kT + 1];
    __shared__ uint8_t sr[kT], sc[kT];
    const int bi = blockIdx.x, bj = bi + d, f = blockIdx.y;
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    const double* Uf = U + (int64_t)f * P * P;
    double* Tf = T + (int64_t)f * P * P;
    const uint8_t* stf = state + (int64_t)f * P;
    if (tid < kT) sr[tid] = stf[bi * kT + tid];
    double acc[4][4] = {};
    for (int k = bi + 1; k <= bj; ++k) {
        __syncthreads();
        if (tid < kT) sc[tid] = stf[k * kT + tid];
        __syncthreads();
        for (int e = tid; e < kT * kT; e += 256) {
            const int r = e >> 6, x = e & 63;
            const double u = Uf[(int64_t)(bi * kT + r) * P + k * kT + x];
            SA[x][r] = (sr[r] == ST_KEPT && sc[x] == ST_KEPT) ? u : 0.0;
            SB[r][x] = Tf[(int64_t)(k * kT + r) * P + bj * kT + x];
        }
        __syncthreads();
        tile_fma(SA, SB, tr, tc, acc);
    }
    __syncthreads();
    for (int e = tid; e < kT * kT; e += 256) {
        const int r = e >> 6, x = e & 63;
        SA[x][r] = Tf[(int64_t)(bi * kT + r) * P + bi * kT + x];
    }
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) SB[tr * 4 + x][tc * 4 + y] = acc[x][y];
    __syncthreads();
    double out[4][4] = {};
    tile_fma(SA, SB, tr, tc, out);
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y)
            Tf[(int64_t)(bi * kT + tr * 4 + x) * P + bj * kT + tc * 4 + y] = -out[x][y];
}

// Ainv tile (bi <= bj) = sum_{k >= bj} T[bi][k] T[bj][k]^T, written with its mirror image; the
// rows and columns of coordinates that are not kept as exact zeros.
__global__ void __launch_bounds__(256) inv_prod_kernel(const double* __restrict__ T, int32_t P,
                                                       const uint8_t* __restrict__ state,
                                                       double* __restrict__ Ainv) {
    __shared__ double SA[kT][kT + 1];
    __shared__ double SB[kT][kT + 1];
    const int f = blockIdx.y;
    const int nb = P / kT;
    int t = blockIdx.x, bi = 0;
    {
        int rowlen = nb;
        while (t >= rowlen) { t -= rowlen; ++bi; --rowlen; }
    }
    const int bj = bi + t;
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    const double* Tf = T + (int64_t)f * P * P;
    double* Af = Ainv + (int64_t)f * P * P;
    const uint8_t* stf = state + (int64_t)f * P;
    double acc[4][4] = {};
    for (int k = bj; k < nb; ++k) {
        __syncthreads();
        for (int e = tid; e < kT * kT; e += 256) {
            const int r = e >> 6, x = e & 63;
            SA[x][r] = Tf[(int64_t)(bi * kT + r) * P + k * kT + x];
            SB[x][r] = Tf[(int64_t)(bj * kT + r) * P + k * kT + x];
        }
        __syncthreads();
        tile_fma(SA, SB, tr, tc, acc);
    }
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const int i = bi * kT + tr * 4 + x;
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int j = bj * kT + tc * 4 + y;
            if (bi < bj || i <= j) {
                const double v =
                    (stf[i] == ST_KEPT && stf[j] == ST_KEPT) ? acc[x][y] : 0.0;
                Af[(int64_t)i * P + j] = v;
                Af[(int64_t)j * P + i] = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------ covariance
// One workgroup per (block, fit).  Blocks 0 .. ng-1 are the groups: columns ca = cb = the
// group's kept coordinates.  The blocks after them are 64 x 64 tiles of C: the diagonal tiles
// (variances), or every tile bi <= bj when the whole of C is asked for.
//   Q[a][b] = sum_r Ainv[ca[a]][r] Z[r][cb[b]],  Z = D Ainv ('model', D = rows < p) or M Ainv
//   ('robust', formed 64 rows at a time from 64-column tiles of M);
//   C = scale (Ainv - lam Q) | scale Ainv | Q.
__global__ void __launch_bounds__(256) cov_block_kernel(
    const double* __restrict__ Ainv, int32_t P, int32_t p, const int32_t* __restrict__ asrc,
    const uint8_t* __restrict__ state, const double* __restrict__ M, int32_t cov_type,
    const double* __restrict__ lam, const double* __restrict__ scale,
    const double* __restrict__ beta, const int32_t* __restrict__ goff,
    const int32_t* __restrict__ gcols, int32_t ng, double* __restrict__ var,
    double* __restrict__ stat, int32_t* __restrict__ dof, int32_t* __restrict__ status,
    double* __restrict__ cov) {
    __shared__ double S1[kT][kT + 1];
    __shared__ double S2[kT][kT + 1];
    __shared__ double S3[kT][kT + 1];
    __shared__ double zz[kCovK];
    __shared__ int ca[kCovK], cb[kCovK];
    __shared__ int s_k;
    const int f = blockIdx.y;
    const int a_i = asrc ? asrc[f] : f;
    const double* Af = Ainv + (int64_t)a_i * P * P;
    const uint8_t* stf = state + (int64_t)a_i * P;
    const double* Mf = M ? M + (int64_t)f * P * P : nullptr;
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    const bool group = (int)blockIdx.x < ng;
    const int g = blockIdx.x;
    int bi = 0, bj = 0;
    if (group) {
        const int o = goff[g], kraw = goff[g + 1] - o;
        if (tid == 0) {
            int k = 0;
            for (int e = 0; e < kraw; ++e) {
                const int c = gcols[o + e];
                if (stf[c] == ST_KEPT) {
                    if (k < kCovK) ca[k] = cb[k] = c;
                    ++k;
                }
            }
            s_k = k;
            for (int e = k; e < kCovK; ++e) ca[e] = cb[e] = -1;
        }
        __syncthreads();
        const int k = s_k;
        if (kraw > kCovK || k == 0) {
            if (tid == 0) {
                const int64_t o2 = (int64_t)f * ng + g;
                stat[o2] = kraw > kCovK ? (double)NAN : 0.0;
                dof[o2] = k;
                status[o2] = kraw > kCovK ? 2 : 0;
            }
            return;
        }
    } else {
        int t = (int)blockIdx.x - ng;
        if (cov) {
            int rowlen = P / kT;
            while (t >= rowlen) { t -= rowlen; ++bi; --rowlen; }
            bj = bi + t;
        } else {
            bi = bj = t;
        }
        if (tid < kT) {
            ca[tid] = bi * kT + tid;
            cb[tid] = bj * kT + tid;
        }
        if (tid == 0) s_k = kT;
        __syncthreads();
    }
    double acc[4][4] = {};
    if (cov_type != 1) {
        for (int r0 = 0; r0 < P; r0 += kT) {
            if (cov_type == 2) {
                // S3 = Z tile: Z[r0 + rr][cb[b]] = sum_c M[r0 + rr][c] Ainv[cb[b]][c]
                double az[4][4] = {};
                for (int c0 = 0; c0 < P; c0 += kT) {
                    __syncthreads();
                    for (int e = tid; e < kT * kT; e += 256) {
                        const int r = e >> 6, x = e & 63;
                        S1[x][r] = Mf[(int64_t)(r0 + r) * P + c0 + x];
                        const int cc = cb[r];
                        S2[x][r] = cc >= 0 ? Af[(int64_t)cc * P + c0 + x] : 0.0;
                    }
                    __syncthreads();
                    tile_fma(S1, S2, tr, tc, az);
                }
                __syncthreads();
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 4; ++y) S3[tr * 4 + x][tc * 4 + y] = az[x][y];
            } else {
                __syncthreads();
                for (int e = tid; e < kT * kT; e += 256) {
                    const int b = e >> 6, x = e & 63;
                    const int cc = cb[b];
                    S3[x][b] = (cc >= 0 && r0 + x < p) ? Af[(int64_t)cc * P + r0 + x] : 0.0;
                }
            }
            for (int e = tid; e < kT * kT; e += 256) {
                const int a = e >> 6, x = e & 63;
                const int cc = ca[a];
                S1[x][a] = cc >= 0 ? Af[(int64_t)cc * P + r0 + x] : 0.0;
            }
            __syncthreads();
            tile_fma(S1, S3, tr, tc, acc);
        }
    }
    __syncthreads();
    {
        const double ph = scale ? scale[f] : 1.0, lm = lam ? lam[f] : 0.0;
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                const int a = tr * 4 + x, b = tc * 4 + y;
                double v = acc[x][y];
                if (cov_type != 2) {
                    const double ai =
                        (ca[a] >= 0 && cb[b] >= 0) ? Af[(int64_t)ca[a] * P + cb[b]] : 0.0;
                    v = cov_type == 1 ? ph * ai : ph * (ai - lm * v);
                }
                S3[a][b] = v;
            }
    }
    __syncthreads();
    if (!group) {
        if (bi == bj && tid < kT) var[(int64_t)f * P + ca[tid]] = S3[tid][tid];
        if (cov) {
            double* Cf = cov + (int64_t)f * P * P;
            for (int e = tid; e < kT * kT; e += 256) {
                const int a = e >> 6, b = e & 63;
                if (bi < bj || a <= b) {
                    const double v = S3[a][b];
                    Cf[(int64_t)ca[a] * P + cb[b]] = v;
                    Cf[(int64_t)cb[b] * P + ca[a]] = v;
                }
            }
        }
        return;
    }
    // the group's Wald statistic: C_gg = R^T R (upper, only a <= b read), stat = |R^-T beta_g|^2
    const int k = s_k;
    bool bad = false;
    for (int j = 0; j < k; ++j) {
        const double piv = S3[j][j];
        if (!(piv > 0.0)) { bad = true; break; }      // the same value on every thread
        const double r = sqrt(piv);
        __syncthreads();
        if (tid == j) S3[j][j] = r;
        else if (tid > j && tid < k) S3[j][tid] /= r;
        __syncthreads();
        if (tid > j && tid < k) {
            const double ujc = S3[j][tid];
            for (int i = j + 1; i <= tid; ++i) S3[i][tid] = fma(-S3[j][i], ujc, S3[i][tid]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t o2 = (int64_t)f * ng + g;
        double s = (double)NAN;
        if (!bad) {
            s = 0.0;
            for (int i = 0; i < k; ++i) {
                double z = beta[(int64_t)f * P + ca[i]];
                for (int l = 0; l < i; ++l) z = fma(-S3[l][i], zz[l], z);
                z /= S3[i][i];
                zz[i] = z;
                s = fma(z, z, s);
            }
        }
        stat[o2] = s;
        dof[o2] = k;
        status[o2] = bad ? 1 : 0;
    }
}

}  // namespace
}  // namespace sglm

using namespace sglm;

extern "C" size_t sglm_infer_rows_work_bytes(int32_t B, int64_t ld) {
    if (B < 1 || ld < 1) return 0;
    return (size_t)B * rows_blocks(ld) * 2 * sizeof(double);
}

extern "C" int sglm_infer_rows(int32_t family, float power, int32_t mode, int64_t n, int64_t ld,
                               int32_t B, const int32_t* slots, const float* eta, const float* Y,
                               const uint8_t* M, const int32_t* fit_resp,
                               const int32_t* fit_mask, float* Wp, double* sums, void* work,
                               sglm_stream_t stream) {
    if (B <= 0) return SGLM_OK;
    if (!eta || !Y || !M || !fit_resp || !fit_mask || !Wp || n < 0 || ld < n || B > 65535 ||
        family < SGLM_FAM_SQUARED || family > SGLM_FAM_NB2_LOG || (mode != 0 && mode != 1) ||
        (sums && !work) || (family == SGLM_FAM_NB2_LOG && !(power > 0.0f))) {
        set_error("sglm_infer_rows: bad args (family=%d mode=%d B=%d)", family, mode, B);
        return SGLM_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    const int nblk = rows_blocks(ld);
    infer_rows_kernel<<<dim3((unsigned)nblk, (unsigned)B), 256, 0, s>>>(
        family, power, mode, n, ld, B, slots, eta, Y, M, fit_resp, fit_mask, Wp,
        sums ? (double*)work : nullptr);
    int st = check_launch("infer_rows_kernel");
    if (st || !sums) return st;
    infer_rows_sum_kernel<<<(unsigned)B, 64, 0, s>>>((const double*)work, nblk, sums);
    return check_launch("infer_rows_sum_kernel");
}

extern "C" size_t sglm_chol64_inverse_work_bytes(int32_t P, int32_t nf) {
    if (P < 1 || nf < 1) return 0;
    return (size_t)nf * P * P * sizeof(double);
}

extern "C" int sglm_chol64_inverse(const double* U, int32_t P, const uint8_t* state, int32_t nf,
                                   double* Ainv, void* work, sglm_stream_t stream) {
    if (nf <= 0) return SGLM_OK;
    if (!U || !state || !Ainv || !work || P < kT || P % kT || P > kMaxP || nf > 65535) {
        set_error("sglm_chol64_inverse: bad args (P=%d, a multiple of %d up to %d; nf=%d)", P, kT,
                  kMaxP, nf);
        return SGLM_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    double* T = (double*)work;
    const int nb = P / kT;
    const size_t lds = 2 * (size_t)kT * kT * sizeof(double) + kT;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&inv_diag_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        set_error("inv_diag_kernel: %zu bytes of LDS refused", lds);
        return SGLM_EHIP;
    }
    inv_diag_kernel<<<dim3((unsigned)nb, (unsigned)nf), 64, lds, s>>>(U, P, state, T);
    int st = check_launch("inv_diag_kernel");
    for (int d = 1; d < nb && !st; ++d) {
        inv_off_kernel<<<dim3((unsigned)(nb - d), (unsigned)nf), 256, 0, s>>>(U, P, state, d, T);
        st = check_launch("inv_off_kernel");
    }
    if (st) return st;
    inv_prod_kernel<<<dim3((unsigned)(nb * (nb + 1) / 2), (unsigned)nf), 256, 0, s>>>(T, P, state,
                                                                                    Ainv);
    return check_launch("inv_prod_kernel");
}

extern "C" int32_t sglm_cov_groups_kmax(void) { return kCovK; }

extern "C" int sglm_cov_groups(const double* Ainv, int32_t P, int32_t p, const int32_t* asrc,
                               const uint8_t* state, const double* M, int32_t cov_type,
                               int32_t nfit, const double* lam, const double* scale,
                               const double* beta, const int32_t* goff, const int32_t* gcols,
                               int32_t ng, double* var, double* stat, int32_t* dof,
                               int32_t* status, double* cov, sglm_stream_t stream) {
    if (nfit <= 0) return SGLM_OK;
    if (!Ainv || !state || !var || P < kT || P % kT || P > kMaxP || p < 1 || p >= P ||
        nfit > 65535 || cov_type < 0 || cov_type > 2 || (cov_type == 2 && !M) ||
        (cov_type == 0 && (!lam || !scale)) || (cov_type == 1 && !scale) || ng < 0 || ng > p ||
        (ng > 0 && (!goff || !gcols || !beta || !stat || !dof || !status))) {
        set_error("sglm_cov_groups: bad args (P=%d p=%d cov_type=%d ng=%d nfit=%d)", P, p,
                  cov_type, ng, nfit);
        return SGLM_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    if (ng > 0) {
        int32_t kmax = 0;
        const int st = read_groups("sglm_cov_groups", p, goff, gcols, ng, s, &kmax);
        if (st) return st;
    }
    const int nt = P / kT;
    const unsigned nblk = (unsigned)ng + (unsigned)(cov ? nt * (nt + 1) / 2 : nt);
    cov_block_kernel<<<dim3(nblk, (unsigned)nfit), 256, 0, s>>>(
        Ainv, P, p, asrc, state, M, cov_type, lam, scale, beta, goff, gcols, ng, var, stat, dof,
        status, cov);
    return check_launch("cov_block_kernel");
}
