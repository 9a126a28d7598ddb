// Reduced (column-deleted) squared-loss solves off the float64 factor of the FULL model.
//
// The reference's production drivers refit the whole model once per left-out event
// (leave_one_out_list: the full design, then one run per event with its columns removed).  In
// Gram space the reduced model's normal equations are a principal submatrix of the full
// model's, so with A = G + diag(lam') = U^T U (sglm_chol64_factor), z = U^-T c and a drop set S
// of k coordinates,
//
//   W = U^-T E_S                  (P x k: the columns of the identity picked by S, forward
//                                  solved; rows above min(S) are zero)
//   T = W^T W = (A^-1)_SS         (k x k, symmetric positive definite)
//   x = U^-1 (z - W T^-1 W^T z)   = A^-1 c - A^-1 E_S T^-1 (A^-1 c)_S
//
// is the solution of A[keep, keep] x_keep = c_keep on the kept coordinates and 0 on S (the
// block-inverse identity): z is projected off the span of W before the back solve.
//
//   sglm_chol64_drop_prep       per (factor, drop set) pair: W, the Cholesky factor R of T
//                               (T = R^T R, upper) and a status word.
//   sglm_chol64_drop_solve_add  x[fit] += the reduced solve of a right-hand side, exact 0.0 on S.
//
// Float64 throughout, plain FMA, fixed reduction orders (bitwise repeatable).
#include <math.h>

#include "common.h"

namespace sglm {
namespace {

constexpr int kB = 64;
constexpr int kMaxP64 = 8192;
constexpr int kDropKmax = 64;
constexpr int kLd = kB + 1;         // LDS row stride of the 64-wide tiles
constexpr int kChunk = 32;          // rows of U / W staged per step of the tile products
constexpr uint8_t ST_KEPT = 0;

// One workgroup per pair.  Block rows b = min(S) / 64 .. P / 64 - 1 in turn: the tile product
// E - U[done rows][block]^T W[done rows] (4 x 4 register tiles), then the block's 64 x 64
// triangular solve with the k right-hand sides (lane = right-hand side), then the rows of W are
// written.  T = W^T W by the same tile product, its Cholesky factor in LDS (lane = column).
__global__ void __launch_bounds__(256) c64_drop_prep_kernel(
    const double* __restrict__ U, int32_t P, const uint8_t* __restrict__ state,
    const int32_t* __restrict__ counts, const int32_t* __restrict__ pf,
    const int32_t* __restrict__ pg, const int32_t* __restrict__ sets,
    const int32_t* __restrict__ lens, int32_t kmax, double* __restrict__ W,
    double* __restrict__ R, int32_t* __restrict__ status) {
    extern __shared__ double sh[];
    double (*A)[kLd] = reinterpret_cast<double (*)[kLd]>(sh);                    // [kChunk]
    double (*Bw)[kLd] = reinterpret_cast<double (*)[kLd]>(sh + kChunk * kLd);    // [kChunk]
    double (*D)[kLd] = reinterpret_cast<double (*)[kLd]>(sh);                    // [kB], over A, Bw
    double (*X)[kLd] = reinterpret_cast<double (*)[kLd]>(sh + kB * kLd);         // [kB]
    __shared__ int32_t sidx[kB];
    __shared__ uint8_t st[kB];
    const int pair = blockIdx.x, f = pf[pair], gs = pg[pair];
    const int tid = threadIdx.x;
    const int len = lens[gs];
    if (counts[2 * f + 1] != 0 || len < 0 || len > kmax) {     // dependent coordinates: not here
        if (tid == 0) status[pair] = 2;
        return;
    }
    const double* Uf = U + (int64_t)f * P * P;
    const uint8_t* sf = state + (int64_t)f * P;
    double* Wp = W + (int64_t)pair * P * kmax;
    double* Rp = R + (int64_t)pair * kB * kB;
    if (tid < kB) {
        const int s = tid < len ? sets[(int64_t)gs * kmax + tid] : -1;
        sidx[tid] = (s >= 0 && s < P && sf[s] == ST_KEPT) ? s : -1;   // absent already: no column
    }
    __syncthreads();
    int smin = P;
    for (int j = 0; j < kB; ++j)
        if (sidx[j] >= 0 && sidx[j] < smin) smin = sidx[j];
    const int nb = P / kB;
    const int b0 = smin / kB;               // nb when no coordinate of S is kept in f
    const int r0 = (b0 < nb ? b0 : nb) * kB;
    for (int64_t e = tid; e < (int64_t)r0 * kmax; e += 256) Wp[e] = 0.0;
    const int tr = tid >> 4, tc = tid & 15;
    for (int b = b0; b < nb; ++b) {
        double acc[4][4] = {};
        for (int i0 = r0; i0 < b * kB; i0 += kChunk) {
            __syncthreads();
            for (int e = tid; e < kChunk * kB; e += 256) {
                const int i = e >> 6, c = e & 63;
                A[i][c] = Uf[(int64_t)(i0 + i) * P + b * kB + c];
                Bw[i][c] = c < kmax ? Wp[(int64_t)(i0 + i) * kmax + c] : 0.0;
            }
            __syncthreads();
            for (int i = 0; i < kChunk; ++i) {
                double a[4], w[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    a[q] = A[i][tr * 4 + q];
                    w[q] = Bw[i][tc * 4 + q];
                }
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 4; ++y) acc[x][y] = fma(a[x], w[y], acc[x][y]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                const int r = tr * 4 + x, j = tc * 4 + y;
                X[r][j] = (sidx[j] == b * kB + r ? 1.0 : 0.0) - acc[x][y];
            }
        for (int e = tid; e < kB * kB; e += 256) {
            const int r = e >> 6, c = e & 63;
            D[r][c] = r <= c ? Uf[(int64_t)(b * kB + r) * P + b * kB + c] : 0.0;
        }
        if (tid < kB) st[tid] = sf[b * kB + tid];
        __syncthreads();
        if (tid < kB) {                         // U_bb^T w = rhs, right-hand side tid
            for (int j = 0; j < kB; ++j) {
                const double xj = st[j] == ST_KEPT ? X[j][tid] / D[j][j] : 0.0;
                X[j][tid] = xj;
                for (int i = j + 1; i < kB; ++i) X[i][tid] = fma(-D[j][i], xj, X[i][tid]);
            }
        }
        __syncthreads();
        for (int e = tid; e < kB * kmax; e += 256) {
            const int r = e / kmax, j = e - r * kmax;
            Wp[(int64_t)(b * kB + r) * kmax + j] = X[r][j];
        }
        __threadfence_block();
    }
    // T = W^T W (+ 1 on the diagonal of the columns that are no coordinate of this factor)
    double acc[4][4] = {};
    for (int i0 = r0; i0 < P; i0 += kChunk) {
        __syncthreads();
        for (int e = tid; e < kChunk * kB; e += 256) {
            const int i = e >> 6, c = e & 63;
            Bw[i][c] = c < kmax ? Wp[(int64_t)(i0 + i) * kmax + c] : 0.0;
        }
        __syncthreads();
        for (int i = 0; i < kChunk; ++i) {
            double a[4], w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = Bw[i][tr * 4 + q];
                w[q] = Bw[i][tc * 4 + q];
            }
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) acc[x][y] = fma(a[x], w[y], acc[x][y]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int r = tr * 4 + x, j = tc * 4 + y;
            X[r][j] = acc[x][y] + ((r == j && sidx[j] < 0) ? 1.0 : 0.0);
        }
    __syncthreads();
    int bad = 0;
    for (int j = 0; j < kB; ++j) {              // every thread walks the loop (barriers)
        const double piv = X[j][j];
        __syncthreads();
        if (!(piv > 0.0) || isinf(piv)) {
            bad = 1;
            break;
        }
        const double r = sqrt(piv);
        if (tid == j) X[j][j] = r;
        else if (tid < kB && tid > j) X[j][tid] /= r;
        __syncthreads();
        if (tid < kB && tid > j) {
            const double ujc = X[j][tid];
            for (int i = j + 1; i <= tid; ++i) X[i][tid] = fma(-X[j][i], ujc, X[i][tid]);
        }
        __syncthreads();
    }
    if (!bad)
        for (int e = tid; e < kB * kB; e += 256) {
            const int r = e >> 6, c = e & 63;
            Rp[e] = r <= c ? X[r][c] : 0.0;
        }
    if (tid == 0) status[pair] = bad;
}

// One workgroup per right-hand side: z = U^-T g (forward, as c64_solve_kernel), t = W^T z,
// u = T^-1 t on the pair's factor R, z -= W u, x = U^-1 z (back), then x[fit] += x with exact
// 0.0 stored on the set's coordinates.  A pair whose status is not 0 is left alone.
__global__ void __launch_bounds__(256) c64_drop_solve_kernel(
    const double* __restrict__ U, int32_t P, const uint8_t* __restrict__ state,
    const int32_t* __restrict__ fits, const int32_t* __restrict__ fsrc,
    const int32_t* __restrict__ gsrc, const int32_t* __restrict__ psrc,
    const double* __restrict__ g, double* __restrict__ xout, const int32_t* __restrict__ pg,
    const int32_t* __restrict__ sets, const int32_t* __restrict__ lens, int32_t kmax,
    const double* __restrict__ W, const double* __restrict__ R,
    const int32_t* __restrict__ status) {
    extern __shared__ double z[];               // [P] doubles, then [P] set flags
    uint8_t* inS = reinterpret_cast<uint8_t*>(z + P);
    __shared__ double part[4][kB];
    __shared__ double tail[kB];
    __shared__ double uvec[kB];
    __shared__ int32_t sidx[kB];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    const int q = blockIdx.x, fit = fits[q], f = fsrc[q], pair = psrc[q];
    if (status[pair] != 0) return;
    const int gs = pg[pair];
    const int len = lens[gs];
    const double* Uf = U + (int64_t)f * P * P;
    const uint8_t* sf = state + (int64_t)f * P;
    const double* Wp = W + (int64_t)pair * P * kmax;
    const double* Rp = R + (int64_t)pair * kB * kB;
    const int nb = P / kB;
    for (int i = tid; i < P; i += 256) inS[i] = 0;
    if (tid < kB) {
        const int s = tid < len ? sets[(int64_t)gs * kmax + tid] : -1;
        sidx[tid] = (s >= 0 && s < P) ? s : -1;
    }
    __syncthreads();
    if (tid < kB && sidx[tid] >= 0) inS[sidx[tid]] = 1;
    int smin = P;
    for (int j = 0; j < kB; ++j) {
        const int s = sidx[j];
        if (s >= 0 && s < smin && sf[s] == ST_KEPT) smin = s;
    }
    const int r0 = (smin / kB) * kB;            // W is zero above this row
    const double* gf = g + (int64_t)(gsrc ? gsrc[q] : fit) * P;
    // forward: U^T z = g, block by block
    for (int b = 0; b < nb; ++b) {
        const int c = b * kB + l;
        double acc = 0.0;
        for (int i = w; i < b * kB; i += 4) acc = fma(Uf[(int64_t)i * P + c], z[i], acc);
        part[w][l] = acc;
        __syncthreads();
        if (w == 0) {
            double tv = gf[c] - (part[0][l] + part[1][l] + part[2][l] + part[3][l]);
            for (int j = 0; j < kB; ++j) {
                const int cj = b * kB + j;
                double zj = 0.0;
                if (l == j && sf[cj] == ST_KEPT) zj = tv / Uf[(int64_t)cj * P + cj];
                zj = __shfl(zj, j, 64);
                if (l > j) tv = fma(-Uf[(int64_t)cj * P + c], zj, tv);
                if (l == j) z[cj] = zj;
            }
        }
        __syncthreads();
    }
    // t = W^T z: lane = column of W, the rows dealt over the four waves, summed in wave order
    {
        double acc = 0.0;
        if (l < kmax)
            for (int i = r0 + w; i < P; i += 4) acc = fma(Wp[(int64_t)i * kmax + l], z[i], acc);
        part[w][l] = acc;
    }
    __syncthreads();
    if (w == 0) {
        double tv = part[0][l] + part[1][l] + part[2][l] + part[3][l];
        double a = 0.0, u = 0.0;
        for (int j = 0; j < kB; ++j) {          // R^T a = t
            double aj = 0.0;
            if (l == j) aj = tv / Rp[j * kB + j];
            aj = __shfl(aj, j, 64);
            if (l > j) tv = fma(-Rp[j * kB + l], aj, tv);
            if (l == j) a = aj;
        }
        tv = a;
        for (int j = kB - 1; j >= 0; --j) {     // R u = a
            double uj = 0.0;
            if (l == j) uj = tv / Rp[j * kB + j];
            uj = __shfl(uj, j, 64);
            if (l < j) tv = fma(-Rp[l * kB + j], uj, tv);
            if (l == j) u = uj;
        }
        uvec[l] = u;
    }
    __syncthreads();
    // z -= W u: a wave per row
    for (int i = r0 + w; i < P; i += 4) {
        double acc = l < kmax ? Wp[(int64_t)i * kmax + l] * uvec[l] : 0.0;
        acc = wave_sum_d(acc);
        if (l == 0) z[i] -= acc;
    }
    __syncthreads();
    // back: U x = z in place, block by block from the last
    for (int b = nb - 1; b >= 0; --b) {
        for (int rr = w; rr < kB; rr += 4) {
            const int r = b * kB + rr;
            double acc = 0.0;
            for (int c = (b + 1) * kB + l; c < P; c += kB)
                acc = fma(Uf[(int64_t)r * P + c], z[c], acc);
            acc = wave_sum_d(acc);
            if (l == 0) tail[rr] = acc;
        }
        __syncthreads();
        if (w == 0) {
            const int r = b * kB + l;
            double tv = z[r] - tail[l];
            for (int j = kB - 1; j >= 0; --j) {
                const int rj = b * kB + j;
                double xj = 0.0;
                if (l == j && sf[rj] == ST_KEPT) xj = tv / Uf[(int64_t)rj * P + rj];
                xj = __shfl(xj, j, 64);
                if (l < j) tv = fma(-Uf[(int64_t)r * P + rj], xj, tv);
                if (l == j) z[rj] = xj;
            }
        }
        __syncthreads();
    }
    double* xf = xout + (int64_t)fit * P;
    for (int i = tid; i < P; i += 256) xf[i] = inS[i] ? 0.0 : xf[i] + z[i];
}

template <typename K>
int allow_lds(K kernel, size_t bytes) {
    if (bytes <= 65536) return SGLM_OK;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
        set_error("chol64_drop: cannot reserve %zu bytes of LDS", bytes);
        return SGLM_EHIP;
    }
    return SGLM_OK;
}

size_t w_bytes(int32_t P, int32_t npair, int32_t kmax) {
    return (size_t)npair * (size_t)P * (size_t)kmax * sizeof(double);
}

}  // namespace
}  // namespace sglm

using namespace sglm;

extern "C" int32_t sglm_chol64_drop_kmax(void) { return kDropKmax; }

extern "C" size_t sglm_chol64_drop_work_bytes(int32_t P, int32_t npair, int32_t kmax) {
    if (P <= 0 || npair <= 0 || kmax <= 0) return 0;
    return w_bytes(P, npair, kmax) + (size_t)npair * kB * kB * sizeof(double);
}

extern "C" int sglm_chol64_drop_prep(const double* U, int32_t P, const uint8_t* state,
                                     const int32_t* counts, const int32_t* pf, const int32_t* pg,
                                     int32_t npair, const int32_t* sets, const int32_t* lens,
                                     int32_t kmax, void* work, int32_t* status,
                                     sglm_stream_t stream) {
    if (npair <= 0) return SGLM_OK;
    if (!U || !state || !counts || !pf || !pg || !sets || !lens || !work || !status || P <= 0 ||
        P % kB || P > kMaxP64 || kmax <= 0 || kmax > kDropKmax) {
        set_error("sglm_chol64_drop_prep: bad args (P=%d must be a multiple of %d, <= %d; "
                  "kmax=%d must be in 1 .. %d)", P, kB, kMaxP64, kmax, kDropKmax);
        return SGLM_EINVAL;
    }
    double* W = (double*)work;
    double* R = (double*)((char*)work + w_bytes(P, npair, kmax));
    const size_t lds = (size_t)2 * kB * kLd * sizeof(double);
    if (int st = allow_lds(c64_drop_prep_kernel, lds)) return st;
    c64_drop_prep_kernel<<<npair, 256, lds, as_stream(stream)>>>(U, P, state, counts, pf, pg, sets,
                                                                 lens, kmax, W, R, status);
    return check_launch("sglm_chol64_drop_prep");
}

extern "C" int sglm_chol64_drop_solve_add(const double* U, int32_t P, const uint8_t* state,
                                          const int32_t* fits, const int32_t* fsrc,
                                          const int32_t* gsrc, const int32_t* psrc, int32_t nq,
                                          const double* g, double* x, const int32_t* pg,
                                          int32_t npair, const int32_t* sets,
                                          const int32_t* lens, int32_t kmax, const void* work,
                                          const int32_t* status, sglm_stream_t stream) {
    if (nq <= 0) return SGLM_OK;
    if (!U || !state || !fits || !fsrc || !psrc || !g || !x || !pg || !sets || !lens || !work ||
        !status || npair <= 0 || P <= 0 || P % kB || P > kMaxP64 || kmax <= 0 ||
        kmax > kDropKmax) {
        set_error("sglm_chol64_drop_solve_add: bad args (P=%d, kmax=%d)", P, kmax);
        return SGLM_EINVAL;
    }
    const double* W = (const double*)work;
    const double* R = (const double*)((const char*)work + w_bytes(P, npair, kmax));
    const size_t lds = (size_t)P * (sizeof(double) + 1);
    if (int st = allow_lds(c64_drop_solve_kernel, lds)) return st;
    c64_drop_solve_kernel<<<nq, 256, lds, as_stream(stream)>>>(
        U, P, state, fits, fsrc, gsrc, psrc, g, x, pg, sets, lens, kmax, W, R, status);
    return check_launch("sglm_chol64_drop_solve_add");
}
