// NB2 dispersion by maximum likelihood: the two row passes behind sglm_hip/nb2.py.
//
//  sglm_count_hist      integer histogram of every (mask, response) pair: the y-only terms of
//                       the count likelihoods (sum log1p(k j), sum j / (1 + k j), lgamma(y + 1))
//                       become host sums over its tail, exact for every kappa and family.
//  sglm_nb2_kappa_sums  the eta-dependent half of the NB2 log-likelihood and of its derivative
//                       in kappa, for K dispersions per fit from one exp per row, float64, in
//                       the cancellation-free form.
#include "common.h"

namespace sglm {
namespace {

constexpr int64_t kRowChunk = 8192;          // rows per workgroup, as the row sums of api.hip
int32_t row_chunks(int64_t n) { return (int32_t)((n + kRowChunk - 1) / kRowChunk); }

// ------------------------------------------------------------------------------ histogram
// Bins below kLdsBins are counted in a per-workgroup LDS histogram (uint32: a chunk holds at
// most 8192 * 255 counts) and flushed with one global atomic per non-empty bin; higher bins go
// straight to global atomics (counts that large are rare).  Integer adds only: the result does
// not depend on the order.
constexpr int kLdsBins = 1024;

__global__ void __launch_bounds__(256) count_hist_kernel(const uint8_t* __restrict__ M,
                                                         const double* __restrict__ Y, int64_t n,
                                                         int64_t ldm, int32_t F, int64_t nbins,
                                                         unsigned long long* __restrict__ hist,
                                                         int32_t* __restrict__ flags) {
    __shared__ unsigned int lds[kLdsBins];
    const int f = blockIdx.y, r = blockIdx.z;
    const uint8_t* m = M + (int64_t)f * ldm;
    const double* y = Y + (int64_t)r * n;
    unsigned long long* h = hist + ((int64_t)r * F + f) * nbins;
    for (int b = threadIdx.x; b < kLdsBins; b += 256) lds[b] = 0u;
    __syncthreads();
    bool bad = false;
    const int64_t i0 = (int64_t)blockIdx.x * kRowChunk;
    const int64_t i1 = min(i0 + kRowChunk, n);
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const unsigned int w = m[i];
        if (w == 0u) continue;
        const double yi = y[i];
        // (a NaN fails the first comparison)
        if (!(yi >= 0.0 && yi < (double)nbins && yi == floor(yi))) { bad = true; continue; }
        const int64_t v = (int64_t)yi;           // 0 <= v < nbins
        if (v < kLdsBins) atomicAdd(&lds[v], w);
        else atomicAdd(&h[v], (unsigned long long)w);
    }
    __syncthreads();
    const int nlow = (int)min((int64_t)kLdsBins, nbins);
    for (int b = threadIdx.x; b < nlow; b += 256) {
        const unsigned int c = lds[b];
        if (c) atomicAdd(&h[b], (unsigned long long)c);
    }
    if (bad) atomicOr(&flags[(int64_t)r * F + f], 1);
}

// ------------------------------------------------------------------------------ kappa sums
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
    v = wave_sum_d(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += sh[w];
    return s;
}

// g(x) = (log1p(x) - x / (1 + x)) / x^2 = sum_k (-1)^k (k + 1) / (k + 2) x^k and its derivative
// g'(x) = sum_{k >= 1} (-1)^k k (k + 1) / (k + 2) x^(k - 1), by Horner below kSeriesX: the
// closed form loses a factor 2 / x to cancellation there.  At x < 1/8 the first dropped term
// is 8^-20 < 1e-18 of the leading one.
constexpr double kSeriesX = 0.125;
constexpr int kSeriesTerms = 20;

__device__ __forceinline__ void g_series(double x, double& g, double& dg) {
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int k = kSeriesTerms - 1; k >= 1; --k) {
        const double c = (double)(k + 1) / (double)(k + 2);
        const double s = (k & 1) ? -c : c;
        a = a * x + s;
        b = b * x + s * (double)k;
    }
    g = a * x + 0.5;
    dg = b;
}

constexpr int kMaxKappa = 8;
constexpr int kSums = 3;

// One workgroup per (row chunk, launch row f).  Each thread takes four consecutive rows per
// pass: one 16 B load of eta, one of y, one 4 B load of the mask.  part[((f K + k) 3 + q)][chunk].
// KM >= K is the number of accumulator sets compiled in (1, 2, 4 or 8): a K = 1 pass keeps the
// registers of one.
template <int KM>
__global__ void __launch_bounds__(256) kappa_sums_kernel(
    int64_t n, int64_t ld, const int32_t* __restrict__ slots, const float* __restrict__ eta,
    const float* __restrict__ Y, const uint8_t* __restrict__ M,
    const int32_t* __restrict__ fit_resp, const int32_t* __restrict__ fit_mask,
    const double* __restrict__ kappa, int32_t K, double* __restrict__ part) {
    __shared__ double sh[4];
    const int f = blockIdx.y;
    const int slot = slots ? slots[f] : f;
    const float* e = eta + (int64_t)slot * ld;
    const float* y = Y + (int64_t)fit_resp[f] * ld;
    const uint8_t* m = M + (int64_t)fit_mask[f] * ld;
    double kap[KM], ik[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        kap[k] = k < K ? kappa[(int64_t)f * K + k] : 1.0;
        ik[k] = 1.0 / kap[k];
    }
    double acc[KM][kSums];
#pragma unroll
    for (int k = 0; k < KM; ++k)
#pragma unroll
        for (int q = 0; q < kSums; ++q) acc[k][q] = 0.0;

    auto row = [&](double w, double yi, double ei) {
        const double mu = exp(ei);               // one exponential for the K values
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            if (k >= K) continue;
            const double x = kap[k] * mu;
            const double L = log1p(x);
            const double inv = 1.0 / (1.0 + x);
            const double r = mu * inv;           // mu / (1 + kappa mu)
            double G, G3;
            if (x < kSeriesX) {
                double g, dg;
                g_series(x, g, dg);
                G = mu * mu * g;
                G3 = mu * mu * mu * dg;
            } else {                             // no mu^2: finite at every eta
                G = (L - x * inv) * ik[k] * ik[k];
                G3 = (r * r - 2.0 * G) * ik[k];
            }
            acc[k][0] += w * (yi * ei - (yi + ik[k]) * L);
            acc[k][1] += w * (G - yi * r);
            acc[k][2] += w * (G3 + yi * r * r);
        }
    };

    const int64_t i0 = (int64_t)blockIdx.x * kRowChunk;
    const int64_t i1 = min(i0 + kRowChunk, n);
    for (int64_t i = i0 + 4 * (int64_t)threadIdx.x; i < i1; i += 1024) {
        if (i + 4 <= i1) {
            const uint32_t m4 = *reinterpret_cast<const uint32_t*>(m + i);
            if (m4 == 0u) continue;
            const f32x4 e4 = *reinterpret_cast<const f32x4*>(e + i);
            const f32x4 y4 = *reinterpret_cast<const f32x4*>(y + i);
            // one copy of the row arithmetic (the float64 exp / log1p expansions are long):
            // the quad's elements are picked by selects, not by unrolling
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                const uint32_t w = (m4 >> (8 * j)) & 0xffu;
                const float yj = j == 0 ? y4[0] : j == 1 ? y4[1] : j == 2 ? y4[2] : y4[3];
                const float ej = j == 0 ? e4[0] : j == 1 ? e4[1] : j == 2 ? e4[2] : e4[3];
                if (w) row((double)w, (double)yj, (double)ej);
            }
        } else {
            for (int64_t q = i; q < i1; ++q)
                if (m[q]) row((double)m[q], (double)y[q], (double)e[q]);
        }
    }
    const int64_t nch = gridDim.x;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        if (k >= K) continue;            // (uniform: every thread reaches block_sum_d alike)
#pragma unroll
        for (int q = 0; q < kSums; ++q) {
            const double s = block_sum_d(acc[k][q], sh);
            if (threadIdx.x == 0)
                part[(((int64_t)f * K + k) * kSums + q) * nch + blockIdx.x] = s;
        }
    }
}

// reduce_chunks_d of api.hip: one wave per output row, lane l sums chunks l, l + 64, ... in
// ascending order, then the fixed butterfly -- one order whatever the scheduling.
constexpr int kReduceRows = 4;
__global__ void __launch_bounds__(256) kappa_reduce_chunks_d(const double* __restrict__ part,
                                                             int64_t rows, int32_t nchunks,
                                                             double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * kReduceRows + (threadIdx.x >> 6);
    if (e >= rows) return;                       // wave-uniform
    const double* p = part + e * nchunks;
    double s = 0.0;
    for (int c = lane; c < nchunks; c += 64) s += p[c];
    s = wave_sum_d(s);
    if (lane == 0) out[e] = s;
}

}  // namespace
}  // namespace sglm

using namespace sglm;

extern "C" {

int sglm_count_hist(const uint8_t* M, int64_t ldm, int32_t F, const double* Y, int32_t R,
                    int64_t n, int64_t nbins, uint64_t* hist, int32_t* flags,
                    sglm_stream_t stream) {
    if (F <= 0 || R <= 0) return SGLM_OK;
    if (!M || !Y || !hist || !flags || ldm < n || n <= 0 || nbins <= 0) {
        set_error("sglm_count_hist: bad args");
        return SGLM_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(hist, 0, (size_t)R * F * nbins * sizeof(uint64_t), s) != hipSuccess ||
        hipMemsetAsync(flags, 0, (size_t)R * F * sizeof(int32_t), s) != hipSuccess) {
        set_error("sglm_count_hist: hipMemsetAsync failed");
        return SGLM_EHIP;
    }
    count_hist_kernel<<<dim3((unsigned)row_chunks(n), (unsigned)F, (unsigned)R), 256, 0, s>>>(
        M, Y, n, ldm, F, nbins, reinterpret_cast<unsigned long long*>(hist), flags);
    return check_launch("count_hist_kernel");
}

size_t sglm_nb2_kappa_sums_work_bytes(int32_t nfit, int32_t K, int64_t n) {
    return (size_t)nfit * K * kSums * row_chunks(n) * sizeof(double);
}

int sglm_nb2_kappa_sums(int64_t n, int64_t ld, int32_t nfit, const int32_t* slots,
                        const float* eta, const float* Y, const uint8_t* M,
                        const int32_t* fit_resp, const int32_t* fit_mask, const double* kappa,
                        int32_t K, double* out, void* work, sglm_stream_t stream) {
    if (nfit <= 0) return SGLM_OK;
    if (!eta || !Y || !M || !fit_resp || !fit_mask || !kappa || !out || !work || n <= 0 ||
        n > ld || ld % 4 || K < 1 || K > kMaxKappa) {
        set_error("sglm_nb2_kappa_sums: bad args (K=%d, max %d)", K, kMaxKappa);
        return SGLM_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    const int32_t nc = row_chunks(n);
    const dim3 grid((unsigned)nc, (unsigned)nfit);
#define SGLM_KAPPA_SUMS(KM) kappa_sums_kernel<KM><<<grid, 256, 0, s>>>( \
        n, ld, slots, eta, Y, M, fit_resp, fit_mask, kappa, K, (double*)work)
    if (K == 1) SGLM_KAPPA_SUMS(1);
    else if (K == 2) SGLM_KAPPA_SUMS(2);
    else if (K <= 4) SGLM_KAPPA_SUMS(4);
    else SGLM_KAPPA_SUMS(8);
#undef SGLM_KAPPA_SUMS
    int st = check_launch("kappa_sums_kernel");
    if (st) return st;
    const int64_t rows = (int64_t)nfit * K * kSums;
    kappa_reduce_chunks_d<<<dim3((unsigned)((rows + kReduceRows - 1) / kReduceRows)), 256, 0,
                            s>>>((const double*)work, rows, nc, out);
    return check_launch("kappa_reduce_chunks_d");
}

}  // extern "C"
