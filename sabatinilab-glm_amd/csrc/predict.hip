// Pointwise bands of fitted traces: for each evaluated row i of a 0/1 design and each fit,
//   eta_i  = x~_i^T beta,     v_i  = x~_i^T C x~_i        (x~ = (x, 1), C the covariance of
//   eta_gi = x_gi^T w_g,      v_gi = x_gi^T C_gg x_gi      sglm_cov_groups, float64 [P][P])
// (statsmodels get_prediction().summary_frame(): mean_se^2 on the link scale), from the row-major
// bit planes of the design (rbits: one 64-bit word per row and 64-column block).
//
//   sglm_predict_rows    one wave per (row, fit).  Lane t reads the row's word t, puts it into
//                        column order and the wave lists the row's m set columns in LDS, ascending
//                        (the intercept coordinate p last when the fit has one).  The m (m + 1) / 2
//                        terms C[j][k], j <= k, of the quadratic form are enumerated in ascending
//                        (j, k) order and dealt to the lanes round-robin: lane l adds the terms
//                        l, l + 64, ... in that order, diagonal and upper terms apart, then a
//                        fixed butterfly adds the lanes and v = diag + 2 upper.  A set-bit walk:
//                        O(m^2) reads of C per row where a product with C costs O(m P); at 6 %
//                        ones that is 1 / 270 of P^2.  The reads of one j run along row j of C
//                        (lag blocks are consecutive columns), all of C stays in L2 (P <= 512) or
//                        the Infinity Cache.
//   sglm_predict_groups  one workgroup per (1024 rows, group, fit): C_gg (<= 64 x 64, 32 KB),
//                        w_g and the kept flags in LDS, one thread per row: the row's bits of the
//                        group's columns gathered into a 64-bit mask, then the set-bit walk over
//                        LDS in ascending (a, b) order.  A row with no bit in the group gets 0, 0.
//
// Float64 throughout; the products are by 0 / 1, so only the sums round.  The order of a row's
// terms depends on the row's bits alone: not on the launch, the batch or the row list.  No
// atomics; a repeated call returns the same bits, a fit's outputs are the same alone or in a
// batch.  A row with a set bit at a coordinate that is not kept (state != 0) gets v = NaN.
#include <math.h>

#include <vector>

#include "common.h"

namespace sglm {

// gcd.hip: the group CSR read back and validated on the host
int read_groups(const char* who, int32_t p, const int32_t* goff, const int32_t* gcols, int32_t ng,
                hipStream_t s, int32_t* kmax);

namespace {

constexpr int kMaxP = 4096;       // columns of a row's list (one word per lane)
constexpr int kGK = 64;           // columns of a group (sglm_cov_groups_kmax)
constexpr int kGRows = 1024;      // rows of a group workgroup, four per thread
constexpr int kMaxBlocks = 16384;

// a fragment-ordered word (common.h: element rho at bit rho / 2 + 16 (rho % 2)) in element order:
// the low half holds the even elements, the high half the odd ones
__device__ __forceinline__ uint32_t spread16(uint32_t x) {
    x &= 0xFFFFu;
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}

__device__ __forceinline__ uint64_t natural_bits(u32x2 w) {
    const uint32_t lo = spread16(w.x) | (spread16(w.x >> 16) << 1);
    const uint32_t hi = spread16(w.y) | (spread16(w.y >> 16) << 1);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

// bit of column c (0..63 of its block) in the block's fragment-ordered word pair
__device__ __forceinline__ uint32_t frag_bit(u32x2 w, int c) {
    const uint32_t word = c < 32 ? w.x : w.y;
    const int rho = c & 31;
    return (word >> ((rho >> 1) + 16 * (rho & 1))) & 1u;
}

__global__ void __launch_bounds__(64) predict_rows_kernel(
    const u32x2* __restrict__ rbits, int64_t ld, int32_t P, int32_t p,
    const int32_t* __restrict__ rows, int64_t nr, const double* __restrict__ beta,
    const double* __restrict__ cov, const uint8_t* __restrict__ state,
    const int32_t* __restrict__ icpt, double* __restrict__ eta, double* __restrict__ var) {
    __shared__ uint16_t list[kMaxP];
    const int f = blockIdx.y, lane = threadIdx.x;
    const double* bf = beta + (int64_t)f * P;
    const double* Cf = cov + (int64_t)f * P * P;
    const uint8_t* stf = state + (int64_t)f * P;
    const bool ic = icpt[f] != 0;
    const int nw = P / 64;
    for (int64_t k = blockIdx.x; k < nr; k += gridDim.x) {
        const int64_t i = rows ? (int64_t)rows[k] : k;
        uint64_t mask = 0;
        if (lane < nw) {
            mask = natural_bits(rbits[(int64_t)lane * ld + i]);
            const int keep = p - 64 * lane;          // columns >= p are padding, never data
            if (keep <= 0) mask = 0;
            else if (keep < 64) mask &= ((uint64_t)1 << keep) - 1;
            if (ic && (p >> 6) == lane) mask |= (uint64_t)1 << (p & 63);
        }
        const int cnt = __popcll(mask);
        int off = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(off, d, 64);
            if (lane >= d) off += t;
        }
        const int m = __shfl(off, 63, 64);
        off -= cnt;
        __syncthreads();                             // the previous row's list is no longer read
        bool bad = false;
        while (mask) {
            const int col = 64 * lane + __builtin_ctzll(mask);
            list[off++] = (uint16_t)col;
            bad |= stf[col] != 0;
            mask &= mask - 1;
        }
        bad = __ballot(bad) != 0;
        __syncthreads();
        double e = 0.0;
        for (int a = lane; a < m; a += 64) e += bf[list[a]];
        e = wave_sum_d(e);
        // term t of the ascending (a, b >= a) enumeration: row a of the triangle has m - a terms
        double sd = 0.0, su = 0.0;
        int a = 0, rem = lane;
        while (a < m && rem >= m - a) { rem -= m - a; ++a; }
        while (a < m) {
            const double c = Cf[(int64_t)list[a] * P + list[a + rem]];
            if (rem == 0) sd += c;
            else su += c;
            rem += 64;
            while (a < m && rem >= m - a) { rem -= m - a; ++a; }
        }
        sd = wave_sum_d(sd);
        su = wave_sum_d(su);
        if (lane == 0) {
            eta[(int64_t)f * nr + k] = e;
            var[(int64_t)f * nr + k] = bad ? (double)NAN : sd + 2.0 * su;
        }
    }
}

__global__ void __launch_bounds__(256) predict_groups_kernel(
    const u32x2* __restrict__ rbits, int64_t ld, int32_t P, const int32_t* __restrict__ rows,
    int64_t nr, const double* __restrict__ beta, const double* __restrict__ cov,
    const uint8_t* __restrict__ state, const int32_t* __restrict__ goff,
    const int32_t* __restrict__ gcols, int32_t ng, double* __restrict__ geta,
    double* __restrict__ gvar) {
    __shared__ double Cg[kGK][kGK + 1];
    __shared__ double bg[kGK];
    __shared__ int cols[kGK];
    __shared__ uint8_t sg[kGK];
    const int g = blockIdx.y, f = blockIdx.z, tid = threadIdx.x;
    const int o = goff[g], k = goff[g + 1] - o;
    const int64_t k0 = (int64_t)blockIdx.x * kGRows;
    double* ge = geta + ((int64_t)f * ng + g) * nr;
    double* gv = gvar + ((int64_t)f * ng + g) * nr;
    if (k > kGK) {                                   // as sglm_cov_groups' status 2
        for (int r = tid; r < kGRows && k0 + r < nr; r += 256) ge[k0 + r] = gv[k0 + r] = (double)NAN;
        return;
    }
    const double* Cf = cov + (int64_t)f * P * P;
    if (tid < k) {
        const int c = gcols[o + tid];
        cols[tid] = c;
        bg[tid] = beta[(int64_t)f * P + c];
        sg[tid] = state[(int64_t)f * P + c];
    }
    __syncthreads();
    for (int e = tid; e < k * k; e += 256) {
        const int a = e / k, b = e - a * k;
        Cg[a][b] = Cf[(int64_t)cols[a] * P + cols[b]];
    }
    __syncthreads();
    for (int r = tid; r < kGRows && k0 + r < nr; r += 256) {
        const int64_t i = rows ? (int64_t)rows[k0 + r] : k0 + r;
        uint64_t mask = 0;
        int tcur = -1;
        u32x2 w = {0u, 0u};
        for (int a = 0; a < k; ++a) {
            const int c = cols[a], t = c >> 6;
            if (t != tcur) {
                w = rbits[(int64_t)t * ld + i];
                tcur = t;
            }
            mask |= (uint64_t)frag_bit(w, c & 63) << a;
        }
        double e = 0.0, sd = 0.0, su = 0.0;
        bool bad = false;
        for (uint64_t ma = mask; ma; ma &= ma - 1) {
            const int a = __builtin_ctzll(ma);
            e += bg[a];
            bad |= sg[a] != 0;
            sd += Cg[a][a];
            for (uint64_t mb = ma & (ma - 1); mb; mb &= mb - 1) su += Cg[a][__builtin_ctzll(mb)];
        }
        ge[k0 + r] = e;
        gv[k0 + r] = bad ? (double)NAN : sd + 2.0 * su;
    }
}

// the row list read back and validated on the host: 0 <= rows[k] < n
int read_rows(const char* who, const int32_t* rows, int64_t nr, int64_t n, hipStream_t s) {
    std::vector<int32_t> r((size_t)nr);
    if (hipMemcpyAsync(r.data(), rows, r.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        set_error("%s: reading the row list failed", who);
        return SGLM_EHIP;
    }
    for (int64_t k = 0; k < nr; ++k)
        if (r[k] < 0 || (int64_t)r[k] >= n) {
            set_error("%s: rows[%lld]=%d is outside [0, n=%lld)", who, (long long)k, r[k],
                      (long long)n);
            return SGLM_EINVAL;
        }
    return SGLM_OK;
}

bool bad_common(const void* rbits, int64_t ld, int32_t P, int32_t p, int64_t n,
                const int32_t* rows, int64_t nr, const void* beta, const void* cov,
                const void* state, int32_t B) {
    return !rbits || !beta || !cov || !state || P < 64 || P % 64 || P > kMaxP || p < 1 || p >= P ||
           n < 1 || ld < n || ld >= ((int64_t)1 << 31) || nr >= ((int64_t)1 << 31) ||
           (!rows && nr > n) || B > 65535;
}

}  // namespace
}  // namespace sglm

using namespace sglm;

extern "C" int sglm_predict_rows(const uint32_t* rbits, int64_t ld, int32_t P, int32_t p,
                                 int64_t n, const int32_t* rows, int64_t nr, const double* beta,
                                 const double* cov, const uint8_t* state, const int32_t* icpt,
                                 int32_t B, double* eta, double* var, sglm_stream_t stream) {
    if (B <= 0 || nr <= 0) return SGLM_OK;
    if (bad_common(rbits, ld, P, p, n, rows, nr, beta, cov, state, B) || !icpt || !eta || !var) {
        set_error("sglm_predict_rows: bad args (P=%d, a multiple of 64 up to %d; p=%d < P; "
                  "n=%lld <= ld=%lld < 2^31; nr=%lld; B=%d)", P, kMaxP, p, (long long)n,
                  (long long)ld, (long long)nr, B);
        return SGLM_EINVAL;
    }
    hipStream_t st = as_stream(stream);
    if (rows) {
        const int rs = read_rows("sglm_predict_rows", rows, nr, n, st);
        if (rs) return rs;
    }
    const unsigned nblk = (unsigned)(nr < kMaxBlocks ? nr : kMaxBlocks);
    predict_rows_kernel<<<dim3(nblk, (unsigned)B), 64, 0, st>>>(
        reinterpret_cast<const u32x2*>(rbits), ld, P, p, rows, nr, beta, cov, state, icpt, eta,
        var);
    return check_launch("predict_rows_kernel");
}

extern "C" int sglm_predict_groups(const uint32_t* rbits, int64_t ld, int32_t P, int32_t p,
                                   int64_t n, const int32_t* rows, int64_t nr, const double* beta,
                                   const double* cov, const uint8_t* state, int32_t B,
                                   const int32_t* goff, const int32_t* gcols, int32_t ng,
                                   double* geta, double* gvar, sglm_stream_t stream) {
    if (B <= 0 || nr <= 0 || ng <= 0) return SGLM_OK;
    const int64_t nchunk = (nr + kGRows - 1) / kGRows;
    if (bad_common(rbits, ld, P, p, n, rows, nr, beta, cov, state, B) || !goff || !gcols ||
        ng > p || ng > 65535 || !geta || !gvar) {
        set_error("sglm_predict_groups: bad args (P=%d, a multiple of 64 up to %d; p=%d < P; "
                  "n=%lld <= ld=%lld < 2^31; nr=%lld; ng=%d; B=%d)", P, kMaxP, p, (long long)n,
                  (long long)ld, (long long)nr, ng, B);
        return SGLM_EINVAL;
    }
    hipStream_t st = as_stream(stream);
    int32_t kmax = 0;
    const int gs = read_groups("sglm_predict_groups", p, goff, gcols, ng, st, &kmax);
    if (gs) return gs;
    if (rows) {
        const int rs = read_rows("sglm_predict_groups", rows, nr, n, st);
        if (rs) return rs;
    }
    predict_groups_kernel<<<dim3((unsigned)nchunk, (unsigned)ng, (unsigned)B), 256, 0, st>>>(
        reinterpret_cast<const u32x2*>(rbits), ld, P, rows, nr, beta, cov, state, goff, gcols, ng,
        geta, gvar);
    return check_launch("predict_groups_kernel");
}
