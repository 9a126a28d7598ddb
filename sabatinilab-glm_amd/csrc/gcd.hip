// Gram-space block descent for the group lasso (one penalty term per event kernel).
//
// Objective per fit, in the scaling of cd.hip (sklearn's ElasticNet objective times n, on the
// centred Gram Q and q = X_c^T y_c), with the L1 term replaced by a sum of group norms:
//   1/2 w^T Q w - q^T w + sum_g lam_g |w_g|_2 + l2/2 |w|^2,
//   lam_g = lam_scale sqrt(k_g),  lam_scale = alpha rho n,  l2 = alpha (1 - rho) n,
// g over disjoint column groups that cover 0..p-1 (k_g columns each, not necessarily
// contiguous).  With every group a single column this is the ElasticNet objective.
//
// Solver: block-wise majorised descent (Yang & Zou 2015, GMD).  For group g with majoriser
// gam_g >= lambda_max(Q_gg) + l2:
//   grad_g = q_g - (Q w)_g - l2 w_g,   z = w_g + grad_g / gam_g,
//   w_g <- z max(0, 1 - (lam_g / gam_g) / |z|)      (exact zeros when |z| <= lam_g / gam_g).
// Replacing Q_gg by gam_g I in the block's quadratic majorises the objective, so every block
// step descends for ANY gam_g that bounds lambda_max(Q_gg) + l2 from above; group_bound_kernel
// takes the largest absolute row sum of Q_gg (|A|_2 <= |A|_inf for a symmetric A), which a
// singleton group attains exactly (gam = Q_jj: the step is then cd.hip's coordinate step).
//
// Layout (group_cd_kernel): one 256-thread workgroup solves up to FPW consecutive fits that
// share one Q.  The running vector hv = Q w - q of every fit lives in registers (thread t
// owns coordinates t + 256 r, as enet_cd_reg_kernel does); the coefficients w [FPW][p] and one
// block's staging area [FPW][kmax] live in LDS.  A block step:
//   1. the owners publish hv at the block's columns to the staging area;
//   2. one wave per fit forms z, |z| (per-lane partial sums in a fixed order, then an xor
//      butterfly: the same bits on every lane and on every call), the new w_g and the move
//      d = w_new - w_old, which replaces z in the staging area;
//   3. if any fit moved, the k_g rows of Q of the block are read ONCE for all FPW fits (next
//      row prefetched into registers) and folded into the hv registers.
// A block that does not move costs its k_g-long gradient read only; a converged fit moves no
// more.  Three workgroup barriers per block step, none per column.
#include "common.h"

#include <vector>

namespace sglm {

constexpr int kGT = 256;          // threads per workgroup
constexpr int kGW = kGT / 64;     // waves per workgroup
constexpr int kGMaxP = 4096;      // as sglm_enet_cd_shared

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// gamma[m][g] = max_i sum_j |Q_m[c_i][c_j]| over the columns c of group g: an upper bound of
// lambda_max of the block (Gershgorin).  Groups of more than one column carry a relative
// 1e-12 on top, which covers the rounding of the k-term sums (k <= 4096: below 1e-12).
__global__ void __launch_bounds__(kGT) group_bound_kernel(const double* __restrict__ Qall,
                                                          int32_t p,
                                                          const int32_t* __restrict__ goff,
                                                          const int32_t* __restrict__ gcols,
                                                          int32_t ng,
                                                          double* __restrict__ gamma) {
    __shared__ double s_m[kGW];
    const int g = blockIdx.x, m = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* Q = Qall + (int64_t)m * p * p;
    const int o = goff[g], k = goff[g + 1] - o;
    double mx = 0.0;
    for (int e = wave; e < k; e += kGW) {
        const double* row = Q + (int64_t)gcols[o + e] * p;
        double s = 0.0;
        for (int f = lane; f < k; f += 64) s += fabs(row[gcols[o + f]]);
        mx = fmax(mx, wave_sum_d(s));
    }
    if (lane == 0) s_m[wave] = mx;
    __syncthreads();
    if (tid == 0) {
        double v = s_m[0];
        for (int i = 1; i < kGW; ++i) v = fmax(v, s_m[i]);
        gamma[(int64_t)m * ng + g] = k > 1 ? v * (1.0 + 1e-12) : v;
    }
}

template <int FPW, int RR>
__global__ void __launch_bounds__(kGT) group_cd_kernel(
    const double* __restrict__ Qall, int32_t p, const int32_t* __restrict__ qidx, int32_t nfit,
    const double* __restrict__ qv, const int32_t* __restrict__ goff,
    const int32_t* __restrict__ gcols, int32_t ng, int32_t kmax,
    const double* __restrict__ gamma, const double* __restrict__ lamv,
    const double* __restrict__ l2v, int32_t max_sweeps, double tol, double* __restrict__ wout,
    int32_t* __restrict__ sweeps_out) {
    extern __shared__ double lds[];
    double* s_w = lds;                                    // [FPW][p] coefficients
    double* s_g = lds + (size_t)FPW * p;                  // [FPW][kmax] hv -> z -> move
    int* s_cols = (int*)(s_g + (size_t)FPW * kmax);       // [p] the groups' column lists
    constexpr int FW = (FPW + kGW - 1) / kGW;             // fits decided by one wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // group id and position inside its group of every owned coordinate (inverse of the CSR),
    // through a temporary in the coefficient area
    int gid[RR], gpos[RR];
    {
        int* t_gid = (int*)s_w;
        int* t_pos = t_gid + p;
        for (int e = tid; e < p; e += kGT) {
            int lo = 0, hi = ng;                          // goff[lo] <= e < goff[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (goff[mid] <= e) lo = mid; else hi = mid;
            }
            const int c = gcols[e];
            s_cols[e] = c;
            t_gid[c] = lo;
            t_pos[c] = e - goff[lo];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RR; ++r) {
            const int k = tid + r * kGT;
            gid[r] = k < p ? t_gid[k] : -1;
            gpos[r] = k < p ? t_pos[k] : 0;
        }
        __syncthreads();
    }

    // the workgroup's fits, one run of equal Q after the other (one run when the caller has
    // sorted the fits by Q, but for a chunk that straddles two Q)
    const int f0 = blockIdx.x * FPW;
    const int f1 = f0 + FPW < nfit ? f0 + FPW : nfit;
    for (int s = f0; s < f1;) {
        const int qi = qidx[s];
        int fe = s + 1;
        while (fe < f1 && qidx[fe] == qi) ++fe;
        const int nf = fe - s;
        const double* Q = Qall + (int64_t)qi * p * p;
        const double* gam = gamma + (int64_t)qi * ng;

        double hv[FPW][RR];
#pragma unroll
        for (int r = 0; r < RR; ++r) {
            const int k = tid + r * kGT;
#pragma unroll
            for (int i = 0; i < FPW; ++i)
                hv[i][r] = (k < p && i < nf) ? -qv[(int64_t)(s + i) * p + k] : 0.0;
        }
        for (int j = tid; j < FPW * p; j += kGT) s_w[j] = 0.0;
        bool act[FW];
        double lam[FW], l2[FW];
        int sw_done[FW];
#pragma unroll
        for (int u = 0; u < FW; ++u) {
            const int i = wave + kGW * u;
            act[u] = i < FPW && i < nf;
            lam[u] = act[u] ? lamv[s + i] : 0.0;
            l2[u] = act[u] ? l2v[s + i] : 0.0;
            sw_done[u] = max_sweeps;
        }
        __syncthreads();

        for (int sweep = 0; sweep < max_sweeps; ++sweep) {
            bool anyact = false;
#pragma unroll
            for (int u = 0; u < FW; ++u) anyact |= act[u];
            if (!__syncthreads_or(anyact ? 1 : 0)) break;
            double mdw[FW], mw[FW];
#pragma unroll
            for (int u = 0; u < FW; ++u) { mdw[u] = 0.0; mw[u] = 0.0; }

            for (int g = 0; g < ng; ++g) {
                const int o = goff[g], k = goff[g + 1] - o;
                // 1. the owners publish hv at the block's columns
#pragma unroll
                for (int r = 0; r < RR; ++r) {
                    if (gid[r] == g) {
#pragma unroll
                        for (int i = 0; i < FPW; ++i) s_g[(size_t)i * kmax + gpos[r]] = hv[i][r];
                    }
                }
                __syncthreads();
                // 2. one wave per fit: trial point, its norm, the shrunk block and the move
                bool moved = false;
                const double gq = gam[g];
                const double sk = sqrt((double)k);
#pragma unroll
                for (int u = 0; u < FW; ++u) {
                    const int i = wave + kGW * u;
                    if (i >= FPW) continue;
                    double* zi = s_g + (size_t)i * kmax;
                    double* wi = s_w + (size_t)i * p;
                    const double G = gq + l2[u];
                    if (act[u] && G > 0.0) {
                        const double inv = 1.0 / G;
                        const double thr = lam[u] * sk * inv;
                        double ss = 0.0;
                        for (int e = lane; e < k; e += 64) {
                            const double wc = wi[s_cols[o + e]];
                            const double z = wc - (zi[e] + l2[u] * wc) * inv;
                            zi[e] = z;
                            ss = fma(z, z, ss);
                        }
                        const double nrm = sqrt(wave_sum_d(ss));
                        const double sc = nrm > thr ? 1.0 - thr / nrm : 0.0;
                        for (int e = lane; e < k; e += 64) {
                            const int c = s_cols[o + e];
                            const double wc = wi[c];
                            const double nw = sc > 0.0 ? sc * zi[e] : 0.0;
                            const double d = nw - wc;
                            wi[c] = nw;
                            zi[e] = d;
                            mdw[u] = fmax(mdw[u], fabs(d));
                            mw[u] = fmax(mw[u], fabs(nw));
                            moved |= d != 0.0;
                        }
                    } else {
                        for (int e = lane; e < k; e += 64) zi[e] = 0.0;
                        if (act[u])                      // a null block (Q_gg = 0, l2 = 0)
                            for (int e = lane; e < k; e += 64)
                                mw[u] = fmax(mw[u], fabs(wi[s_cols[o + e]]));
                    }
                }
                // 3. fold the block's rows of Q into every fit's running vector
                if (__syncthreads_or(moved ? 1 : 0)) {
                    double qn[RR];
                    {
                        const double* Qn = Q + (int64_t)s_cols[o] * p;
#pragma unroll
                        for (int r = 0; r < RR; ++r) {
                            const int kk = tid + r * kGT;
                            qn[r] = kk < p ? Qn[kk] : 0.0;
                        }
                    }
                    for (int e = 0; e < k; ++e) {
                        double qc[RR];
#pragma unroll
                        for (int r = 0; r < RR; ++r) qc[r] = qn[r];
                        if (e + 1 < k) {
                            const double* Qn = Q + (int64_t)s_cols[o + e + 1] * p;
#pragma unroll
                            for (int r = 0; r < RR; ++r) {
                                const int kk = tid + r * kGT;
                                if (kk < p) qn[r] = Qn[kk];
                            }
                        }
                        double dv[FPW];
                        bool any = false;
#pragma unroll
                        for (int i = 0; i < FPW; ++i) {
                            dv[i] = s_g[(size_t)i * kmax + e];
                            any |= dv[i] != 0.0;
                        }
                        if (any) {
#pragma unroll
                            for (int r = 0; r < RR; ++r)
#pragma unroll
                                for (int i = 0; i < FPW; ++i)
                                    hv[i][r] = fma(qc[r], dv[i], hv[i][r]);
                        }
                    }
                    __syncthreads();                     // the moves are read before the next publish
                }
            }
            // per-fit stopping rule on the deciding wave (enet's: max|dw| <= tol max|w|)
#pragma unroll
            for (int u = 0; u < FW; ++u) {
                if (!act[u]) continue;
                const double a = wave_max_d(mdw[u]), b = wave_max_d(mw[u]);
                if (b == 0.0 || a <= tol * b) {
                    act[u] = false;
                    sw_done[u] = sweep + 1;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < FW; ++u) {
            const int i = wave + kGW * u;
            if (lane == 0 && i < FPW && i < nf) sweeps_out[s + i] = sw_done[u];
        }
        for (int i = 0; i < nf; ++i)
            for (int j = tid; j < p; j += kGT) wout[(int64_t)(s + i) * p + j] = s_w[(size_t)i * p + j];
        __syncthreads();
        s = fe;
    }
}

// The group CSR on the host (it is validated there; at most 2 x 4097 ints): offsets start at 0,
// end at p and increase strictly; the column list is a permutation of 0..p-1.  (Shared with
// sglm_cov_groups, infer.hip.)
int read_groups(const char* who, int32_t p, const int32_t* goff, const int32_t* gcols,
                       int32_t ng, hipStream_t s, int32_t* kmax) {
    std::vector<int32_t> off((size_t)ng + 1), cols((size_t)p);
    if (hipMemcpyAsync(off.data(), goff, off.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        hipMemcpyAsync(cols.data(), gcols, cols.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                       s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        set_error("%s: reading the group lists failed", who);
        return SGLM_EHIP;
    }
    if (off[0] != 0 || off[ng] != p) {
        set_error("%s: group offsets must run from 0 to p=%d", who, p);
        return SGLM_EINVAL;
    }
    int32_t km = 0;
    for (int g = 0; g < ng; ++g) {
        const int32_t k = off[g + 1] - off[g];
        if (k < 1) {
            set_error("%s: group %d is empty or its offsets decrease", who, g);
            return SGLM_EINVAL;
        }
        km = k > km ? k : km;
    }
    std::vector<char> seen((size_t)p, 0);
    for (int e = 0; e < p; ++e) {
        const int32_t c = cols[e];
        if (c < 0 || c >= p || seen[c]) {
            set_error("%s: gcols[%d]=%d is outside [0, %d) or listed twice", who, e, c, p);
            return SGLM_EINVAL;
        }
        seen[c] = 1;
    }
    *kmax = km;
    return SGLM_OK;
}

template <int FPW, int RR>
static int launch_group_cd(const double* Q, int32_t p, const int32_t* qidx, int32_t nfit,
                           const double* q, const int32_t* goff, const int32_t* gcols, int32_t ng,
                           int32_t kmax, const double* gamma, const double* lam, const double* l2,
                           int32_t max_sweeps, double tol, double* w, int32_t* sweeps,
                           hipStream_t s) {
    const size_t lds = (size_t)FPW * ((size_t)p + kmax) * sizeof(double) + (size_t)p * sizeof(int);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&group_cd_kernel<FPW, RR>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        set_error("group_cd_kernel: %zu bytes of LDS refused", lds);
        return SGLM_EHIP;
    }
    const unsigned nwg = (unsigned)((nfit + FPW - 1) / FPW);
    group_cd_kernel<FPW, RR><<<nwg, kGT, lds, s>>>(Q, p, qidx, nfit, q, goff, gcols, ng, kmax,
                                                  gamma, lam, l2, max_sweeps, tol, w, sweeps);
    return check_launch("group_cd_kernel");
}

}  // namespace sglm

using namespace sglm;

// consecutive fits that one workgroup of sglm_group_cd_shared solves together (they share the
// row stream of Q when their qidx are equal): the hv registers hold FPW x ceil(p / 256) doubles
extern "C" int32_t sglm_group_cd_fits_per_wg(int32_t p) {
    return p <= 4 * kGT ? 8 : p <= 8 * kGT ? 4 : 2;
}

extern "C" int sglm_group_bound(const double* Q, int32_t p, int32_t nq, const int32_t* goff,
                                const int32_t* gcols, int32_t ng, double* gamma,
                                sglm_stream_t stream) {
    if (nq <= 0) return SGLM_OK;
    if (!Q || !goff || !gcols || !gamma || p < 1 || p > kGMaxP || ng < 1 || ng > p ||
        nq > 65535) {
        set_error("sglm_group_bound: bad args (p=%d, max %d; ng=%d nq=%d)", p, kGMaxP, ng, nq);
        return SGLM_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    int32_t kmax = 0;
    const int st = read_groups("sglm_group_bound", p, goff, gcols, ng, s, &kmax);
    if (st) return st;
    group_bound_kernel<<<dim3((unsigned)ng, (unsigned)nq), kGT, 0, s>>>(Q, p, goff, gcols, ng,
                                                                        gamma);
    return check_launch("group_bound_kernel");
}

extern "C" int sglm_group_cd_shared(const double* Q, int32_t p, const int32_t* qidx, int32_t nfit,
                                    const double* q, const int32_t* goff, const int32_t* gcols,
                                    int32_t ng, const double* gamma, const double* lam_scale,
                                    const double* l2, int32_t max_sweeps, double tol, double* w,
                                    int32_t* sweeps, sglm_stream_t stream) {
    if (nfit <= 0) return SGLM_OK;
    if (!Q || !qidx || !q || !goff || !gcols || !gamma || !lam_scale || !l2 || !w || !sweeps ||
        p < 1 || p > kGMaxP || ng < 1 || ng > p) {
        set_error("sglm_group_cd_shared: bad args (p=%d, max %d; ng=%d)", p, kGMaxP, ng);
        return SGLM_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    int32_t kmax = 0;
    const int st = read_groups("sglm_group_cd_shared", p, goff, gcols, ng, s, &kmax);
    if (st) return st;
#define SGLM_GCD(FPW, RR)                                                                      \
    return launch_group_cd<FPW, RR>(Q, p, qidx, nfit, q, goff, gcols, ng, kmax, gamma,         \
                                    lam_scale, l2, max_sweeps, tol, w, sweeps, s)
    if (p <= kGT) SGLM_GCD(8, 1);
    if (p <= 2 * kGT) SGLM_GCD(8, 2);
    if (p <= 4 * kGT) SGLM_GCD(8, 4);
    if (p <= 8 * kGT) SGLM_GCD(4, 8);
    SGLM_GCD(2, 16);
#undef SGLM_GCD
}
