// Proximal Newton for the elastic-net penalised log-link fits (sglm_hip/pn.py).
//
// Objective per fit, in the engine's sum scaling (n = rows of the fit):
//   sum_i m_i loss(y_i, eta_i) + l1 |w|_1 + l2/2 |w|^2,  eta = X w + b,  b unpenalised,
//   l1 = alpha rho n, l2 = alpha (1 - rho) n.
// One outer iteration takes the exact float64-summed gradient g = X~^T (m loss') and the
// weighted Gram H = X~^T diag(m loss'') X~ (bf16 weights, f32 upper triangle, ones column at
// index p) from the IRLS kernels, and runs the three kernels of this file:
//   pn_model:  the intercept eliminated from the quadratic model (float64)
//                Q = H_xx - h h^T / H_pp,  g~ = g_x - h g_p / H_pp,  q = Q w - g~
//              (Q = H_xx, q = H_xx w - g_x without an intercept), so that the model over
//              u = w + delta_w is 1/2 u^T Q u - q^T u + l1 |u|_1 + l2/2 |u|^2;
//   enet_cd_warm: cyclic coordinate descent on that model from u = w with an active set;
//   pn_step:   delta_w = u - w, delta_b = -(g_p + h^T delta_w) / H_pp, the Armijo decrease, the
//              penalty at every trial step, the KKT violation of the current point.
// The Hessian only shapes the step: the fixed point (delta = 0) is where the exact gradient
// meets the KKT conditions, whatever the rounding of H.
#include "common.h"

namespace sglm {

constexpr int kPNT = 256;          // threads per workgroup (4 waves)
constexpr int kPNTile = 64;        // Q tile edge of pn_model
constexpr int kPNMaxP = 4096;      // as the other CD kernels
constexpr int kPNMaxT = 16;        // trial steps of pn_step

__device__ __forceinline__ float pn_gram_at(const float* G, int P, int a, int b) {
    return a <= b ? G[(int64_t)a * P + b] : G[(int64_t)b * P + a];
}

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// Q tile (ta, tb), ta <= tb, of fit blockIdx.y: the upper-triangle entries of H are read along
// rows (coalesced), centred, and written along rows of Q twice -- as tile (ta, tb) and, through
// LDS, transposed as tile (tb, ta).  h_a h_b is commutative, so Q is bitwise symmetric.
__global__ void __launch_bounds__(kPNT) pn_model_q_kernel(
    const float* __restrict__ Hall, int32_t P, int32_t p, const int32_t* __restrict__ slots,
    const uint8_t* __restrict__ icpt, int32_t ntile, double* __restrict__ Qall) {
    __shared__ double tile[kPNTile][kPNTile + 1];
    const int f = blockIdx.y;
    const float* H = Hall + (int64_t)slots[f] * P * P;
    double* Q = Qall + (int64_t)f * p * p;
    // tile pair from the linear index (row-major over the upper triangle of tiles)
    int ta = 0, rem = blockIdx.x;
    while (rem >= ntile - ta) { rem -= ntile - ta; ++ta; }
    const int tb = ta + rem;
    const double hpp = (double)H[(int64_t)p * P + p];
    const bool center = icpt[f] != 0 && hpp > 0.0;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int b = tb * kPNTile + tx;
    const double hb = (center && b < p) ? (double)H[(int64_t)b * P + p] : 0.0;
    for (int r = ty; r < kPNTile; r += 4) {
        const int a = ta * kPNTile + r;
        double v = 0.0;
        if (a < p && b < p && a <= b) {
            v = (double)H[(int64_t)a * P + b];
            if (center) v -= (double)H[(int64_t)a * P + p] * hb / hpp;
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < kPNTile; r += 4) {
        const int a = ta * kPNTile + r;
        if (a < p && b < p) {
            // a diagonal tile holds its upper half only: the lower half is its transpose
            Q[(int64_t)a * p + b] = (ta == tb && r > tx) ? tile[tx][r] : tile[r][tx];
        }
        if (ta != tb) {
            const int a2 = tb * kPNTile + r, b2 = ta * kPNTile + tx;
            if (a2 < p && b2 < p) Q[(int64_t)a2 * p + b2] = tile[tx][r];
        }
    }
}

// q_a = sum_b Q_ab w_b - g~_a: one wave per row of Q, lanes strided over b, butterfly sum
// (a fixed order).
__global__ void __launch_bounds__(kPNT) pn_model_q_vec_kernel(
    const float* __restrict__ Hall, int32_t P, int32_t p, const int32_t* __restrict__ slots,
    const uint8_t* __restrict__ icpt, const double* __restrict__ Qall,
    const double* __restrict__ gall, const double* __restrict__ ball, double* __restrict__ qall) {
    const int f = blockIdx.y;
    const int k = slots[f];
    const int a = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= p) return;
    const int lane = threadIdx.x & 63;
    const float* H = Hall + (int64_t)k * P * P;
    const double* Qa = Qall + ((int64_t)f * p + a) * p;
    const double* w = ball + (int64_t)k * P;
    const double* g = gall + (int64_t)k * P;
    double s = 0.0;
    for (int b = lane; b < p; b += 64) s += Qa[b] * w[b];
    s = wave_sum_d(s);
    if (lane == 0) {
        const double hpp = (double)H[(int64_t)p * P + p];
        double gt = g[a];
        if (icpt[f] != 0 && hpp > 0.0) gt -= (double)H[(int64_t)a * P + p] * g[p] / hpp;
        qall[(int64_t)f * p + a] = s - gt;
    }
}

// Warm-started cyclic CD with an active set, one workgroup per fit, float64.  Every thread
// holds the same copy of the coordinate decision (w, hv and Q's diagonal live in LDS), so a
// coordinate costs a barrier pair, and only when it moves.  Schedule: a full sweep; sweeps over
// the coordinates with u_j != 0 until max|du| <= tol max|u|; a full sweep again; until a full
// sweep meets the tolerance too.  A start that already meets it in the first full sweep is
// returned as it came (bitwise).
__global__ void __launch_bounds__(kPNT) enet_cd_warm_kernel(
    const double* __restrict__ Qall, int32_t p, const double* __restrict__ qv,
    const double* __restrict__ l1v, const double* __restrict__ l2v, int32_t max_sweeps,
    double tol, double* __restrict__ wio, int32_t* __restrict__ sweeps_out,
    int32_t* __restrict__ nnz_out) {
    extern __shared__ __attribute__((aligned(16))) char pn_smem[];
    double* w = reinterpret_cast<double*>(pn_smem);
    double* hv = w + p;
    double* qd = hv + p;
    int32_t* act = reinterpret_cast<int32_t*>(qd + p);
    const int f = blockIdx.x;
    const double* Q = Qall + (int64_t)f * p * p;
    const double l1 = l1v[f], l2 = l2v[f];
    const int tid = threadIdx.x;
    for (int j = tid; j < p; j += kPNT) {
        w[j] = wio[(int64_t)f * p + j];
        hv[j] = -qv[(int64_t)f * p + j];
        qd[j] = Q[(int64_t)j * p + j];
    }
    __syncthreads();
    // hv = Q u - q at the start, rows in ascending order (Q is symmetric)
    for (int j = 0; j < p; ++j) {
        const double uj = w[j];
        if (uj != 0.0) {
            const double* Qj = Q + (int64_t)j * p;
            for (int k = tid; k < p; k += kPNT) hv[k] += Qj[k] * uj;
        }
    }
    __syncthreads();
    int nfull = 0, nact_sw = 0, na = 0;
    bool changed = false, full = true, done = false;
    while (!done && nfull + nact_sw < max_sweeps) {
        const int cnt = full ? p : na;
        double mdu = 0.0, mu = 0.0;
        // the next coordinate's row of Q is loaded while this one is decided and applied (the
        // first 2 x 256 columns in registers: the serial chain otherwise waits for each row)
        int j = cnt > 0 ? (full ? 0 : act[0]) : 0;
        double c0 = tid < p ? Q[(int64_t)j * p + tid] : 0.0;
        double c1 = tid + kPNT < p ? Q[(int64_t)j * p + tid + kPNT] : 0.0;
        for (int i = 0; i < cnt; ++i) {
            const int jn = i + 1 < cnt ? (full ? i + 1 : act[i + 1]) : j;
            const double n0 = tid < p ? Q[(int64_t)jn * p + tid] : 0.0;
            const double n1 = tid + kPNT < p ? Q[(int64_t)jn * p + tid + kPNT] : 0.0;
            const double qjj = qd[j], wj = w[j];
            double nu = 0.0;
            if (qjj > 0.0) {
                const double rho = qjj * wj - hv[j];
                const double mag = fabs(rho) - l1;
                nu = mag > 0.0 ? copysign(mag, rho) / (qjj + l2) : 0.0;
            }
            const double d = nu - wj;
            mu = fmax(mu, fabs(nu));
            if (d != 0.0) {                     // the same d in every thread: a uniform branch
                mdu = fmax(mdu, fabs(d));
                const double* Qj = Q + (int64_t)j * p;
                __syncthreads();                // every thread has read w[j] and hv[j]
                if (tid < p) hv[tid] += c0 * d;
                if (tid + kPNT < p) hv[tid + kPNT] += c1 * d;
                for (int k = tid + 2 * kPNT; k < p; k += kPNT) hv[k] += Qj[k] * d;
                if (tid == 0) w[j] = nu;
                __syncthreads();
            }
            j = jn;
            c0 = n0;
            c1 = n1;
        }
        if (full) ++nfull; else ++nact_sw;
        if (mdu != 0.0) changed = true;
        const bool ok = mu == 0.0 || mdu <= tol * mu;
        if (full) {
            if (ok) {
                done = true;
            } else {
                // the active set: the coordinates this full sweep left non-zero
                __syncthreads();
                if (tid == 0) {
                    int c = 0;
                    for (int j = 0; j < p; ++j)
                        if (w[j] != 0.0) act[c++] = j;
                    act[p] = c;
                }
                __syncthreads();
                na = act[p];
                full = na == p;                 // nothing to restrict: full sweeps only
            }
        } else if (ok) {
            full = true;
        }
    }
    __syncthreads();
    // a start that met the tolerance in its first full sweep stays as it came
    const bool keep = done && nfull == 1 && nact_sw == 0;
    if (!keep && changed)
        for (int j = tid; j < p; j += kPNT) wio[(int64_t)f * p + j] = w[j];
    if (tid == 0) {
        int c = 0;
        if (keep) {
            for (int j = 0; j < p; ++j) c += wio[(int64_t)f * p + j] != 0.0;
        } else {
            for (int j = 0; j < p; ++j) c += w[j] != 0.0;
        }
        sweeps_out[2 * f] = nfull;
        sweeps_out[2 * f + 1] = nact_sw;
        nnz_out[f] = c;
    }
}

// block sums / maxima of `cnt` per-thread values in a fixed order (wave butterflies, then the
// four waves in order); the results land in red[0..cnt)
template <int N>
__device__ __forceinline__ void pn_block_reduce(double (&vals)[N], int cnt, bool is_max,
                                                double (*part)[4], double* red) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (i < cnt) {
            const double r = is_max ? wave_max_d(vals[i]) : wave_sum_d(vals[i]);
            if (lane == 0) part[i][wv] = r;
        }
    }
    __syncthreads();
    if (threadIdx.x < cnt) {
        const double* q = part[threadIdx.x];
        red[threadIdx.x] = is_max ? fmax(fmax(q[0], q[1]), fmax(q[2], q[3]))
                                  : ((q[0] + q[1]) + q[2]) + q[3];
    }
    __syncthreads();
}

// Per fit: the direction, the Armijo decrease, the penalties and coefficient scales of the
// trial steps, the KKT violation.  rec[f]: { delta_b, decrease, kkt, max|delta_w|,
// pen[0..T), maxb[0..T) } with pen[j] = l1 sum|w + t_j d| + l2/2 sum (w + t_j d)^2 and
// maxb[j] = max|w + t_j d| over the predictors (t_j == 1 evaluates u itself).
__global__ void __launch_bounds__(kPNT) pn_step_kernel(
    const float* __restrict__ Hall, int32_t P, int32_t p, const int32_t* __restrict__ slots,
    const uint8_t* __restrict__ icpt, const double* __restrict__ gall,
    const double* __restrict__ ball, const double* __restrict__ uall,
    const double* __restrict__ l1v, const double* __restrict__ l2v,
    const double* __restrict__ ts, int32_t T, float* __restrict__ dall,
    double* __restrict__ rec) {
    __shared__ double part[kPNMaxT + 8][4];
    __shared__ double red[kPNMaxT + 8];
    const int f = blockIdx.x;
    const int k = slots[f];
    const float* H = Hall + (int64_t)k * P * P;
    const double* g = gall + (int64_t)k * P;
    const double* w = ball + (int64_t)k * P;
    const double* u = uall + (int64_t)f * p;
    float* dl = dall + (int64_t)k * P;
    const double l1 = l1v[f], l2 = l2v[f];
    const double hpp = (double)H[(int64_t)p * P + p];
    const bool fi = icpt[f] != 0 && hpp > 0.0;
    const int tid = threadIdx.x;
    double tv[kPNMaxT];
#pragma unroll
    for (int j = 0; j < kPNMaxT; ++j) tv[j] = j < T ? ts[j] : 0.0;
    // sums: h.d, g.d, w.d, |u|_1, |w|_1, then the T penalties; maxima: kkt, max|d|, T scales
    double sv[5 + kPNMaxT], mv[2 + kPNMaxT];
    for (int i = 0; i < 5 + kPNMaxT; ++i) sv[i] = 0.0;
    for (int i = 0; i < 2 + kPNMaxT; ++i) mv[i] = 0.0;
    for (int j = tid; j < p; j += kPNT) {
        const double wj = w[j], uj = u[j], gj = g[j];
        const double d = uj - wj;
        dl[j] = (float)d;
        if (fi) sv[0] += (double)H[(int64_t)j * P + p] * d;
        sv[1] += gj * d;
        sv[2] += wj * d;
        sv[3] += fabs(uj);
        sv[4] += fabs(wj);
        const double gs = gj + l2 * wj;
        const double v = wj != 0.0 ? fabs(gs + (wj > 0.0 ? l1 : -l1)) : fmax(fabs(gs) - l1, 0.0);
        mv[0] = fmax(mv[0], v);
        mv[1] = fmax(mv[1], fabs(d));
#pragma unroll
        for (int q = 0; q < kPNMaxT; ++q) {
            if (q < T) {
                const double x = tv[q] == 1.0 ? uj : wj + tv[q] * d;
                sv[5 + q] += l1 * fabs(x) + 0.5 * l2 * x * x;
                mv[2 + q] = fmax(mv[2 + q], fabs(x));
            }
        }
    }
    for (int j = p + 1 + tid; j < P; j += kPNT) dl[j] = 0.0f;
    double out_s[5 + kPNMaxT];
    pn_block_reduce(sv, 5 + T, false, part, red);
#pragma unroll
    for (int i = 0; i < 5 + kPNMaxT; ++i) out_s[i] = i < 5 + T ? red[i] : 0.0;
    __syncthreads();
    pn_block_reduce(mv, 2 + T, true, part, red);
    if (tid == 0) {
        double* r = rec + (int64_t)f * (4 + 2 * T);
        const double gp = fi ? g[p] : 0.0;
        const double db = fi ? -(gp + out_s[0]) / hpp : 0.0;
        dl[p] = (float)db;
        r[0] = db;
        r[1] = out_s[1] + gp * db + l2 * out_s[2] + l1 * (out_s[3] - out_s[4]);
        r[2] = icpt[f] != 0 ? fmax(red[0], fabs(g[p])) : red[0];
        r[3] = red[1];
#pragma unroll
        for (int q = 0; q < kPNMaxT; ++q) {
            if (q < T) {
                r[4 + q] = out_s[5 + q];
                r[4 + T + q] = red[2 + q];
            }
        }
    }
}

// The step taken: w = u where t == 1 (zeros stay exact), else w + t (u - w); b += t delta_b.
__global__ void __launch_bounds__(kPNT) pn_update_kernel(
    int32_t P, int32_t p, const int32_t* __restrict__ slots, const double* __restrict__ step,
    const double* __restrict__ uall, const double* __restrict__ rec, int32_t rec_stride,
    double* __restrict__ ball) {
    const int f = blockIdx.x;
    const double t = step[f];
    if (t == 0.0) return;
    double* w = ball + (int64_t)slots[f] * P;
    const double* u = uall + (int64_t)f * p;
    for (int j = threadIdx.x; j < p; j += kPNT) w[j] = t == 1.0 ? u[j] : w[j] + t * (u[j] - w[j]);
    if (threadIdx.x == 0) w[p] += t * rec[(int64_t)f * rec_stride];
}

}  // namespace sglm

using namespace sglm;

extern "C" int sglm_pn_model(const float* H, int32_t P, int32_t p, const int32_t* slots,
                             const uint8_t* icpt, int32_t nfit, const double* g,
                             const double* beta, double* Q, double* q, sglm_stream_t stream) {
    if (nfit <= 0) return SGLM_OK;
    if (!H || !slots || !icpt || !g || !beta || !Q || !q || p < 1 || p >= P) {
        set_error("sglm_pn_model: bad args (p=%d, P=%d)", p, P);
        return SGLM_EINVAL;
    }
    const int ntile = (p + kPNTile - 1) / kPNTile;
    const unsigned pairs = (unsigned)(ntile * (ntile + 1) / 2);
    pn_model_q_kernel<<<dim3(pairs, (unsigned)nfit), kPNT, 0, as_stream(stream)>>>(
        H, P, p, slots, icpt, ntile, Q);
    int st = check_launch("pn_model_q_kernel");
    if (st != SGLM_OK) return st;
    pn_model_q_vec_kernel<<<dim3((unsigned)((p + 3) / 4), (unsigned)nfit), kPNT, 0,
                            as_stream(stream)>>>(H, P, p, slots, icpt, Q, g, beta, q);
    return check_launch("pn_model_q_vec_kernel");
}

extern "C" int sglm_enet_cd_warm(const double* Q, int32_t p, int32_t nfit, const double* q,
                                 const double* l1, const double* l2, int32_t max_sweeps,
                                 double tol, double* w, int32_t* sweeps, int32_t* nnz,
                                 sglm_stream_t stream) {
    if (nfit <= 0) return SGLM_OK;
    if (!Q || !q || !l1 || !l2 || !w || !sweeps || !nnz || p < 1 || p > kPNMaxP) {
        set_error("sglm_enet_cd_warm: bad args (p=%d, max %d)", p, kPNMaxP);
        return SGLM_EINVAL;
    }
    // w, hv, diag(Q) as doubles, then the active list and its count
    const size_t lds = (size_t)3 * p * sizeof(double) + ((size_t)p + 4) * sizeof(int32_t);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&enet_cd_warm_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        set_error("enet_cd_warm_kernel: %zu bytes of LDS refused", lds);
        return SGLM_EHIP;
    }
    enet_cd_warm_kernel<<<nfit, kPNT, lds, as_stream(stream)>>>(Q, p, q, l1, l2, max_sweeps, tol,
                                                               w, sweeps, nnz);
    return check_launch("enet_cd_warm_kernel");
}

extern "C" int sglm_pn_step(const float* H, int32_t P, int32_t p, const int32_t* slots,
                            const uint8_t* icpt, int32_t nfit, const double* g,
                            const double* beta, const double* u, const double* l1,
                            const double* l2, const double* ts, int32_t T, float* delta,
                            double* rec, sglm_stream_t stream) {
    if (nfit <= 0) return SGLM_OK;
    if (!H || !slots || !icpt || !g || !beta || !u || !l1 || !l2 || !ts || !delta || !rec ||
        p < 1 || p >= P || T < 1 || T > kPNMaxT) {
        set_error("sglm_pn_step: bad args (p=%d, P=%d, T=%d, max %d)", p, P, T, kPNMaxT);
        return SGLM_EINVAL;
    }
    pn_step_kernel<<<nfit, kPNT, 0, as_stream(stream)>>>(H, P, p, slots, icpt, g, beta, u, l1, l2,
                                                        ts, T, delta, rec);
    return check_launch("pn_step_kernel");
}

extern "C" int sglm_pn_update(int32_t P, int32_t p, const int32_t* slots, int32_t nfit,
                              const double* step, const double* u, const double* rec,
                              int32_t rec_stride, double* beta, sglm_stream_t stream) {
    if (nfit <= 0) return SGLM_OK;
    if (!slots || !step || !u || !rec || !beta || p < 1 || p >= P || rec_stride < 1) {
        set_error("sglm_pn_update: bad args");
        return SGLM_EINVAL;
    }
    pn_update_kernel<<<nfit, kPNT, 0, as_stream(stream)>>>(P, p, slots, step, u, rec, rec_stride,
                                                          beta);
    return check_launch("pn_update_kernel");
}
