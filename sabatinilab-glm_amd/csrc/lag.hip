// Gradient of a time-shifted event design, from the events themselves.
//
// The design of the north-star configuration is a timeshift expansion (backend/sglm_pp.py:
// 23-103, sglm_ez.timeshift_cols): column (b, a) of X is event column a of the base matrix E
// shifted by s_b rows, X[t, (b, a)] = E[t + row0 - s_b, a].  For a 0/1 event matrix
//     g[(b, a)] = sum_t R[t] X[t, (b, a)] = sum over occurrences u of event a of R[u - row0 + s_b],
// so X^T R needs every R value once per occurrence window (K lags), not once per predictor:
// ~ nnz(E) * K adds per fit instead of n * p.  (The dense bit-plane MFMA path, xtr_bits, reads
// each R row for every 128-predictor panel and needs three bf16 pieces of R to be exact.)
//
// Work split: a workgroup owns a fit group (FG fits, lanes = (fit, lag) pairs) and a range of
// row tiles (kLagU design rows each).  Per tile it stages R[f][t0 .. t0 + kLagU) in LDS, then
// walks every event's occurrences whose window reaches the tile (offsets precomputed per tile)
// and adds R[u - row0 + s_b] for its lag when that row lies in the tile: consecutive lanes read
// consecutive LDS words (conflict-free), all lanes walk the same occurrence list (uniform
// control flow).  One float64 accumulator per event stays in registers across the tiles of the
// range; the range's partial sums go to `work` and a fixed-order pass sums the ranges (the
// result does not depend on scheduling).  The intercept column p is the plain sum of R.
#include "common.h"

namespace sglm {
namespace {

constexpr int kLagT = 256;        // threads per workgroup: (fit, lag) pairs
constexpr int kLagU = 4096;       // design rows per tile
constexpr int kLagFG = 6;         // fits per workgroup at most (LDS: kLagFG x kLagU floats)
constexpr int kLagC = 8192;       // occurrences staged in LDS per chunk
constexpr int kLagMaxM = 64;      // events (register accumulators per lane)

struct LagArgs {
    const int32_t* occ;           // occurrence rows u of every event, event-major, ascending
    const int32_t* tbeg;          // [m][ntiles]: first occurrence index of event a whose
    const int32_t* tend;          //   window reaches tile i / one past the last
    const int32_t* shifts;        // [K]
    int32_t m, K, layout, P;      // layout 0: column b*m + a (shift-major), 1: a*K + b
    int64_t row0, n, ntiles;
};

// LDS: R tile [kLagFG][kLagU] f32 | occurrences [kLagC] i32 | per-event chunk ranges
struct LagLds {
    float r[kLagFG * kLagU];
    int32_t occ[kLagC];
    int32_t beg[kLagMaxM], len[kLagMaxM];          // this tile's segment of each event
    int32_t lo[kLagMaxM], hi[kLagMaxM];            // its part in the current chunk
    int32_t src[kLagMaxM];                         // occ index of lo
    int32_t done;                                  // all segments staged
};

template <int MAXM>
__global__ void __launch_bounds__(kLagT) lag_xtr_kernel(LagArgs a, const float* __restrict__ R,
                                                        int64_t ld,
                                                        const int32_t* __restrict__ slots,
                                                        int32_t nact, int32_t FG,
                                                        int32_t tiles_per,
                                                        double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    LagLds& L = *reinterpret_cast<LagLds*>(lds_raw);
    const int tid = threadIdx.x;
    const int f = tid / a.K, b = tid - f * a.K;
    const int q = blockIdx.y * FG + f;             // index in the active list
    const bool on = f < FG && q < nact;
    const int64_t range = blockIdx.x;
    const int64_t tile0 = range * tiles_per;
    const int64_t tile1 = tile0 + tiles_per < a.ntiles ? tile0 + tiles_per : a.ntiles;
    const int s = on ? a.shifts[b] : 0;
    const int nf = (nact - (int)blockIdx.y * FG) < FG ? (nact - (int)blockIdx.y * FG) : FG;
    double acc[MAXM];
#pragma unroll
    for (int e = 0; e < MAXM; ++e) acc[e] = 0.0;
    // intercept column: the plain sum of R, accumulated by the staging threads (thread tid,
    // fit ff: rows tid, tid + 256, ... of every tile), reduced in a fixed order at the end
    double accI[kLagFG];
#pragma unroll
    for (int ff = 0; ff < kLagFG; ++ff) accI[ff] = 0.0;
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t t0 = tile * kLagU;
        __syncthreads();                           // the previous tile's reads are done
        // R rows of the tile, float4 loads (kLagU and t0 are multiples of 4; ld >= n, and
        // rows past n are masked to 0)
#pragma unroll
        for (int ff = 0; ff < kLagFG; ++ff) {
            if (ff < nf) {
                const float* r = R + (int64_t)slots[blockIdx.y * FG + ff] * ld;
                f32x4 v[kLagU / 4 / kLagT];
#pragma unroll
                for (int j = 0; j < kLagU / 4 / kLagT; ++j) {
                    const int64_t t = t0 + 4 * (tid + j * kLagT);
                    v[j] = t + 4 <= a.n ? *reinterpret_cast<const f32x4*>(r + t)
                                        : f32x4{t < a.n ? r[t] : 0.0f,
                                                t + 1 < a.n ? r[t + 1] : 0.0f,
                                                t + 2 < a.n ? r[t + 2] : 0.0f, 0.0f};
                }
#pragma unroll
                for (int j = 0; j < kLagU / 4 / kLagT; ++j) {
                    *reinterpret_cast<f32x4*>(&L.r[ff * kLagU + 4 * (tid + j * kLagT)]) = v[j];
                    accI[ff] += ((double)v[j][0] + (double)v[j][1]) +
                                ((double)v[j][2] + (double)v[j][3]);
                }
            }
        }
        if (tid < a.m) {
            const int32_t i0 = a.tbeg[(int64_t)tid * a.ntiles + tile];
            L.beg[tid] = i0;
            L.len[tid] = a.tend[(int64_t)tid * a.ntiles + tile] - i0;
        }
        if (tid == 0) L.done = 0;
        const int64_t off = s - a.row0 - t0;       // tile row of occurrence u: u + off
        int e_cur = 0, i_cur = 0;                  // next segment position (uniform)
        while (true) {
            __syncthreads();
            if (L.done) break;
            // chunk layout (thread 0, which alone carries the resume point): whole or partial
            // event segments from (e_cur, i_cur), at most kLagC occurrences
            if (tid == 0) {
                int fill = 0, e = e_cur, i = i_cur;
                for (int x = 0; x < a.m; ++x) { L.lo[x] = 0; L.hi[x] = 0; }
                while (e < a.m && fill < kLagC) {
                    const int take = min(L.len[e] - i, kLagC - fill);
                    L.lo[e] = fill; L.hi[e] = fill + take; L.src[e] = L.beg[e] + i;
                    fill += take;
                    i += take;
                    if (i == L.len[e]) { ++e; i = 0; }
                }
                L.done = e >= a.m ? 2 : 0;                        // 2: the last chunk
                e_cur = e;
                i_cur = i;
            }
            __syncthreads();
            // stage the chunk's occurrences: flattened position j -> (event, index); each
            // thread walks j = tid, tid + 256, ... with a monotone event cursor, 4 loads in
            // flight at a time
            {
                int fill = 0;
                for (int x = 0; x < a.m; ++x) fill = L.hi[x] > fill ? L.hi[x] : fill;
                int e = 0;
                for (int j0 = tid; j0 < fill; j0 += 4 * kLagT) {
                    int32_t v[4];
                    int jj[4];
#pragma unroll
                    for (int z = 0; z < 4; ++z) {
                        const int j = j0 + z * kLagT;
                        jj[z] = j;
                        v[z] = 0;
                        if (j < fill) {
                            while (L.hi[e] <= j) ++e;
                            int ez = e;
                            while (L.lo[ez] > j) --ez;
                            v[z] = a.occ[L.src[ez] + (j - L.lo[ez])];
                        }
                    }
#pragma unroll
                    for (int z = 0; z < 4; ++z)
                        if (jj[z] < fill) L.occ[jj[z]] = v[z];
                }
            }
            __syncthreads();
            const float* rf = L.r + f * kLagU;
#pragma unroll
            for (int e = 0; e < MAXM; ++e) {
                if (e < a.m) {
                    const int i0 = L.lo[e], i1 = L.hi[e];
                    // 8 occurrences per step: their LDS reads are independent, the f64 sum is
                    // a fixed pairwise tree (deterministic)
                    double se = 0.0;
                    int i = i0;
                    for (; i + 8 <= i1; i += 8) {
                        float v[8];
#pragma unroll
                        for (int z = 0; z < 8; ++z) {
                            const int64_t tr = (int64_t)L.occ[i + z] + off;
                            v[z] = (on && tr >= 0 && tr < kLagU) ? rf[tr] : 0.0f;
                        }
                        se += (((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3])) +
                              (((double)v[4] + (double)v[5]) + ((double)v[6] + (double)v[7]));
                    }
                    for (; i < i1; ++i) {
                        const int64_t tr = (int64_t)L.occ[i] + off;
                        if (on && tr >= 0 && tr < kLagU) se += (double)rf[tr];
                    }
                    acc[e] += se;
                }
            }
            __syncthreads();
            if (tid == 0) L.done = L.done == 2 ? 1 : 0;
        }
    }
    __syncthreads();                               // LDS reused for the intercept sums
    double* red = reinterpret_cast<double*>(lds_raw);  // [nf][kLagT]
#pragma unroll
    for (int ff = 0; ff < kLagFG; ++ff)
        if (ff < nf) red[ff * kLagT + tid] = accI[ff];
    __syncthreads();
    double I = 0.0;
    if (on && b == 0)
        for (int i = 0; i < kLagT; ++i) I += red[f * kLagT + i];
    if (!on) return;
    double* out = part + (range * nact + q) * (int64_t)a.P;
#pragma unroll
    for (int e = 0; e < MAXM; ++e) {
        if (e < a.m) {
            const int col = a.layout ? e * a.K + b : b * a.m + e;
            out[col] = acc[e];
        }
    }
    if (b == 0) out[(int64_t)a.m * a.K] = I;
}

// g[slots[q]][c] = sum over ranges of part[range][q][c] (fixed order); padding columns 0
__global__ void __launch_bounds__(256) lag_reduce_kernel(const double* __restrict__ part,
                                                         int64_t nranges, int32_t nact,
                                                         int32_t P, int32_t ncols,
                                                         const int32_t* __restrict__ slots,
                                                         double* __restrict__ g) {
    const int64_t len = (int64_t)nact * P;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < len;
         e += (int64_t)gridDim.x * 256) {
        const int64_t q = e / P, c = e - q * P;
        double v = 0.0;
        if (c < ncols)
            for (int64_t r = 0; r < nranges; ++r) v += part[(r * nact) * (int64_t)P + e];
        g[(int64_t)slots[q] * P + c] = v;
    }
}

struct LagPlan {
    int FG, groups, tiles_per;
    int64_t ntiles, nranges;
};

LagPlan lag_plan(int32_t K, int32_t nact, int64_t n) {
    LagPlan p;
    p.FG = kLagT / K;
    if (p.FG > kLagFG) p.FG = kLagFG;              // LDS: FG x kLagU floats
    p.groups = (nact + p.FG - 1) / p.FG;
    p.ntiles = (n + kLagU - 1) / kLagU;
    // ~3 workgroups per CU over the fit groups x row ranges
    int64_t nr = (768 + p.groups - 1) / p.groups;
    if (nr > p.ntiles) nr = p.ntiles;
    if (nr < 1) nr = 1;
    p.tiles_per = (int)((p.ntiles + nr - 1) / nr);
    p.nranges = (p.ntiles + p.tiles_per - 1) / p.tiles_per;
    return p;
}

}  // namespace
}  // namespace sglm

using namespace sglm;

extern "C" int32_t sglm_lag_tile_rows(void) { return kLagU; }

extern "C" size_t sglm_lag_xtr_work_bytes(int32_t P, int32_t K, int32_t B, int64_t n) {
    if (K <= 0 || K > kLagT) return 0;
    size_t mx = 0;
    for (int32_t b = 1; b <= B; ++b) {
        const LagPlan p = lag_plan(K, b, n);
        const size_t w = (size_t)p.nranges * b * P * sizeof(double);
        if (w > mx) mx = w;
    }
    return mx;
}

extern "C" int sglm_lag_xtr(const int32_t* occ, const int32_t* tbeg, const int32_t* tend,
                            const int32_t* shifts, int32_t m, int32_t K, int32_t layout,
                            int64_t row0, int64_t n, int32_t P, const float* R, int64_t ld,
                            const int32_t* slots, int32_t nact, double* g, void* work,
                            sglm_stream_t stream) {
    if (nact <= 0) return SGLM_OK;
    if (!occ || !tbeg || !tend || !shifts || !R || !slots || !g || !work || m < 1 ||
        m > kLagMaxM || K < 1 || K > kLagT || (int64_t)m * K + 1 > P || n > ld || n <= 0) {
        set_error("sglm_lag_xtr: bad args (m=%d <= %d, K=%d, P=%d)", m, kLagMaxM, K, P);
        return SGLM_EINVAL;
    }
    const LagPlan pl = lag_plan(K, nact, n);
    LagArgs a;
    a.occ = occ; a.tbeg = tbeg; a.tend = tend; a.shifts = shifts;
    a.m = m; a.K = K; a.layout = layout; a.P = P; a.row0 = row0; a.n = n; a.ntiles = pl.ntiles;
    hipStream_t s = as_stream(stream);
    const size_t lds = sizeof(LagLds);
    double* part = (double*)work;
    dim3 grid((unsigned)pl.nranges, (unsigned)pl.groups);
    static bool attr = false;                      // > 64 KB of dynamic LDS (gfx950: 160 KB)
    if (!attr) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&lag_xtr_kernel<16>),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)sizeof(LagLds)) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void*>(&lag_xtr_kernel<kLagMaxM>),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)sizeof(LagLds)) != hipSuccess) {
            set_error("lag_xtr_kernel: %d bytes of LDS refused", (int)sizeof(LagLds));
            return SGLM_EHIP;
        }
        attr = true;
    }
    if (m <= 16)
        lag_xtr_kernel<16><<<grid, kLagT, lds, s>>>(a, R, ld, slots, nact, pl.FG, pl.tiles_per,
                                                    part);
    else
        lag_xtr_kernel<kLagMaxM><<<grid, kLagT, lds, s>>>(a, R, ld, slots, nact, pl.FG,
                                                          pl.tiles_per, part);
    int st = check_launch("lag_xtr_kernel");
    if (st) return st;
    const int64_t len = (int64_t)nact * P;
    lag_reduce_kernel<<<(unsigned)((len + 255) / 256 < 4096 ? (len + 255) / 256 : 4096), 256, 0,
                        s>>>(part, pl.nranges, nact, P, m * K + 1, slots, g);
    return check_launch("lag_reduce_kernel");
}

// ---- the occurrence walk at LDS rate on the packed R (sglm_lag_xtr_packed_bp) ---------------
// The same sum as lag_xtr_kernel, g[(b, a)] = sum over occurrences u of R[u - row0 + s_b], read
// from the packed three-piece R rows the link writes (no f32 rows needed) and laid out so that
// the inner loop is one wave-uniform occurrence -> K/4 ds_read_b32 + K/4 f32 adds per lane:
//   * a workgroup (4 waves) owns 16 fits and a range of row tiles.  A tile is kPxU design rows
//     plus a halo of H rows in front (H >= K, a multiple of 8), staged in LDS as [row][fit] f32
//     ((hi + mid) + lo, exactly the f32 the link split); rows outside [0, n) are zeros;
//   * the shifts are a contiguous range smin..smax, so an occurrence's window is K consecutive
//     design rows from v = u - row0 + smin.  The occurrence belongs to the tile whose staged
//     rows start at or before v and whose next tile starts after it (tile i: v in
//     [i U - H, (i + 1) U - H)): the whole window lies in the staged rows, so the inner loop has
//     no per-lane bounds test;
//   * lane = (fit f = lane & 15, phase q = lane >> 4) takes sorted lags j = q + 4 i: one
//     ds_read_b32 of the wave reads rows v + 4 i .. + 3 of all 16 fits = 64 consecutive words,
//     64 distinct banks.  Wave w owns events a = w + 4 e; the f32 accumulators [e][i] stay in
//     registers across the whole row range (statically unrolled);
//   * the staging store transposes (a thread holds 8 consecutive rows of one fit): lane group
//     g = lane >> 4 stores its element k ^ g in step k, so the four groups of a wave hit four
//     different rows mod 4 -- again 64 distinct banks;
//   * the occurrence indices are wave-uniform: a tile's [event] offsets are one coalesced load
//     (prefetched a tile ahead), the first 64 occurrences of every event of the wave are
//     loaded lane-parallel before the staging and broadcast with v_readlane.
// Range partials go to `work` (f32, the accumulators themselves; the intercept's in float64)
// and px_reduce_kernel sums them in float64 in a fixed order.
namespace sglm {
namespace {

constexpr int kPxT = 256;          // threads per workgroup
constexpr int kPxU = 1024;         // owned design rows per tile
constexpr int kPxF = 16;           // fits per workgroup
constexpr int kPxMaxM = 64;        // events: one lane of the offset load each
constexpr int kPxMaxK = 40;        // lags: 4 phases x 10 accumulators per event
constexpr int kPxWgTarget = 512;   // workgroups aimed at: two per CU
constexpr int kPxPadBlocks = 64;   // blocks of the reduction that zero the padding columns
// bytes of one (row range, 16-fit group) of partials at the largest instantiation: 4 waves x 16
// events x NI lags x 64 lanes f32, and 16 float64 intercepts
constexpr size_t px_group_bytes(int ni) { return (size_t)4 * 16 * ni * 64 * 4 + kPxF * 8; }

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct PxArgs {
    const int32_t* occ;            // raw occurrence rows, event-major, ascending per event
    const int32_t* toff;           // [ntiles + 1][m]: first occurrence of event a owned by tile i
    const int32_t* lagpos;         // [K]: lag index b of sorted position j (shifts[b] = smin + j)
    int32_t nocc, m, K, layout, P, H;
    int32_t voff;                  // design row of an occurrence's first lag = u + voff
    int32_t ntiles, tiles_per;
    int64_t n, ld;
};

__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xFFFF0000u); }

template <int ME, int NI, int UN>
__global__ void __launch_bounds__(kPxT)
lag_xtr_packed_kernel(PxArgs a, const uint16_t* __restrict__ Rp, int64_t plane, int32_t count,
                      float* __restrict__ part, double* __restrict__ partI) {
    static_assert(NI % 2 == 0, "accumulators are paired");
    extern __shared__ __attribute__((aligned(16))) char px_lds[];
    float* L = reinterpret_cast<float*>(px_lds);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int range = blockIdx.x, grp = blockIdx.y;
    const int tile0 = range * a.tiles_per;
    const int tile1 = min(tile0 + a.tiles_per, a.ntiles);
    const int nch = (kPxU + a.H) >> 3;             // 8-row chunks staged per tile
    const int hch = a.H >> 3;                      // of which halo (counted by the tile before)
    // staging: this thread's fit (256 % 16 == 0: one fit per thread) and lane group
    const int sf = tid & 15, sg = (tid >> 4) & 3;
    const bool son = grp * kPxF + sf < count;
    const uint16_t* rrow = Rp + (int64_t)(grp * kPxF + sf) * a.ld;
    double accI = 0.0;                             // intercept: plain sum of the owned rows
    f32x2 acc[ME][NI / 2];
#pragma unroll
    for (int e = 0; e < ME; ++e)
#pragma unroll
        for (int i = 0; i < NI / 2; ++i) acc[e][i] = (f32x2){0.0f, 0.0f};
    int32_t nxt = 0, cur_b = 0;
    if (lane < a.m) {
        cur_b = a.toff[(int64_t)tile0 * a.m + lane];
        nxt = a.toff[(int64_t)(tile0 + 1) * a.m + lane];
    }
    for (int tile = tile0; tile < tile1; ++tile) {
        const int32_t tb = cur_b, te = nxt;
        cur_b = te;
        if (tile + 1 < tile1 && lane < a.m) nxt = a.toff[(int64_t)(tile + 2) * a.m + lane];
        // the first 64 occurrences of each of the wave's events (lands during the staging)
        int32_t ov[ME];
#pragma unroll
        for (int e = 0; e < ME; ++e) {
            const int ae = w + 4 * e;
            ov[e] = 0;
            if (ae < a.m) {
                const int b0 = __builtin_amdgcn_readlane(tb, ae);
                const int c0 = __builtin_amdgcn_readlane(te, ae) - b0;
                if (lane < c0 && b0 >= 0 && b0 + lane < a.nocc) ov[e] = a.occ[b0 + lane];
            }
        }
        const int t0 = tile * kPxU - a.H;          // design row of staged row 0
        __syncthreads();                           // the previous tile's reads are done
        for (int cb = tid >> 4; cb < nch; cb += 48) {
            u32x4 hi[3], mi[3], lo[3];
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const int c = cb + 16 * x;
                const int64_t t = (int64_t)t0 + 8 * c;
                hi[x] = mi[x] = lo[x] = (u32x4){0u, 0u, 0u, 0u};
                if (son && c < nch && t >= 0 && t < a.n) {
                    const uint16_t* p = rrow + t;
                    hi[x] = *reinterpret_cast<const u32x4*>(p);
                    mi[x] = *reinterpret_cast<const u32x4*>(p + plane);
                    lo[x] = *reinterpret_cast<const u32x4*>(p + 2 * plane);
                }
            }
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const int c = cb + 16 * x;
                if (c >= nch) break;
                const int64_t t = (int64_t)t0 + 8 * c;
                float v[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v[2 * k] = (bf_lo(hi[x][k]) + bf_lo(mi[x][k])) + bf_lo(lo[x][k]);
                    v[2 * k + 1] = (bf_hi(hi[x][k]) + bf_hi(mi[x][k])) + bf_hi(lo[x][k]);
                }
                if (t + 8 > a.n) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = t + k < a.n ? v[k] : 0.0f;
                }
                if (c >= hch)
                    accI += (((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3])) +
                            (((double)v[4] + (double)v[5]) + ((double)v[6] + (double)v[7]));
                // element k ^ sg in step k (two conditional swap stages)
                float s1[8], s2[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) s1[k] = (sg & 1) ? v[k ^ 1] : v[k];
#pragma unroll
                for (int k = 0; k < 8; ++k) s2[k] = (sg & 2) ? s1[k ^ 2] : s1[k];
                float* dst = L + c * (8 * kPxF) + sf;
#pragma unroll
                for (int k = 0; k < 8; ++k) dst[(k ^ sg) * kPxF] = s2[k];
            }
        }
        __syncthreads();
        const int uoff = a.voff - t0;              // staged row of the first lag: u + uoff
        const float* Ll = L + lane;
#pragma unroll
        for (int e = 0; e < ME; ++e) {
            const int ae = w + 4 * e;
            if (ae >= a.m) continue;
            const int b0 = __builtin_amdgcn_readlane(tb, ae);
            const int c0 = __builtin_amdgcn_readlane(te, ae) - b0;
            int32_t cur = ov[e];
            for (int base = 0; base < c0; base += 64) {
                const int nn = min(64, c0 - base);
                if (base) {
                    cur = 0;
                    if (lane < nn && b0 >= 0 && b0 + base + lane < a.nocc)
                        cur = a.occ[b0 + base + lane];
                }
                int z = 0;
                for (; z + UN <= nn; z += UN) {
                    float r[UN][NI];
#pragma unroll
                    for (int y = 0; y < UN; ++y) {
                        int u = __builtin_amdgcn_readlane(cur, z + y) + uoff;
                        u = min(max(u, 0), kPxU - 1);
                        const float* p = Ll + u * kPxF;
#pragma unroll
                        for (int i = 0; i < NI; ++i) r[y][i] = p[i * (4 * kPxF)];
                    }
#pragma unroll
                    for (int y = 0; y < UN; ++y)
#pragma unroll
                        for (int i = 0; i < NI / 2; ++i)
                            acc[e][i] += (f32x2){r[y][2 * i], r[y][2 * i + 1]};
                }
                for (; z < nn; ++z) {
                    int u = __builtin_amdgcn_readlane(cur, z) + uoff;
                    u = min(max(u, 0), kPxU - 1);
                    const float* p = Ll + u * kPxF;
                    float r[NI];
#pragma unroll
                    for (int i = 0; i < NI; ++i) r[i] = p[i * (4 * kPxF)];
#pragma unroll
                    for (int i = 0; i < NI / 2; ++i) acc[e][i] += (f32x2){r[2 * i], r[2 * i + 1]};
                }
            }
        }
    }
    // the range's partial sums, in the accumulators' own order [wave][e][i][lane] (every store
    // of a wave is 64 consecutive floats; px_reduce_kernel maps them to columns): f32, exactly
    // the accumulators.  Measured with float64 partials by (fit, column), 8-byte stores 16 KB
    // apart: 0.21 ms per call at 6 fits, against an LDS floor of 0.012 ms
    {
        const int ngrp = gridDim.y;
        float* out = part + ((((int64_t)range * ngrp + grp) * 4 + w) * ME) * (NI * 64) + lane;
#pragma unroll
        for (int e = 0; e < ME; ++e)
#pragma unroll
            for (int i = 0; i < NI; ++i) out[(e * NI + i) * 64] = acc[e][i / 2][i & 1];
    }
    __syncthreads();                               // LDS reused for the intercept sums
    double* red = reinterpret_cast<double*>(px_lds);
    red[tid] = accI;
    __syncthreads();
    if (tid < kPxF) {
        double I = 0.0;
        for (int k = 0; k < kPxT / kPxF; ++k) I += red[tid + kPxF * k];
        partI[((int64_t)range * gridDim.y + grp) * kPxF + tid] = I;
    }
}

// g[slots[fit]][c] = the sum over the ranges of the partials, in a fixed order: a block sums 64
// consecutive accumulators (or 64 intercepts) in four range segments, seg 0..3 added in that
// order; the last blocks zero the padding columns
template <int ME, int NI>
__global__ void __launch_bounds__(256)
px_reduce_kernel(const float* __restrict__ part, const double* __restrict__ partI, int32_t nranges,
                 int32_t ngrp, int32_t count, int32_t m, int32_t K, int32_t layout, int32_t P,
                 const int32_t* __restrict__ lagpos, const int32_t* __restrict__ slots,
                 double* __restrict__ g) {
    __shared__ double red[256];
    const int tid = threadIdx.x, lane = tid & 63, seg = tid >> 6;
    const int64_t nmain = (int64_t)ngrp * 4 * ME * NI;          // blocks of 64 accumulators
    const int64_t nint = ((int64_t)ngrp * kPxF + 63) / 64;      // blocks of 64 intercepts
    const int64_t blk = blockIdx.x;
    const int r0 = (int)((int64_t)nranges * seg / 4), r1 = (int)((int64_t)nranges * (seg + 1) / 4);
    if (blk < nmain + nint) {
        const bool main_ = blk < nmain;
        const int64_t t = main_ ? blk * 64 + lane : (blk - nmain) * 64 + lane;
        const int64_t stride = main_ ? nmain * 64 : (int64_t)ngrp * kPxF;
        const bool live = main_ || t < stride;
        double s0 = 0.0, s1 = 0.0;
        if (live) {
            int r = r0;
            if (main_) {
                for (; r + 2 <= r1; r += 2) {
                    s0 += (double)part[r * stride + t];
                    s1 += (double)part[(r + 1) * stride + t];
                }
                if (r < r1) s0 += (double)part[r * stride + t];
            } else {
                for (; r + 2 <= r1; r += 2) {
                    s0 += partI[r * stride + t];
                    s1 += partI[(r + 1) * stride + t];
                }
                if (r < r1) s0 += partI[r * stride + t];
            }
        }
        red[tid] = s0 + s1;
        __syncthreads();
        if (seg == 0 && live) {
            const double v = ((red[lane] + red[64 + lane]) + red[128 + lane]) + red[192 + lane];
            if (main_) {
                int64_t x = blk;
                const int i = (int)(x % NI); x /= NI;
                const int e = (int)(x % ME); x /= ME;
                const int w = (int)(x & 3), grp = (int)(x >> 2);
                const int fit = grp * kPxF + (lane & 15), j = (lane >> 4) + 4 * i, ae = w + 4 * e;
                if (fit < count && j < K && ae < m) {
                    const int b = lagpos[j];
                    g[(int64_t)slots[fit] * P + (layout ? ae * K + b : b * m + ae)] = v;
                }
            } else if (t < count) {
                g[(int64_t)slots[t] * P + (int64_t)m * K] = v;
            }
        }
        return;
    }
    const int pad = P - (m * K + 1);
    const int64_t len = (int64_t)count * pad;
    for (int64_t x = (blk - nmain - nint) * 256 + tid; x < len; x += (int64_t)kPxPadBlocks * 256)
        g[(int64_t)slots[x / pad] * P + (m * K + 1) + x % pad] = 0.0;
}

struct PxPlan {
    int H, me, ni;                                 // halo rows; the instantiation's tiers
    int64_t ntiles, nranges, tiles_per;
};

bool px_shape_ok(int32_t m, int32_t K, int32_t smin, int32_t smax) {
    return m >= 1 && m <= kPxMaxM && K >= 1 && K <= kPxMaxK && (int64_t)smax - smin + 1 == K;
}

// Row ranges: a function of (n, ceil(count / 32)) alone, so a fit's bits depend on the number of
// 32-fit groups only (the engine's carried-row rule assumes the same of the dense kernel)
PxPlan px_plan(int64_t n, int32_t count, int32_t K) {
    PxPlan p;
    p.ni = K <= 8 ? 2 : 10;
    p.me = 0;
    p.H = (4 * p.ni + 7) / 8 * 8;
    p.ntiles = (n + p.H + kPxU - 1) / kPxU;
    const int64_t g32 = ((int64_t)count + 31) / 32;
    int64_t nr = kPxWgTarget / (2 * g32);
    if (nr > p.ntiles) nr = p.ntiles;
    if (nr < 1) nr = 1;
    p.tiles_per = (p.ntiles + nr - 1) / nr;
    p.nranges = (p.ntiles + p.tiles_per - 1) / p.tiles_per;
    return p;
}

size_t px_work_bytes(int64_t n, int32_t count, int32_t K, int32_t P) {
    size_t mx = 0;                                 // any call with at most `count` fits
    for (int32_t b = 1; b <= count; ++b) {
        const PxPlan pl = px_plan(n, b, K);
        const size_t wbytes = (size_t)pl.nranges * ((b + kPxF - 1) / kPxF) * px_group_bytes(pl.ni);
        mx = wbytes > mx ? wbytes : mx;
    }
    return mx;
}

template <int ME, int NI>
int px_launch(const PxArgs& a, const PxPlan& pl, const uint16_t* Rp, int64_t plane, int32_t count,
              void* work, size_t lds, const int32_t* slots, double* G, hipStream_t s) {
    auto* kern = &lag_xtr_packed_kernel<ME, NI, (NI > 2 ? 2 : 4)>;
    static bool attr = false;                      // > 64 KB of dynamic LDS (gfx950: 160 KB)
    if (!attr) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                kPxF * (kPxU + 40) * 4 * 2) != hipSuccess) {
            set_error("lag_xtr_packed_kernel: dynamic LDS refused");
            return SGLM_EHIP;
        }
        attr = true;
    }
    const int ngrp = (count + kPxF - 1) / kPxF;
    float* part = reinterpret_cast<float*>(work);
    double* partI = reinterpret_cast<double*>(
        reinterpret_cast<char*>(work) + (size_t)pl.nranges * ngrp * 4 * ME * NI * 64 * sizeof(float));
    dim3 grid((unsigned)pl.nranges, (unsigned)ngrp);
    kern<<<grid, kPxT, lds, s>>>(a, Rp, plane, count, part, partI);
    int st = check_launch("lag_xtr_packed_kernel");
    if (st) return st;
    const int64_t blocks = (int64_t)ngrp * 4 * ME * NI + ((int64_t)ngrp * kPxF + 63) / 64 +
                           (a.P > a.m * a.K + 1 ? kPxPadBlocks : 0);
    px_reduce_kernel<ME, NI><<<(unsigned)blocks, 256, 0, s>>>(
        part, partI, (int32_t)pl.nranges, ngrp, count, a.m, a.K, a.layout, a.P, a.lagpos, slots, G);
    return check_launch("px_reduce_kernel");
}

}  // namespace
}  // namespace sglm

extern "C" int32_t sglm_lag_xtr_packed_ok(int32_t m, int32_t K, int32_t smin, int32_t smax) {
    return px_shape_ok(m, K, smin, smax) ? 1 : 0;
}

extern "C" int sglm_lag_xtr_plan(int64_t n, int32_t count, int32_t K, int32_t P, int64_t* out) {
    if (!out || n <= 0 || count < 1 || K < 1 || K > kPxMaxK || P < 1 ||
        n > ((int64_t)1 << 31) - 4 * kPxU) {
        set_error("sglm_lag_xtr_plan: bad args (n=%lld, count=%d, K=%d <= %d)", (long long)n,
                  count, K, kPxMaxK);
        return SGLM_EINVAL;
    }
    const PxPlan pl = px_plan(n, count, K);
    out[0] = kPxU;
    out[1] = pl.H;
    out[2] = pl.ntiles;
    out[3] = pl.nranges;
    out[4] = pl.tiles_per;
    out[5] = (int64_t)px_work_bytes(n, count, K, P);
    out[6] = (int64_t)px_group_bytes(pl.ni);
    return SGLM_OK;
}

extern "C" int sglm_lag_xtr_packed_bp(const int32_t* occ, int32_t nocc, const int32_t* toff,
                                      const int32_t* lagpos, int32_t m, int32_t K, int32_t smin,
                                      int32_t smax, int32_t layout, int64_t row0, int64_t n,
                                      int64_t ld, int32_t P, const void* Rp, int32_t B,
                                      int32_t Bp, const int32_t* slots, double* G, void* work,
                                      int32_t wg_per_cu, sglm_stream_t stream) {
    if (B <= 0) return SGLM_OK;
    if (!px_shape_ok(m, K, smin, smax)) {
        set_error("sglm_lag_xtr_packed_bp: shape not covered (m=%d <= %d, K=%d <= %d, shifts "
                  "%d..%d contiguous)", m, kPxMaxM, K, kPxMaxK, smin, smax);
        return SGLM_EINVAL;
    }
    if (!occ || !toff || !lagpos || !Rp || !slots || !G || !work || nocc < 0 || n <= 0 ||
        n > ld || ld % 8 || (int64_t)m * K + 1 > P || Bp < B ||
        n > ((int64_t)1 << 31) - 4 * kPxU || row0 - smin > ((int64_t)1 << 30) ||
        smin - row0 > ((int64_t)1 << 30)) {
        set_error("sglm_lag_xtr_packed_bp: bad args");
        return SGLM_EINVAL;
    }
    const PxPlan pl = px_plan(n, B, K);
    PxArgs a;
    a.occ = occ; a.toff = toff; a.lagpos = lagpos; a.nocc = nocc;
    a.m = m; a.K = K; a.layout = layout; a.P = P; a.H = pl.H;
    a.voff = (int32_t)(smin - row0);
    a.ntiles = (int32_t)pl.ntiles; a.tiles_per = (int32_t)pl.tiles_per;
    a.n = n; a.ld = ld;
    hipStream_t s = as_stream(stream);
    // one workgroup per CU on request (beside a factorisation chain): LDS padded past half a CU's
    size_t lds = (size_t)kPxF * (kPxU + pl.H) * sizeof(float);
    if (wg_per_cu == 1) lds = (size_t)kPxF * (kPxU + 40) * sizeof(float) * 2;
    const uint16_t* rp = reinterpret_cast<const uint16_t*>(Rp);
    const int64_t plane = (int64_t)Bp * ld;
    const int me = (m + 3) / 4;
    if (pl.ni == 2)
        return me <= 4 ? px_launch<4, 2>(a, pl, rp, plane, B, work, lds, slots, G, s)
                       : px_launch<16, 2>(a, pl, rp, plane, B, work, lds, slots, G, s);
    return me <= 4    ? px_launch<4, 10>(a, pl, rp, plane, B, work, lds, slots, G, s)
           : me <= 13 ? px_launch<13, 10>(a, pl, rp, plane, B, work, lds, slots, G, s)
                      : px_launch<16, 10>(a, pl, rp, plane, B, work, lds, slots, G, s);
}
