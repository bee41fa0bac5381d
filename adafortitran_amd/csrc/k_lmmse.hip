// The LMMSE (Wiener) baseline estimator (include/adafortitran_amd.h "the LMMSE (Wiener) baseline estimator"; adafortitran_amd/lmmse.py
// is the definition and the float64 twin).  One workgroup per frame, one launch per batch; a frame's estimate is a function of its own
// pilots and conditions only.
//
//   1. every thread picks the frame's three table indices (a wave-uniform scan of at most 16 values each, in double so that the host
//      picks the same index; no hand-over needed);
//   2. the frame's Ps x Pt pilots go to LDS;
//   3. Y = U_f^H P U_t as two small products through LDS (one thread per output element), then C = D o Y with
//      D[k][l] = 1 / (lf[k] lt[l] + noise_var);
//   4. per time tile of 16 symbols: V = C T'^T goes to LDS (one thread per (k, t)); then a thread takes one subcarrier and 8 of the
//      tile's columns and accumulates F'[s][k] V[k][col ..] over k.  F' is stored k-major, so consecutive lanes read consecutive
//      subcarriers (one coalesced 8-byte load per lane and k); V[k][col] is read by every lane of the wave from the same LDS address (a
//      broadcast: no bank conflicts).  A thread's 8 results are 64 contiguous bytes of the row-major [S, T] plane and leave as four
//      16-byte stores (T even, base 16-byte aligned; 8-byte stores otherwise) -- the row-tile pass of frame_device.h, shared with
//      the simulator, which is what lets T be anything: LDS holds one tile whatever the grid's length.
//
// No atomics, every output element written exactly once.  The rounding behind tests/test_lmmse_gpu.py's bound: every product stage is a
// chain of fused multiply-adds in sequence, the table entries are float32 roundings of the host's double tables.
#include "frame_device.h"

namespace aft {
namespace {

constexpr int kLmMaxPs = AFT_CHANSIM_MAX_PILOT_SCS, kLmMaxPt = AFT_CHANSIM_MAX_PILOT_SYMBOLS;

struct LmmseArgs {
    aft_lmmse c;
    const float *tables;
    const float2 *pilots;
    const float *snr, *ds, *dop;
    float2 *est;
    unsigned long long fblock, tblock;      // floats per delay-spread block / per Doppler block of the image
    int wide;                               // 1: 16-byte stores into est
};

// index of the value nearest to v: |v - value[i]| in double (exact for two floats of like size), ties to the lower index, NaN -> 0
__device__ __forceinline__ int nearest(const float *value, int n, float v) {
    int best = 0;
    double bd = fabs((double)v - (double)value[0]);
    for (int i = 1; i < n; ++i) {
        const double d = fabs((double)v - (double)value[i]);
        if (d < bd) { bd = d; best = i; }
    }
    return best;
}

__global__ __launch_bounds__(kFrameThreads) void lmmse_kernel(const LmmseArgs a) {
    __shared__ float2 pc[kLmMaxPs * kLmMaxPt];       // the pilots, then C = D o Y
    __shared__ float2 y1[kLmMaxPs * kLmMaxPt];       // U_f^H P
    __shared__ float2 v[kLmMaxPs][kFrameTile];       // C T'^T, one time tile
    const aft_lmmse &c = a.c;
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int S = c.num_scs, T = c.num_symbols, Ps = c.pilot_scs, Pt = c.pilot_symbols;
    const int i_snr = c.fixed_snr >= 0 ? c.fixed_snr : nearest(c.snr_db, c.n_snr, a.snr[b]);
    const int i_ds = c.fixed_ds >= 0 ? c.fixed_ds : nearest(c.delay_spread_ns, c.n_ds, a.ds[b]);
    const int i_dop = c.fixed_dop >= 0 ? c.fixed_dop : nearest(c.doppler_hz, c.n_dop, a.dop[b]);
    AFT_DEV_ASSERT(i_snr >= 0 && i_snr < c.n_snr && i_ds >= 0 && i_ds < c.n_ds && i_dop >= 0 && i_dop < c.n_dop);
    AFT_DEV_ASSERT(Ps >= 1 && Ps <= kLmMaxPs && Pt >= 1 && Pt <= kLmMaxPt);
    const float sigma2 = c.noise_var[i_snr];
    const float *fb = a.tables + (size_t)i_ds * a.fblock, *tb = a.tables + (size_t)c.n_ds * a.fblock + (size_t)i_dop * a.tblock;
    const float2 *ufh = reinterpret_cast<const float2 *>(fb);                       // [Ps(k)][Ps(i)]
    const float2 *fp = ufh + (size_t)Ps * Ps;                                        // [Ps(k)][S]
    const float *lf = fb + 2 * ((size_t)Ps * Ps + (size_t)Ps * S);                   // [Ps]
    const float *ut = tb, *tp = tb + Pt * Pt, *lt = tp + (size_t)Pt * T;             // [Pt(j)][Pt(l)], [Pt(l)][T], [Pt]

    for (int i = tid; i < Ps * Pt; i += kFrameThreads) pc[i] = a.pilots[b * (size_t)(Ps * Pt) + i];
    __syncthreads();
    for (int i = tid; i < Ps * Pt; i += kFrameThreads) {                            // y1[k][j] = sum_i conj(U_f[i][k]) P[i][j]
        const int k = i / Pt, j = i - k * Pt;
        float re = 0.f, im = 0.f;
        for (int q = 0; q < Ps; ++q) {
            AFT_DEV_ASSERT(k * Ps + q < Ps * Ps && q * Pt + j < Ps * Pt);
            const float2 u = ufh[k * Ps + q], p = pc[q * Pt + j];
            re = fmaf(u.x, p.x, fmaf(-u.y, p.y, re));
            im = fmaf(u.x, p.y, fmaf(u.y, p.x, im));
        }
        y1[i] = make_float2(re, im);
    }
    __syncthreads();                                                                // the pilots have been read: pc is free for C
    for (int i = tid; i < Ps * Pt; i += kFrameThreads) {                            // C[k][l] = D[k][l] sum_j y1[k][j] U_t[j][l]
        const int k = i / Pt, l = i - k * Pt;
        float re = 0.f, im = 0.f;
        for (int j = 0; j < Pt; ++j) {
            AFT_DEV_ASSERT(k * Pt + j < Ps * Pt && j * Pt + l < Pt * Pt);
            const float2 y = y1[k * Pt + j];
            const float u = ut[j * Pt + l];
            re = fmaf(y.x, u, re);
            im = fmaf(y.y, u, im);
        }
        const float d = 1.f / fmaf(lf[k], lt[l], sigma2);
        pc[i] = make_float2(d * re, d * im);
    }
    __syncthreads();

    for (int t0 = 0; t0 < T; t0 += kFrameTile) {
        if (t0 != 0) __syncthreads();                                   // the previous tile's readers are done with `v`
        for (int i = tid; i < Ps * kFrameTile; i += kFrameThreads) {    // v[k][tt] = sum_l C[k][l] T'[t0 + tt][l]
            const int k = i / kFrameTile, tt = i - k * kFrameTile, t = t0 + tt;
            float re = 0.f, im = 0.f;
            if (t < T)
                for (int l = 0; l < Pt; ++l) {
                    AFT_DEV_ASSERT(k < Ps && (size_t)l * T + t < (size_t)Pt * T);
                    const float2 z = pc[k * Pt + l];
                    const float w = tp[(size_t)l * T + t];
                    re = fmaf(z.x, w, re);
                    im = fmaf(z.y, w, im);
                }
            v[k][tt] = make_float2(re, im);
        }
        __syncthreads();

        const int groups = (min(T - t0, kFrameTile) + kFrameCols - 1) / kFrameCols;
        for (int i = tid; i < S * groups; i += kFrameThreads) {
            const int hg = i / S, s = i - hg * S, col = kFrameCols * hg;
            float2 acc[kFrameCols];
#pragma unroll
            for (int j = 0; j < kFrameCols; ++j) acc[j] = make_float2(0.f, 0.f);
            for (int k = 0; k < Ps; ++k) {
                AFT_DEV_ASSERT(s < S && col + kFrameCols <= kFrameTile);
                const float2 f = fp[(size_t)k * S + s];
#pragma unroll
                for (int j = 0; j < kFrameCols; ++j) cfma(acc[j], f, v[k][col + j]);
            }
            const int n = min(kFrameCols, T - t0 - col);                // valid columns; even when T is
            AFT_DEV_ASSERT(s < S && t0 + col + n <= T);
            store_row_piece(a.est + (b * S + s) * (size_t)T + t0 + col, acc, n, a.wide);
        }
    }
}

}  // namespace

size_t lmmse_fblock_floats(const aft_lmmse &p) {
    const size_t Ps = (size_t)p.pilot_scs;
    return 2 * Ps * Ps + 2 * Ps * (size_t)p.num_scs + Ps + (Ps & 1);
}

size_t lmmse_tblock_floats(const aft_lmmse &p) {
    const size_t Pt = (size_t)p.pilot_symbols;
    return Pt * Pt + Pt * (size_t)p.num_symbols + Pt;
}

hipError_t launch_lmmse(const aft_lmmse &plan, const float *tables, const float *pilots, const float *snr, const float *ds,
                        const float *dop, float *est, int batch, hipStream_t st) {
    LmmseArgs a{};
    a.c = plan;
    a.tables = tables;
    a.pilots = reinterpret_cast<const float2 *>(pilots);
    a.snr = snr; a.ds = ds; a.dop = dop;
    a.est = reinterpret_cast<float2 *>(est);
    a.fblock = lmmse_fblock_floats(plan);
    a.tblock = lmmse_tblock_floats(plan);
    a.wide = wide_ok(plan.num_symbols, est);
    hipLaunchKernelGGL(lmmse_kernel, dim3((unsigned)batch), dim3(kFrameThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace aft
