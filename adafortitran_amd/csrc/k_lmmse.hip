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
// The multi-slot form (lmmse_seq_kernel, aft_lmmse_seq_f32) is the same body over a WINDOW of slots: target frame (seq, k, m) of a
// batch of K-slot sequences of groups of G frames reads the pilots of member m in the w = min(W, k - h + 1) slots that end at slot
// k - h, side by side along time (P is [Ps, w Pt]; step 2 gathers them from the w source frames), and the Doppler tables are those of
// w: `Pt` becomes `w Pt` in steps 2 to 4, nothing else changes.  A frame with no slot to look at (k < h) skips steps 1 to 3 and runs
// step 4 over zero terms: +0 everywhere through the same stores, nothing read.  LDS: two [64][32] complex tiles and the time tile,
// 40 KB, static; a second instantiation with [64][16] tiles (24 KB, this file's other kernel's) takes the windows that fit it.
//
// The full-grid smoother (lmmse_grid_kernel, aft_lmmse_grid_f32) is the same estimator with every grid position an observation: its own
// first product, S-deep, is described where it stands below; from Y1 on it runs lmmse_tail, the code of steps 3 and 4 of the two
// kernels above, with (Ps, Pt) = (Kf, T).
//
// No atomics, every output element written exactly once.  The rounding behind tests/test_lmmse_gpu.py's bound: every product stage is a
// chain of fused multiply-adds in sequence, the table entries are float32 roundings of the host's double tables.
#include "frame_device.h"

namespace aft {
namespace {

constexpr int kLmMaxPs = AFT_CHANSIM_MAX_PILOT_SCS, kLmMaxPt = AFT_CHANSIM_MAX_PILOT_SYMBOLS, kLmMaxPw = AFT_LMMSE_MAX_WINDOW_PILOTS;

struct LmmseArgs {
    aft_lmmse c;
    const float *tables;
    const float2 *pilots;
    const float *snr, *ds, *dop;
    float2 *est;
    unsigned long long fblock, tblock;      // floats per delay-spread block / per Doppler block of the image
    int wide;                               // 1: 16-byte stores into est
    static constexpr bool kSeq = false;
    [[maybe_unused]] static constexpr int kMaxPw = kLmMaxPt; // the widest pilot matrix a frame filters
};

template <int kPw>                          // the widest window, in pilot symbols, this instantiation's LDS holds
struct LmmseSeqArgs : LmmseArgs {
    int group, slots, window, horizon;      // G, K, W, h; tblock is a Doppler's W sub-blocks
    static constexpr bool kSeq = true;
    [[maybe_unused]] static constexpr int kMaxPw = kPw;
};

// floats of a Doppler's sub-blocks 1 .. w - 1, each v Pt (v Pt + T + 1) floats: where sub-block w starts inside the Doppler's block
__host__ __device__ inline unsigned long long lmmse_wblock_offset(unsigned long long Pt, unsigned long long T, unsigned long long w) {
    const unsigned long long m = w - 1;
    return Pt * Pt * (m * (m + 1) * (2 * m + 1) / 6) + Pt * (T + 1) * (m * (m + 1) / 2);
}

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

// Steps 3 (from Y1 on) and 4, shared by every kernel of this file: y1 is [K][Pt] in LDS and the caller has synchronised after writing
// it; C = D o (Y1 U_t) goes to pc, then per time tile V = C T'^T to v and est = F' V to the frame's plane at `est`.  K eigen-directions
// along frequency (lf [K], fp [K][S] k-major), Pt along time (ut [Pt][Pt], tp [Pt][T] l-major, lt [Pt]); Pk = K, or 0 for a frame with
// nothing to look at (the last product then runs over zero terms).
__device__ __forceinline__ void lmmse_tail(int tid, int S, int T, int K, int Pt, int Pk, const float *ut, const float *tp, const float *lt,
                                           const float *lf, const float2 *fp, float sigma2, float2 *pc, const float2 *y1,
                                           float2 (*v)[kFrameTile], float2 *est, int wide) {
    for (int i = tid; i < K * Pt; i += kFrameThreads) {                             // C[k][l] = D[k][l] sum_j y1[k][j] U_t[j][l]
        const int k = i / Pt, l = i - k * Pt;
        float re = 0.f, im = 0.f;
        for (int j = 0; j < Pt; ++j) {
            AFT_DEV_ASSERT(k * Pt + j < K * Pt && j * Pt + l < Pt * Pt);
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
        for (int i = tid; i < K * kFrameTile; i += kFrameThreads) {     // v[k][tt] = sum_l C[k][l] T'[t0 + tt][l]
            const int k = i / kFrameTile, tt = i - k * kFrameTile, t = t0 + tt;
            float re = 0.f, im = 0.f;
            if (t < T)
                for (int l = 0; l < Pt; ++l) {
                    AFT_DEV_ASSERT(k < K && (size_t)l * T + t < (size_t)Pt * T);
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
            for (int k = 0; k < Pk; ++k) {
                AFT_DEV_ASSERT(s < S && col + kFrameCols <= kFrameTile);
                const float2 f = fp[(size_t)k * S + s];
#pragma unroll
                for (int j = 0; j < kFrameCols; ++j) cfma(acc[j], f, v[k][col + j]);
            }
            const int n = min(kFrameCols, T - t0 - col);                // valid columns; even when T is
            AFT_DEV_ASSERT(s < S && t0 + col + n <= T);
            store_row_piece(est + (size_t)s * (size_t)T + t0 + col, acc, n, wide);
        }
    }
}

// The body of both pilot kernels.  pc: the pilots, then C = D o Y; y1: U_f^H P (both [Ps][Pw], Pw <= Args::kMaxPw); v: C T'^T, one time tile.
template <class Args>
__device__ __forceinline__ void lmmse_body(const Args &a, float2 *pc, float2 *y1, float2 (*v)[kFrameTile]) {
    const aft_lmmse &c = a.c;
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int S = c.num_scs, T = c.num_symbols, Ps = c.pilot_scs;
    int w = 1;                                                                       // slots in the frame's window; 0: none, est = 0
    size_t first = b;                                                                // the oldest source frame
    int hop = 0;                                                                     // frames from one source to the next
    if constexpr (Args::kSeq) {
        const int unit = a.slots * a.group;
        const size_t seq = b / (size_t)unit;
        const int r = (int)(b - seq * (size_t)unit), k = r / a.group, m = r - k * a.group, n = k - a.horizon + 1;
        w = n <= 0 ? 0 : min(a.window, n);
        hop = a.group;
        first = (seq * (size_t)a.slots + (size_t)max(k - a.horizon - w + 1, 0)) * (size_t)a.group + (size_t)m;
        AFT_DEV_ASSERT(k >= 0 && k < a.slots && w <= a.window && (w == 0 || k - a.horizon - w + 1 >= 0));
    }
    const bool live = w > 0;
    const int Pt = c.pilot_symbols * w;                                              // the window's pilot symbols, w Pt
    const int Pk = live ? Ps : 0;                                                    // terms of the last product: none without a window
    const int i_snr = !live ? 0 : c.fixed_snr >= 0 ? c.fixed_snr : nearest(c.snr_db, c.n_snr, a.snr[b]);
    const int i_ds = !live ? 0 : c.fixed_ds >= 0 ? c.fixed_ds : nearest(c.delay_spread_ns, c.n_ds, a.ds[b]);
    const int i_dop = !live ? 0 : c.fixed_dop >= 0 ? c.fixed_dop : nearest(c.doppler_hz, c.n_dop, a.dop[b]);
    AFT_DEV_ASSERT(i_snr >= 0 && i_snr < c.n_snr && i_ds >= 0 && i_ds < c.n_ds && i_dop >= 0 && i_dop < c.n_dop);
    AFT_DEV_ASSERT(Ps >= 1 && Ps <= kLmMaxPs && Pt >= 0 && Pt <= Args::kMaxPw);
    const float sigma2 = c.noise_var[i_snr];
    const float *fb = a.tables + (size_t)i_ds * a.fblock, *tb = a.tables + (size_t)c.n_ds * a.fblock + (size_t)i_dop * a.tblock;
    if constexpr (Args::kSeq) tb += lmmse_wblock_offset(c.pilot_symbols, T, live ? w : 1);
    const float2 *ufh = reinterpret_cast<const float2 *>(fb);                       // [Ps(k)][Ps(i)]
    const float2 *fp = ufh + (size_t)Ps * Ps;                                        // [Ps(k)][S]
    const float *lf = fb + 2 * ((size_t)Ps * Ps + (size_t)Ps * S);                   // [Ps]
    const float *ut = tb, *tp = tb + Pt * Pt, *lt = tp + (size_t)Pt * T;             // [Pt(j)][Pt(l)], [Pt(l)][T], [Pt]

    for (int i = tid; i < Ps * Pt; i += kFrameThreads) {
        if constexpr (Args::kSeq) {                                                  // column q of row r: symbol j of the window's slot q / Pt
            const int p1 = c.pilot_symbols, r = i / Pt, q = i - r * Pt, sl = q / p1, j = q - sl * p1;
            AFT_DEV_ASSERT(sl < w && r < Ps);
            pc[i] = a.pilots[(first + (size_t)sl * (size_t)hop) * (size_t)(Ps * p1) + (size_t)(r * p1 + j)];
        } else {
            pc[i] = a.pilots[b * (size_t)(Ps * Pt) + i];
        }
    }
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
    lmmse_tail(tid, S, T, Ps, Pt, Pk, ut, tp, lt, lf, fp, sigma2, pc, y1, v, a.est + b * (size_t)S * (size_t)T, a.wide);
}

__global__ __launch_bounds__(kFrameThreads) void lmmse_kernel(const LmmseArgs a) {
    __shared__ float2 pc[kLmMaxPs * kLmMaxPt];
    __shared__ float2 y1[kLmMaxPs * kLmMaxPt];
    __shared__ float2 v[kLmMaxPs][kFrameTile];
    lmmse_body(a, pc, y1, v);
}

// kPw = 32: 40 KB of LDS, any window; kPw = 16: the single-slot kernel's 24 KB, for windows of at most 16 pilot symbols (two more
// workgroups per CU).  The same body: a frame's bits do not depend on which of the two ran.
template <int kPw>
__global__ __launch_bounds__(kFrameThreads) void lmmse_seq_kernel(const LmmseSeqArgs<kPw> a) {
    __shared__ float2 pc[kLmMaxPs * kPw];
    __shared__ float2 y1[kLmMaxPs * kPw];
    __shared__ float2 v[kLmMaxPs][kFrameTile];
    lmmse_body(a, pc, y1, v);
}

// ---- the full-grid smoother (aft_lmmse_grid_f32; lmmse.py "the full-grid smoother"): every grid position is an observation ----
//
// est = F_g [ D o (U_g^H Z U_tg) ] T_g^T with Z the frame's [S, T] observations.  The new work is the first product, Y1 = U_g^H Z,
// [Kf, T] from an S-deep sum; from Y1 on it is lmmse_tail with (K, Pt) = (Kf, T), Kf <= 32 and T <= 32.
//   * Z is read once, straight through: rows s0 .. s0 + 32 of the row-major plane are ONE contiguous run of 32 T values, so a chunk goes
//     to LDS by consecutive lanes on consecutive 8-byte addresses (whole cache lines, whatever T is); the time tiles of frame_device.h
//     would cut every row into 128-byte pieces instead, and are kept for the stores, whose rows a thread owns.
//   * U_g^H is stored s-major, [S(s)][Kf(k)], so the same 32 rows of it are one contiguous run too and stage the same way; every
//     frame of a delay spread reads the same table, which therefore stays in L2 while Z streams from memory.
//   * a thread owns up to four of the Kf T <= 1024 outputs (i = tid + 256 n, k = i / T, j = i % T) and keeps them in registers over the
//     chunks: per term one LDS read of U_g^H[s][k] (the lanes of a wave share k for T lanes in a row: a broadcast) and one of Z[s][j]
//     (consecutive lanes, consecutive addresses), four fused multiply-adds, in increasing s from +0 -- the chain of lmmse_body's Y1.
// Any S: LDS holds one chunk.  28 KB of static LDS.  No atomics, every output element written exactly once.
constexpr int kGridMaxK = AFT_CHANSIM_MAX_TAPS, kGridMaxT = kLmMaxPw, kGridRows = 32, kGridOut = kGridMaxK * kGridMaxT / kFrameThreads;
static_assert(kGridMaxK <= kLmMaxPs && kGridRows * kGridMaxT <= kGridMaxK * kGridMaxT, "a chunk of Z fits the tile that later holds C");

struct LmmseGridArgs {
    aft_lmmse c;
    const float *tables;
    const float2 *z;
    const float *snr, *ds, *dop;
    float2 *est;
    unsigned long long gblock, tblock;      // floats per delay-spread block / per Doppler block of the grid image
    int kf;                                 // eigen-directions kept along frequency
    int wide;                               // 1: 16-byte stores into est
};

__global__ __launch_bounds__(kFrameThreads) void lmmse_grid_kernel(const LmmseGridArgs a) {
    __shared__ float2 pc[kGridMaxK * kGridMaxT];                // a chunk of Z, [rows][T]; then C
    __shared__ float2 y1[kGridMaxK * kGridMaxT];
    __shared__ float2 uc[kGridRows * kGridMaxK];                // the chunk's rows of U_g^H, [rows][Kf]
    __shared__ float2 v[kGridMaxK][kFrameTile];
    const aft_lmmse &c = a.c;
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int S = c.num_scs, T = c.num_symbols, Kf = a.kf;
    AFT_DEV_ASSERT(Kf >= 1 && Kf <= kGridMaxK && Kf <= S && T >= 1 && T <= kGridMaxT);
    const int i_snr = c.fixed_snr >= 0 ? c.fixed_snr : nearest(c.snr_db, c.n_snr, a.snr[b]);
    const int i_ds = c.fixed_ds >= 0 ? c.fixed_ds : nearest(c.delay_spread_ns, c.n_ds, a.ds[b]);
    const int i_dop = c.fixed_dop >= 0 ? c.fixed_dop : nearest(c.doppler_hz, c.n_dop, a.dop[b]);
    AFT_DEV_ASSERT(i_snr >= 0 && i_snr < c.n_snr && i_ds >= 0 && i_ds < c.n_ds && i_dop >= 0 && i_dop < c.n_dop);
    const float sigma2 = c.noise_var[i_snr];
    const float *gb = a.tables + (size_t)i_ds * a.gblock, *tb = a.tables + (size_t)c.n_ds * a.gblock + (size_t)i_dop * a.tblock;
    const float2 *ugh = reinterpret_cast<const float2 *>(gb);                       // [S(s)][Kf(k)]
    const float2 *fp = ugh + (size_t)S * Kf;                                         // [Kf(k)][S]
    const float *lf = gb + 4 * (size_t)S * Kf;                                       // [Kf]
    const float *ut = tb, *tp = tb + T * T, *lt = tp + T * T;                        // [T(j)][T(l)], [T(l)][T], [T]
    const float2 *zf = a.z + b * (size_t)S * (size_t)T;

    const int outs = Kf * T;
    int ko[kGridOut], jo[kGridOut];
    float re[kGridOut], im[kGridOut];
#pragma unroll
    for (int n = 0; n < kGridOut; ++n) {
        const int i = min(tid + n * kFrameThreads, outs - 1);                       // a thread without an n-th output repeats the last one
        ko[n] = i / T;
        jo[n] = i - ko[n] * T;
        re[n] = im[n] = 0.f;
    }
    for (int s0 = 0; s0 < S; s0 += kGridRows) {
        const int rows = min(kGridRows, S - s0);
        if (s0 != 0) __syncthreads();                                               // the previous chunk's readers are done
        for (int i = tid; i < rows * T; i += kFrameThreads) pc[i] = zf[(size_t)s0 * T + i];
        for (int i = tid; i < rows * Kf; i += kFrameThreads) uc[i] = ugh[(size_t)s0 * Kf + i];
        __syncthreads();
#pragma unroll
        for (int n = 0; n < kGridOut; ++n) {
            if (tid + n * kFrameThreads >= outs) continue;
            for (int q = 0; q < rows; ++q) {                                        // y1[k][j] += conj(U_g[s][k]) Z[s][j]
                AFT_DEV_ASSERT(q * Kf + ko[n] < kGridRows * kGridMaxK && q * T + jo[n] < kGridMaxK * kGridMaxT);
                const float2 u = uc[q * Kf + ko[n]], p = pc[q * T + jo[n]];
                re[n] = fmaf(u.x, p.x, fmaf(-u.y, p.y, re[n]));
                im[n] = fmaf(u.x, p.y, fmaf(u.y, p.x, im[n]));
            }
        }
    }
#pragma unroll
    for (int n = 0; n < kGridOut; ++n)
        if (tid + n * kFrameThreads < outs) y1[tid + n * kFrameThreads] = make_float2(re[n], im[n]);
    __syncthreads();                                                                // the last chunk has been read: pc is free for C
    lmmse_tail(tid, S, T, Kf, T, Kf, ut, tp, lt, lf, fp, sigma2, pc, y1, v, a.est + b * (size_t)S * (size_t)T, a.wide);
}

}  // namespace

size_t lmmse_grid_gblock_floats(const aft_lmmse &p, int kf) {
    return 4 * (size_t)p.num_scs * (size_t)kf + (size_t)kf + (size_t)(kf & 1);
}

size_t lmmse_grid_tblock_floats(const aft_lmmse &p) {
    const size_t T = (size_t)p.num_symbols;
    return 2 * T * T + T;
}

hipError_t launch_lmmse_grid(const aft_lmmse &plan, int kf, const float *tables, const float *z, const float *snr, const float *ds,
                             const float *dop, float *est, int batch, hipStream_t st) {
    LmmseGridArgs a{};
    a.c = plan;
    a.tables = tables;
    a.z = reinterpret_cast<const float2 *>(z);
    a.snr = snr; a.ds = ds; a.dop = dop;
    a.est = reinterpret_cast<float2 *>(est);
    a.gblock = lmmse_grid_gblock_floats(plan, kf);
    a.tblock = lmmse_grid_tblock_floats(plan);
    a.kf = kf;
    a.wide = wide_ok(plan.num_symbols, est);
    hipLaunchKernelGGL(lmmse_grid_kernel, dim3((unsigned)batch), dim3(kFrameThreads), 0, st, a);
    return hipGetLastError();
}

size_t lmmse_fblock_floats(const aft_lmmse &p) {
    const size_t Ps = (size_t)p.pilot_scs;
    return 2 * Ps * Ps + 2 * Ps * (size_t)p.num_scs + Ps + (Ps & 1);
}

size_t lmmse_tblock_floats(const aft_lmmse &p) {
    const size_t Pt = (size_t)p.pilot_symbols;
    return Pt * Pt + Pt * (size_t)p.num_symbols + Pt;
}

size_t lmmse_seq_tblock_floats(const aft_lmmse &p, int window) {
    return (size_t)lmmse_wblock_offset((unsigned long long)p.pilot_symbols, (unsigned long long)p.num_symbols, (unsigned long long)window + 1);
}

namespace {

template <class Args>
void fill_args(Args &a, const aft_lmmse &plan, const float *tables, const float *pilots, const float *snr, const float *ds,
               const float *dop, float *est) {
    a.c = plan;
    a.tables = tables;
    a.pilots = reinterpret_cast<const float2 *>(pilots);
    a.snr = snr; a.ds = ds; a.dop = dop;
    a.est = reinterpret_cast<float2 *>(est);
    a.fblock = lmmse_fblock_floats(plan);
    a.tblock = lmmse_tblock_floats(plan);
    a.wide = wide_ok(plan.num_symbols, est);
}

}  // namespace

hipError_t launch_lmmse(const aft_lmmse &plan, const float *tables, const float *pilots, const float *snr, const float *ds,
                        const float *dop, float *est, int batch, hipStream_t st) {
    LmmseArgs a{};
    fill_args(a, plan, tables, pilots, snr, ds, dop, est);
    hipLaunchKernelGGL(lmmse_kernel, dim3((unsigned)batch), dim3(kFrameThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_lmmse_seq(const aft_lmmse &plan, int group, int slots, int window, int horizon, const float *tables,
                            const float *pilots, const float *snr, const float *ds, const float *dop, float *est, int batch,
                            hipStream_t st) {
    auto launch = [&](auto a) {
        fill_args(a, plan, tables, pilots, snr, ds, dop, est);
        a.tblock = lmmse_seq_tblock_floats(plan, window);
        a.group = group; a.slots = slots; a.window = window; a.horizon = horizon;
        hipLaunchKernelGGL(lmmse_seq_kernel<decltype(a)::kMaxPw>, dim3((unsigned)batch), dim3(kFrameThreads), 0, st, a);
    };
    if (window * plan.pilot_symbols <= kLmMaxPt) launch(LmmseSeqArgs<kLmMaxPt>{});
    else launch(LmmseSeqArgs<kLmMaxPw>{});
    return hipGetLastError();
}

}  // namespace aft
