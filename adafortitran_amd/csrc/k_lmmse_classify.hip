// Blind LMMSE: the design point of a window from its pilots (include/adafortitran_amd.h "choosing the design point from the pilots";
// adafortitran_amd/lmmse.py is the definition, lmmse_classify_host the float64 twin).  One workgroup per UNIT -- a group of G frames
// when pooling, a frame otherwise -- one launch per batch.  Candidate c = (s, d, e) = (i_snr, i_ds, i_dop):
//
//     score(c) = -( m logdet[d][e][w][s] + sum_kl E_kl / (lf[d]_k lt^(w)[e]_l + noise_var[s]) ),   E_kl = sum_members |Z_kl|^2,
//     Z = U_f[d]^H P U_t^(w)[e],   P the member's [Ps, w Pt] window (k_lmmse.hip's, gathered the same way), m the members pooled.
//
// The loop nest, outermost first: delay spread d; chunk of Dopplers; member; Doppler e of the chunk.  A chunk is as many Dopplers
// as have their E tiles ([Ps][w Pt] floats each) in the 8 KB of LDS kept for them: ALL of them while n_dop Ps w Pt <= 2048 (the
// default grids up to w Pt = 24), so that there are n_ds first products per member and n_ds n_dop second products.
//   1. the member's window goes to LDS (once per unit when the unit is one frame, once per (d, chunk, member) otherwise);
//   2. Y1 = U_f[d]^H P, one thread per element, into LDS: one first product, shared by every Doppler of the chunk;
//   3. per Doppler Z = Y1 U_t^(w)[e], one thread per (e, element): the threads split into 256 / npad groups (npad = Ps w Pt rounded
//      up to 64, 128 or 256; above 256 one group walks the elements in passes of 256), group g takes the chunk's Dopplers g,
//      g + groups, ...; |Z|^2 is added to E[e][k][l] in LDS by the one thread that owns the element in steps 3 and 4: the sum over
//      members comes before any division;
//   4. after the last member, per Doppler step: a thread divides its E by V for every SNR (one division per candidate and element,
//      whatever m), adds its elements in increasing index, the wave adds its lanes by shuffles (offsets 32, 16, .. 1), lane 0 writes
//      LDS, and after a barrier thread (g, s) adds the waves of its Doppler in increasing wave, forms the score with one fused
//      multiply-add, writes it (scores != NULL) and keeps its best (strictly greater wins: its candidates come in increasing index);
//   5. thread 0 scans the at most 64 kept (score, index) pairs in LDS in a fixed order: greater wins, equal goes to the lower flat
//      index, a NaN never wins; it writes idx and the three table values for every member of the unit.
// A unit with no slot to look at (k < horizon), or a plan that pins all three conditions, reads nothing: the choice is the pinned
// index or 0, competing scores are +0.  A candidate a pin excludes has score -inf.  No atomics; every output element is written once.
//
// LDS, static: two [64][kPw] complex tiles and the 8 KB of E tiles: 40 KB at kPw = 32, 24 KB at kPw = 16 (k_lmmse.hip's figures).
// The per-wave sums (2 x 4 x 16 floats, double-buffered so a step needs one barrier) and the kept pairs lie over Y1, which is dead in
// steps 4 and 5.  A unit's bits depend on its window's pilots only: the element a thread owns, the order of every sum and the tables do
// not depend on batch, position or kPw (nor does the chunk: the E tiles are 8 KB in both instantiations).
#include "frame_device.h"

namespace aft {
namespace {

constexpr int kClMaxPs = AFT_CHANSIM_MAX_PILOT_SCS, kClMaxPt = AFT_CHANSIM_MAX_PILOT_SYMBOLS, kClMaxPw = AFT_LMMSE_MAX_WINDOW_PILOTS;
constexpr int kClValues = AFT_CHANSIM_MAX_VALUES, kClWaves = kFrameThreads / 64, kClKept = kClWaves * kClValues;
constexpr int kClEnergy = 2048;            // floats of E tiles in LDS: one tile at the largest Ps w Pt

struct ClassifyArgs {
    aft_lmmse c;
    const float *tables, *logdet;
    const float2 *pilots;
    int32_t *idx;
    float *snr, *ds, *dop, *scores;          // scores may be NULL
    unsigned long long fblock, tblock;       // floats per delay-spread block / per Doppler block (its W sub-blocks) of the image
    int group, slots, window, horizon, pool;
};

// floats of a Doppler's sub-blocks 1 .. w - 1 (k_lmmse.hip's lmmse_wblock_offset: the layout of the sequence image)
__device__ __forceinline__ unsigned long long classify_wblock_offset(unsigned long long Pt, unsigned long long T, unsigned long long w) {
    const unsigned long long m = w - 1;
    return Pt * Pt * (m * (m + 1) * (2 * m + 1) / 6) + Pt * (T + 1) * (m * (m + 1) / 2);
}

template <int kPw>                           // the widest window, in pilot symbols, this instantiation's LDS holds
__global__ __launch_bounds__(kFrameThreads) void lmmse_classify_kernel(const ClassifyArgs a) {
    __shared__ float2 pc[kClMaxPs * kPw];
    __shared__ float2 y1[kClMaxPs * kPw];
    __shared__ float en[kClEnergy];
    static_assert(sizeof(float2) * kClMaxPs * kPw >= sizeof(float) * (2 * kClKept + kClKept) + sizeof(int) * kClKept, "the sums lie over y1");
    float (*red)[kClWaves][kClValues] = reinterpret_cast<float (*)[kClWaves][kClValues]>(y1);   // [2][waves][values], steps 4 and 5 only
    float *kept_score = reinterpret_cast<float *>(y1) + 2 * kClKept;
    int *kept_index = reinterpret_cast<int *>(kept_score + kClKept);
    const aft_lmmse &c = a.c;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t u = blockIdx.x;
    const int G = a.group, K = a.slots, Ps = c.pilot_scs, p1 = c.pilot_symbols, T = c.num_symbols;
    const int n_snr = c.n_snr, n_ds = c.n_ds, n_dop = c.n_dop, ncand = n_snr * n_ds * n_dop;

    size_t seq;
    int k, a0, m;                                                                    // slot, first member, members pooled
    if (a.pool) {
        seq = u / (size_t)K;
        k = (int)(u - seq * (size_t)K);
        a0 = 0;
        m = G;
    } else {
        const int unit = K * G;
        seq = u / (size_t)unit;
        const int r = (int)(u - seq * (size_t)unit);
        k = r / G;
        a0 = r - k * G;
        m = 1;
    }
    const int nlook = k - a.horizon + 1, w = nlook <= 0 ? 0 : min(a.window, nlook);
    const size_t frame0 = (seq * (size_t)K + (size_t)k) * (size_t)G + (size_t)a0;    // the first frame this unit decides for
    const size_t first = (seq * (size_t)K + (size_t)max(k - a.horizon - w + 1, 0)) * (size_t)G + (size_t)a0;   // its oldest source
    const int Pt = p1 * w, np = Ps * Pt;
    AFT_DEV_ASSERT(k >= 0 && k < K && w <= a.window && Ps >= 1 && Ps <= kClMaxPs && Pt <= kPw && np <= kClEnergy);
    const int s0 = max(c.fixed_snr, 0), d0 = max(c.fixed_ds, 0), e0 = max(c.fixed_dop, 0);     // the lowest competing index
    const bool computed = w > 0 && min(min(c.fixed_snr, c.fixed_ds), c.fixed_dop) < 0;
    float *scores = a.scores ? a.scores + u * (size_t)ncand : nullptr;

    if (scores)                                                                      // what no step below writes: excluded candidates
        for (int i = tid; i < ncand; i += kFrameThreads) {
            const int s = i / (n_ds * n_dop), d = (i - s * n_ds * n_dop) / n_dop, e = i - (s * n_ds + d) * n_dop;
            const bool out = (c.fixed_snr >= 0 && s != c.fixed_snr) || (c.fixed_ds >= 0 && d != c.fixed_ds) || (c.fixed_dop >= 0 && e != c.fixed_dop);
            if (out) scores[i] = -INFINITY;
            else if (!computed) scores[i] = 0.f;
        }

    int pick = (s0 * n_ds + d0) * n_dop + e0;
    if (computed) {
        const int npad = np <= 64 ? 64 : np <= 128 ? 128 : kFrameThreads, groups = kFrameThreads / npad, wpg = npad / 64;
        const int eg = tid / npad, it = tid - eg * npad;                             // Doppler group (wave-uniform), element inside it
        const int ne = c.fixed_dop >= 0 ? 1 : n_dop, chunk = min(ne, kClEnergy / np);
        const int gk = tid / kClValues, sk = tid - gk * kClValues;                   // the (group, SNR) whose score this thread keeps
        const bool keeper = gk < groups && sk < n_snr && (c.fixed_snr < 0 || sk == c.fixed_snr);
        const float *tbase = a.tables + (size_t)n_ds * a.fblock + classify_wblock_offset(p1, T, w);   // Doppler e's sub-block w: + e tblock
        float best = -INFINITY;
        int besti = pick;
        int stage = 0;
        bool loaded = false;
        for (int d = 0; d < n_ds; ++d) {
            if (c.fixed_ds >= 0 && d != c.fixed_ds) continue;
            const float *fb = a.tables + (size_t)d * a.fblock;
            const float2 *ufh = reinterpret_cast<const float2 *>(fb);                // [Ps(k)][Ps(i)]
            const float *lf = fb + 2 * ((size_t)Ps * Ps + (size_t)Ps * c.num_scs);   // [Ps]
            for (int c0 = 0; c0 < ne; c0 += chunk) {
                const int cn = min(chunk, ne - c0), steps = (cn + groups - 1) / groups;
                for (int mem = 0; mem < m; ++mem) {
                    if (!loaded || m > 1) {                                          // pc's last readers passed the barrier after step 2
                        for (int i = tid; i < np; i += kFrameThreads) {
                            const int r = i / Pt, q = i - r * Pt, sl = q / p1, j = q - sl * p1;
                            AFT_DEV_ASSERT(sl < w && r < Ps);
                            pc[i] = a.pilots[(first + (size_t)mem + (size_t)sl * (size_t)G) * (size_t)(Ps * p1) + (size_t)(r * p1 + j)];
                        }
                        loaded = true;
                    }
                    __syncthreads();                                                 // pc is whole; y1's last readers (and the sums') are done
                    for (int i = tid; i < np; i += kFrameThreads) {                  // y1[k][j] = sum_i conj(U_f[i][k]) P[i][j]
                        const int kk = i / Pt, j = i - kk * Pt;
                        float re = 0.f, im = 0.f;
                        for (int q = 0; q < Ps; ++q) {
                            AFT_DEV_ASSERT(kk * Ps + q < Ps * Ps && q * Pt + j < np);
                            const float2 uu = ufh[kk * Ps + q], p = pc[q * Pt + j];
                            re = fmaf(uu.x, p.x, fmaf(-uu.y, p.y, re));
                            im = fmaf(uu.x, p.y, fmaf(uu.y, p.x, im));
                        }
                        y1[i] = make_float2(re, im);
                    }
                    __syncthreads();
                    for (int je = 0; je < steps; ++je) {                             // Z = Y1 U_t^(w)[e]; E += |Z|^2
                        const int ec = eg + groups * je;
                        if (ec >= cn) break;                                         // wave-uniform; no barrier in this loop
                        const float *ut = tbase + (size_t)(c.fixed_dop >= 0 ? c.fixed_dop : c0 + ec) * a.tblock;
                        for (int i = it; i < np; i += kFrameThreads) {
                            const int kk = i / Pt, l = i - kk * Pt;
                            float re = 0.f, im = 0.f;
                            for (int q = 0; q < Pt; ++q) {
                                AFT_DEV_ASSERT(kk * Pt + q < np && q * Pt + l < Pt * Pt);
                                const float2 y = y1[kk * Pt + q];
                                const float t = ut[q * Pt + l];
                                re = fmaf(y.x, t, re);
                                im = fmaf(y.y, t, im);
                            }
                            AFT_DEV_ASSERT(ec * np + i < kClEnergy);
                            en[ec * np + i] = fmaf(re, re, fmaf(im, im, mem == 0 ? 0.f : en[ec * np + i]));   // its only reader and writer
                        }
                    }
                }
                __syncthreads();                                                     // y1 is dead: the sums may lie over it
                for (int je = 0; je < steps; ++je) {                                 // the scores of (., d, e) for this step's Dopplers
                    const int ec = eg + groups * je;
                    const bool live = ec < cn;
                    const int e = c.fixed_dop >= 0 ? c.fixed_dop : c0 + min(ec, cn - 1);
                    const float *lt = tbase + (size_t)e * a.tblock + Pt * Pt + (size_t)Pt * T;   // [w Pt]
                    float part[kClValues];
#pragma unroll
                    for (int s = 0; s < kClValues; ++s) part[s] = 0.f;
                    if (live)
                        for (int i = it; i < np; i += kFrameThreads) {
                            const int kk = i / Pt, l = i - kk * Pt;
                            const float f = lf[kk], t = lt[l], x = en[ec * np + i];
#pragma unroll
                            for (int s = 0; s < kClValues; ++s)
                                if (s < n_snr && (c.fixed_snr < 0 || s == c.fixed_snr)) part[s] += x / fmaf(f, t, c.noise_var[s]);
                        }
#pragma unroll
                    for (int s = 0; s < kClValues; ++s)
                        if (s < n_snr && (c.fixed_snr < 0 || s == c.fixed_snr)) {
                            float v = part[s];
                            for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
                            if (lane == 0) red[stage & 1][wave][s] = v;
                        }
                    __syncthreads();                                                 // one barrier per step: red is double-buffered
                    const int ek = gk + groups * je;
                    if (keeper && ek < cn) {
                        const int e2 = c.fixed_dop >= 0 ? c.fixed_dop : c0 + ek;
                        float q = red[stage & 1][gk * wpg][sk];
                        for (int v = 1; v < wpg; ++v) q += red[stage & 1][gk * wpg + v][sk];
                        const float ld = a.logdet[(((size_t)d * n_dop + e2) * (size_t)a.window + (size_t)(w - 1)) * (size_t)n_snr + sk];
                        const float score = -fmaf((float)m, ld, q);
                        const int flat = (sk * n_ds + d) * n_dop + e2;
                        AFT_DEV_ASSERT(flat < ncand);
                        if (scores) scores[flat] = score;
                        if (score > best) { best = score; besti = flat; }            // a NaN never wins; equal keeps the earlier, lower index
                    }
                    ++stage;
                }
            }
        }
        if (tid < kClKept) {                                                         // beside red, not over it: no barrier needed before
            kept_score[tid] = keeper ? best : -INFINITY;
            kept_index[tid] = keeper ? besti : pick;
        }
        __syncthreads();
        if (tid == 0) {
            float b = -INFINITY;
            for (int i = 0; i < kClKept; ++i) {
                const float sc = kept_score[i];
                const int ix = kept_index[i];
                if (sc > b || (sc == b && ix < pick)) { b = sc; pick = ix; }
            }
        }
    }
    if (tid == 0) {
        const int s = pick / (n_ds * n_dop), d = (pick - s * n_ds * n_dop) / n_dop, e = pick - (s * n_ds + d) * n_dop;
        AFT_DEV_ASSERT(s < n_snr && d < n_ds && e < n_dop);
        for (int mem = 0; mem < m; ++mem) {
            const size_t f = frame0 + (size_t)mem;
            a.idx[3 * f + 0] = s;
            a.idx[3 * f + 1] = d;
            a.idx[3 * f + 2] = e;
            a.snr[f] = c.snr_db[s];
            a.ds[f] = c.delay_spread_ns[d];
            a.dop[f] = c.doppler_hz[e];
        }
    }
}

}  // namespace

size_t lmmse_classify_table_floats(const aft_lmmse &p, int window) {
    return (size_t)p.n_ds * (size_t)p.n_dop * (size_t)window * (size_t)p.n_snr;
}

hipError_t launch_lmmse_classify(const aft_lmmse &plan, int group, int slots, int window, int horizon, int pool, const float *tables,
                                 const float *logdet, const float *pilots, int32_t *idx, float *snr, float *ds, float *dop, float *scores,
                                 int batch, hipStream_t st) {
    ClassifyArgs a{};
    a.c = plan;
    a.tables = tables; a.logdet = logdet;
    a.pilots = reinterpret_cast<const float2 *>(pilots);
    a.idx = idx; a.snr = snr; a.ds = ds; a.dop = dop; a.scores = scores;
    a.fblock = lmmse_fblock_floats(plan);
    a.tblock = lmmse_seq_tblock_floats(plan, window);
    a.group = group; a.slots = slots; a.window = window; a.horizon = horizon; a.pool = pool;
    const unsigned units = (unsigned)(pool ? batch / group : batch);
    if (window * plan.pilot_symbols <= kClMaxPt) hipLaunchKernelGGL(lmmse_classify_kernel<kClMaxPt>, dim3(units), dim3(kFrameThreads), 0, st, a);
    else hipLaunchKernelGGL(lmmse_classify_kernel<kClMaxPw>, dim3(units), dim3(kFrameThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace aft
