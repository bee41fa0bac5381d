// The link-level error count (include/adafortitran_amd.h "link-level bit errors"; adafortitran_amd/linksim.py is the definition and
// the float64 twin).  One workgroup per frame, one launch per batch; a frame's two counts are a function of its own key, noise scale,
// true channel and estimate only.
//
//   1. the pilot positions go to LDS (two sorted lists of at most 64 and 16 entries);
//   2. a thread walks grid elements q = s T + t, consecutive lanes on consecutive addresses: two elements per 16-byte load of H and of E
//      (T even -- a pair never straddles a row -- and both bases 16-byte aligned), one per 8-byte load otherwise.  An element whose
//      column and row are both in the lists is a pilot and is skipped (two binary searches; the row's only when the column hit);
//   3. per data element: three words of the counter-based hash (sent bits, noise radius, noise angle), the Gray-coded square-QAM
//      symbol, y = H x + noise (frame_device.h: the simulator's hash and Box-Muller), c = y conj(E), p = |E|^2 and, per axis, the
//      count of inner boundaries beta_b p at or below the component of c -- zero-forcing with a hard decision and without a division,
//      total at p = 0;
//   4. the two integer counts stay in registers, are summed in the wave with shuffles and across the four waves through LDS, and two
//      threads store the frame's pair, one count each.
//
// No atomics: integer sums do not depend on their order, so a frame's counts depend neither on the batch nor on the run.  The rounding
// behind tests/test_linksim_gpu.py's margin: every product is a fused multiply-add chain, the angle is formed in turns, no fast-math.
#include "frame_device.h"

namespace aft {
namespace {

constexpr int kLinkWaves = kFrameThreads / kWave;

struct LinkArgs {
    aft_link c;
    const float2 *ideal, *est;
    const unsigned long long *keys;
    const float *sigma;
    int *counts;
    unsigned elems;             // S T - 1 fits; S T itself may be 2^31
    float d, d2;                // float(sqrt(3 / (2 (L^2 - 1)))) and twice that
    int wide;                   // 1: 16-byte loads of ideal and est
};

// v in sorted[0 .. n): n <= 64
__device__ __forceinline__ bool link_listed(const int *sorted, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sorted[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && sorted[lo] == v;
}

// level index of a Gray code of at most four bits: k ^ (k >> 1) = g
__device__ __forceinline__ unsigned gray_level(unsigned g) {
    g ^= g >> 1;
    return g ^ (g >> 2);
}

// #{b in 1 .. L-1 : comp >= beta_b p}, beta_b p = (b - L/2) (2 d p): `step` is float(2 d p)
template <int L>
__device__ __forceinline__ unsigned decide(float comp, float step) {
    unsigned k = 0;
#pragma unroll
    for (int b = 1; b < L; ++b) k += comp >= (float)(b - L / 2) * step ? 1u : 0u;
    return k;
}

struct LinkCounts {
    int bits, symbols;
};

// M = bits per symbol: one instantiation per modulation order, so the boundary loops unroll
template <int M>
__device__ __forceinline__ void link_element(const LinkArgs &a, unsigned long long kf, float sigma, unsigned q, float2 h, float2 e,
                                             LinkCounts &n) {
    constexpr int half = M / 2, L = 1 << half;
    const unsigned w = (unsigned)(frame_word(kf, kStreamDataBits, q) >> (64 - M));
    const unsigned gi = w >> half, gq = w & (unsigned)(L - 1);
    const float xr = a.d * (float)(2 * (int)gray_level(gi) - (L - 1)), xi = a.d * (float)(2 * (int)gray_level(gq) - (L - 1));
    const FrameNoise nz = frame_noise(kf, kStreamDataNoiseRadius, kStreamDataNoiseAngle, q, sigma);
    const float yr = fmaf(nz.r, nz.c, fmaf(h.x, xr, -(h.y * xi)));
    const float yi = fmaf(nz.r, nz.s, fmaf(h.x, xi, h.y * xr));
    const float cr = fmaf(yr, e.x, yi * e.y);                   // y conj(E)
    const float ci = fmaf(yi, e.x, -(yr * e.y));
    const float step = a.d2 * fmaf(e.x, e.x, e.y * e.y);
    const unsigned ki = decide<L>(cr, step), kq = decide<L>(ci, step);
    const int wrong = __popc(gi ^ ki ^ (ki >> 1)) + __popc(gq ^ kq ^ (kq >> 1));
    n.bits += wrong;
    n.symbols += wrong != 0 ? 1 : 0;
}

template <int M>
__global__ __launch_bounds__(kFrameThreads) void link_errors_kernel(const LinkArgs a) {
    __shared__ int psc[AFT_CHANSIM_MAX_PILOT_SCS], psym[AFT_CHANSIM_MAX_PILOT_SYMBOLS];
    __shared__ int part[kLinkWaves][2];
    const aft_link &c = a.c;
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int Ps = c.pilot_scs, Pt = c.pilot_symbols;
    const unsigned T = (unsigned)c.num_symbols, last = a.elems;
    AFT_DEV_ASSERT(Ps >= 1 && Ps <= AFT_CHANSIM_MAX_PILOT_SCS && Pt >= 1 && Pt <= AFT_CHANSIM_MAX_PILOT_SYMBOLS);
    if (tid < Ps) psc[tid] = c.pilot_sc_index[tid];
    if (tid >= kWave && tid - kWave < Pt) psym[tid - kWave] = c.pilot_symbol_index[tid - kWave];
    __syncthreads();
    const unsigned long long kf = a.keys[b];
    const float sigma = a.sigma[b];
    const size_t base = b * ((size_t)last + 1);                 // the frame's first element
    const float2 *hp = a.ideal + base, *ep = a.est + base;
    LinkCounts n{0, 0};
    auto data = [&](unsigned q) {                               // not a pilot position
        const unsigned s = q / T, t = q - s * T;
        return !(link_listed(psym, Pt, (int)t) && link_listed(psc, Ps, (int)s));
    };
    if (a.wide) {
        const unsigned pairs = (last >> 1) + 1;                 // S T is even here
        for (unsigned i = tid; i < pairs; i += kFrameThreads) {
            const unsigned q = 2 * i;
            AFT_DEV_ASSERT(q + 1 <= last);
            const f32x4 h = *reinterpret_cast<const f32x4 *>(hp + q), e = *reinterpret_cast<const f32x4 *>(ep + q);
            if (data(q)) link_element<M>(a, kf, sigma, q, make_float2(h[0], h[1]), make_float2(e[0], e[1]), n);
            if (data(q + 1)) link_element<M>(a, kf, sigma, q + 1, make_float2(h[2], h[3]), make_float2(e[2], e[3]), n);
        }
    } else {
        for (unsigned i = tid; i <= last; i += kFrameThreads)    // last < 2^31: the index cannot wrap
            if (data(i)) link_element<M>(a, kf, sigma, i, hp[i], ep[i], n);
    }
#pragma unroll
    for (int o = kWave / 2; o >= 1; o >>= 1) {
        n.bits += __shfl_xor(n.bits, o);
        n.symbols += __shfl_xor(n.symbols, o);
    }
    if ((tid & (kWave - 1)) == 0) {
        part[tid / kWave][0] = n.bits;
        part[tid / kWave][1] = n.symbols;
    }
    __syncthreads();
    if (tid < 2) {                                              // thread 0 the bit errors, thread 1 the symbol errors
        int total = 0;
#pragma unroll
        for (int w = 0; w < kLinkWaves; ++w) total += part[w][tid];
        a.counts[2 * b + tid] = total;
    }
}

}  // namespace

hipError_t launch_link_errors(const aft_link &link, const float *ideal, const float *est, const unsigned long long *keys,
                              const float *sigma, int32_t *counts, int batch, hipStream_t st) {
    LinkArgs a{};
    a.c = link;
    a.ideal = reinterpret_cast<const float2 *>(ideal);
    a.est = reinterpret_cast<const float2 *>(est);
    a.keys = keys; a.sigma = sigma; a.counts = counts;
    const unsigned long long elems = (unsigned long long)link.num_scs * (unsigned long long)link.num_symbols;
    a.elems = (unsigned)(elems - 1);
    const int L = 1 << (link.bits_per_symbol / 2);
    a.d = (float)sqrt(3.0 / (2.0 * ((double)L * L - 1.0)));
    a.d2 = 2.f * a.d;
    a.wide = wide_ok(link.num_symbols, ideal, est);
    const dim3 grid((unsigned)batch), block(kFrameThreads);
    switch (link.bits_per_symbol) {
        case 2: hipLaunchKernelGGL(link_errors_kernel<2>, grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL(link_errors_kernel<4>, grid, block, 0, st, a); break;
        case 6: hipLaunchKernelGGL(link_errors_kernel<6>, grid, block, 0, st, a); break;
        case 8: hipLaunchKernelGGL(link_errors_kernel<8>, grid, block, 0, st, a); break;
        default: return hipErrorInvalidValue;           // aft_link_errors_f32 has refused it
    }
    return hipGetLastError();
}

}  // namespace aft
