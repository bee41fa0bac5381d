// The link-level error count and its soft half (include/adafortitran_amd.h "link-level bit errors"; adafortitran_amd/linksim.py is the
// definition and the float64 twin).  One workgroup per frame, one launch per batch; a frame's two counts are a function of its own key, noise scale,
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
//
// The soft half (aft_link_soft_f32; the second kernel below) shares step 1 and the front of step 3 -- link_front, so both kernels see the
// same bits of c and p -- and goes on per axis with the L metrics a_k (a_k p - 2 comp) in registers, the m/2 pairs of minima, the LLRs
// scale (min1 - min0) and, per factor, softplus of the LLR against its sent bit.  The K float sums stay in registers and are reduced in
// a fixed order (shuffles, then the four waves through LDS); a thread takes the same element pairs whichever load form runs, so a
// frame's loss depends neither on the batch, nor on the run, nor on the alignment of the bases, nor on whether the LLRs are stored.
#include "link_device.h"

namespace aft {
namespace {

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

struct LinkCounts {
    int bits, symbols;
};

// one instantiation per modulation order, so the boundary loops unroll
template <int M>
__device__ __forceinline__ void link_element(const LinkArgs &a, unsigned long long kf, float sigma, unsigned q, float2 h, float2 e,
                                             LinkCounts &n) {
    constexpr int L = 1 << (M / 2);
    const LinkFront f = link_front<M>(a.d, kf, sigma, q, h, e);
    const float step = a.d2 * f.p;
    const unsigned ki = decide<L>(f.cr, step), kq = decide<L>(f.ci, step);
    const int wrong = __popc(f.gi ^ ki ^ (ki >> 1)) + __popc(f.gq ^ kq ^ (kq >> 1));
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


// ---- the soft half: max-log LLRs and the loss the achievable rate is read from (linksim.py "the soft link") ----

struct LinkSoftArgs {
    aft_link c;
    const float2 *ideal, *est;
    const unsigned long long *keys;
    const float *sigma, *scale, *factors;
    float *loss, *llr;          // llr may be NULL
    unsigned elems;             // S T - 1, as in LinkArgs
    float d;
    int n_factors;              // 1 .. kMaxFactors
    int wide;                   // 1: 16-byte loads of ideal and est
    int store;                  // bytes per store of llr: 16, 8 or 4
};

// A data element: its M LLRs into v (I-axis bits first, MSB first: the order of the sent word) and, for each factor, the sum over its
// bits of softplus(z) = max(z, 0) + log1p(exp(-|z|)) in nats, z = -(1 - 2 b) factor Lambda with b the sent bit.
template <int M>
__device__ __forceinline__ void link_soft_element(const LinkSoftArgs &a, unsigned long long kf, float sigma, float scale,
                                                  const float (&fac)[kMaxFactors], unsigned q, float2 h, float2 e, float *v,
                                                  float (&acc)[kMaxFactors]) {
#pragma clang fp contract(off)
    constexpr int half = M / 2, L = 1 << half;
    const LinkFront f = link_front<M>(a.d, kf, sigma, q, h, e);
    link_axis_llrs<L>(a.d, f.cr, f.p, scale, v);
    link_axis_llrs<L>(a.d, f.ci, f.p, scale, v + half);
    link_soft_losses<M>(v, f.gi, f.gq, fac, a.n_factors, acc);
}

// A thread takes the element pairs (2 i, 2 i + 1), i = tid, tid + 256, ..., whichever load form runs: the order of a frame's float
// sums, and so its loss, depends neither on the alignment of the bases nor on anything outside the frame.
template <int M>
__global__ __launch_bounds__(kFrameThreads) void link_soft_kernel(const LinkSoftArgs a) {
    __shared__ int psc[AFT_CHANSIM_MAX_PILOT_SCS], psym[AFT_CHANSIM_MAX_PILOT_SYMBOLS];
    __shared__ float part[kLinkWaves][kMaxFactors];
    const aft_link &c = a.c;
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int Ps = c.pilot_scs, Pt = c.pilot_symbols, nf = a.n_factors;
    const unsigned T = (unsigned)c.num_symbols, last = a.elems;
    AFT_DEV_ASSERT(Ps >= 1 && Ps <= AFT_CHANSIM_MAX_PILOT_SCS && Pt >= 1 && Pt <= AFT_CHANSIM_MAX_PILOT_SYMBOLS);
    AFT_DEV_ASSERT(nf >= 1 && nf <= kMaxFactors);
    if (tid < Ps) psc[tid] = c.pilot_sc_index[tid];
    if (tid >= kWave && tid - kWave < Pt) psym[tid - kWave] = c.pilot_symbol_index[tid - kWave];
    __syncthreads();
    const unsigned long long kf = a.keys[b];
    const float sigma = a.sigma[b], scale = a.scale[b];
    float fac[kMaxFactors], acc[kMaxFactors];
#pragma unroll
    for (int k = 0; k < kMaxFactors; ++k) {
        fac[k] = k < nf ? a.factors[k] : 0.f;
        acc[k] = 0.f;
    }
    const size_t base = b * ((size_t)last + 1);                 // the frame's first element
    const float2 *hp = a.ideal + base, *ep = a.est + base;
    float *lp = a.llr != nullptr ? a.llr + base * M : nullptr;
    auto data = [&](unsigned q) {                               // not a pilot position
        const unsigned s = q / T, t = q - s * T;
        return !(link_listed(psym, Pt, (int)t) && link_listed(psc, Ps, (int)s));
    };
    const unsigned pairs = (last >> 1) + 1;                     // the last pair of an odd grid holds one element
    for (unsigned i = tid; i < pairs; i += kFrameThreads) {      // pairs <= 2^30: the index cannot wrap
        const unsigned q = 2 * i;
        const bool two = q < last;
        AFT_DEV_ASSERT(q <= last && (two || !a.wide));
        float2 h0, e0, h1 = make_float2(0.f, 0.f), e1 = h1;
        if (a.wide) {
            const f32x4 h = *reinterpret_cast<const f32x4 *>(hp + q), e = *reinterpret_cast<const f32x4 *>(ep + q);
            h0 = make_float2(h[0], h[1]); e0 = make_float2(e[0], e[1]);
            h1 = make_float2(h[2], h[3]); e1 = make_float2(e[2], e[3]);
        } else {
            h0 = hp[q]; e0 = ep[q];
            if (two) { h1 = hp[q + 1]; e1 = ep[q + 1]; }
        }
        float v[2 * M];
#pragma unroll
        for (int j = 0; j < 2 * M; ++j) v[j] = 0.f;             // what a pilot position carries
#pragma unroll 1
        for (int s = 0; s < 2; ++s) {                           // one copy of the element's code: 52 KB at m = 8, two are 100 KB
            if ((s == 0 || two) && data(q + s)) {
                float w[M];
                link_soft_element<M>(a, kf, sigma, scale, fac, q + s, s ? h1 : h0, s ? e1 : e0, w, acc);
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    if (s) v[M + j] = w[j];
                    else v[j] = w[j];
                }
            }
        }
        if (lp != nullptr) link_store_llrs<M>(lp + (size_t)q * M, v, two ? 2 * M : M, a.store);
    }
#pragma unroll
    for (int k = 0; k < kMaxFactors; ++k)
        if (k < nf) {
#pragma unroll
            for (int o = kWave / 2; o >= 1; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
            if ((tid & (kWave - 1)) == 0) part[tid / kWave][k] = acc[k];
        }
    __syncthreads();
    if (tid < nf) {                                             // thread k the loss at factor k: the four waves in a fixed order
        float total = part[0][tid];
#pragma unroll
        for (int w = 1; w < kLinkWaves; ++w) total += part[w][tid];
        a.loss[b * (size_t)nf + tid] = total * kInvLn2;
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

hipError_t launch_link_soft(const aft_link &link, const float *ideal, const float *est, const unsigned long long *keys,
                            const float *sigma, const float *scale, const float *factors, int n_factors, float *loss, float *llr,
                            int batch, hipStream_t st) {
    LinkSoftArgs a{};
    a.c = link;
    a.ideal = reinterpret_cast<const float2 *>(ideal);
    a.est = reinterpret_cast<const float2 *>(est);
    a.keys = keys; a.sigma = sigma; a.scale = scale; a.factors = factors; a.loss = loss; a.llr = llr;
    a.n_factors = n_factors;
    const unsigned long long elems = (unsigned long long)link.num_scs * (unsigned long long)link.num_symbols;
    a.elems = (unsigned)(elems - 1);
    const int m = link.bits_per_symbol, L = 1 << (m / 2);
    a.d = (float)sqrt(3.0 / (2.0 * ((double)L * L - 1.0)));
    a.wide = wide_ok(link.num_symbols, ideal, est);
    a.store = link_llr_store_bytes(llr, m, elems);
    const dim3 grid((unsigned)batch), block(kFrameThreads);
    switch (m) {
        case 2: hipLaunchKernelGGL(link_soft_kernel<2>, grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL(link_soft_kernel<4>, grid, block, 0, st, a); break;
        case 6: hipLaunchKernelGGL(link_soft_kernel<6>, grid, block, 0, st, a); break;
        case 8: hipLaunchKernelGGL(link_soft_kernel<8>, grid, block, 0, st, a); break;
        default: return hipErrorInvalidValue;           // aft_link_soft_f32 has refused it
    }
    return hipGetLastError();
}

}  // namespace aft
