// Two-stream spatial multiplexing on the link (include/adafortitran_amd.h "spatial multiplexing"; adafortitran_amd/linksim.py "the
// spatial-multiplexing link" is the definition and the float64 twin): linear ZF / MMSE detection of N = 2 streams on R antennas.  One
// workgroup per GROUP of 2 R consecutive frames -- frame r 2 + s is the pair (antenna r, stream s) --, one launch per batch; a group's
// counts, losses and LLRs are a function of its own keys, noise scales, weights, true channels and estimates and of its leader's LLR
// scale and regulariser only.  The walk is k_link.hip's link_walk with the combiner replaced by the detector:
//
//   1. the pilot positions go to LDS and the R keys, noise scales and weights of the frames (r, 0); the key of frame (0, 1) is the
//      second stream's;
//   2. a thread takes the element pairs (2 i, 2 i + 1), i = tid, tid + 256, ...: the same pair-to-thread map, the same load rule per
//      plane (16 bytes per pair when T is even and both bases are 16-byte aligned, 8 bytes per element otherwise; the last pair of an
//      odd grid holds one element) and the same pilot lookup;
//   3. per data element both sent words are hashed once (link_sent, from the keys of frames (0, 0) and (0, 1)).  The antenna loop, not
//      unrolled, loads the four planes H_r0, E_r0, H_r1, E_r1 of the pair, hashes the antenna's two noise words, forms
//      y_r = H_r0 x_0 + H_r1 x_1 + noise (link_sample2: stream 0's product is link_branch's chain, stream 1's products are added by
//      fused multiply-adds, the noise last) and adds the eight sums of the element (link_sm_accumulate: m_0, m_1, g00, g11, g01), one
//      fused multiply-add per term in increasing r, the sums starting at -0;
//   4. the two demappers run after it, in a stream loop around an element loop, neither unrolled: one copy of the soft code (at m = 8
//      it is about 50 KB).  Per (stream, element) the adjugate detector (link_sm_detect: c_s, p_s, eff_s = scale / a_other) and then
//      link_walk's measures on them: the hard decision against the stream's sent Gray codes, the max-log LLRs eff_s (min1 - min0)
//      and, per factor, softplus of the LLR against its sent bit.  A stream's LLRs of the pair leave by link_store_llrs, in the
//      soft link's store forms;
//   5. per stream the two integer counts and the K float sums stay in registers and are reduced in link_walk's fixed order: shuffles
//      in the wave, then the four waves through LDS.
//
// No atomics and no workspace: a group's outputs depend neither on the batch, nor on its position in it, nor on the run, nor on the
// load or store form or the alignment of the bases, nor on whether the LLRs are stored.  Rounding: the build has no fast-math, and
// without it the compiler's default for HIP is a correctly rounded float32 division (-fhip-fp32-correctly-rounded-divide-sqrt), so
// `scale / a_other` is ONE rounding; every product is a fused multiply-add chain written as such, and the detector and the soft
// pieces are compiled under `fp contract(off)`, so nothing is contracted behind the source.  With an unheard second stream
// (H_r1 = E_r1 = 0) and reg scale = 1 in powers of two, stream 0 is link_mrc_kernel's output on the frames (r, 0), bit for bit.
#include <type_traits>

#include "link_device.h"

namespace aft {
namespace {

constexpr int kSmStreams = AFT_LINK_MAX_STREAMS;

struct LinkSmArgs {
    aft_link c;
    const float2 *ideal, *est;
    const unsigned long long *keys;
    const float *sigma, *rho, *scale, *reg, *factors;
    int *counts;
    float *loss, *llr;          // llr may be NULL
    unsigned elems;             // S T - 1 fits; S T itself may be 2^31
    float d, d2;                // float(sqrt(3 / (2 (L^2 - 1)))) and twice that
    int n_factors;              // 1 .. kMaxFactors
    int branches;               // 2 .. AFT_LINK_MAX_BRANCHES
    int wide;                   // 1: 16-byte loads of ideal and est
    int store;                  // bytes per store of llr: 16, 8 or 4
};

template <int M>
__global__ __launch_bounds__(kFrameThreads) void link_sm_kernel(const LinkSmArgs a) {
    constexpr int half = M / 2, L = 1 << half;
    __shared__ int psc[AFT_CHANSIM_MAX_PILOT_SCS], psym[AFT_CHANSIM_MAX_PILOT_SYMBOLS];
    __shared__ unsigned long long bkey[AFT_LINK_MAX_BRANCHES];
    __shared__ float bsigma[AFT_LINK_MAX_BRANCHES], brho[AFT_LINK_MAX_BRANCHES];
    __shared__ float part[kLinkWaves][kSmStreams * kMaxFactors];
    __shared__ int ipart[kLinkWaves][kSmStreams * 2];
    const aft_link &c = a.c;
    const int tid = threadIdx.x;
    const size_t g = blockIdx.x;
    const int Ps = c.pilot_scs, Pt = c.pilot_symbols, nf = a.n_factors, R = a.branches;
    const unsigned T = (unsigned)c.num_symbols, last = a.elems;
    AFT_DEV_ASSERT(nf >= 1 && nf <= kMaxFactors);
    AFT_DEV_ASSERT(R >= 2 && R <= AFT_LINK_MAX_BRANCHES);
    const size_t first = g * (size_t)(kSmStreams * R);          // the group's leader, frame (0, 0)
    link_stage_pilots(c, tid, psc, psym);
    if (tid >= 2 * kWave && tid - 2 * kWave < R) {              // the frames (r, 0): the antennas' noise keys, noise scales and weights
        const int r = tid - 2 * kWave;
        bkey[r] = a.keys[first + kSmStreams * r];
        bsigma[r] = a.sigma[first + kSmStreams * r];
        brho[r] = a.rho[first + kSmStreams * r];
    }
    __syncthreads();
    const unsigned long long k0 = bkey[0], k1 = a.keys[first + 1];      // one transmission per stream: the keys of frames (0, s)
    const float scale = a.scale[g], reg = a.reg[g];
    float fac[kMaxFactors], acc0[kMaxFactors], acc1[kMaxFactors];
#pragma unroll
    for (int k = 0; k < kMaxFactors; ++k) {
        fac[k] = k < nf ? a.factors[k] : 0.f;
        acc0[k] = acc1[k] = 0.f;
    }
    const size_t frame = (size_t)last + 1;                      // elements per frame
    const float2 *hp = a.ideal + first * frame, *ep = a.est + first * frame;
    float *lp = a.llr != nullptr ? a.llr + g * kSmStreams * frame * M : nullptr;
    int bits0 = 0, symbols0 = 0, bits1 = 0, symbols1 = 0;
    const unsigned pairs = (last >> 1) + 1;                     // the last pair of an odd grid holds one element
    for (unsigned i = tid; i < pairs; i += kFrameThreads) {      // pairs <= 2^30: the index cannot wrap
        const unsigned q = 2 * i;
        const bool two = q < last;
        AFT_DEV_ASSERT(q <= last && (two || !a.wide));
        const bool d0 = link_is_data(psc, Ps, psym, Pt, T, q), d1 = two && link_is_data(psc, Ps, psym, Pt, T, q + 1);
        const LinkSent none{0u, 0u, 0.f, 0.f};
        LinkSent s00 = none, s01 = none, s10 = none, s11 = none;     // s<stream><element>
        if (d0) { s00 = link_sent<M>(a.d, k0, q); s10 = link_sent<M>(a.d, k1, q); }
        if (d1) { s01 = link_sent<M>(a.d, k0, q + 1); s11 = link_sent<M>(a.d, k1, q + 1); }
        const LinkSm zero{-0.f, -0.f, -0.f, -0.f, -0.f, -0.f, -0.f, -0.f};      // x + (-0) = x for every x
        LinkSm e0 = zero, e1 = zero;                            // the sums of elements q and q + 1
#pragma unroll 1
        for (int r = 0; r < R; ++r) {
            LinkPair h0{}, g0{}, h1{}, g1{};                    // H and E of the pairs (r, 0) and (r, 1)
            const size_t at = (size_t)(kSmStreams * r) * frame + q;
            link_load_pairs(hp + at, ep + at, a.wide, two, h0, g0);
            link_load_pairs(hp + at + frame, ep + at + frame, a.wide, two, h1, g1);
            const unsigned long long kf = bkey[r];
            const float sr = bsigma[r], rho = brho[r];
            if (d0) link_sm_accumulate(e0, rho, link_sample2(kf, sr, q, s00, s10, h0.a, h1.a), g0.a, g1.a);
            if (d1) link_sm_accumulate(e1, rho, link_sample2(kf, sr, q + 1, s01, s11, h0.b, h1.b), g0.b, g1.b);
        }
#pragma unroll 1
        for (int t = 0; t < kSmStreams; ++t) {                  // the stream; the element inside: one copy of the demapper
            float v[2 * M], acc[kMaxFactors];
#pragma unroll
            for (int j = 0; j < 2 * M; ++j) v[j] = 0.f;         // what a pilot position carries
#pragma unroll
            for (int k = 0; k < kMaxFactors; ++k) acc[k] = t ? acc1[k] : acc0[k];
            int bits = 0, symbols = 0;
#pragma unroll 1
            for (int s = 0; s < 2; ++s) {
                if (s ? d1 : d0) {
                    const LinkSent x = t ? (s ? s11 : s10) : (s ? s01 : s00);
                    const LinkDetected m = link_sm_detect(s ? e1 : e0, reg, scale, t != 0);
                    const float step = a.d2 * m.p;
                    const unsigned ki = decide<L>(m.cr, step), kq = decide<L>(m.ci, step);
                    const int wrong = __popc(x.gi ^ ki ^ (ki >> 1)) + __popc(x.gq ^ kq ^ (kq >> 1));
                    bits += wrong;
                    symbols += wrong != 0 ? 1 : 0;
                    float w[M];                                 // the M LLRs: I-axis bits first, MSB first, the order of the sent word
                    link_axis_llrs<L>(a.d, m.cr, m.p, m.eff, w);
                    link_axis_llrs<L>(a.d, m.ci, m.p, m.eff, w + half);
                    link_soft_losses<M>(w, x.gi, x.gq, fac, nf, acc);
#pragma unroll
                    for (int j = 0; j < M; ++j) {
                        if (s) v[M + j] = w[j];
                        else v[j] = w[j];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kMaxFactors; ++k) {
                if (t) acc1[k] = acc[k];
                else acc0[k] = acc[k];
            }
            if (t) { bits1 += bits; symbols1 += symbols; }
            else { bits0 += bits; symbols0 += symbols; }
            if (lp != nullptr) link_store_llrs<M>(lp + ((size_t)t * frame + q) * M, v, two ? 2 * M : M, a.store);
        }
    }
    link_wave_sum(bits0, tid, ipart, 0);
    link_wave_sum(symbols0, tid, ipart, 1);
    link_wave_sum(bits1, tid, ipart, 2);
    link_wave_sum(symbols1, tid, ipart, 3);
#pragma unroll
    for (int k = 0; k < kMaxFactors; ++k)
        if (k < nf) {
            link_wave_sum(acc0[k], tid, part, k);
            link_wave_sum(acc1[k], tid, part, kMaxFactors + k);
        }
    __syncthreads();
    if (tid < kSmStreams * kMaxFactors) {                       // thread t 8 + k the loss of stream t at factor k
        const int t = tid / kMaxFactors, k = tid % kMaxFactors;
        if (k < nf) a.loss[(g * kSmStreams + t) * (size_t)nf + k] = link_block_sum(part, tid) * kInvLn2;
    }
    // the second wave: per stream the bit errors, then the symbol errors
    if (tid >= kWave && tid < kWave + 2 * kSmStreams) a.counts[2 * kSmStreams * g + (tid - kWave)] = link_block_sum(ipart, tid - kWave);
}

}  // namespace

hipError_t launch_link_sm(const aft_link &link, const float *ideal, const float *est, const unsigned long long *keys,
                          const float *sigma, const float *rho, const float *scale, const float *reg, const float *factors,
                          int n_factors, int branches, int32_t *counts, float *loss, float *llr, int batch, hipStream_t st) {
    LinkSmArgs a{};
    a.c = link;
    a.ideal = reinterpret_cast<const float2 *>(ideal);
    a.est = reinterpret_cast<const float2 *>(est);
    a.keys = keys; a.sigma = sigma; a.rho = rho; a.scale = scale; a.reg = reg; a.factors = factors;
    a.counts = counts; a.loss = loss; a.llr = llr;
    a.n_factors = n_factors; a.branches = branches;
    const unsigned long long elems = (unsigned long long)link.num_scs * (unsigned long long)link.num_symbols;
    a.elems = (unsigned)(elems - 1);
    const int m = link.bits_per_symbol, L = 1 << (m / 2);
    a.d = (float)sqrt(3.0 / (2.0 * ((double)L * L - 1.0)));
    a.d2 = 2.f * a.d;
    a.wide = wide_ok(link.num_symbols, ideal, est);
    a.store = link_llr_store_bytes(llr, m, elems);
    const dim3 grid((unsigned)(batch / (branches * kSmStreams)));
    switch (m) {
        case 2: hipLaunchKernelGGL(link_sm_kernel<2>, grid, dim3(kFrameThreads), 0, st, a); break;
        case 4: hipLaunchKernelGGL(link_sm_kernel<4>, grid, dim3(kFrameThreads), 0, st, a); break;
        case 6: hipLaunchKernelGGL(link_sm_kernel<6>, grid, dim3(kFrameThreads), 0, st, a); break;
        case 8: hipLaunchKernelGGL(link_sm_kernel<8>, grid, dim3(kFrameThreads), 0, st, a); break;
        default: return hipErrorInvalidValue;           // the entry point has refused it
    }
    return hipGetLastError();
}

}  // namespace aft
