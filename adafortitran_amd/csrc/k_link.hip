// The link front end (include/adafortitran_amd.h "link-level bit errors", "soft link", "receive diversity"; adafortitran_amd/linksim.py is
// the definition and the float64 twin): ONE frame walk, link_walk, and three instantiations of it.  One workgroup per GROUP of R
// consecutive frames (R = 1: per frame), one launch per batch; a group's counts, losses and LLRs are a function of its own R keys, noise
// scales, weights, true channels and estimates and of its leader's LLR scale only.
//
//   1. the pilot positions go to LDS (two sorted lists of at most 64 and 16 entries) and, where there are branches, the group's R keys,
//      noise scales and weights;
//   2. a thread takes the element pairs (2 i, 2 i + 1), i = tid, tid + 256, ..., consecutive lanes on consecutive addresses, whichever
//      load form runs: 16 bytes of H and of E for the pair (T even -- a pair never straddles a row -- and both bases 16-byte aligned),
//      8 bytes per element otherwise; the last pair of an odd grid holds one element.  An element whose column and row are both in
//      the lists is a pilot and is skipped (two binary searches; the row's only when the column hit);
//   3. per data element the sent word is hashed once, from the leader's key (link_sent: the Gray-coded square-QAM symbol), and a branch
//      hashes its own two noise words (link_branch: y = H x + noise with the simulator's hash and Box-Muller, c = y conj(E), p = |E|^2).
//      With one branch c and p are that branch's own.  With R at run time a loop over the branches loads each H_r and E_r and adds
//      c = fma(rho_r, c_r, c), p = fma(rho_r, p_r, p) in increasing r; the sums start at -0, so with R = 1 and rho_0 = 1 they are c_0
//      and p_0 bit for bit, the sign of a zero included;
//   4. the enabled measures on this c and p, in a loop over the pair's two elements that is not unrolled where there is a soft half
//      (one copy of that code: at m = 8 it is large) and unrolled for the counts alone.  Counts:
//      per axis the number of inner boundaries beta_b p at or below the component of c -- zero-forcing with a hard decision and without
//      a division, total at p = 0 -- against the sent Gray code.  Soft: per axis the L metrics a_k (a_k p - 2 comp) in registers, the
//      m/2 pairs of minima, the LLRs scale (min1 - min0) and, per factor, softplus of the LLR against its sent bit;
//   5. the two integer counts and the K float sums stay in registers and are reduced in a fixed order: shuffles in the wave, then the
//      four waves through LDS; the second wave's first two threads store the counts, thread k the loss at factor k.
//
// No atomics and no workspace: a group's outputs depend neither on the batch, nor on its position in it, nor on the run, nor on the
// load form or the alignment of the bases, nor on whether the LLRs are stored.  The rounding behind tests/test_linksim_gpu.py's margin:
// every product is a fused multiply-add chain, the angle is formed in turns, no fast-math.
//
//   link_errors_kernel  (aft_link_errors_f32)  counts,              one branch
//   link_soft_kernel    (aft_link_soft_f32)    losses and LLRs,     one branch
//   link_mrc_kernel     (aft_link_mrc_f32)     counts, losses, LLRs, R branches; with R = 1 bit for bit both of the above
#include "link_device.h"

namespace aft {
namespace {

// One instantiation per modulation order, so the boundary loops unroll.  Counts: the bit and symbol errors.  Soft: the losses and, when
// a.llr is there, the LLRs.  Branches: a.branches frames per group, combined with a.rho; otherwise one frame is the group.
template <int M, bool Counts, bool Soft, bool Branches>
__device__ __forceinline__ void link_walk(const LinkArgs &a) {
    constexpr int half = M / 2, L = 1 << half;
    // copies of an element's code: one where there is a soft half (52 KB at m = 8, two are 100 KB), both in line for the counts alone
    constexpr int kCopies = Soft ? 1 : 2;
    __shared__ int psc[AFT_CHANSIM_MAX_PILOT_SCS], psym[AFT_CHANSIM_MAX_PILOT_SYMBOLS];
    __shared__ unsigned long long bkey[AFT_LINK_MAX_BRANCHES];
    __shared__ float bsigma[AFT_LINK_MAX_BRANCHES], brho[AFT_LINK_MAX_BRANCHES];
    __shared__ float part[kLinkWaves][kMaxFactors];
    __shared__ int ipart[kLinkWaves][2];
    const aft_link &c = a.c;
    const int tid = threadIdx.x;
    const size_t g = blockIdx.x;
    const int Ps = c.pilot_scs, Pt = c.pilot_symbols, nf = Soft ? a.n_factors : 0, R = Branches ? a.branches : 1;
    const unsigned T = (unsigned)c.num_symbols, last = a.elems;
    AFT_DEV_ASSERT(!Soft || (nf >= 1 && nf <= kMaxFactors));
    AFT_DEV_ASSERT(R >= 1 && R <= AFT_LINK_MAX_BRANCHES);
    const size_t first = g * (size_t)R;                         // the group's leader
    link_stage_pilots(c, tid, psc, psym);
    if constexpr (Branches) {
        if (tid >= 2 * kWave && tid - 2 * kWave < R) {
            const int r = tid - 2 * kWave;
            bkey[r] = a.keys[first + r];
            bsigma[r] = a.sigma[first + r];
            brho[r] = a.rho[first + r];
        }
    }
    __syncthreads();
    unsigned long long kl;                                      // one transmission per group: the leader's key
    float sigma = 0.f, scale = 0.f;
    if constexpr (Branches) kl = bkey[0];
    else { kl = a.keys[g]; sigma = a.sigma[g]; }
    float fac[kMaxFactors], acc[kMaxFactors];
    if constexpr (Soft) {
        scale = a.scale[g];
#pragma unroll
        for (int k = 0; k < kMaxFactors; ++k) {
            fac[k] = k < nf ? a.factors[k] : 0.f;
            acc[k] = 0.f;
        }
    }
    const size_t frame = (size_t)last + 1;                      // elements per frame
    const float2 *hp = a.ideal + first * frame, *ep = a.est + first * frame;
    float *lp = Soft && a.llr != nullptr ? a.llr + g * frame * M : nullptr;
    int bits = 0, symbols = 0;
    const unsigned pairs = (last >> 1) + 1;                     // the last pair of an odd grid holds one element
    for (unsigned i = tid; i < pairs; i += kFrameThreads) {      // pairs <= 2^30: the index cannot wrap
        const unsigned q = 2 * i;
        const bool two = q < last;
        AFT_DEV_ASSERT(q <= last && (two || !a.wide));
        auto data = [&](int s) { return (s == 0 || two) && link_is_data(psc, Ps, psym, Pt, T, q + s); };
        LinkPair h{}, e{};
        bool d0 = false, d1 = false;
        LinkSent s0{0u, 0u, 0.f, 0.f}, s1 = s0;
        LinkBranch m0{-0.f, -0.f, -0.f}, m1 = m0;               // x + (-0) = x for every x: the first branch at rho = 1 is exact
        if constexpr (!Branches) {
            link_load_pairs(hp + q, ep + q, a.wide, two, h, e);
        } else {                                                // both elements' lookups and sent words, once for all branches
            d0 = data(0);
            d1 = data(1);
            if (d0) s0 = link_sent<M>(a.d, kl, q);
            if (d1) s1 = link_sent<M>(a.d, kl, q + 1);
#pragma unroll 1
            for (int r = 0; r < R; ++r) {
                link_load_pairs(hp + (size_t)r * frame + q, ep + (size_t)r * frame + q, a.wide, two, h, e);
                const unsigned long long kf = bkey[r];
                const float sr = bsigma[r], rho = brho[r];
                if (d0) link_combine(m0, rho, link_branch(kf, sr, q, s0.xr, s0.xi, h.a, e.a));
                if (d1) link_combine(m1, rho, link_branch(kf, sr, q + 1, s1.xr, s1.xi, h.b, e.b));
            }
        }
        float v[2 * M];
        if constexpr (Soft) {
#pragma unroll
            for (int j = 0; j < 2 * M; ++j) v[j] = 0.f;         // what a pilot position carries
        }
#pragma unroll kCopies
        for (int s = 0; s < 2; ++s) {
            if (Branches ? (s ? d1 : d0) : data(s)) {
                LinkSent x = s ? s1 : s0;
                LinkBranch m = s ? m1 : m0;
                if constexpr (!Branches) {                      // the one branch's own c and p: no weight
                    x = link_sent<M>(a.d, kl, q + s);
                    m = link_branch(kl, sigma, q + s, x.xr, x.xi, s ? h.b : h.a, s ? e.b : e.a);
                }
                if constexpr (Counts) {
                    const float step = a.d2 * m.p;
                    const unsigned ki = decide<L>(m.cr, step), kq = decide<L>(m.ci, step);
                    const int wrong = __popc(x.gi ^ ki ^ (ki >> 1)) + __popc(x.gq ^ kq ^ (kq >> 1));
                    bits += wrong;
                    symbols += wrong != 0 ? 1 : 0;
                }
                if constexpr (Soft) {
                    float w[M];                                 // the M LLRs: I-axis bits first, MSB first, the order of the sent word
                    link_axis_llrs<L>(a.d, m.cr, m.p, scale, w);
                    link_axis_llrs<L>(a.d, m.ci, m.p, scale, w + half);
                    link_soft_losses<M>(w, x.gi, x.gq, fac, nf, acc);
#pragma unroll
                    for (int j = 0; j < M; ++j) {
                        if (s) v[M + j] = w[j];
                        else v[j] = w[j];
                    }
                }
            }
        }
        if constexpr (Soft) {
            if (lp != nullptr) link_store_llrs<M>(lp + (size_t)q * M, v, two ? 2 * M : M, a.store);
        }
    }
    if constexpr (Counts) {
        link_wave_sum(bits, tid, ipart, 0);
        link_wave_sum(symbols, tid, ipart, 1);
    }
    if constexpr (Soft) {
#pragma unroll
        for (int k = 0; k < kMaxFactors; ++k)
            if (k < nf) link_wave_sum(acc[k], tid, part, k);
    }
    __syncthreads();
    if constexpr (Soft) {
        if (tid < nf) a.loss[g * (size_t)nf + tid] = link_block_sum(part, tid) * kInvLn2;     // thread k the loss at factor k
    }
    if constexpr (Counts) {                                     // the second wave: the bit errors, then the symbol errors
        if (tid >= kWave && tid < kWave + 2) a.counts[2 * g + (tid - kWave)] = link_block_sum(ipart, tid - kWave);
    }
}

template <int M>
__global__ __launch_bounds__(kFrameThreads) void link_errors_kernel(const LinkArgs a) {
    link_walk<M, true, false, false>(a);
}

template <int M>
__global__ __launch_bounds__(kFrameThreads) void link_soft_kernel(const LinkArgs a) {
    link_walk<M, false, true, false>(a);
}

template <int M>
__global__ __launch_bounds__(kFrameThreads) void link_mrc_kernel(const LinkArgs a) {
    link_walk<M, true, true, true>(a);
}

}  // namespace

hipError_t launch_link_errors(const aft_link &link, const float *ideal, const float *est, const unsigned long long *keys,
                              const float *sigma, int32_t *counts, int batch, hipStream_t st) {
    const LinkArgs a = link_args(link, ideal, est, keys, sigma, nullptr, nullptr, nullptr, 1, 1, counts, nullptr, nullptr);
    return link_dispatch(link.bits_per_symbol, [&](auto m) {
        hipLaunchKernelGGL(link_errors_kernel<decltype(m)::value>, dim3((unsigned)batch), dim3(kFrameThreads), 0, st, a);
    });
}

hipError_t launch_link_soft(const aft_link &link, const float *ideal, const float *est, const unsigned long long *keys,
                            const float *sigma, const float *scale, const float *factors, int n_factors, float *loss, float *llr,
                            int batch, hipStream_t st) {
    const LinkArgs a = link_args(link, ideal, est, keys, sigma, nullptr, scale, factors, n_factors, 1, nullptr, loss, llr);
    return link_dispatch(link.bits_per_symbol, [&](auto m) {
        hipLaunchKernelGGL(link_soft_kernel<decltype(m)::value>, dim3((unsigned)batch), dim3(kFrameThreads), 0, st, a);
    });
}

hipError_t launch_link_mrc(const aft_link &link, const float *ideal, const float *est, const unsigned long long *keys,
                           const float *sigma, const float *rho, const float *scale, const float *factors, int n_factors, int branches,
                           int32_t *counts, float *loss, float *llr, int batch, hipStream_t st) {
    const LinkArgs a = link_args(link, ideal, est, keys, sigma, rho, scale, factors, n_factors, branches, counts, loss, llr);
    return link_dispatch(link.bits_per_symbol, [&](auto m) {
        hipLaunchKernelGGL(link_mrc_kernel<decltype(m)::value>, dim3((unsigned)(batch / branches)), dim3(kFrameThreads), 0, st, a);
    });
}

}  // namespace aft
