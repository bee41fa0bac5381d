// Receive diversity on the link: maximum-ratio combining over R branches (include/adafortitran_amd.h "receive diversity";
// adafortitran_amd/linksim.py "the diversity link" is the definition and the float64 twin).  One workgroup per GROUP of R consecutive
// frames, one launch per batch; a group's counts, losses and LLRs are a function of its own R keys, noise scales, weights, true channels
// and estimates and of its leader's LLR scale only.
//
//   1. the pilot positions and the group's R keys, noise scales and weights go to LDS;
//   2. a thread takes the element pairs (2 i, 2 i + 1), i = tid, tid + 256, ..., as link_soft_kernel does, whichever load form runs;
//   3. per data element the sent word is hashed once, from the leader's key (link_sent);
//   4. a loop over the branches with a run-time bound: each branch loads its own H_r and E_r (16 bytes for the pair when T is even and
//      the bases are aligned, 8 bytes per element otherwise), hashes its own two noise words (link_branch: the single-branch kernels'
//      y, c_r and p_r) and adds c = fma(rho_r, c_r, c), p = fma(rho_r, p_r, p).  The sums start at -0, so with R = 1 and rho_0 = 1
//      they are c_0 and p_0 bit for bit, the sign of a zero included;
//   5. the hard decision, the LLRs with the leader's scale and the softplus losses are the single-branch kernels' device functions
//      (link_device.h) on this c and p -- one copy of that code per kernel, inside a loop that is not unrolled (at m = 8 it is large);
//   6. the two integer counts and the K float sums stay in registers and are reduced in a fixed order: shuffles, then the four waves
//      through LDS.  No atomics and no workspace: a group's outputs depend neither on the batch, nor on its position in it, nor on the
//      run, nor on the load form, nor on whether the LLRs are stored.
#include "link_device.h"

namespace aft {
namespace {

struct LinkMrcArgs {
    aft_link c;
    const float2 *ideal, *est;
    const unsigned long long *keys;
    const float *sigma, *rho, *scale, *factors;
    int *counts;
    float *loss, *llr;          // llr may be NULL
    unsigned elems;             // S T - 1 fits; S T itself may be 2^31
    float d, d2;                // float(sqrt(3 / (2 (L^2 - 1)))) and twice that
    int n_factors;              // 1 .. kMaxFactors
    int branches;               // 1 .. AFT_LINK_MAX_BRANCHES
    int wide;                   // 1: 16-byte loads of ideal and est
    int store;                  // bytes per store of llr: 16, 8 or 4
};

struct MrcSum {
    float cr, ci, p;
};

// c += rho c_r, p += rho p_r: one fused multiply-add each, the product exact inside it
__device__ __forceinline__ void mrc_add(MrcSum &s, float rho, const LinkBranch &b) {
    s.cr = fmaf(rho, b.cr, s.cr);
    s.ci = fmaf(rho, b.ci, s.ci);
    s.p = fmaf(rho, b.p, s.p);
}

template <int M>
__global__ __launch_bounds__(kFrameThreads) void link_mrc_kernel(const LinkMrcArgs a) {
    constexpr int half = M / 2, L = 1 << half;
    __shared__ int psc[AFT_CHANSIM_MAX_PILOT_SCS], psym[AFT_CHANSIM_MAX_PILOT_SYMBOLS];
    __shared__ unsigned long long bkey[AFT_LINK_MAX_BRANCHES];
    __shared__ float bsigma[AFT_LINK_MAX_BRANCHES], brho[AFT_LINK_MAX_BRANCHES];
    __shared__ float part[kLinkWaves][kMaxFactors];
    __shared__ int ipart[kLinkWaves][2];
    const aft_link &c = a.c;
    const int tid = threadIdx.x;
    const size_t g = blockIdx.x;
    const int Ps = c.pilot_scs, Pt = c.pilot_symbols, nf = a.n_factors, R = a.branches;
    const unsigned T = (unsigned)c.num_symbols, last = a.elems;
    AFT_DEV_ASSERT(Ps >= 1 && Ps <= AFT_CHANSIM_MAX_PILOT_SCS && Pt >= 1 && Pt <= AFT_CHANSIM_MAX_PILOT_SYMBOLS);
    AFT_DEV_ASSERT(nf >= 1 && nf <= kMaxFactors && R >= 1 && R <= AFT_LINK_MAX_BRANCHES);
    const size_t first = g * (size_t)R;                         // the group's leader
    if (tid < Ps) psc[tid] = c.pilot_sc_index[tid];
    if (tid >= kWave && tid - kWave < Pt) psym[tid - kWave] = c.pilot_symbol_index[tid - kWave];
    if (tid >= 2 * kWave && tid - 2 * kWave < R) {
        const int r = tid - 2 * kWave;
        bkey[r] = a.keys[first + r];
        bsigma[r] = a.sigma[first + r];
        brho[r] = a.rho[first + r];
    }
    __syncthreads();
    const unsigned long long kl = bkey[0];                      // one transmission per group: the leader's key
    const float scale = a.scale[g];
    float fac[kMaxFactors], acc[kMaxFactors];
#pragma unroll
    for (int k = 0; k < kMaxFactors; ++k) {
        fac[k] = k < nf ? a.factors[k] : 0.f;
        acc[k] = 0.f;
    }
    const size_t frame = (size_t)last + 1;                      // elements per frame
    const float2 *hp = a.ideal + first * frame, *ep = a.est + first * frame;
    float *lp = a.llr != nullptr ? a.llr + g * frame * M : nullptr;
    int bits = 0, symbols = 0;
    auto data = [&](unsigned q) {                               // not a pilot position
        const unsigned s = q / T, t = q - s * T;
        return !(link_listed(psym, Pt, (int)t) && link_listed(psc, Ps, (int)s));
    };
    const unsigned pairs = (last >> 1) + 1;                     // the last pair of an odd grid holds one element
    for (unsigned i = tid; i < pairs; i += kFrameThreads) {      // pairs <= 2^30: the index cannot wrap
        const unsigned q = 2 * i;
        const bool two = q < last;
        AFT_DEV_ASSERT(q <= last && (two || !a.wide));
        const bool d0 = data(q), d1 = two && data(q + 1);
        LinkSent s0{0u, 0u, 0.f, 0.f}, s1 = s0;
        if (d0) s0 = link_sent<M>(a.d, kl, q);
        if (d1) s1 = link_sent<M>(a.d, kl, q + 1);
        MrcSum m0{-0.f, -0.f, -0.f}, m1 = m0;                   // x + (-0) = x for every x: the first branch at rho = 1 is exact
#pragma unroll 1
        for (int r = 0; r < R; ++r) {
            const float2 *hr = hp + (size_t)r * frame + q, *er = ep + (size_t)r * frame + q;
            float2 h0, e0, h1 = make_float2(0.f, 0.f), e1 = h1;
            if (a.wide) {
                const f32x4 h = *reinterpret_cast<const f32x4 *>(hr), e = *reinterpret_cast<const f32x4 *>(er);
                h0 = make_float2(h[0], h[1]); e0 = make_float2(e[0], e[1]);
                h1 = make_float2(h[2], h[3]); e1 = make_float2(e[2], e[3]);
            } else {
                h0 = hr[0]; e0 = er[0];
                if (two) { h1 = hr[1]; e1 = er[1]; }
            }
            const unsigned long long kf = bkey[r];
            const float sigma = bsigma[r], rho = brho[r];
            if (d0) mrc_add(m0, rho, link_branch(kf, sigma, q, s0.xr, s0.xi, h0, e0));
            if (d1) mrc_add(m1, rho, link_branch(kf, sigma, q + 1, s1.xr, s1.xi, h1, e1));
        }
        float v[2 * M];
#pragma unroll
        for (int j = 0; j < 2 * M; ++j) v[j] = 0.f;             // what a pilot position carries
#pragma unroll 1
        for (int s = 0; s < 2; ++s) {                           // one copy of the element's code, as in link_soft_kernel
            if (s ? d1 : d0) {
                const MrcSum m = s ? m1 : m0;
                const unsigned gi = s ? s1.gi : s0.gi, gq = s ? s1.gq : s0.gq;
                const float step = a.d2 * m.p;
                const unsigned ki = decide<L>(m.cr, step), kq = decide<L>(m.ci, step);
                const int wrong = __popc(gi ^ ki ^ (ki >> 1)) + __popc(gq ^ kq ^ (kq >> 1));
                bits += wrong;
                symbols += wrong != 0 ? 1 : 0;
                float w[M];
                link_axis_llrs<L>(a.d, m.cr, m.p, scale, w);
                link_axis_llrs<L>(a.d, m.ci, m.p, scale, w + half);
                link_soft_losses<M>(w, gi, gq, fac, nf, acc);
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
    for (int o = kWave / 2; o >= 1; o >>= 1) {
        bits += __shfl_xor(bits, o);
        symbols += __shfl_xor(symbols, o);
    }
    if ((tid & (kWave - 1)) == 0) {
        ipart[tid / kWave][0] = bits;
        ipart[tid / kWave][1] = symbols;
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
        a.loss[g * (size_t)nf + tid] = total * kInvLn2;
    }
    if (tid >= kWave && tid < kWave + 2) {                      // the second wave: the bit errors, then the symbol errors
        const int which = tid - kWave;
        int total = 0;
#pragma unroll
        for (int w = 0; w < kLinkWaves; ++w) total += ipart[w][which];
        a.counts[2 * g + which] = total;
    }
}

}  // namespace

hipError_t launch_link_mrc(const aft_link &link, const float *ideal, const float *est, const unsigned long long *keys,
                           const float *sigma, const float *rho, const float *scale, const float *factors, int n_factors, int branches,
                           int32_t *counts, float *loss, float *llr, int batch, hipStream_t st) {
    LinkMrcArgs a{};
    a.c = link;
    a.ideal = reinterpret_cast<const float2 *>(ideal);
    a.est = reinterpret_cast<const float2 *>(est);
    a.keys = keys; a.sigma = sigma; a.rho = rho; a.scale = scale; a.factors = factors;
    a.counts = counts; a.loss = loss; a.llr = llr;
    a.n_factors = n_factors; a.branches = branches;
    const unsigned long long elems = (unsigned long long)link.num_scs * (unsigned long long)link.num_symbols;
    a.elems = (unsigned)(elems - 1);
    const int m = link.bits_per_symbol, L = 1 << (m / 2);
    a.d = (float)sqrt(3.0 / (2.0 * ((double)L * L - 1.0)));
    a.d2 = 2.f * a.d;
    a.wide = wide_ok(link.num_symbols, ideal, est);
    a.store = link_llr_store_bytes(llr, m, elems);
    const dim3 grid((unsigned)(batch / branches)), block(kFrameThreads);
    switch (m) {
        case 2: hipLaunchKernelGGL(link_mrc_kernel<2>, grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL(link_mrc_kernel<4>, grid, block, 0, st, a); break;
        case 6: hipLaunchKernelGGL(link_mrc_kernel<6>, grid, block, 0, st, a); break;
        case 8: hipLaunchKernelGGL(link_mrc_kernel<8>, grid, block, 0, st, a); break;
        default: return hipErrorInvalidValue;           // aft_link_mrc_f32 has refused it
    }
    return hipGetLastError();
}

}  // namespace aft
