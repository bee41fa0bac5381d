// Joint max-log detection on the two-stream link (include/adafortitran_amd.h "joint detection"; adafortitran_amd/linksim.py "the joint
// link" is the definition and the float64 twin): the exact max-log LLR of every bit of both streams, 2 M candidate evaluations per data
// element instead of M^2, because for a fixed symbol of one stream the best symbol of the other separates per axis.  Layout, keys,
// launch shape and steps 1 to 3 and 5 are k_linksm.hip's, piece for piece from link_device.h: one workgroup per GROUP of 2 R consecutive
// frames, one launch per batch;
//
//   1. the pilot positions go to LDS and the R keys, noise scales and weights of the frames (r, 0);
//   2. a thread takes the element pairs (2 i, 2 i + 1), i = tid, tid + 256, ...: the same pair-to-thread map and load rule per plane;
//   3. per data element both sent words are hashed once (link_sent); the antenna loop, not unrolled, forms y_r (link_sample2) and adds
//      the eight sums m_0, m_1, g00, g11, g01 (link_sm_accumulate), one fused multiply-add per term in increasing r, from -0;
//   4. the joint demapper (link_joint_llrs) runs in a stream loop around an element loop, neither unrolled: one copy of the code.  For
//      stream e with the other stream o, over the candidates x_e = a_ki + j a_kq, ki outside (a rolled loop) and kq inside (unrolled:
//      the L column minima and the L Q-axis terms t(kq) = mu_kq(Im m_e, g_ee) live in registers under constant indices):
//        per row        a_ki, t(ki) = mu_ki(Re m_e, g_ee) and the row's share of z: base = m_o - g_oe a_ki, two fused multiply-adds;
//        per candidate  z = base - j g_oe a_kq, two more (the four of z(x_e) = m_o - g_oe x_e, the a_ki terms first); per axis of z
//                       the inner minimum over the L / 2 positive levels of fma(-2 a_k, |comp|, a_k^2 g_oo) -- mu_k of the level
//                       on comp's side; the mirrored level is never smaller --; f = (t(ki) + t(kq)) + (r_I + r_Q); the row and
//                       the column minimum;
//        per row        the I-axis bits' two minima take the row minimum by the Gray label of ki;
//        at the end     the Q-axis bits' two minima take the column minima by the labels of kq; Lambda_j = scale (min1 - min0).
//      The two axes of z run as one float2: z's second fused multiply-add and each level's are one v_pk_fma_f32 for both axes (the
//      same correctly rounded results as two scalar ones), so a candidate is 1 + L / 2 packed fused multiply-adds, L minima of the
//      two scans, 3 additions and 2 minima: 3 L / 2 + 6 VALU operations by the source (30 at 256-QAM; the compiled row of 16
//      candidates is 544, 34 each, with the |comp| masks and moves) and 2 m + L live minima; no LDS.  The hard decision is
//      the sign of the stream's own LLRs (bit j is 1 iff Lambda_j < 0), counted against the sent Gray codes; the loss is
//      link_soft_losses on them.  A stream's LLRs of the pair leave by link_store_llrs;
//   5. per stream the two integer counts and the K float sums stay in registers and are reduced in link_walk's fixed order.
//
// No atomics and no workspace: a group's outputs depend neither on the batch, nor on its position in it, nor on the run, nor on the
// load or store form or the alignment of the bases, nor on whether the LLRs are stored.  No division anywhere; every product is a
// fused multiply-add chain written as such, compiled under `fp contract(off)`.  The minima start at +infinity and every bit has
// candidates on both sides, so finite operands give finite LLRs; all-zero estimates give f = 0 for every candidate and LLRs of 0.
#include "link_device.h"

namespace aft {
namespace {

constexpr int kJointStreams = AFT_LINK_MAX_STREAMS;

struct LinkJointArgs {
    aft_link c;
    const float2 *ideal, *est;
    const unsigned long long *keys;
    const float *sigma, *rho, *scale, *factors;
    int *counts;
    float *loss, *llr;          // llr may be NULL
    unsigned elems;             // S T - 1 fits; S T itself may be 2^31
    float d;                    // float(sqrt(3 / (2 (L^2 - 1))))
    int n_factors;              // 1 .. kMaxFactors
    int branches;               // 2 .. AFT_LINK_MAX_BRANCHES
    int wide;                   // 1: 16-byte loads of ideal and est
    int store;                  // bytes per store of llr: 16, 8 or 4
};

// r = min_k mu_k(z.x, p) + min_k mu_k(z.y, p), mu_k(comp, p) = a_k (a_k p - 2 comp): both axes of z at once, each scanned over the
// positive levels against |comp| -- neg2a[i] = -2 a and pk[i] = a^2 p of level a = (2 i + 1) d.  The two axes' fused multiply-adds
// are one packed instruction (v_pk_fma_f32: the same two correctly rounded results), which matters where one wave owns a SIMD
template <int H>
__device__ __forceinline__ float link_joint_inner_min(f32x2 z, const float (&neg2a)[H], const float (&pk)[H]) {
#pragma clang fp contract(off)
    const f32x2 c = f32x2{fabsf(z.x), fabsf(z.y)};
    f32x2 best = __builtin_elementwise_fma(f32x2{neg2a[0], neg2a[0]}, c, f32x2{pk[0], pk[0]});
#pragma unroll
    for (int i = 1; i < H; ++i) {
        const f32x2 mu = __builtin_elementwise_fma(f32x2{neg2a[i], neg2a[i]}, c, f32x2{pk[i], pk[i]});
        best = f32x2{fminf(best.x, mu.x), fminf(best.y, mu.y)};
    }
    return best.x + best.y;
}

// The M max-log LLRs of stream e (`second` picks the roles) from an element's eight sums: out[j] = scale (min1 - min0) of
// f(x_e) = g_ee |x_e|^2 - 2 Re(conj(x_e) m_e) + min over x_o of (g_oo |x_o|^2 - 2 Re(conj(x_o) (m_o - g_oe x_e))), I-axis bits first,
// MSB first: the order of the sent word.
template <int M>
__device__ __forceinline__ void link_joint_llrs(float d, const LinkSm &a, float scale, bool second, float *out) {
#pragma clang fp contract(off)
    constexpr int half = M / 2, L = 1 << half, H = L / 2;
    const float ge = second ? a.g11 : a.g00, go = second ? a.g00 : a.g11;
    const float mer = second ? a.m1r : a.m0r, mei = second ? a.m1i : a.m0i;
    const float mor = second ? a.m0r : a.m1r, moi = second ? a.m0i : a.m1i;
    const float gxr = a.g01r, gxi = second ? a.g01i : -a.g01i;  // g_oe: g01 for stream 1, conj(g01) for stream 0
    float neg2a[H], pk[H];
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const float ak = d * (float)(2 * i + 1);
        neg2a[i] = -2.f * ak;
        pk[i] = (ak * ak) * go;
    }
    const float m2q = -2.f * mei, m2i = -2.f * mer;
    float tq[L], col[L];
#pragma unroll
    for (int k = 0; k < L; ++k) {
        const float ak = d * (float)(2 * k - (L - 1));
        tq[k] = ak * fmaf(ak, ge, m2q);
        col[k] = INFINITY;
    }
    float i0[half], i1[half];
#pragma unroll
    for (int j = 0; j < half; ++j) i0[j] = i1[j] = INFINITY;
#pragma unroll 1
    for (int ki = 0; ki < L; ++ki) {
        const float ai = d * (float)(2 * ki - (L - 1));
        const float ti = ai * fmaf(ai, ge, m2i);
        const f32x2 base = f32x2{fmaf(-gxr, ai, mor), fmaf(-gxi, ai, moi)}, turn = f32x2{gxi, -gxr};    // z = base - j g_oe a_kq
        float row = INFINITY;
#pragma unroll
        for (int kq = 0; kq < L; ++kq) {
            const float aq = d * (float)(2 * kq - (L - 1));
            const f32x2 z = __builtin_elementwise_fma(turn, f32x2{aq, aq}, base);
            const float r = link_joint_inner_min<H>(z, neg2a, pk);
            const float f = (ti + tq[kq]) + r;
            row = fminf(row, f);
            col[kq] = fminf(col[kq], f);
        }
        const unsigned label = (unsigned)ki ^ ((unsigned)ki >> 1);
#pragma unroll
        for (int j = 0; j < half; ++j) {
            const bool one = (label >> (half - 1 - j)) & 1u;
            i1[j] = one ? fminf(i1[j], row) : i1[j];
            i0[j] = one ? i0[j] : fminf(i0[j], row);
        }
    }
#pragma unroll
    for (int j = 0; j < half; ++j) {
        float q0 = INFINITY, q1 = INFINITY;
#pragma unroll
        for (int k = 0; k < L; ++k) {
            if (((k ^ (k >> 1)) >> (half - 1 - j)) & 1) q1 = fminf(q1, col[k]);
            else q0 = fminf(q0, col[k]);
        }
        out[j] = scale * (i1[j] - i0[j]);
        out[half + j] = scale * (q1 - q0);
    }
}

template <int M>
__global__ __launch_bounds__(kFrameThreads) void link_joint_kernel(const LinkJointArgs a) {
    constexpr int half = M / 2;
    __shared__ int psc[AFT_CHANSIM_MAX_PILOT_SCS], psym[AFT_CHANSIM_MAX_PILOT_SYMBOLS];
    __shared__ unsigned long long bkey[AFT_LINK_MAX_BRANCHES];
    __shared__ float bsigma[AFT_LINK_MAX_BRANCHES], brho[AFT_LINK_MAX_BRANCHES];
    __shared__ float part[kLinkWaves][kJointStreams * kMaxFactors];
    __shared__ int ipart[kLinkWaves][kJointStreams * 2];
    const aft_link &c = a.c;
    const int tid = threadIdx.x;
    const size_t g = blockIdx.x;
    const int Ps = c.pilot_scs, Pt = c.pilot_symbols, nf = a.n_factors, R = a.branches;
    const unsigned T = (unsigned)c.num_symbols, last = a.elems;
    AFT_DEV_ASSERT(nf >= 1 && nf <= kMaxFactors);
    AFT_DEV_ASSERT(R >= 2 && R <= AFT_LINK_MAX_BRANCHES);
    const size_t first = g * (size_t)(kJointStreams * R);       // the group's leader, frame (0, 0)
    link_stage_pilots(c, tid, psc, psym);
    if (tid >= 2 * kWave && tid - 2 * kWave < R) {              // the frames (r, 0): the antennas' noise keys, noise scales and weights
        const int r = tid - 2 * kWave;
        bkey[r] = a.keys[first + kJointStreams * r];
        bsigma[r] = a.sigma[first + kJointStreams * r];
        brho[r] = a.rho[first + kJointStreams * r];
    }
    __syncthreads();
    const unsigned long long k0 = bkey[0], k1 = a.keys[first + 1];      // one transmission per stream: the keys of frames (0, s)
    const float scale = a.scale[g];
    float fac[kMaxFactors], acc0[kMaxFactors], acc1[kMaxFactors];
#pragma unroll
    for (int k = 0; k < kMaxFactors; ++k) {
        fac[k] = k < nf ? a.factors[k] : 0.f;
        acc0[k] = acc1[k] = 0.f;
    }
    const size_t frame = (size_t)last + 1;                      // elements per frame
    const float2 *hp = a.ideal + first * frame, *ep = a.est + first * frame;
    float *lp = a.llr != nullptr ? a.llr + g * kJointStreams * frame * M : nullptr;
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
            const size_t at = (size_t)(kJointStreams * r) * frame + q;
            link_load_pairs(hp + at, ep + at, a.wide, two, h0, g0);
            link_load_pairs(hp + at + frame, ep + at + frame, a.wide, two, h1, g1);
            const unsigned long long kf = bkey[r];
            const float sr = bsigma[r], rho = brho[r];
            if (d0) link_sm_accumulate(e0, rho, link_sample2(kf, sr, q, s00, s10, h0.a, h1.a), g0.a, g1.a);
            if (d1) link_sm_accumulate(e1, rho, link_sample2(kf, sr, q + 1, s01, s11, h0.b, h1.b), g0.b, g1.b);
        }
#pragma unroll 1
        for (int t = 0; t < kJointStreams; ++t) {               // the stream; the element inside: one copy of the demapper
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
                    float w[M];                                 // the M LLRs: I-axis bits first, MSB first, the order of the sent word
                    link_joint_llrs<M>(a.d, s ? e1 : e0, scale, t != 0, w);
                    unsigned hi = 0, hq = 0;                    // the decided Gray codes: bit j is 1 iff its LLR is negative
#pragma unroll
                    for (int j = 0; j < half; ++j) {
                        hi = (hi << 1) | (w[j] < 0.f ? 1u : 0u);
                        hq = (hq << 1) | (w[half + j] < 0.f ? 1u : 0u);
                    }
                    const int wrong = __popc(x.gi ^ hi) + __popc(x.gq ^ hq);
                    bits += wrong;
                    symbols += wrong != 0 ? 1 : 0;
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
    if (tid < kJointStreams * kMaxFactors) {                    // thread t 8 + k the loss of stream t at factor k
        const int t = tid / kMaxFactors, k = tid % kMaxFactors;
        if (k < nf) a.loss[(g * kJointStreams + t) * (size_t)nf + k] = link_block_sum(part, tid) * kInvLn2;
    }
    // the second wave: per stream the bit errors, then the symbol errors
    if (tid >= kWave && tid < kWave + 2 * kJointStreams) a.counts[2 * kJointStreams * g + (tid - kWave)] = link_block_sum(ipart, tid - kWave);
}

}  // namespace

hipError_t launch_link_joint(const aft_link &link, const float *ideal, const float *est, const unsigned long long *keys,
                             const float *sigma, const float *rho, const float *scale, const float *factors, int n_factors,
                             int branches, int32_t *counts, float *loss, float *llr, int batch, hipStream_t st) {
    LinkJointArgs a{};
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
    a.wide = wide_ok(link.num_symbols, ideal, est);
    a.store = link_llr_store_bytes(llr, m, elems);
    const dim3 grid((unsigned)(batch / (branches * kJointStreams)));
    switch (m) {
        case 2: hipLaunchKernelGGL(link_joint_kernel<2>, grid, dim3(kFrameThreads), 0, st, a); break;
        case 4: hipLaunchKernelGGL(link_joint_kernel<4>, grid, dim3(kFrameThreads), 0, st, a); break;
        case 6: hipLaunchKernelGGL(link_joint_kernel<6>, grid, dim3(kFrameThreads), 0, st, a); break;
        case 8: hipLaunchKernelGGL(link_joint_kernel<8>, grid, dim3(kFrameThreads), 0, st, a); break;
        default: return hipErrorInvalidValue;           // the entry point has refused it
    }
    return hipGetLastError();
}

}  // namespace aft
