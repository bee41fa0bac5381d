// The two-stream link (include/adafortitran_amd.h "spatial multiplexing", "joint detection"; adafortitran_amd/linksim.py "the
// spatial-multiplexing link", "the joint link", "the successive-cancellation link" and "the codeword-cancellation link" are the
// definitions and the float64 twins): N = 2 streams on R antennas, ONE frame walk, link2_walk, and four detectors in its step 4.
// One workgroup per GROUP of 2 R consecutive frames -- frame r 2 + s is the pair (antenna r, stream s) --, one launch per batch; a group's counts, losses and LLRs are a function of its own keys, noise scales,
// weights, true channels and estimates and of its leader's LLR scale (and, for the linear detector, regulariser) only.  The walk is
// k_link.hip's link_walk with the combiner replaced by a detector:
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
//   4. the detector runs after it, in a stream loop around an element loop, neither unrolled: one copy of its code (the linear one
//      is about 50 KB at m = 8).  Per (stream, element) it turns the eight sums into the M LLRs and the number of wrong bits; the
//      loss is link_soft_losses on those LLRs, per factor softplus of the LLR against its sent bit, and a stream's LLRs of the pair
//      leave by link_store_llrs, in the soft link's store forms.
//        linear (link2_linear)  the adjugate detector (link_sm_detect: c_s, p_s, eff_s = scale / a_other) and then link_walk's
//          measures on them: the hard decision against the stream's sent Gray codes and the max-log LLRs eff_s (min1 - min0);
//        joint (link2_joint)  the exact max-log LLR of every bit, 2 M candidate evaluations per element instead of M^2, because for
//          a fixed symbol of one stream the best symbol of the other separates per axis (link_joint_llrs).  For stream e with the
//          other stream o, over the candidates x_e = a_ki + j a_kq, ki outside (a rolled loop) and kq inside (unrolled: the L column
//          minima and the L Q-axis terms t(kq) = mu_kq(Im m_e, g_ee) live in registers under constant indices):
//            per row        a_ki, t(ki) = mu_ki(Re m_e, g_ee) and the row's share of z: base = m_o - g_oe a_ki, two fused
//                           multiply-adds;
//            per candidate  z = base - j g_oe a_kq, two more (the four of z(x_e) = m_o - g_oe x_e, the a_ki terms first); per axis of
//                           z the inner minimum over the L / 2 positive levels of fma(-2 a_k, |comp|, a_k^2 g_oo) -- mu_k of the
//                           level on comp's side; the mirrored level is never smaller --; f = (t(ki) + t(kq)) + (r_I + r_Q); the
//                           row and the column minimum;
//            per row        the I-axis bits' two minima take the row minimum by the Gray label of ki;
//            at the end     the Q-axis bits' two minima take the column minima by the labels of kq; Lambda_j = scale (min1 - min0).
//          The two axes of z run as one float2: z's second fused multiply-add and each level's are one v_pk_fma_f32 for both axes
//          (the same correctly rounded results as two scalar ones), so a candidate is 1 + L / 2 packed fused multiply-adds, L minima
//          of the two scans, 3 additions and 2 minima: 3 L / 2 + 6 VALU operations by the source (30 at 256-QAM; the compiled row of
//          16 candidates is 544, 34 each, with the |comp| masks and moves) and 2 m + L live minima; no LDS.  The hard decision is
//          the sign of the stream's own LLRs (bit j is 1 iff Lambda_j < 0), counted against the sent Gray codes;
//        successive cancellation (link2_sic; linksim.py "the successive-cancellation link")  the order is per element, so step 4 is an
//          element loop around both streams, neither unrolled: still one copy of the linear detector's code.  f = g11 > g00 picks
//          the first stream; its stage is link2_linear's calls (link_sm_detect, decide, link_axis_llrs), so its LLRs and decisions
//          are the linear kernel's bits for that (element, stream).  The decided levels a_ki + j a_kq (link_level: link_sent's
//          expression) leave the other stream's matched sum by four fused multiply-adds (link_sic_cancel: c_o = m_o - gx x^,
//          p_o = g_oo), and the second stage is link_walk's measures on (c_o, p_o) with the group's scale: no regulariser, no
//          division, no second walk over the antennas.  The 2 M LLRs of an element are all that is live; a stream loop (rolled)
//          then routes them BY STREAM into the losses, the counts and the store (link_store_element_llrs: an element at a time),
//          so the decoders read the tensor as they read the other detectors'.  Three more integers per thread -- elements detected
//          in swapped order, first decisions with a symbol error, of those the ones whose other stream is wrong too -- are reduced
//          with the counts; no scratch;
//        codeword cancellation (link2_cancel; linksim.py "the codeword-cancellation link")  the second pass of a receiver that
//          cancels a stream only after its decoder has acknowledged it.  `failed` holds the first pass's block-error count per
//          (group, stream), read at a stride (the LDPC decoder's counts in place: counts + 1, stride 3); every thread forms
//          redo_s = failed_s != 0 && failed_other == 0 from two wave-uniform words, so AT MOST ONE stream of a group is detected
//          again.  A group without one skips the pilot lookup, the hashing and the antenna walk by a uniform branch and its pair
//          loop only stores zeros.  Otherwise stream t = the one with redo: the SENT symbol of the acknowledged stream (link_sent's
//          levels: an acknowledged codeword re-encodes to the sent bits) leaves m_t by link_sic_cancel's four fused multiply-adds,
//          and link_walk's measures run on (c_t, g_tt) with the group's scale -- link2_sic's second stage, call for call, with the
//          sent levels in the decided ones' place.  There is no stream loop: the detected stream's sums run in stream 0's registers
//          and change places with the zeros after the walk when it is stream 1.  The element's eight sums are COPIED (`e = s ? e1 :
//          e0`, as link2_sic's caller does): handed on as a reference to one of the two, both sets stayed in scratch, 68 bytes a
//          lane.  The other stream's counts, losses and LLRs are zeros; state[g][s] = redo_s;
//   5. per stream the two integer counts and the K float sums stay in registers and are reduced in link_walk's fixed order: shuffles
//      in the wave, then the four waves through LDS.
//
// No atomics and no workspace: a group's outputs depend neither on the batch, nor on its position in it, nor on the run, nor on the
// load or store form or the alignment of the bases, nor on whether the LLRs are stored.  Rounding: the build has no fast-math, and
// without it the compiler's default for HIP is a correctly rounded float32 division (-fhip-fp32-correctly-rounded-divide-sqrt), so
// the linear detector's `scale / a_other` is ONE rounding (the joint one has no division anywhere); every product is a fused
// multiply-add chain written as such, and the detectors and the soft pieces are compiled under `fp contract(off)`, so nothing is
// contracted behind the source.  Linear: with an unheard second stream (H_r1 = E_r1 = 0) and reg scale = 1 in powers of two, stream 0
// is link_mrc_kernel's output on the frames (r, 0), bit for bit.  Joint: the minima start at +infinity and every bit has candidates on
// both sides, so finite operands give finite LLRs; all-zero estimates give f = 0 for every candidate and LLRs of 0.
//
//   link_sm_kernel     (aft_link_sm_f32)     the linear ZF / MMSE detector
//   link_joint_kernel  (aft_link_joint_f32)  the joint max-log demapper
//   link_sic_kernel    (aft_link_sic_f32)    ordered successive cancellation: the linear detector, then a diversity stage
//   link_cancel_kernel (aft_link_cancel_f32) codeword cancellation: the acknowledged stream's sent symbol out, then a diversity stage
#include "link_device.h"

namespace aft {
namespace {

constexpr int kSmStreams = AFT_LINK_MAX_STREAMS;

// link_args' struct and, per group, the linear detector's regulariser: NULL, and never read, on the joint launch; the
// successive-cancellation launch's three integers per group, which may be NULL
struct Link2Args : LinkArgs {
    const float *reg;
    int *stats;
};

// what the codeword-cancellation launch adds: the first pass's block-error counts, failed[(g 2 + s) failed_stride], and the flags it
// forms from them, state [groups][2], which may be NULL.  Its own struct: the other three kernels' arguments stay as they are
struct LinkCancelArgs : Link2Args {
    const int *failed;
    int failed_stride;
    int *state;
};

// the detector of an instantiation's step 4
constexpr int kLinear = 0, kJoint = 1, kSic = 2, kCancel = 3;
constexpr int kSicStats = 3;

// Step 4, linear: the M LLRs of stream `second` of an element with the sums e into w -- I-axis bits first, MSB first, the order of the
// sent word --; returns the number of bits decided against the sent Gray codes gi, gq.  (The codes by value and w by pointer: with
// the sent word and the array by reference link_joint_kernel<2> takes 4 more VGPRs.)
template <int M>
__device__ __forceinline__ int link2_linear(float d, float d2, const LinkSm &e, float reg, float scale, bool second, unsigned gi,
                                            unsigned gq, float *w) {
    constexpr int half = M / 2, L = 1 << half;
    const LinkDetected m = link_sm_detect(e, reg, scale, second);
    const float step = d2 * m.p;
    const unsigned ki = decide<L>(m.cr, step), kq = decide<L>(m.ci, step);
    link_axis_llrs<L>(d, m.cr, m.p, m.eff, w);
    link_axis_llrs<L>(d, m.ci, m.p, m.eff, w + half);
    return __popc(gi ^ ki ^ (ki >> 1)) + __popc(gq ^ kq ^ (kq >> 1));
}

// Step 4, joint: the same results from link_joint_llrs; the decided Gray codes are the signs of the LLRs
template <int M>
__device__ __forceinline__ int link2_joint(float d, const LinkSm &e, float scale, bool second, unsigned gi, unsigned gq, float *w) {
    constexpr int half = M / 2;
    link_joint_llrs<M>(d, e, scale, second, w);
    unsigned hi = 0, hq = 0;                                    // bit j is 1 iff its LLR is negative
#pragma unroll
    for (int j = 0; j < half; ++j) {
        hi = (hi << 1) | (w[j] < 0.f ? 1u : 0u);
        hq = (hq << 1) | (w[half + j] < 0.f ? 1u : 0u);
    }
    return __popc(gi ^ hi) + __popc(gq ^ hq);
}

// Step 4, successive cancellation: BOTH streams of an element with the sums e, because the order is per element.  The first stage is
// link2_linear's calls on stream f (link_sm_detect, decide, link_axis_llrs) and keeps the decided levels; the second stage takes the
// decided symbol out of the other stream's matched sum (link_sic_cancel) and is link_walk's measures on (c_o, g_oo, scale).  wf and wo
// take the M LLRs of the first and of the second detected stream; returns their wrong bits against the sent Gray codes.
struct LinkSicWrong {
    int first, other;
};

template <int M>
__device__ __forceinline__ LinkSicWrong link2_sic(float d, float d2, const LinkSm &e, float reg, float scale, bool f, const LinkSent &xf,
                                                  const LinkSent &xo, float *wf, float *wo) {
    constexpr int half = M / 2, L = 1 << half;
    const LinkDetected m = link_sm_detect(e, reg, scale, f);
    const float step = d2 * m.p;
    const unsigned ki = decide<L>(m.cr, step), kq = decide<L>(m.ci, step);
    link_axis_llrs<L>(d, m.cr, m.p, m.eff, wf);
    link_axis_llrs<L>(d, m.ci, m.p, m.eff, wf + half);
    const LinkBranch c = link_sic_cancel(e, f, link_level<L>(d, ki), link_level<L>(d, kq));
    const float step2 = d2 * c.p;
    const unsigned oi = decide<L>(c.cr, step2), oq = decide<L>(c.ci, step2);
    link_axis_llrs<L>(d, c.cr, c.p, scale, wo);
    link_axis_llrs<L>(d, c.ci, c.p, scale, wo + half);
    const int first = __popc(xf.gi ^ ki ^ (ki >> 1)) + __popc(xf.gq ^ kq ^ (kq >> 1));
    const int other = __popc(xo.gi ^ oi ^ (oi >> 1)) + __popc(xo.gq ^ oq ^ (oq >> 1));
    return LinkSicWrong{first, other};
}

// Step 4, codeword cancellation: the M LLRs of stream `second` of an element with the sums e into w after the SENT symbol xr + j xi of
// the other stream has left its matched sum -- link2_sic's second stage with the sent levels --; returns the wrong bits against gi, gq
template <int M>
__device__ __forceinline__ int link2_cancel(float d, float d2, const LinkSm &e, float scale, bool second, float xr, float xi, unsigned gi,
                                            unsigned gq, float *w) {
    constexpr int half = M / 2, L = 1 << half;
    const LinkBranch c = link_sic_cancel(e, !second, xr, xi);
    const float step2 = d2 * c.p;
    const unsigned oi = decide<L>(c.cr, step2), oq = decide<L>(c.ci, step2);
    link_axis_llrs<L>(d, c.cr, c.p, scale, w);
    link_axis_llrs<L>(d, c.ci, c.p, scale, w + half);
    return __popc(gi ^ oi ^ (oi >> 1)) + __popc(gq ^ oq ^ (oq >> 1));
}

// One instantiation per modulation order and detector; Args is Link2Args, or LinkCancelArgs for the codeword-cancellation detector
template <int M, int Det, class Args>
__device__ __forceinline__ void link2_walk(const Args &a) {
    constexpr bool Joint = Det == kJoint;
    constexpr int kCounts = kSmStreams * 2 + (Det == kSic ? kSicStats : 0);
    __shared__ int psc[AFT_CHANSIM_MAX_PILOT_SCS], psym[AFT_CHANSIM_MAX_PILOT_SYMBOLS];
    __shared__ unsigned long long bkey[AFT_LINK_MAX_BRANCHES];
    __shared__ float bsigma[AFT_LINK_MAX_BRANCHES], brho[AFT_LINK_MAX_BRANCHES];
    __shared__ float part[kLinkWaves][kSmStreams * kMaxFactors];
    __shared__ int ipart[kLinkWaves][kCounts];
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
    const float scale = a.scale[g];
    float reg = 0.f;
    if constexpr (Det == kLinear || Det == kSic) reg = a.reg[g];
    bool redo0 = false, redo1 = false;                          // codeword cancellation: wave-uniform, at most one of them set
    if constexpr (Det == kCancel) {
        AFT_DEV_ASSERT(a.failed_stride >= 1);
        const size_t at = g * (size_t)kSmStreams * (size_t)a.failed_stride;
        const int f0 = __builtin_amdgcn_readfirstlane(a.failed[at]), f1 = __builtin_amdgcn_readfirstlane(a.failed[at + (size_t)a.failed_stride]);
        redo0 = f0 != 0 && f1 == 0;
        redo1 = f1 != 0 && f0 == 0;
    }
    const bool go = Det != kCancel || redo0 || redo1;           // a constant for the other detectors
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
    int swapped = 0, first_wrong = 0, both_wrong = 0;           // the successive-cancellation launch's three integers
    const unsigned pairs = (last >> 1) + 1;                     // the last pair of an odd grid holds one element
    for (unsigned i = tid; i < pairs; i += kFrameThreads) {      // pairs <= 2^30: the index cannot wrap
        const unsigned q = 2 * i;
        const bool two = q < last;
        AFT_DEV_ASSERT(q <= last && (two || !a.wide));
        const bool d0 = go && link_is_data(psc, Ps, psym, Pt, T, q), d1 = go && two && link_is_data(psc, Ps, psym, Pt, T, q + 1);
        const LinkSent none{0u, 0u, 0.f, 0.f};
        LinkSent s00 = none, s01 = none, s10 = none, s11 = none;     // s<stream><element>
        if (d0) { s00 = link_sent<M>(a.d, k0, q); s10 = link_sent<M>(a.d, k1, q); }
        if (d1) { s01 = link_sent<M>(a.d, k0, q + 1); s11 = link_sent<M>(a.d, k1, q + 1); }
        const LinkSm zero{-0.f, -0.f, -0.f, -0.f, -0.f, -0.f, -0.f, -0.f};      // x + (-0) = x for every x
        LinkSm e0 = zero, e1 = zero;                            // the sums of elements q and q + 1
#pragma unroll 1
        for (int r = 0; r < (go ? R : 0); ++r) {
            LinkPair h0{}, g0{}, h1{}, g1{};                    // H and E of the pairs (r, 0) and (r, 1)
            const size_t at = (size_t)(kSmStreams * r) * frame + q;
            link_load_pairs(hp + at, ep + at, a.wide, two, h0, g0);
            link_load_pairs(hp + at + frame, ep + at + frame, a.wide, two, h1, g1);
            const unsigned long long kf = bkey[r];
            const float sr = bsigma[r], rho = brho[r];
            if (d0) link_sm_accumulate(e0, rho, link_sample2(kf, sr, q, s00, s10, h0.a, h1.a), g0.a, g1.a);
            if (d1) link_sm_accumulate(e1, rho, link_sample2(kf, sr, q + 1, s01, s11, h0.b, h1.b), g0.b, g1.b);
        }
        if constexpr (Det == kSic) {
#pragma unroll 1
            for (int s = 0; s < 2; ++s) {                       // the element; both streams inside: one copy of the two stages
                if (!(s == 0 || two)) break;
                const bool data = s ? d1 : d0;
                float wf[M], wo[M];
#pragma unroll
                for (int j = 0; j < M; ++j) wf[j] = wo[j] = 0.f;     // what a pilot position carries
                bool f = false;
                LinkSicWrong wrong{0, 0};
                if (data) {
                    const LinkSm e = s ? e1 : e0;
                    f = link_sic_second_first(e);
                    const LinkSent x0 = s ? s01 : s00, x1 = s ? s11 : s10;
                    wrong = link2_sic<M>(a.d, a.d2, e, reg, scale, f, f ? x1 : x0, f ? x0 : x1, wf, wo);
                    swapped += f ? 1 : 0;
                    first_wrong += wrong.first != 0 ? 1 : 0;
                    both_wrong += wrong.first != 0 && wrong.other != 0 ? 1 : 0;
                }
#pragma unroll 1
                for (int t = 0; t < kSmStreams; ++t) {          // by STREAM, not by detection order: the decoders' layout
                    const bool is_first = (t != 0) == f;
                    float w[M];
#pragma unroll
                    for (int j = 0; j < M; ++j) w[j] = is_first ? wf[j] : wo[j];
                    if (data) {
                        const LinkSent x = t ? (s ? s11 : s10) : (s ? s01 : s00);
                        const int wr = is_first ? wrong.first : wrong.other;
                        float acc[kMaxFactors];
#pragma unroll
                        for (int k = 0; k < kMaxFactors; ++k) acc[k] = t ? acc1[k] : acc0[k];
                        link_soft_losses<M>(w, x.gi, x.gq, fac, nf, acc);
#pragma unroll
                        for (int k = 0; k < kMaxFactors; ++k) {
                            if (t) acc1[k] = acc[k];
                            else acc0[k] = acc[k];
                        }
                        if (t) { bits1 += wr; symbols1 += wr != 0 ? 1 : 0; }
                        else { bits0 += wr; symbols0 += wr != 0 ? 1 : 0; }
                    }
                    if (lp != nullptr) link_store_element_llrs<M>(lp + ((size_t)t * frame + q + s) * M, w, a.store);
                }
            }
        } else if constexpr (Det == kCancel) {
            // at most one stream of the group is detected again: stream 1 iff redo1 (wave-uniform).  Its sums run in acc0, bits0 and
            // symbols0 whichever stream it is -- they change places with the other stream's zeros after the walk --, and the other
            // stream stores zeros.  Without a redo d0 and d1 are false: nothing is detected and both streams store zeros
            float v[2 * M], none[2 * M];
#pragma unroll
            for (int j = 0; j < 2 * M; ++j) v[j] = none[j] = 0.f;   // what a pilot position and a stream without redo carry
#pragma unroll 1
            for (int s = 0; s < 2; ++s) {                       // the element: one copy of the detector
                if (s ? d1 : d0) {
                    const LinkSent x0 = s ? s01 : s00, x1 = s ? s11 : s10;
                    const LinkSent x = redo1 ? x1 : x0, xo = redo1 ? x0 : x1;
                    const LinkSm e = s ? e1 : e0;
                    float w[M];
                    const int wrong = link2_cancel<M>(a.d, a.d2, e, scale, redo1, xo.xr, xo.xi, x.gi, x.gq, w);
                    bits0 += wrong;
                    symbols0 += wrong != 0 ? 1 : 0;
                    link_soft_losses<M>(w, x.gi, x.gq, fac, nf, acc0);
#pragma unroll
                    for (int j = 0; j < M; ++j) {
                        if (s) v[M + j] = w[j];
                        else v[j] = w[j];
                    }
                }
            }
            if (lp != nullptr) {
                const size_t again = redo1 ? 1 : 0;
                link_store_llrs<M>(lp + (again * frame + q) * M, v, two ? 2 * M : M, a.store);
                link_store_llrs<M>(lp + ((1 - again) * frame + q) * M, none, two ? 2 * M : M, a.store);
            }
        } else {
#pragma unroll 1
            for (int t = 0; t < kSmStreams; ++t) {              // the stream; the element inside: one copy of the detector
                float v[2 * M], acc[kMaxFactors];
#pragma unroll
                for (int j = 0; j < 2 * M; ++j) v[j] = 0.f;     // what a pilot position carries
#pragma unroll
                for (int k = 0; k < kMaxFactors; ++k) acc[k] = t ? acc1[k] : acc0[k];
                int bits = 0, symbols = 0;
#pragma unroll 1
                for (int s = 0; s < 2; ++s) {
                    if (s ? d1 : d0) {
                        const LinkSent x = t ? (s ? s11 : s10) : (s ? s01 : s00);
                        float w[M];
                        int wrong;
                        if constexpr (Joint) wrong = link2_joint<M>(a.d, s ? e1 : e0, scale, t != 0, x.gi, x.gq, w);
                        else wrong = link2_linear<M>(a.d, a.d2, s ? e1 : e0, reg, scale, t != 0, x.gi, x.gq, w);
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
    }
    if constexpr (Det == kCancel) {
        if (redo1) {                                            // wave-uniform: the sums are stream 1's, stream 0's are the zeros
            bits1 = bits0; symbols1 = symbols0;
            bits0 = symbols0 = 0;
#pragma unroll
            for (int k = 0; k < kMaxFactors; ++k) {
                acc1[k] = acc0[k];
                acc0[k] = 0.f;
            }
        }
    }
    link_wave_sum(bits0, tid, ipart, 0);
    link_wave_sum(symbols0, tid, ipart, 1);
    link_wave_sum(bits1, tid, ipart, 2);
    link_wave_sum(symbols1, tid, ipart, 3);
    if constexpr (Det == kSic) {
        link_wave_sum(swapped, tid, ipart, 4);
        link_wave_sum(first_wrong, tid, ipart, 5);
        link_wave_sum(both_wrong, tid, ipart, 6);
    }
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
    if constexpr (Det == kSic) {                                // the third wave: swapped order, first-decision errors, propagated errors
        if (a.stats != nullptr && tid >= 2 * kWave && tid < 2 * kWave + kSicStats)
            a.stats[kSicStats * g + (tid - 2 * kWave)] = link_block_sum(ipart, 2 * kSmStreams + (tid - 2 * kWave));
    }
    if constexpr (Det == kCancel) {                             // the third wave: the two flags
        if (a.state != nullptr && tid >= 2 * kWave && tid < 2 * kWave + kSmStreams)
            a.state[kSmStreams * g + (tid - 2 * kWave)] = (tid - 2 * kWave ? redo1 : redo0) ? 1 : 0;
    }
}

template <int M>
__global__ __launch_bounds__(kFrameThreads) void link_sm_kernel(const Link2Args a) {
    link2_walk<M, kLinear>(a);
}

template <int M>
__global__ __launch_bounds__(kFrameThreads) void link_joint_kernel(const Link2Args a) {
    link2_walk<M, kJoint>(a);
}

template <int M>
__global__ __launch_bounds__(kFrameThreads) void link_sic_kernel(const Link2Args a) {
    link2_walk<M, kSic>(a);
}

template <int M>
__global__ __launch_bounds__(kFrameThreads) void link_cancel_kernel(const LinkCancelArgs a) {
    link2_walk<M, kCancel>(a);
}

}  // namespace

hipError_t launch_link2(bool joint, const aft_link &link, const float *ideal, const float *est, const unsigned long long *keys,
                        const float *sigma, const float *rho, const float *scale, const float *reg, const float *factors, int n_factors,
                        int branches, int32_t *counts, float *loss, float *llr, int batch, hipStream_t st) {
    const Link2Args a{link_args(link, ideal, est, keys, sigma, rho, scale, factors, n_factors, branches, counts, loss, llr), reg, nullptr};
    const dim3 grid((unsigned)(batch / (branches * kSmStreams)));
    return link_dispatch(link.bits_per_symbol, [&](auto m) {
        if (joint) hipLaunchKernelGGL(link_joint_kernel<decltype(m)::value>, grid, dim3(kFrameThreads), 0, st, a);
        else hipLaunchKernelGGL(link_sm_kernel<decltype(m)::value>, grid, dim3(kFrameThreads), 0, st, a);
    });
}

hipError_t launch_link_sic(const aft_link &link, const float *ideal, const float *est, const unsigned long long *keys,
                           const float *sigma, const float *rho, const float *scale, const float *reg, const float *factors, int n_factors,
                           int branches, int32_t *counts, float *loss, float *llr, int32_t *stats, int batch, hipStream_t st) {
    Link2Args a{link_args(link, ideal, est, keys, sigma, rho, scale, factors, n_factors, branches, counts, loss, llr), reg, stats};
    a.store = link_llr_element_store_bytes(llr, link.bits_per_symbol);      // an element's LLRs leave on their own: the order is per element
    const dim3 grid((unsigned)(batch / (branches * kSmStreams)));
    return link_dispatch(link.bits_per_symbol, [&](auto m) {
        hipLaunchKernelGGL(link_sic_kernel<decltype(m)::value>, grid, dim3(kFrameThreads), 0, st, a);
    });
}

hipError_t launch_link_cancel(const aft_link &link, const float *ideal, const float *est, const unsigned long long *keys,
                              const float *sigma, const float *rho, const float *scale, const float *factors, int n_factors, int branches,
                              const int32_t *failed, int failed_stride, int32_t *counts, float *loss, float *llr, int32_t *state,
                              int batch, hipStream_t st) {
    const LinkCancelArgs a{{link_args(link, ideal, est, keys, sigma, rho, scale, factors, n_factors, branches, counts, loss, llr), nullptr,
                            nullptr}, failed, failed_stride, state};
    const dim3 grid((unsigned)(batch / (branches * kSmStreams)));
    return link_dispatch(link.bits_per_symbol, [&](auto m) {
        hipLaunchKernelGGL(link_cancel_kernel<decltype(m)::value>, grid, dim3(kFrameThreads), 0, st, a);
    });
}

}  // namespace aft
