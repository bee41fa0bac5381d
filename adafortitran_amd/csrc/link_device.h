// What the link front end is made of (k_link.hip), each piece written once, so every instantiation sees the same bits: the pilot staging
// and lookup, the pair loads, the Gray map, the hard decision, the front of a data element -- split into the sent word (one per
// transmission) and a branch (one per receive antenna: y = H x + noise, c = y conj(E), p = |E|^2) --, the combiner's step, an axis's
// max-log LLRs, the softplus step of the loss, the LLR store, the reduction of a workgroup's sums and, on the host, a launch's
// arguments and its dispatch on the modulation order; and what two-stream detection (k_linksm.hip) adds to them: the two-stream
// received sample, the Gram / matched sums, the adjugate detector with its LLR scale, the order, the decided level and the cancellation
// of the successive-cancellation detector and the joint max-log demapper; and what transmit
// diversity (k_linkalamouti.hip) adds: a line's k-th data element, the Alamouti combiner's step and the store of one element's LLRs;
// and what closed-loop precoding (k_linkprecode.hip) adds: the exact product with a codebook entry, a subband's selection sum and its
// decision, and the combiner's step on the effective estimate; and what the decision-directed observation (k_linkobserve.hip) adds:
// the received sample on its own (link_received, which link_branch is built on), one plane's pair load and a pilot's place in its list.
// adafortitran_amd/linksim.py holds the definitions.
#pragma once

#include <type_traits>

#include "frame_device.h"

namespace aft {
namespace {

constexpr int kLinkWaves = kFrameThreads / kWave;

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

// The pilot positions to LDS: the first wave the columns' list (at most 64), the second the rows' (at most 16).  The caller syncs.
__device__ __forceinline__ void link_stage_pilots(const aft_link &c, int tid, int *psc, int *psym) {
    AFT_DEV_ASSERT(c.pilot_scs >= 1 && c.pilot_scs <= AFT_CHANSIM_MAX_PILOT_SCS && c.pilot_symbols >= 1 &&
                   c.pilot_symbols <= AFT_CHANSIM_MAX_PILOT_SYMBOLS);
    if (tid < c.pilot_scs) psc[tid] = c.pilot_sc_index[tid];
    if (tid >= kWave && tid - kWave < c.pilot_symbols) psym[tid - kWave] = c.pilot_symbol_index[tid - kWave];
}

// element q = s T + t is not a pilot position: two binary searches, the row's only when the column hit
__device__ __forceinline__ bool link_is_data(const int *psc, int Ps, const int *psym, int Pt, unsigned T, unsigned q) {
    const unsigned s = q / T, t = q - s * T;
    return !(link_listed(psym, Pt, (int)t) && link_listed(psc, Ps, (int)s));
}

// The elements (q, q + 1) of a frame's H and E, hq and eq their element q: one 16-byte load each when `wide` (T even -- a pair never
// straddles a row -- and both bases 16-byte aligned), one 8-byte load per element otherwise; the lone last element of an odd grid
// (`two` false) leaves b zero.  One branch for both planes, so their loads issue together.
struct LinkPair {
    float2 a, b;
};

__device__ __forceinline__ void link_load_pairs(const float2 *hq, const float2 *eq, int wide, bool two, LinkPair &h, LinkPair &e) {
    if (wide) {
        const f32x4 hv = *reinterpret_cast<const f32x4 *>(hq), ev = *reinterpret_cast<const f32x4 *>(eq);
        h = LinkPair{make_float2(hv[0], hv[1]), make_float2(hv[2], hv[3])};
        e = LinkPair{make_float2(ev[0], ev[1]), make_float2(ev[2], ev[3])};
    } else {
        h.a = hq[0]; e.a = eq[0];
        h.b = e.b = make_float2(0.f, 0.f);
        if (two) { h.b = hq[1]; e.b = eq[1]; }
    }
}

// the elements (q, q + 1) of ONE plane, by link_load_pairs' rules
__device__ __forceinline__ LinkPair link_load_pair(const float2 *hq, int wide, bool two) {
    if (wide) {
        const f32x4 hv = *reinterpret_cast<const f32x4 *>(hq);
        return LinkPair{make_float2(hv[0], hv[1]), make_float2(hv[2], hv[3])};
    }
    return LinkPair{hq[0], two ? hq[1] : make_float2(0.f, 0.f)};
}

// the index of v in sorted[0 .. n), or -1: link_listed's search, for a caller that needs the place as well
__device__ __forceinline__ int link_position(const int *sorted, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sorted[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && sorted[lo] == v ? lo : -1;
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

// The sent word of a data element: one word of the counter-based hash of the transmission's key, its two Gray codes and the symbol
// x = xr + j xi.  M = bits per symbol.
struct LinkSent {
    unsigned gi, gq;            // the sent Gray codes of the I and the Q axis
    float xr, xi;
};

template <int M>
__device__ __forceinline__ LinkSent link_sent(float d, unsigned long long kf, unsigned q) {
    constexpr int half = M / 2, L = 1 << half;
    const unsigned w = (unsigned)(frame_word(kf, kStreamDataBits, q) >> (64 - M));
    const unsigned gi = w >> half, gq = w & (unsigned)(L - 1);
    const float xr = d * (float)(2 * (int)gray_level(gi) - (L - 1)), xi = d * (float)(2 * (int)gray_level(gq) - (L - 1));
    return LinkSent{gi, gq, xr, xi};
}

// One receive branch of a data element: the two noise words of the branch's own key, y = H x + noise, c = y conj(E) and p = |E|^2
struct LinkBranch {
    float cr, ci, p;
};

// the branch's received sample alone, y = H x + noise: link_branch's own first step, for a caller that also needs y (k_linkobserve.hip)
struct LinkReceived {
    float yr, yi;
};

__device__ __forceinline__ LinkReceived link_received(unsigned long long kf, float sigma, unsigned q, float xr, float xi, float2 h) {
    const FrameNoise nz = frame_noise(kf, kStreamDataNoiseRadius, kStreamDataNoiseAngle, q, sigma);
    return LinkReceived{fmaf(nz.r, nz.c, fmaf(h.x, xr, -(h.y * xi))), fmaf(nz.r, nz.s, fmaf(h.x, xi, h.y * xr))};
}

// ... and the branch from a sample already formed: c = y conj(E), p = |E|^2, link_branch's second step
__device__ __forceinline__ LinkBranch link_branch_of(const LinkReceived &y, float2 e) {
    const float yr = y.yr, yi = y.yi;
    const float cr = fmaf(yr, e.x, yi * e.y);                   // y conj(E)
    const float ci = fmaf(yi, e.x, -(yr * e.y));
    return LinkBranch{cr, ci, fmaf(e.x, e.x, e.y * e.y)};
}

__device__ __forceinline__ LinkBranch link_branch(unsigned long long kf, float sigma, unsigned q, float xr, float xi, float2 h, float2 e) {
    return link_branch_of(link_received(kf, sigma, q, xr, xi, h), e);
}

// The combiner's step: c += rho c_r, p += rho p_r, one fused multiply-add each, the product exact inside it
__device__ __forceinline__ void link_combine(LinkBranch &sum, float rho, const LinkBranch &b) {
    sum.cr = fmaf(rho, b.cr, sum.cr);
    sum.ci = fmaf(rho, b.ci, sum.ci);
    sum.p = fmaf(rho, b.p, sum.p);
}

// ---- two-stream spatial multiplexing (k_linksm.hip; linksim.py "the spatial-multiplexing link") ----

// The received sample of one antenna under two streams, y = H0 x0 + H1 x1 + noise, with the noise words of the antenna's own key.
// Stream 0's product is link_branch's own chain; stream 1's two products are added by fused multiply-adds and the noise last, so with
// H1 = 0 the sample is link_branch's bit for bit.
struct LinkSample {
    float yr, yi;
};

__device__ __forceinline__ LinkSample link_sample2(unsigned long long kf, float sigma, unsigned q, const LinkSent &x0, const LinkSent &x1,
                                                   float2 h0, float2 h1) {
    const FrameNoise nz = frame_noise(kf, kStreamDataNoiseRadius, kStreamDataNoiseAngle, q, sigma);
    float tr = fmaf(h0.x, x0.xr, -(h0.y * x0.xi));
    float ti = fmaf(h0.x, x0.xi, h0.y * x0.xr);
    tr = fmaf(-h1.y, x1.xi, fmaf(h1.x, x1.xr, tr));
    ti = fmaf(h1.y, x1.xr, fmaf(h1.x, x1.xi, ti));
    return LinkSample{fmaf(nz.r, nz.c, tr), fmaf(nz.r, nz.s, ti)};
}

// An element's eight sums over the antennas: the matched filters m_s = sum rho conj(E_s) y and the Gram matrix g00, g11, g01 = sum rho
// conj(E_0) E_1.  Each term is link_branch's y conj(E) / |E|^2 chain and enters by one fused multiply-add, as link_combine's; the
// sums start at -0.
struct LinkSm {
    float m0r, m0i, m1r, m1i, g00, g11, g01r, g01i;
};

__device__ __forceinline__ void link_sm_accumulate(LinkSm &a, float rho, const LinkSample &y, float2 e0, float2 e1) {
    a.m0r = fmaf(rho, fmaf(y.yr, e0.x, y.yi * e0.y), a.m0r);
    a.m0i = fmaf(rho, fmaf(y.yi, e0.x, -(y.yr * e0.y)), a.m0i);
    a.m1r = fmaf(rho, fmaf(y.yr, e1.x, y.yi * e1.y), a.m1r);
    a.m1i = fmaf(rho, fmaf(y.yi, e1.x, -(y.yr * e1.y)), a.m1i);
    a.g00 = fmaf(rho, fmaf(e0.x, e0.x, e0.y * e0.y), a.g00);
    a.g11 = fmaf(rho, fmaf(e1.x, e1.x, e1.y * e1.y), a.g11);
    a.g01r = fmaf(rho, fmaf(e0.x, e1.x, e0.y * e1.y), a.g01r);
    a.g01i = fmaf(rho, fmaf(e0.x, e1.y, -(e0.y * e1.x)), a.g01i);
}

// The adjugate detector of one stream: c = a_other m_self - gx m_other with gx = g01 for stream 0 and conj(g01) for stream 1,
// p = g_self a_other - |g01|^2, and the LLR scale eff = scale / a_other (one correctly rounded division; 0 where a_other <= 0).
// One body for both streams (`second` picks the roles), two roundings per product pair, nothing contracted behind the source's back.
struct LinkDetected {
    float cr, ci, p, eff;
};

__device__ __forceinline__ LinkDetected link_sm_detect(const LinkSm &a, float reg, float scale, bool second) {
#pragma clang fp contract(off)
    const float a00 = a.g00 + reg, a11 = a.g11 + reg;
    const float ao = second ? a00 : a11, gs = second ? a.g11 : a.g00;
    const float msr = second ? a.m1r : a.m0r, msi = second ? a.m1i : a.m0i;
    const float mor = second ? a.m0r : a.m1r, moi = second ? a.m0i : a.m1i;
    const float gxr = a.g01r, gxi = second ? -a.g01i : a.g01i;
    const float tr = fmaf(gxr, mor, -(gxi * moi)), ti = fmaf(gxr, moi, gxi * mor);      // gx m_other
    const float n01 = fmaf(a.g01r, a.g01r, a.g01i * a.g01i);
    return LinkDetected{fmaf(ao, msr, -tr), fmaf(ao, msi, -ti), fmaf(gs, ao, -n01), ao > 0.f ? scale / ao : 0.f};
}

// ---- successive cancellation of the two streams (k_linksm.hip; linksim.py "the successive-cancellation link") ----

// The detection order of an element: true iff stream 1 is detected first, g11 > g00 (a tie and NaN give stream 0).  This is the order
// of the linear detector's post-detection SINRs for every reg >= 0: p_0 a00 - p_1 a11 = (g00 - g11) det(A).
__device__ __forceinline__ bool link_sic_second_first(const LinkSm &a) {
    return a.g11 > a.g00;
}

// The level a_k = d (2 k - (L - 1)) of a decided index, by link_sent's expression: a correct decision is the very float32 that was sent
template <int L>
__device__ __forceinline__ float link_level(float d, unsigned k) {
    return d * (float)(2 * (int)k - (L - 1));
}

// The second stage's operands: the decided symbol xr + j xi of the first stream taken out of the other stream's matched sum,
// c_o = m_o - gx x^ with gx = g01 when the other stream is 0 (`second_first`) and conj(g01) when it is 1, two fused multiply-adds per
// component, the x^.im term first; p_o = g_oo, the diversity link's p: no regulariser, no division.
__device__ __forceinline__ LinkBranch link_sic_cancel(const LinkSm &a, bool second_first, float xr, float xi) {
#pragma clang fp contract(off)
    const float mor = second_first ? a.m0r : a.m1r, moi = second_first ? a.m0i : a.m1i;
    const float gxr = a.g01r, gxi = second_first ? a.g01i : -a.g01i;
    return LinkBranch{fmaf(-gxr, xr, fmaf(gxi, xi, mor)), fmaf(-gxr, xi, fmaf(-gxi, xr, moi)), second_first ? a.g00 : a.g11};
}

// ---- joint max-log detection of the two streams (k_linksm.hip; linksim.py "the joint link") ----

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

// ---- transmit diversity: Alamouti pairs over time or frequency (k_linkalamouti.hip; linksim.py "the transmit-diversity link") ----

// The position in its line of the line's k-th data element, k from 0: `pilots` is the sorted list of the line's n pilot positions
// (n = 0: a line without pilots, position k); every pilot at or below the running position moves it one on.  k is below the line's
// number of data elements, so the result is inside the line.
__device__ __forceinline__ unsigned link_line_data(const int *pilots, int n, unsigned k) {
    unsigned pos = k;
    for (int i = 0; i < n && (unsigned)pilots[i] <= pos; ++i) ++pos;
    return pos;
}

// y conj(E), link_branch's chain of a product and a fused multiply-add per component; E conj(y) is its conjugate
struct LinkTerm {
    float r, i;
};

__device__ __forceinline__ LinkTerm link_matched(const LinkSample &y, float2 e) {
    return LinkTerm{fmaf(y.yr, e.x, y.yi * e.y), fmaf(y.yi, e.x, -(y.yr * e.y))};
}

__device__ __forceinline__ float link_norm(float2 e) {
    return fmaf(e.x, e.x, e.y * e.y);
}

// One antenna's share of the six sums of a pair (a, b) from its samples y[a], y[b] and its estimates E_r0, E_r1 at a and at b:
//   c_a += rho (conj(E_r0[a]) y[a] + E_r1[b] conj(y[b])),  p_a += rho (|E_r0[a]|^2 + |E_r1[b]|^2)
//   c_b += rho (conj(E_r1[a]) y[a] - E_r0[b] conj(y[b])),  p_b += rho (|E_r1[a]|^2 + |E_r0[b]|^2)
// the term at a before the term at b, one fused multiply-add per term as link_combine's; negation and conjugation are exact.  A lone
// element is the pair with y[b] = E_r1[a] = E_r0[b] = E_r1[b] = 0: its c_a and p_a are link_combine's of link_branch on the frame (r, 0).
__device__ __forceinline__ void link_alamouti_accumulate(LinkBranch &ma, LinkBranch &mb, float rho, const LinkSample &ya,
                                                         const LinkSample &yb, float2 e0a, float2 e1a, float2 e0b, float2 e1b) {
#pragma clang fp contract(off)
    const LinkTerm a0 = link_matched(ya, e0a), a1 = link_matched(ya, e1a);      // conj(E_r0[a]) y[a], conj(E_r1[a]) y[a]
    const LinkTerm b0 = link_matched(yb, e0b), b1 = link_matched(yb, e1b);      // the conjugates of E_r0[b] conj(y[b]), E_r1[b] conj(y[b])
    ma.cr = fmaf(rho, b1.r, fmaf(rho, a0.r, ma.cr));
    ma.ci = fmaf(rho, -b1.i, fmaf(rho, a0.i, ma.ci));
    ma.p = fmaf(rho, link_norm(e1b), fmaf(rho, link_norm(e0a), ma.p));
    mb.cr = fmaf(rho, -b0.r, fmaf(rho, a1.r, mb.cr));
    mb.ci = fmaf(rho, b0.i, fmaf(rho, a1.i, mb.ci));
    mb.p = fmaf(rho, link_norm(e0b), fmaf(rho, link_norm(e1a), mb.p));
}

// ---- closed-loop precoding: a codebook precoder per subband (k_linkprecode.hip; linksim.py "the closed-loop link") ----

// q_i z for the codebook q_0 .. q_3 = 1, -1, j, -j: a swap and negations, exact
__device__ __forceinline__ float2 link_mul_q(int i, float2 z) {
    const float2 t = (i & 2) ? make_float2(-z.y, z.x) : z;      // j z
    return (i & 1) ? make_float2(-t.x, -t.y) : t;
}

// One (element, antenna) term of a subband's sum g += rho conj(E_r0) E_r1: the product is link_sm_accumulate's g01 chain, and it
// enters by one fused multiply-add per component
__device__ __forceinline__ void link_pmi_accumulate(float &gr, float &gi, float rho, float2 e0, float2 e1) {
    gr = fmaf(rho, fmaf(e0.x, e1.x, e0.y * e1.y), gr);
    gi = fmaf(rho, fmaf(e0.x, e1.y, -(e0.y * e1.x)), gi);
}

// The precoder of a subband from its sum g: the LOWEST index i that attains the maximum of v_i = Re(q_i g) = (Re g, -Re g, -Im g,
// Im g); g = 0 gives 0
__device__ __forceinline__ int link_pmi(float gr, float gi) {
    const float v[4] = {gr, -gr, -gi, gi};
    int best = 0;
    float top = v[0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (v[i] > top) { top = v[i]; best = i; }
    return best;
}

// One antenna's share of the combiner's sums under the precoder q: with the effective estimate e = E_r0 + qE_r1 (qe1 = q E_r1 is
// exact, the sum is one rounding per component), c += rho y conj(e) and p += rho |e|^2: link_branch's chain per term, link_combine's
// fused multiply-add per sum.  With E_r1 = 0 it is link_combine of link_branch on the frame (r, 0).
__device__ __forceinline__ void link_precoded_accumulate(LinkBranch &m, float rho, const LinkSample &y, float2 e0, float2 qe1) {
#pragma clang fp contract(off)
    const float2 e = make_float2(e0.x + qe1.x, e0.y + qe1.y);
    const LinkTerm t = link_matched(y, e);
    link_combine(m, rho, LinkBranch{t.r, t.i, link_norm(e)});
}

// ---- the soft half: max-log LLRs and the loss the achievable rate is read from (linksim.py "the soft link") ----

constexpr int kMaxFactors = 8;
constexpr float kInvLn2 = 1.44269504088896341f;

// One axis: the L metrics mu_k = a_k (a_k p - 2 comp) in registers, and per bit of the Gray code (MSB first) the scaled difference of
// the two minima.  Two roundings per metric (the fused multiply-add and the product) and nothing contracted behind the source's back.
template <int L>
__device__ __forceinline__ void link_axis_llrs(float d, float comp, float p, float scale, float *out) {
#pragma clang fp contract(off)
    constexpr int half = L == 2 ? 1 : L == 4 ? 2 : L == 8 ? 3 : 4;
    const float m2c = -2.f * comp;
    float mu[L];
#pragma unroll
    for (int k = 0; k < L; ++k) {
        const float ak = d * (float)(2 * k - (L - 1));
        mu[k] = ak * fmaf(ak, p, m2c);
    }
#pragma unroll
    for (int j = 0; j < half; ++j) {
        float m0 = 0.f, m1 = 0.f;
        bool have0 = false, have1 = false;                      // constants once the loop over k is unrolled
#pragma unroll
        for (int k = 0; k < L; ++k) {
            if (((k ^ (k >> 1)) >> (half - 1 - j)) & 1) {
                m1 = have1 ? fminf(m1, mu[k]) : mu[k];
                have1 = true;
            } else {
                m0 = have0 ? fminf(m0, mu[k]) : mu[k];
                have0 = true;
            }
        }
        out[j] = scale * (m1 - m0);
    }
}

// The softplus step: for each of the n_factors factors, the sum over an element's M LLRs v (I-axis bits first, MSB first: the order of
// the sent word) of softplus(z) = max(z, 0) + log1p(exp(-|z|)) in nats, z = -(1 - 2 b) factor Lambda with b the sent bit.
template <int M>
__device__ __forceinline__ void link_soft_losses(const float *v, unsigned gi, unsigned gq, const float (&fac)[kMaxFactors], int n_factors,
                                                 float (&acc)[kMaxFactors]) {
#pragma clang fp contract(off)
    constexpr int half = M / 2;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const unsigned sent = ((j < half ? gi : gq) >> (half - 1 - j % half)) & 1u;
        const float against = sent ? v[j] : -v[j];              // -(1 - 2 b) Lambda
#pragma unroll
        for (int k = 0; k < kMaxFactors; ++k)
            if (k < n_factors) {
                const float z = fac[k] * against;
                acc[k] += fmaxf(z, 0.f) + log1pf(expf(-fabsf(z)));
            }
    }
}

// the n leading floats of v (n = M or 2 M, a multiple of the store's width) to dst
template <int M>
__device__ __forceinline__ void link_store_llrs(float *dst, const float *v, int n, int bytes) {
    if (bytes == 16) {
#pragma unroll
        for (int j = 0; j < 2 * M; j += 4)
            if (j < n) *reinterpret_cast<f32x4 *>(dst + j) = f32x4{v[j], v[j + 1], v[j + 2], v[j + 3]};
    } else if (bytes == 8) {
#pragma unroll
        for (int j = 0; j < 2 * M; j += 2)
            if (j < n) *reinterpret_cast<float2 *>(dst + j) = make_float2(v[j], v[j + 1]);
    } else {
#pragma unroll
        for (int j = 0; j < 2 * M; ++j)
            if (j < n) dst[j] = v[j];
    }
}

// ONE element's M floats w to dst, for a walk that does not visit the elements in the pairs (2 i, 2 i + 1): `bytes` is
// link_llr_element_store_bytes', 16 only where M is a multiple of 4
template <int M>
__device__ __forceinline__ void link_store_element_llrs(float *dst, const float (&w)[M], int bytes) {
    if (M % 4 == 0 && bytes == 16) {
#pragma unroll
        for (int j = 0; j + 3 < M; j += 4) *reinterpret_cast<f32x4 *>(dst + j) = f32x4{w[j], w[j + 1], w[j + 2], w[j + 3]};
    } else if (bytes >= 8) {
#pragma unroll
        for (int j = 0; j < M; j += 2) *reinterpret_cast<float2 *>(dst + j) = make_float2(w[j], w[j + 1]);
    } else {
#pragma unroll
        for (int j = 0; j < M; ++j) dst[j] = w[j];
    }
}

// A workgroup's sum of one value per thread, in a fixed order: the wave by shuffles (kWave / 2 down to 1), whose result lane 0 leaves in
// part[wave][slot] ...
template <class T, int N>
__device__ __forceinline__ void link_wave_sum(T v, int tid, T (*part)[N], int slot) {
#pragma unroll
    for (int o = kWave / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if ((tid & (kWave - 1)) == 0) part[tid / kWave][slot] = v;
}

// ... and, after a barrier, the four waves in index order
template <class T, int N>
__device__ __forceinline__ T link_block_sum(const T (*part)[N], int slot) {
    T total = part[0][slot];
#pragma unroll
    for (int w = 1; w < kLinkWaves; ++w) total += part[w][slot];
    return total;
}

// bytes per store of an LLR tensor at `llr`: an element's m floats start at a multiple of 4 m bytes, so every pair of elements starts
// on 16 bytes when m is 4 or 8, or when the frames hold an even number of elements (then every pair is whole, too)
inline int link_llr_store_bytes(const float *llr, int m, unsigned long long elems) {
    const uintptr_t at = reinterpret_cast<uintptr_t>(llr);
    return at % 16 == 0 && (m % 4 == 0 || elems % 2 == 0) ? 16 : at % 8 == 0 ? 8 : 4;
}

// bytes per store of ONE element's m floats at `llr` (link_store_element_llrs): an element starts at a multiple of 4 m bytes, which is
// a multiple of 16 when m is 4 or 8 and of 8 always
inline int link_llr_element_store_bytes(const float *llr, int m) {
    const uintptr_t at = reinterpret_cast<uintptr_t>(llr);
    return at % 16 == 0 && m % 4 == 0 ? 16 : at % 8 == 0 ? 8 : 4;
}

// ---- a launch's arguments and its dispatch on the modulation order (k_link.hip, k_linksm.hip, k_linkalamouti.hip, k_linkprecode.hip) ----

// the union of what the front end's kernels read and write; a pointer an instantiation does not use is NULL
struct LinkArgs {
    aft_link c;
    const float2 *ideal, *est;
    const unsigned long long *keys;
    const float *sigma, *rho, *scale, *factors;
    int *counts;
    float *loss, *llr;          // llr may be NULL where there is a loss
    unsigned elems;             // S T - 1 fits; S T itself may be 2^31
    float d, d2;                // float(sqrt(3 / (2 (L^2 - 1)))) and twice that
    int n_factors;              // 1 .. kMaxFactors
    int branches;               // 1 .. AFT_LINK_MAX_BRANCHES
    int wide;                   // 1: 16-byte loads of ideal and est
    int store;                  // bytes per store of llr: 16, 8 or 4
};

// The arguments of a launch from the entry point's: a launcher passes NULL (and 1 factor, 1 branch) for what it does not have.
inline LinkArgs link_args(const aft_link &link, const float *ideal, const float *est, const unsigned long long *keys, const float *sigma,
                          const float *rho, const float *scale, const float *factors, int n_factors, int branches, int32_t *counts,
                          float *loss, float *llr) {
    LinkArgs a{};
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
    return a;
}

// launch(std::integral_constant<int, M>) enqueues the kernel's instantiation for M = a.c.bits_per_symbol
template <class Launch>
hipError_t link_dispatch(int m, Launch &&launch) {
    switch (m) {
        case 2: launch(std::integral_constant<int, 2>{}); break;
        case 4: launch(std::integral_constant<int, 4>{}); break;
        case 6: launch(std::integral_constant<int, 6>{}); break;
        case 8: launch(std::integral_constant<int, 8>{}); break;
        default: return hipErrorInvalidValue;           // the entry point has refused it
    }
    return hipGetLastError();
}

}  // namespace
}  // namespace aft
