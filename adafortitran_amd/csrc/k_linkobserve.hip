// The decision-directed observation (include/adafortitran_amd.h "decision-directed observation"; adafortitran_amd/linksim.py
// link_observe_host is the definition and the float64 twin): what a receiver that re-estimates the channel from its own decisions
// observes of it.  One workgroup per GROUP of R consecutive frames, one launch per batch, link_walk's pair-to-thread map and load rules
// (k_link.hip): a thread takes the element pairs (2 i, 2 i + 1), i = tid, tid + 256, ..., 16-byte accesses for a pair when T is even and
// the bases are 16-byte aligned, 8-byte accesses per element otherwise, the last pair of an odd grid holding one element.
//
//   1. the pilot positions and the group's R keys, noise scales and weights go to LDS;
//   2. per data element the sent word is hashed once from the leader's key (link_sent) and every branch forms its received sample
//      y_r = H_r x + noise_r (link_received) and c_r = y_r conj(E_r), p_r = |E_r|^2 (link_branch_of: the two steps link_branch is made
//      of, called apart so that the sample is hashed once and kept); c and p are link_combine's sums
//      in increasing r from -0: the diversity link's own operands, so the decision below is aft_link_mrc_f32's, bit for bit;
//   3. the decision: per axis k = decide<L>(component of c, float(2 d p)); x^ = link_level(k_i) + j link_level(k_q), or the sent x with
//      source = sent; a decided index that differs from the sent one on either axis is one symbol error;
//   4. every branch's z_r = y_r conj(x^) / |x^|^2.  The chain, per element and branch:
//          n2 = fma(ar, ar, ai ai)                         |x^|^2, ONE fused multiply-add on the product ai ai
//          zr = fma(yr, ar, yi ai) / n2                    one product, one fused multiply-add, one correctly rounded division
//          zi = fma(yi, ar, -(yr ai)) / n2                 likewise
//      with x^ = ar + j ai and y_r = yr + j yi link_received's two chains of fused multiply-adds.  The last branch's y is the one step 2
//      left in registers; an earlier branch's is formed again from the same operands by the same function (the same bits), so no
//      sample is kept per branch and none goes through memory;
//   5. at a pilot position z_r is frame r's own pilot, copied bit for bit, and the decision reads 255.
//
// Every element of z (pilot positions included), of the decision map and of the per-group count is written exactly once; the count is
// reduced in a fixed order (link_wave_sum, link_block_sum).  No atomics and no workspace: a group's outputs depend neither on the batch,
// nor on its position in it, nor on the run, nor on the load and store forms.
#include "link_device.h"

namespace aft {
namespace {

struct ObserveArgs {
    LinkArgs l;                 // the front end's: link, ideal, est, keys, sigma, rho, branches, elems, d, d2, wide
    const float2 *pilots;       // [batch, Ps, Pt]
    float2 *z;                  // [batch, S, T]
    unsigned char *decisions;   // [groups, S, T]
    int *errors;                // [groups]
    int sent;                   // 1: x^ is the sent symbol (the genie bound)
    int zwide;                  // 1: 16-byte stores into z
};

template <int M>
__global__ __launch_bounds__(kFrameThreads) void link_observe_kernel(const ObserveArgs a) {
    constexpr int half = M / 2, L = 1 << half;
    __shared__ int psc[AFT_CHANSIM_MAX_PILOT_SCS], psym[AFT_CHANSIM_MAX_PILOT_SYMBOLS];
    __shared__ unsigned long long bkey[AFT_LINK_MAX_BRANCHES];
    __shared__ float bsigma[AFT_LINK_MAX_BRANCHES], brho[AFT_LINK_MAX_BRANCHES];
    __shared__ int ipart[kLinkWaves][1];
    const aft_link &c = a.l.c;
    const int tid = threadIdx.x;
    const size_t g = blockIdx.x;
    const int Ps = c.pilot_scs, Pt = c.pilot_symbols, R = a.l.branches;
    const unsigned T = (unsigned)c.num_symbols, last = a.l.elems;
    AFT_DEV_ASSERT(R >= 1 && R <= AFT_LINK_MAX_BRANCHES);
    const size_t first = g * (size_t)R;                         // the group's leader
    link_stage_pilots(c, tid, psc, psym);
    if (tid >= 2 * kWave && tid - 2 * kWave < R) {
        const int r = tid - 2 * kWave;
        bkey[r] = a.l.keys[first + r];
        bsigma[r] = a.l.sigma[first + r];
        brho[r] = a.l.rho[first + r];
    }
    __syncthreads();
    const unsigned long long kl = bkey[0];                      // one transmission per group: the leader's key
    const size_t frame = (size_t)last + 1, pframe = (size_t)(Ps * Pt);
    const float2 *hp = a.l.ideal + first * frame, *ep = a.l.est + first * frame, *pp = a.pilots + first * pframe;
    float2 *zp = a.z + first * frame;
    unsigned char *dp = a.decisions + g * frame;
    int wrong = 0;
    const unsigned pairs = (last >> 1) + 1;                     // the last pair of an odd grid holds one element
    for (unsigned i = tid; i < pairs; i += kFrameThreads) {      // pairs <= 2^30: the index cannot wrap
        const unsigned q = 2 * i;
        const bool two = q < last;
        AFT_DEV_ASSERT(q <= last && (two || (!a.l.wide && !a.zwide)));
        int pilot[2];                                           // the element's place in a frame's pilots, -1: a data element
        bool data[2];
        LinkSent x[2];
        LinkBranch m[2];
        LinkReceived y[2];                                      // the LAST branch's samples
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const unsigned e = q + s, row = e / T, col = e - row * T;
            const int pj = link_position(psym, Pt, (int)col), pi = pj < 0 ? -1 : link_position(psc, Ps, (int)row);
            pilot[s] = pi < 0 ? -1 : pi * Pt + pj;
            data[s] = (s == 0 || two) && pilot[s] < 0;
            x[s] = LinkSent{0u, 0u, 0.f, 0.f};
            if (data[s]) x[s] = link_sent<M>(a.l.d, kl, e);
            m[s] = LinkBranch{-0.f, -0.f, -0.f};                // x + (-0) = x for every x: the first branch at rho = 1 is exact
            y[s] = LinkReceived{0.f, 0.f};
        }
#pragma unroll 1
        for (int r = 0; r < R; ++r) {
            LinkPair h{}, e{};
            link_load_pairs(hp + (size_t)r * frame + q, ep + (size_t)r * frame + q, a.l.wide, two, h, e);
            const unsigned long long kf = bkey[r];
            const float sr = bsigma[r], rho = brho[r];
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (data[s]) {
                    const float2 hs = s ? h.b : h.a, es = s ? e.b : e.a;
                    y[s] = link_received(kf, sr, q + s, x[s].xr, x[s].xi, hs);       // link_branch's two steps, the sample kept
                    link_combine(m[s], rho, link_branch_of(y[s], es));
                }
        }
        float ar[2], ai[2], n2[2];
        unsigned char dec[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            ar[s] = ai[s] = 0.f;
            n2[s] = 1.f;
            dec[s] = 255;
            if (data[s]) {
                const float step = a.l.d2 * m[s].p;
                const unsigned ki = decide<L>(m[s].cr, step), kq = decide<L>(m[s].ci, step);
                wrong += ((x[s].gi ^ ki ^ (ki >> 1)) | (x[s].gq ^ kq ^ (kq >> 1))) != 0u ? 1 : 0;
                dec[s] = (unsigned char)(ki | (kq << 4));
                ar[s] = a.sent ? x[s].xr : link_level<L>(a.l.d, ki);
                ai[s] = a.sent ? x[s].xi : link_level<L>(a.l.d, kq);
                n2[s] = fmaf(ar[s], ar[s], ai[s] * ai[s]);
            }
        }
        dp[q] = dec[0];
        if (two) dp[q + 1] = dec[1];
#pragma unroll 1
        for (int r = 0; r < R; ++r) {
            LinkReceived yr[2] = {y[0], y[1]};
            if (r != R - 1) {                                   // an earlier branch: the same function on the same operands
                const LinkPair h = link_load_pair(hp + (size_t)r * frame + q, a.l.wide, two);
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    if (data[s]) yr[s] = link_received(bkey[r], bsigma[r], q + s, x[s].xr, x[s].xi, s ? h.b : h.a);
            }
            float2 zv[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                zv[s] = make_float2(0.f, 0.f);
                if (data[s]) {
                    zv[s].x = fmaf(yr[s].yr, ar[s], yr[s].yi * ai[s]) / n2[s];
                    zv[s].y = fmaf(yr[s].yi, ar[s], -(yr[s].yr * ai[s])) / n2[s];
                } else if (s == 0 || two) {
                    AFT_DEV_ASSERT(pilot[s] >= 0 && pilot[s] < Ps * Pt);
                    zv[s] = pp[(size_t)r * pframe + pilot[s]];
                }
            }
            float2 *zq = zp + (size_t)r * frame + q;
            if (a.zwide) {
                *reinterpret_cast<f32x4 *>(zq) = f32x4{zv[0].x, zv[0].y, zv[1].x, zv[1].y};
            } else {
                zq[0] = zv[0];
                if (two) zq[1] = zv[1];
            }
        }
    }
    link_wave_sum(wrong, tid, ipart, 0);
    __syncthreads();
    if (tid == kWave) a.errors[g] = link_block_sum(ipart, 0);    // the second wave's first thread, as the counts of k_link.hip
}

}  // namespace

hipError_t launch_link_observe(const aft_link &link, const float *ideal, const float *est, const unsigned long long *keys,
                               const float *sigma, const float *rho, const float *pilots, int source, int branches, float *z,
                               unsigned char *decisions, int32_t *symbol_errors, int batch, hipStream_t st) {
    ObserveArgs a{};
    a.l = link_args(link, ideal, est, keys, sigma, rho, nullptr, nullptr, 1, branches, nullptr, nullptr, nullptr);
    a.pilots = reinterpret_cast<const float2 *>(pilots);
    a.z = reinterpret_cast<float2 *>(z);
    a.decisions = decisions;
    a.errors = symbol_errors;
    a.sent = source;
    a.zwide = wide_ok(link.num_symbols, z);
    return link_dispatch(link.bits_per_symbol, [&](auto m) {
        hipLaunchKernelGGL(link_observe_kernel<decltype(m)::value>, dim3((unsigned)(batch / branches)), dim3(kFrameThreads), 0, st, a);
    });
}

}  // namespace aft
