// The closed-loop link (include/adafortitran_amd.h "closed-loop precoding"; adafortitran_amd/linksim.py "the closed-loop link" is the
// definition and the float64 twin): two transmit antennas send ONE stream co-phased by a rank-1 precoder (1, q), q one of 1, -1, j, -j,
// which the receiver picks per SUBBAND of B subcarriers from its own estimates -- the precoding matrix indicator (PMI) --, R antennas
// receive and combine.  One workgroup per GROUP of 2 R consecutive frames -- frame r 2 + s is the pair (receive antenna r, transmit
// antenna s) --, one launch per batch; a group's counts, losses, LLRs and PMIs are a function of its own leader's key, the keys, noise
// scales and weights of its frames (r, 0), its true channels and estimates and its leader's LLR scale only.
//
//   1. the pilot positions go to LDS (link_stage_pilots) and the R keys, noise scales and weights of the frames (r, 0);
//   2. the selection, ONE TEAM PER SUBBAND.  A team is W consecutive threads: W = the power of two at or above the B T elements of a
//      whole subband, at least 8 and at most a wave, doubled up to 256 while there are more teams than subbands and fewer threads
//      than elements (link_precode_team, on the host: one value per launch, so the order of every sum is a function of the grid and
//      B alone; teams wider than a wave pay two barriers per round, so they serve the few wide subbands only); the 256 / W teams take
//      the subbands team, team + 256 / W, ... in rounds the whole workgroup makes together.  A subband's elements are contiguous (q = s T + t, the subcarriers b B .. min(S, (b + 1) B) - 1, pilot
//      positions included); thread l of the team takes its elements l, l + W, ... in increasing order and, per element, the antennas
//      in increasing r, adding rho_r conj(E_r0) E_r1 by one fused multiply-add per component (link_pmi_accumulate: the product is
//      link_sm_accumulate's g01 chain) to a sum that starts at 0.  The team's sums are added by shuffles (xor min(W, 64) / 2, ..., 1:
//      every lane of the team holds the same sum) and, where a team is two or four waves, the waves' sums through LDS in wave order.
//      The team's first thread decides v = (Re g, -Re g, -Im g, Im g), the LOWEST index that attains the maximum (link_pmi), stores
//      pmi[g][b] and keeps it in a table in LDS (one byte per subband, at most 1024).  A component of g is a chain of
//      ceil(n_b / W) R + log2(W) + 1 additions at the most of terms with two roundings each: it is within
//      (ceil(n_b / W) R + 12) 2^-24 sum rho_r |E_r0| |E_r1| of the exact sum (tests/test_linkprecode_gpu.py);
//   3. after a barrier, the element walk: a thread takes the elements tid, tid + 256, ..., consecutive lanes on consecutive addresses,
//      8 bytes per load whatever the alignment of the bases.  A pilot position gets its M zeros.  A data element hashes its sent word
//      once from the leader's key (link_sent) and reads its subband's q from the table.  The antenna loop, not unrolled, loads
//      H_r0, H_r1, E_r0, E_r1, turns H_r1 and E_r1 by q (link_mul_q: a swap and negations, exact), forms y_r = link_sample2(x, x) on
//      (H_r0, q H_r1) -- H_r0 x + (q H_r1) x + noise with the noise words of the key of frame (r, 0) --, e_r = E_r0 + q E_r1 (one
//      rounding per component) and adds c += rho_r y_r conj(e_r), p += rho_r |e_r|^2 (link_precoded_accumulate: link_branch's chain per
//      term, link_combine's fused multiply-add per sum, the sums start at -0 as link_mrc_kernel's).  The precoder is applied to the
//      channel, not to the symbol: q H_r1 holds the same bits when H_r1 is turned by a power of j and q turns back, so the outputs
//      do not depend on the common phase of the second antenna, bit for bit;
//   4. link_walk's measures on (c, p): the hard decision against the sent Gray codes, the max-log LLRs scale (min1 - min0), the
//      softplus losses, and the element's M LLRs leave by link_store_element_llrs: every element of the LLR output is written once;
//   5. the two integer counts and the K float sums stay in registers and are reduced in link_walk's fixed order.
//
// No atomics and no workspace: a group's outputs depend neither on the batch, nor on its position in it, nor on the run, nor on the
// alignment of the bases or the store form, nor on whether the LLRs are stored.  No fast-math; every product is a fused multiply-add
// chain written as such, and the combiner's step and the soft pieces are compiled under `fp contract(off)`.  With H_r1 = E_r1 = 0
// every sum of step 2 is 0, every PMI 0, the sample link_branch's and e_r = E_r0: the LLRs are link_mrc_kernel's on the frames
// (r, 0), bit for bit.
//
// Delayed feedback (aft_link_precoded_delayed_f32; linksim.py "delayed feedback"): the batch is whole sequences of K slots, a slot one
// group, and slot k >= d is sent with the PMIs selected from slot k - d.  The same walk, one workgroup per OUTPUT group
// o = seq (K - d) + (k - d): step 2 reads the estimates and the weights rho of the FEEDBACK group seq K + k - d, steps 1 and 3 to 5 read the
// TRANSMIT group seq K + k (true channels, estimates, keys, noise scales, weights, LLR scale), and every output is indexed by o.  Two
// group numbers are all that differs: no second body, no workspace, no copy; with d = 0 they coincide and the kernel is
// link_precoded_kernel's, bit for bit.
//
//   link_precoded_kernel<M>        (aft_link_precoded_f32)
//   link_precode_delayed_kernel<M> (aft_link_precoded_delayed_f32)
#include "link_device.h"

namespace aft {
namespace {

// link_args' struct, the subband width in subcarriers, the number of subbands, the threads that sum one subband and the PMI output
// [groups][n_sub]; the delayed kernel's slots per sequence and delay in slots behind them
struct LinkPrecodeArgs : LinkArgs {
    int subband, n_sub, team;
    int *pmi;
    int slots, delay;
};

// The threads that sum one subband: the power of two at or above the elements of a whole subband in 8 .. kWave, doubled up to
// kFrameThreads while that leaves no team without a subband's worth of work
inline int link_precode_team(unsigned long long elements, int n_sub) {
    int w = 8;
    while (w < kWave && (unsigned long long)w < elements) w *= 2;
    while (w < kFrameThreads && kFrameThreads / w > n_sub && (unsigned long long)w < elements) w *= 2;
    return w;
}

// One instantiation per modulation order and per feedback form
template <int M, bool kDelayed>
__device__ __forceinline__ void link_precoded_walk(const LinkPrecodeArgs &a) {
    constexpr int half = M / 2, L = 1 << half;
    __shared__ int psc[AFT_CHANSIM_MAX_PILOT_SCS], psym[AFT_CHANSIM_MAX_PILOT_SYMBOLS];
    __shared__ unsigned long long bkey[AFT_LINK_MAX_BRANCHES];
    __shared__ float bsigma[AFT_LINK_MAX_BRANCHES], brho[AFT_LINK_MAX_BRANCHES];
    __shared__ float part[kLinkWaves][kMaxFactors];
    __shared__ int ipart[kLinkWaves][2];
    __shared__ signed char table[AFT_LINK_MAX_SUBBANDS];       // the subbands' PMIs
    __shared__ float gpart[kLinkWaves][2];                      // the waves' sums of a team of several waves
    __shared__ float frho[kDelayed ? AFT_LINK_MAX_BRANCHES : 1];  // the delayed kernel: the weights of the feedback group's frames (r, 0)
    const aft_link &c = a.c;
    const int tid = threadIdx.x;
    const size_t g = blockIdx.x;
    const int Ps = c.pilot_scs, Pt = c.pilot_symbols, nf = a.n_factors, R = a.branches;
    const unsigned S = (unsigned)c.num_scs, T = (unsigned)c.num_symbols, B = (unsigned)a.subband, n_sub = (unsigned)a.n_sub, last = a.elems;
    AFT_DEV_ASSERT(nf >= 1 && nf <= kMaxFactors);
    AFT_DEV_ASSERT(R >= 1 && R <= AFT_LINK_MAX_BRANCHES);
    AFT_DEV_ASSERT(B >= 1 && B <= S && n_sub == (S - 1) / B + 1 && n_sub <= AFT_LINK_MAX_SUBBANDS);
    AFT_DEV_ASSERT(a.team >= 8 && a.team <= kFrameThreads && (a.team & (a.team - 1)) == 0);
    // g numbers the outputs.  The inputs: gt the group that is sent, gf the group the PMIs are selected from -- both g without a delay
    size_t gt = g, gf = g;
    if constexpr (kDelayed) {
        AFT_DEV_ASSERT(a.slots >= 1 && a.delay >= 0 && a.delay < a.slots);
        const size_t sent = (size_t)(a.slots - a.delay), seq = g / sent;
        gt = seq * (size_t)a.slots + (size_t)a.delay + (g - seq * sent);
        gf = gt - (size_t)a.delay;
    }
    const size_t first = gt * (size_t)(2 * R);                  // the group's leader, frame (0, 0)
    link_stage_pilots(c, tid, psc, psym);
    if (tid >= 2 * kWave && tid - 2 * kWave < R) {              // the frames (r, 0): the antennas' noise keys, noise scales and weights
        const int r = tid - 2 * kWave;
        bkey[r] = a.keys[first + 2 * r];
        bsigma[r] = a.sigma[first + 2 * r];
        brho[r] = a.rho[first + 2 * r];
        if constexpr (kDelayed) frho[r] = a.rho[gf * (size_t)(2 * R) + 2 * r];
    }
    __syncthreads();
    const size_t frame = (size_t)last + 1;                      // elements per frame
    const float2 *hp = a.ideal + first * frame, *ep = a.est + first * frame;
    const float2 *sp = kDelayed ? a.est + gf * (size_t)(2 * R) * frame : ep;     // the estimates and weights the selection reads
    const float *srho = kDelayed ? frho : brho;
    // the selection: team `team` the subbands team, team + teams, ..., one per round; every thread makes every round
    const unsigned W = (unsigned)a.team, teams = kFrameThreads / W, team = (unsigned)tid / W, l = (unsigned)tid & (W - 1);
    const unsigned rounds = (n_sub + teams - 1) / teams;
    for (unsigned round = 0; round < rounds; ++round) {
        const unsigned b = round * teams + team;
        const bool mine = b < n_sub;                            // the last round may leave teams without a subband
        float gr = 0.f, gi = 0.f;
        if (mine) {
            const unsigned s0 = b * B, s1 = s0 + B < S ? s0 + B : S;
            const unsigned q0 = s0 * T, n = (s1 - s0) * T;      // n <= S T <= 2^31: e + W does not wrap
            AFT_DEV_ASSERT(s0 < S && (size_t)q0 + n <= frame);
            for (unsigned e = l; e < n; e += W) {
                const float2 *eq = sp + q0 + e;
                for (int r = 0; r < R; ++r)
                    link_pmi_accumulate(gr, gi, srho[r], eq[(size_t)(2 * r) * frame], eq[(size_t)(2 * r + 1) * frame]);
            }
        }
#pragma unroll
        for (unsigned o = kWave / 2; o >= 1; o >>= 1)
            if (o < W) {                                        // the partner is in the lane's own team
                gr += __shfl_xor(gr, (int)o);
                gi += __shfl_xor(gi, (int)o);
            }
        if (W > kWave) {                                        // a team of 2 or 4 waves: their sums in wave order
            if ((tid & (kWave - 1)) == 0) {
                gpart[tid / kWave][0] = gr;
                gpart[tid / kWave][1] = gi;
            }
            __syncthreads();
            if (l == 0) {
                const unsigned w0 = (unsigned)tid / kWave;
                gr = gpart[w0][0];
                gi = gpart[w0][1];
                for (unsigned w = 1; w < W / kWave; ++w) {
                    gr += gpart[w0 + w][0];
                    gi += gpart[w0 + w][1];
                }
            }
        }
        if (mine && l == 0) {
            const int i = link_pmi(gr, gi);
            table[b] = (signed char)i;
            a.pmi[g * (size_t)n_sub + b] = i;
        }
        if (W > kWave) __syncthreads();                         // gpart is free for the next round
    }
    __syncthreads();
    const unsigned long long kl = bkey[0];                      // one transmission per group: the leader's key
    const float scale = a.scale[gt];
    float fac[kMaxFactors], acc[kMaxFactors];
#pragma unroll
    for (int k = 0; k < kMaxFactors; ++k) {
        fac[k] = k < nf ? a.factors[k] : 0.f;
        acc[k] = 0.f;
    }
    float *lp = a.llr != nullptr ? a.llr + g * frame * M : nullptr;
    int bits = 0, symbols = 0;
    for (unsigned q = tid; q <= last; q += kFrameThreads) {      // last < 2^31: the index cannot wrap
        const unsigned s = q / T, t = q - s * T;
        float w[M];                                             // the M LLRs: I-axis bits first, MSB first, the order of the sent word
        if (link_listed(psym, Pt, (int)t) && link_listed(psc, Ps, (int)s)) {
#pragma unroll
            for (int j = 0; j < M; ++j) w[j] = 0.f;             // what a pilot position carries
        } else {
            const unsigned b = s / B;
            AFT_DEV_ASSERT(b < n_sub);
            const int pm = table[b];
            AFT_DEV_ASSERT(pm >= 0 && pm <= 3);
            const LinkSent x = link_sent<M>(a.d, kl, q);
            LinkBranch m{-0.f, -0.f, -0.f};                     // x + (-0) = x for every x
#pragma unroll 1
            for (int r = 0; r < R; ++r) {
                const float2 *h0 = hp + (size_t)(2 * r) * frame + q, *e0 = ep + (size_t)(2 * r) * frame + q;
                const float2 h0q = h0[0], h1q = h0[frame], e0q = e0[0], e1q = e0[frame];
                const LinkSample y = link_sample2(bkey[r], bsigma[r], q, x, x, h0q, link_mul_q(pm, h1q));
                link_precoded_accumulate(m, brho[r], y, e0q, link_mul_q(pm, e1q));
            }
            const float step = a.d2 * m.p;
            const unsigned ki = decide<L>(m.cr, step), kq = decide<L>(m.ci, step);
            const int wrong = __popc(x.gi ^ ki ^ (ki >> 1)) + __popc(x.gq ^ kq ^ (kq >> 1));
            bits += wrong;
            symbols += wrong != 0 ? 1 : 0;
            link_axis_llrs<L>(a.d, m.cr, m.p, scale, w);
            link_axis_llrs<L>(a.d, m.ci, m.p, scale, w + half);
            link_soft_losses<M>(w, x.gi, x.gq, fac, nf, acc);
        }
        if (lp != nullptr) link_store_element_llrs<M>(lp + (size_t)q * M, w, a.store);
    }
    link_wave_sum(bits, tid, ipart, 0);
    link_wave_sum(symbols, tid, ipart, 1);
#pragma unroll
    for (int k = 0; k < kMaxFactors; ++k)
        if (k < nf) link_wave_sum(acc[k], tid, part, k);
    __syncthreads();
    if (tid < nf) a.loss[g * (size_t)nf + tid] = link_block_sum(part, tid) * kInvLn2;         // thread k the loss at factor k
    // the second wave: the bit errors, then the symbol errors
    if (tid >= kWave && tid < kWave + 2) a.counts[2 * g + (tid - kWave)] = link_block_sum(ipart, tid - kWave);
}

template <int M>
__global__ __launch_bounds__(kFrameThreads) void link_precoded_kernel(const LinkPrecodeArgs a) {
    link_precoded_walk<M, false>(a);
}

template <int M>
__global__ __launch_bounds__(kFrameThreads) void link_precode_delayed_kernel(const LinkPrecodeArgs a) {
    link_precoded_walk<M, true>(a);
}

}  // namespace

hipError_t launch_link_precoded(const aft_link &link, const float *ideal, const float *est, const unsigned long long *keys,
                                const float *sigma, const float *rho, const float *scale, const float *factors, int n_factors,
                                int branches, int subband, int32_t *counts, float *loss, float *llr, int32_t *pmi, int batch,
                                hipStream_t st) {
    const int n_sub = (link.num_scs - 1) / subband + 1;
    LinkPrecodeArgs a{link_args(link, ideal, est, keys, sigma, rho, scale, factors, n_factors, branches, counts, loss, llr), subband,
                      n_sub, link_precode_team((unsigned long long)subband * (unsigned long long)link.num_symbols, n_sub), pmi, 1, 0};
    a.wide = 0;                                                 // this walk loads and stores element by element
    a.store = link_llr_element_store_bytes(llr, link.bits_per_symbol);
    const dim3 grid((unsigned)(batch / (2 * branches)));
    return link_dispatch(link.bits_per_symbol, [&](auto m) {
        hipLaunchKernelGGL(link_precoded_kernel<decltype(m)::value>, grid, dim3(kFrameThreads), 0, st, a);
    });
}

hipError_t launch_link_precoded_delayed(const aft_link &link, const float *ideal, const float *est, const unsigned long long *keys,
                                        const float *sigma, const float *rho, const float *scale, const float *factors, int n_factors,
                                        int branches, int subband, int slots, int delay, int32_t *counts, float *loss, float *llr,
                                        int32_t *pmi, int batch, hipStream_t st) {
    const int n_sub = (link.num_scs - 1) / subband + 1;
    LinkPrecodeArgs a{link_args(link, ideal, est, keys, sigma, rho, scale, factors, n_factors, branches, counts, loss, llr), subband,
                      n_sub, link_precode_team((unsigned long long)subband * (unsigned long long)link.num_symbols, n_sub), pmi, slots,
                      delay};
    a.wide = 0;                                                 // this walk loads and stores element by element
    a.store = link_llr_element_store_bytes(llr, link.bits_per_symbol);
    const dim3 grid((unsigned)(batch / (2 * branches) / slots * (slots - delay)));     // the output groups
    return link_dispatch(link.bits_per_symbol, [&](auto m) {
        hipLaunchKernelGGL(link_precode_delayed_kernel<decltype(m)::value>, grid, dim3(kFrameThreads), 0, st, a);
    });
}

}  // namespace aft
