// The transmit-diversity link (include/adafortitran_amd.h "transmit diversity"; adafortitran_amd/linksim.py "the transmit-diversity
// link" is the definition and the float64 twin): two transmit antennas send ONE stream as Alamouti pairs over adjacent data symbols
// of a subcarrier (pairing "time") or adjacent data subcarriers of a symbol (pairing "frequency"), R antennas receive and combine.
// One workgroup per GROUP of 2 R consecutive frames -- frame r 2 + s is the pair (receive antenna r, transmit antenna s) --, one
// launch per batch; a group's counts, losses and LLRs are a function of its own leader's key, the keys, noise scales and weights of
// its frames (r, 0), its true channels and estimates and its leader's LLR scale only.
//
//   1. the pilot positions go to LDS (link_stage_pilots) and the R keys, noise scales and weights of the frames (r, 0);
//   2. a LINE is a subcarrier (time) or a symbol (frequency) and holds ceil(length / 2) SLOTS; slot j of a line is the pair of the
//      line's 2 j-th and 2 j + 1-th DATA elements, found by stepping over the line's sorted pilot positions (link_line_data; a line
//      that is not in the pilot list of its own axis has none).  A slot past the line's data is skipped, an odd line's last slot is a
//      LONE element.  A thread takes the (line, slot) indices tid, tid + 256, ...: time pairing runs the slots of a line in
//      consecutive threads, frequency pairing the lines of a slot, so that in both consecutive lanes read consecutive addresses;
//   3. both sent words of the pair are hashed once from the leader's key (link_sent).  The antenna loop, not unrolled, loads the
//      eight values H_r0, H_r1, E_r0, E_r1 at a and at b (8 bytes each, whatever the alignment of the bases), hashes the two noise
//      words of each element with the key of frame (r, 0), forms y_r[a] = link_sample2(x_a, x_b) and y_r[b] = link_sample2(-conj(x_b),
//      conj(x_a)) -- negation and conjugation are exact -- and adds the six sums c_a, p_a, c_b, p_b (link_alamouti_accumulate: per
//      antenna the term at a before the term at b, one fused multiply-add per term, the sums start at -0 as link_combine's).  A lone
//      element loads H_r0 and E_r0 only and is the pair with everything else 0: antenna 1 sends nothing there;
//   4. per element of the pair, in a loop that is not unrolled (one copy of the soft code), link_walk's measures on (c, p): the hard
//      decision against the sent Gray codes, the max-log LLRs scale (min1 - min0), the softplus losses, and the element's M LLRs
//      leave by link_store_element_llrs;
//   5. the pair walk visits no pilot: a short loop over the pilot_scs x pilot_symbols positions writes their M zeros, so every
//      element of the LLR output is written exactly once;
//   6. the two integer counts and the K float sums stay in registers and are reduced in link_walk's fixed order.
//
// No atomics and no workspace: a group's outputs depend neither on the batch, nor on its position in it, nor on the run, nor on the
// alignment of the bases or the store form, nor on whether the LLRs are stored.  No fast-math; every product is a fused multiply-add
// chain written as such, and the combiner's step and the soft pieces are compiled under `fp contract(off)`.  With H_r1 = E_r1 = 0
// the sample is link_branch's and the second term of every sum adds an exact zero: the LLRs at first and lone elements are
// link_mrc_kernel's on the frames (r, 0), bit for bit.
//
//   link_alamouti_kernel<M, Freq>  (aft_link_alamouti_f32)  Freq: pairing "frequency"
#include "link_device.h"

namespace aft {
namespace {

// One instantiation per modulation order and pairing
template <int M, bool Freq>
__device__ __forceinline__ void link_alamouti_walk(const LinkArgs &a) {
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
    const unsigned S = (unsigned)c.num_scs, T = (unsigned)c.num_symbols;
    AFT_DEV_ASSERT(nf >= 1 && nf <= kMaxFactors);
    AFT_DEV_ASSERT(R >= 1 && R <= AFT_LINK_MAX_BRANCHES);
    const size_t first = g * (size_t)(2 * R);                   // the group's leader, frame (0, 0)
    link_stage_pilots(c, tid, psc, psym);
    if (tid >= 2 * kWave && tid - 2 * kWave < R) {              // the frames (r, 0): the antennas' noise keys, noise scales and weights
        const int r = tid - 2 * kWave;
        bkey[r] = a.keys[first + 2 * r];
        bsigma[r] = a.sigma[first + 2 * r];
        brho[r] = a.rho[first + 2 * r];
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
    const size_t frame = (size_t)a.elems + 1;                   // elements per frame
    const float2 *hp = a.ideal + first * frame, *ep = a.est + first * frame;
    float *lp = a.llr != nullptr ? a.llr + g * frame * M : nullptr;
    // the lines, their length, the pilot list that says which lines carry pilots and the one that says where on such a line
    const unsigned lines = Freq ? T : S, length = Freq ? S : T;
    const int *own = Freq ? psym : psc, *along = Freq ? psc : psym;
    const int n_own = Freq ? Pt : Ps, n_along = Freq ? Ps : Pt;
    const unsigned slots = (length + 1) >> 1;
    const unsigned total = lines * slots;                       // at most (S T + lines) / 2 <= 2^31: neither it nor the index wraps
    int bits = 0, symbols = 0;
    for (unsigned i = tid; i < total; i += kFrameThreads) {
        const unsigned line = Freq ? i % lines : i / slots, slot = Freq ? i / lines : i - line * slots;
        const int np = link_listed(own, n_own, (int)line) ? n_along : 0;
        const unsigned data = length - (unsigned)np, k = 2 * slot;
        if (k >= data) continue;                                // a slot past the line's data
        const bool two = k + 1 < data;                          // false: the lone last element of an odd line
        const unsigned pa = link_line_data(along, np, k), pb = two ? link_line_data(along, np, k + 1) : pa;
        AFT_DEV_ASSERT(pa < length && pb < length);
        const unsigned qa = Freq ? pa * T + line : line * T + pa, qb = Freq ? pb * T + line : line * T + pb;
        AFT_DEV_ASSERT(qa <= a.elems && qb <= a.elems);
        const LinkSent none{0u, 0u, 0.f, 0.f};
        const LinkSent xa = link_sent<M>(a.d, kl, qa);
        LinkSent xb = none;
        if (two) xb = link_sent<M>(a.d, kl, qb);
        const LinkSent tb0{0u, 0u, -xb.xr, xb.xi}, tb1{0u, 0u, xa.xr, -xa.xi};      // what the antennas send at b: -conj(x_b), conj(x_a)
        LinkBranch ma{-0.f, -0.f, -0.f}, mb = ma;               // x + (-0) = x for every x
#pragma unroll 1
        for (int r = 0; r < R; ++r) {
            const float2 *h0 = hp + (size_t)(2 * r) * frame, *e0 = ep + (size_t)(2 * r) * frame;
            const float2 *h1 = h0 + frame, *e1 = e0 + frame;
            const float2 z = make_float2(0.f, 0.f);
            const float2 h0a = h0[qa], e0a = e0[qa];
            float2 h1a = z, e1a = z, h0b = z, h1b = z, e0b = z, e1b = z;
            if (two) {
                h1a = h1[qa]; e1a = e1[qa];
                h0b = h0[qb]; e0b = e0[qb];
                h1b = h1[qb]; e1b = e1[qb];
            }
            const unsigned long long kf = bkey[r];
            const float sr = bsigma[r], rho = brho[r];
            const LinkSample ya = link_sample2(kf, sr, qa, xa, xb, h0a, h1a);
            LinkSample yb{0.f, 0.f};
            if (two) yb = link_sample2(kf, sr, qb, tb0, tb1, h0b, h1b);
            link_alamouti_accumulate(ma, mb, rho, ya, yb, e0a, e1a, e0b, e1b);
        }
#pragma unroll 1
        for (int s = 0; s < (two ? 2 : 1); ++s) {               // the element: one copy of the measures
            const LinkSent x = s ? xb : xa;
            const LinkBranch m = s ? mb : ma;
            const float step = a.d2 * m.p;
            const unsigned ki = decide<L>(m.cr, step), kq = decide<L>(m.ci, step);
            const int wrong = __popc(x.gi ^ ki ^ (ki >> 1)) + __popc(x.gq ^ kq ^ (kq >> 1));
            bits += wrong;
            symbols += wrong != 0 ? 1 : 0;
            float w[M];                                         // the M LLRs: I-axis bits first, MSB first, the order of the sent word
            link_axis_llrs<L>(a.d, m.cr, m.p, scale, w);
            link_axis_llrs<L>(a.d, m.ci, m.p, scale, w + half);
            link_soft_losses<M>(w, x.gi, x.gq, fac, nf, acc);
            if (lp != nullptr) link_store_element_llrs<M>(lp + (size_t)(s ? qb : qa) * M, w, a.store);
        }
    }
    if (lp != nullptr) {                                        // what a pilot position carries
        float w[M];
#pragma unroll
        for (int j = 0; j < M; ++j) w[j] = 0.f;
        for (int i = tid; i < Ps * Pt; i += kFrameThreads) {
            const size_t q = (size_t)psc[i / Pt] * T + (size_t)psym[i % Pt];
            link_store_element_llrs<M>(lp + q * M, w, a.store);
        }
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

template <int M, bool Freq>
__global__ __launch_bounds__(kFrameThreads) void link_alamouti_kernel(const LinkArgs a) {
    link_alamouti_walk<M, Freq>(a);
}

}  // namespace

hipError_t launch_link_alamouti(const aft_link &link, const float *ideal, const float *est, const unsigned long long *keys,
                                const float *sigma, const float *rho, const float *scale, const float *factors, int n_factors,
                                int branches, int pairing, int32_t *counts, float *loss, float *llr, int batch, hipStream_t st) {
    LinkArgs a = link_args(link, ideal, est, keys, sigma, rho, scale, factors, n_factors, branches, counts, loss, llr);
    a.wide = 0;                                                 // this walk loads and stores element by element
    a.store = link_llr_element_store_bytes(llr, link.bits_per_symbol);
    const dim3 grid((unsigned)(batch / (2 * branches)));
    return link_dispatch(link.bits_per_symbol, [&](auto m) {
        if (pairing == AFT_LINK_PAIR_FREQUENCY)
            hipLaunchKernelGGL((link_alamouti_kernel<decltype(m)::value, true>), grid, dim3(kFrameThreads), 0, st, a);
        else
            hipLaunchKernelGGL((link_alamouti_kernel<decltype(m)::value, false>), grid, dim3(kFrameThreads), 0, st, a);
    });
}

}  // namespace aft
