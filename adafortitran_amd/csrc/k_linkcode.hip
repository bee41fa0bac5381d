// The coded link: a rate-1/2, constraint-length-7 convolutional code (133, 171 octal; punctured to 2/3 and 3/4) rides on the link's sent
// bits through a scrambler, and a Viterbi decoder reads the LLR tensor aft_link_soft_f32 writes (include/adafortitran_amd.h "coded link";
// adafortitran_amd/linksim.py is the definition and the integer NumPy twin).  One workgroup per frame, one launch per batch; a frame's two
// counts and its decoded bits are a function of its own key and LLRs only.
//
//   1. the pilot positions go to LDS with, per pilot row, the number of data elements before it: a data-element index becomes a grid
//      index by one binary search over at most 64 entries and, inside a pilot row, a walk over at most 16 columns;
//   2. a wave takes the frame's code blocks b = wave, wave + W, ...; ONE LANE PER TRELLIS STATE.  Per 64 trellis steps, lane l prepares
//      step t0 + l: the information bit of that step from the hash (one ballot makes the 64 bits a word, from which every lane cuts
//      its 7-bit window and so its two codeword bits), the positions of its kept outputs through the interleaver
//      j = (b n + i) stride mod U (a multiply-high by floor(2^64 / U), no division), the sent bit at j and the LOAD of the LLR at j.
//      The loads of steps t0 + 64 .. t0 + 127 are issued before the serial chain of steps t0 .. t0 + 63 runs and are descrambled and
//      quantised to z in [-127, 127] after it.  The two z of a step travel in one register;
//   3. the serial chain then has no memory access but LDS: per step one lane read (the step's two z, wave-uniform), the branch gain
//      g = sA zA + sB zB of the even predecessor (the odd predecessor's outputs are the complements: its gain is -g), the two
//      predecessor metrics from lanes 2 (n & 31) and 2 (n & 31) + 1 by two lane permutes, compare, select, and one ballot: the 64
//      decisions of the step are one 64-bit word in LDS.  int32 metrics: at most 4096 steps of at most 254 each, far from 2^30;
//   4. traceback from state 0: 64 survivor words at a time into registers (one per lane), a wave-uniform walk over lane reads, the
//      decoded bits of the 64 steps as one word; lane l then compares step t0 + l with the information bit from the hash and
//      stores the decoded bit;
//   5. a wave's two counts are ballot population counts; the W waves' counts meet in LDS and two threads store the frame's pair.
//
// No atomics, no workspace: everything is integer after the quantiser, whose one float32 product and round-to-nearest-even are the
// definition's.
#include "linkcode_device.h"

namespace aft {
namespace {

constexpr int kCodeMaxWaves = 16;                               // waves (code blocks in flight) per workgroup
constexpr int kCodeTail = 6;                                    // constraint length 7: six tail bits
constexpr unsigned kGenA = 0x5B, kGenB = 0x79;                  // 133 and 171 octal on the window u_t .. u_{t-6}, u_t the top bit
constexpr size_t kCodeLdsBudget = 159 * 1024;                   // survivor words per workgroup (a CU's 160 KiB less the static arrays)

struct LinkCodeArgs {
    aft_link c;
    const float *llr;
    const unsigned long long *keys;
    int *counts;
    unsigned char *bits;                                        // may be NULL
    unsigned long long used, stride, used_inverse;              // U, the interleaver's stride, floor(2^64 / U)
    unsigned elems;                                             // S T - 1, as in k_link.hip
    unsigned info, steps, coded, blocks;                        // K, K + 6, n, B
    int rate;
    float qgain;
};

// kept outputs before step t, and which of the step's two are kept (rates 1/2, 2/3, 3/4: A0 B0 | A0 B0 A1 | A0 B0 A1 B2)
__device__ __forceinline__ unsigned code_offset(int rate, unsigned t, bool &keep_a, bool &keep_b) {
    if (rate == AFT_LINK_RATE_1_2) {
        keep_a = keep_b = true;
        return 2 * t;
    }
    if (rate == AFT_LINK_RATE_2_3) {
        const unsigned ph = t & 1;
        keep_a = true; keep_b = ph == 0;
        return 3 * (t >> 1) + 2 * ph;
    }
    const unsigned period = t / 3, ph = t - 3 * period;
    keep_a = ph != 2; keep_b = ph != 1;
    return 4 * period + (ph == 0 ? 0 : ph + 1);
}

__global__ __launch_bounds__(kCodeMaxWaves *kWave) void link_decode_kernel(const LinkCodeArgs a) {
    extern __shared__ unsigned long long surv_all[];            // [waves][steps]: a step's 64 decisions
    __shared__ int psc[AFT_CHANSIM_MAX_PILOT_SCS], psym[AFT_CHANSIM_MAX_PILOT_SYMBOLS];
    __shared__ unsigned before[AFT_CHANSIM_MAX_PILOT_SCS];
    __shared__ int part[kCodeMaxWaves][2];
    const aft_link &c = a.c;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, waves = blockDim.x / kWave;
    const size_t f = blockIdx.x;
    const int Ps = c.pilot_scs, Pt = c.pilot_symbols, m = c.bits_per_symbol;
    const unsigned T = (unsigned)c.num_symbols, K = a.info, steps = a.steps;
    AFT_DEV_ASSERT(Ps >= 1 && Ps <= AFT_CHANSIM_MAX_PILOT_SCS && Pt >= 1 && Pt <= AFT_CHANSIM_MAX_PILOT_SYMBOLS && (unsigned)Pt <= T);
    AFT_DEV_ASSERT(waves >= 1 && waves <= kCodeMaxWaves && steps == K + kCodeTail && steps <= AFT_LINK_CODE_MAX_INFO_BITS + kCodeTail);
    code_pilot_tables(c, tid, psc, before, psym);
    __syncthreads();
    const unsigned long long kf = a.keys[f];
    const float *llr = a.llr + f * ((size_t)a.elems + 1) * (size_t)m;
    unsigned long long *surv = surv_all + (size_t)wave * steps;

    // the lane's state n: predecessors r0 = 2 (n & 31) and r0 + 1, input n >> 5; the outputs on the branch from r0
    const int r0 = (lane & 31) << 1;
    const unsigned branch = (unsigned)(lane >> 5) << 6 | (unsigned)r0;
    const int sa = 1 - 2 * (__popc(branch & kGenA) & 1), sb = 1 - 2 * (__popc(branch & kGenB) & 1);

    // Where the LLR of data-bit index j lives, and whether the scrambler s = w_j ^ cbit turns its sign.
    struct Input {
        const float *at;
        bool turn;
    };
    auto locate = [&](unsigned long long j, unsigned cbit) {
        AFT_DEV_ASSERT(j < a.used);
        unsigned e, k;
        code_split(j, m, e, k);
        const unsigned q = code_grid_index(psc, before, psym, Ps, Pt, T, e);
        AFT_DEV_ASSERT(q <= a.elems && k < (unsigned)m);
        const unsigned sent = (unsigned)(frame_word(kf, kStreamDataBits, q) >> (63 - k)) & 1u;
        return Input{llr + ((size_t)q * m + k), (sent ^ cbit) != 0};
    };
    // the descrambled LLR, quantised: one float32 product, to nearest with ties to even, NaN gives 0
    auto quantise = [&](float l, bool turn) { return code_quantise(l, turn, a.qgain); };
    // What lane l prepares of step t0 + l: the two LLRs are LOADED here and quantised by `pack` after the serial chain of the 64
    // steps before them has run, so their latency is the chain's to hide.
    struct Fetched {
        float la, lb;
        bool turn_a, turn_b;
    };
    auto fetch = [&](unsigned b, unsigned t0, unsigned long long &prev) {
        const unsigned t = t0 + lane;
        const unsigned info0 = b * K;                           // B K <= 2^31: the hash's index does not wrap
        const unsigned u = t < K ? (unsigned)(frame_word(kf, kStreamCodeBits, info0 + t) >> 63) : 0u;
        const unsigned long long cur = __ballot(u != 0);
        const unsigned window = (unsigned)(lane >= 6 ? cur >> (lane - 6) : cur << (6 - lane) | prev >> (58 + lane)) & 127u;
        prev = cur;                                             // the information bits of the 64 steps before the next t0
        Fetched f{0.f, 0.f, false, false};                      // a punctured output, or a step past the last: z = 0
        if (t < steps) {
            bool keep_a, keep_b;
            const unsigned i = code_offset(a.rate, t, keep_a, keep_b);
            AFT_DEV_ASSERT(i + (keep_a ? 1u : 0u) + (keep_b ? 1u : 0u) <= a.coded);
            unsigned long long j = code_mulmod((unsigned long long)b * a.coded + i, a.stride, a.used, a.used_inverse);
            if (keep_a) {
                const Input in = locate(j, __popc(window & kGenA) & 1);
                f.la = *in.at; f.turn_a = in.turn;
                j += a.stride;
                j -= j >= a.used ? a.used : 0;
            }
            if (keep_b) {
                const Input in = locate(j, __popc(window & kGenB) & 1);
                f.lb = *in.at; f.turn_b = in.turn;
            }
        }
        return f;
    };
    auto pack = [&](const Fetched &f) { return (quantise(f.la, f.turn_a) & 0xFFFF) | (int)((unsigned)quantise(f.lb, f.turn_b) << 16); };

    int bit_errors = 0, block_errors = 0;
    for (unsigned b = wave; b < a.blocks; b += waves) {
        const unsigned info0 = b * K;
        int metric = lane == 0 ? 0 : -(1 << 30);
        unsigned long long prev = 0;
        Fetched ahead = fetch(b, 0, prev);
        for (unsigned t0 = 0; t0 < steps; t0 += kWave) {
            const int pair = pack(ahead);
            if (t0 + kWave < steps) ahead = fetch(b, t0 + kWave, prev);
            const int count = (int)min(steps - t0, (unsigned)kWave);
            for (int i = 0; i < count; ++i) {                   // the serial chain: add, compare, select
                const int z = __builtin_amdgcn_readlane(pair, i);
                const int g = sa * (int)(short)z + sb * (z >> 16);
                const int m0 = __shfl(metric, r0) + g, m1 = __shfl(metric, r0 | 1) - g;
                const bool odd = m1 > m0;                       // a tie takes r0
                metric = odd ? m1 : m0;
                const unsigned long long word = __ballot(odd);
                if (lane == 0) surv[t0 + i] = word;
            }
        }
        __builtin_amdgcn_wave_barrier();                        // the wave's own words: written by lane 0, read by all below

        unsigned state = 0;
        unsigned long long wrong_any = 0;
        for (int t0 = (int)((steps - 1) / kWave * kWave); t0 >= 0; t0 -= kWave) {
            const int count = (int)min(steps - (unsigned)t0, (unsigned)kWave);
            const unsigned long long mine = lane < count ? surv[t0 + lane] : 0ull;
            const int lo = (int)(unsigned)mine, hi = (int)(unsigned)(mine >> 32);
            unsigned long long decoded = 0;                     // bit i: the input of step t0 + i
            for (int i = count - 1; i >= 0; --i) {
                const unsigned long long word = (unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, i) << 32 |
                                                (unsigned)__builtin_amdgcn_readlane(lo, i);
                decoded |= (unsigned long long)(state >> 5) << i;
                state = (state & 31u) << 1 | (unsigned)(word >> state & 1ull);
            }
            const unsigned t = (unsigned)t0 + lane;
            bool wrong = false;
            if (t < K) {
                const unsigned got = (unsigned)(decoded >> lane) & 1u;
                wrong = got != (unsigned)(frame_word(kf, kStreamCodeBits, info0 + t) >> 63);
                if (a.bits != nullptr) a.bits[(f * a.blocks + b) * (size_t)K + t] = (unsigned char)got;
            }
            const unsigned long long w = __ballot(wrong);
            bit_errors += __popcll(w);
            wrong_any |= w;
        }
        block_errors += wrong_any != 0 ? 1 : 0;
        __builtin_amdgcn_wave_barrier();                        // the next block's words go where these were read
    }
    if (lane == 0) {
        part[wave][0] = bit_errors;
        part[wave][1] = block_errors;
    }
    __syncthreads();
    if (tid < 2) {                                              // thread 0 the bit errors, thread 1 the block errors
        int total = 0;
        for (int w = 0; w < waves; ++w) total += part[w][tid];
        a.counts[2 * f + tid] = total;
    }
}

}  // namespace

int link_code_waves(unsigned steps, unsigned blocks) {
    const size_t fit = kCodeLdsBudget / ((size_t)steps * sizeof(unsigned long long));
    return (int)std::min<size_t>({(size_t)kCodeMaxWaves, (size_t)blocks, std::max<size_t>(fit, 1)});
}

hipError_t launch_link_decode(const aft_link &link, const float *llr, const unsigned long long *keys, int info_bits, int rate,
                              unsigned coded_bits, unsigned blocks, unsigned long long stride, float qgain, int32_t *counts,
                              unsigned char *bits, int batch, hipStream_t st) {
    LinkCodeArgs a{};
    a.c = link;
    a.llr = llr; a.keys = keys; a.counts = counts; a.bits = bits;
    a.elems = (unsigned)((unsigned long long)link.num_scs * (unsigned long long)link.num_symbols - 1);
    a.info = (unsigned)info_bits; a.steps = a.info + kCodeTail; a.coded = coded_bits; a.blocks = blocks;
    a.used = (unsigned long long)blocks * coded_bits;
    a.stride = stride; a.rate = rate; a.qgain = qgain;
    a.used_inverse = (unsigned long long)(((unsigned __int128)1 << 64) / a.used);      // used >= 10
    const int waves = link_code_waves(a.steps, blocks);
    const size_t lds = (size_t)waves * a.steps * sizeof(unsigned long long);
    static PerDeviceOnce lds_attr;
    const hipError_t e = ensure_dynamic_lds(lds_attr, reinterpret_cast<const void *>(link_decode_kernel), kCodeLdsBudget);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(link_decode_kernel, dim3((unsigned)batch), dim3((unsigned)(waves * kWave)), lds, st, a);
    return hipGetLastError();
}

}  // namespace aft
