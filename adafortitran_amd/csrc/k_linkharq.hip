// The HARQ link: hybrid ARQ with rate matching and soft combining on the LDPC-coded link (include/adafortitran_amd.h "HARQ link";
// adafortitran_amd/linksim.py "The HARQ link" is the definition and the integer NumPy twin).  A group of Q consecutive LLR frames is
// the Q transmission rounds of one set of code blocks; a round sends C of the mother code's nb block columns, a window of a circular
// buffer in whole columns.  One workgroup per group, one launch per batch; a group's seven counts and its decoded bits are a function
// of its own Q keys and LLR frames only.
//
//   1. the pilot positions and the base matrix's edges go to LDS as in k_linkldpc.hip;
//   2. a wave takes the group's code blocks b = wave, wave + W, ...; one lane per row of a circulant.  Per wave in LDS: the soft buffer
//      Z (int16 [n]), the posteriors L (int16 [n]) and the messages R (int8 [edges][64]).  The codeword comes from the LEADER's key
//      (ldpc_codeword) and Z starts at zero;
//   3. round t: lane l reads transmitted bits l, 64 + l, ... of the block -- position j = (b E + e) stride mod U as on the coded
//      links, the sent word from round t's OWN key, the LLR from round t's own frame -- and ADDS the quantised input into
//      Z[64 ((s_t + e / 64) mod nb) + l].  A lane owns element l of every column, in every round: no conflict, no barrier;
//   4. the lane copies its elements of Z to L, clears R, and the block is decoded from scratch (ldpc_min_sum, shared with
//      k_linkldpc.hip).  The decoded information words are compared with the sent ones: equal means ACKNOWLEDGED, and the wave
//      leaves the block's remaining rounds alone -- the comparison is on wave-uniform words, so the branch is wave-uniform;
//   5. a block that was never acknowledged adds its last attempt's information-bit errors; every block's bits from the last attempt
//      it ran are stored once; a wave's seven counts are sums over its blocks, the W waves' counts meet in LDS and seven threads
//      store them.
//
// No atomics, no workspace; every output element is written.  |Z| <= 127 Q <= 508 fits int16 and lies inside the decoder's clamp.
#include "linkldpc_device.h"

namespace aft {
namespace {

struct LinkHarqArgs {
    aft_link c;
    const float *llr;
    const unsigned long long *keys;
    int *counts;
    unsigned char *bits;                                        // may be NULL
    unsigned long long used, stride, used_inverse, stride64;    // U = B E, the interleaver's stride, floor(2^64 / U), 64 stride mod U
    unsigned elems;                                             // S T - 1, as in k_link.hip
    unsigned blocks;                                            // B
    int tx_cols, rounds;                                        // C, Q
    int starts[AFT_LINK_HARQ_MAX_ROUNDS];                       // s_t
    int offset, max_iters;
    float qgain;
    LdpcEdges base;                                             // the mother code
};

// a 64-bit word every lane holds alike, as a scalar
__device__ __forceinline__ unsigned long long uniform_word(unsigned long long x) {
    return (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(x >> 32)) << 32 |
           (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x);
}

__global__ __launch_bounds__(kLdpcMaxWaves *kWave) void link_harq_kernel(const LinkHarqArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char state_all[];    // [waves]: Z int16 [n], L int16 [n], R int8 [edges][64]
    __shared__ int psc[AFT_CHANSIM_MAX_PILOT_SCS], psym[AFT_CHANSIM_MAX_PILOT_SYMBOLS];
    __shared__ unsigned before[AFT_CHANSIM_MAX_PILOT_SCS];
    __shared__ unsigned short edge[AFT_LINK_LDPC_MAX_EDGES];
    __shared__ int first[kLdpcMaxRows + 1];
    __shared__ unsigned long long sent_all[kLdpcMaxWaves][kLdpcMaxCols], hard_all[kLdpcMaxWaves][kLdpcMaxCols];
    __shared__ int part[kLdpcMaxWaves][AFT_LINK_HARQ_COUNTS];
    const aft_link &c = a.c;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), waves = blockDim.x / kWave;
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const size_t g = blockIdx.x;
    const int Ps = c.pilot_scs, Pt = c.pilot_symbols, m = c.bits_per_symbol;
    const int mb = a.base.rows, nb = a.base.cols, kb = nb - mb, edges = a.base.edges, C = a.tx_cols, Q = a.rounds;
    const unsigned T = (unsigned)c.num_symbols, n = (unsigned)nb * kWave, K = (unsigned)kb * kWave, E = (unsigned)C * kWave;
    AFT_DEV_ASSERT(Ps >= 1 && Ps <= AFT_CHANSIM_MAX_PILOT_SCS && Pt >= 1 && Pt <= AFT_CHANSIM_MAX_PILOT_SYMBOLS && (unsigned)Pt <= T);
    AFT_DEV_ASSERT(waves >= 1 && waves <= kLdpcMaxWaves && Q >= 1 && Q <= AFT_LINK_HARQ_MAX_ROUNDS && C > kb && C <= nb);
    code_pilot_tables(c, tid, psc, before, psym);
    ldpc_edge_tables(a.base, tid, (int)blockDim.x, edge, first);
    __syncthreads();
    const size_t frame = ((size_t)a.elems + 1) * (size_t)m;     // floats of one LLR frame
    const unsigned long long k0 = a.keys[g * (size_t)Q];        // the leader's key: the information bits
    const size_t per_wave = 2 * (size_t)n * sizeof(short) + (size_t)edges * kWave;
    short *Z = reinterpret_cast<short *>(state_all + (size_t)wave * per_wave);
    short *L = Z + n;
    signed char *R = reinterpret_cast<signed char *>(L + n);
    unsigned long long *sent = sent_all[wave], *hard = hard_all[wave];

    int acked[AFT_LINK_HARQ_MAX_ROUNDS] = {0, 0, 0, 0};
    int bit_errors = 0, failed = 0, iterations = 0;
    for (unsigned b = (unsigned)wave; b < a.blocks; b += (unsigned)waves) {
        ldpc_codeword(k0, b * K, edge, first, mb, nb, sent, hard, lane);       // B K <= 2^31: the hash's index does not wrap
        for (int col = 0; col < nb; ++col) Z[col * kWave + lane] = 0;          // this lane's elements only, here and below
        // transmitted bit e = 64 i + lane of the block sits at j = (b E + e) stride mod U, in every round
        const unsigned long long j0 = code_mulmod((unsigned long long)b * E + (unsigned)lane, a.stride, a.used, a.used_inverse);
        LdpcDecoded d{0, 0, 0};
        bool delivered = false;
#pragma unroll 1
        for (int t = 0; t < Q; ++t) {
            const unsigned long long kt = a.keys[g * (size_t)Q + (size_t)t];
            const float *llr = a.llr + (g * (size_t)Q + (size_t)t) * frame;
            AFT_DEV_ASSERT(a.starts[t] >= 0 && a.starts[t] < nb);
            unsigned long long j = j0;
            int col = a.starts[t];
            for (int i = 0; i < C; ++i) {
                AFT_DEV_ASSERT(j < a.used && col >= 0 && col < nb);
                unsigned e, k;
                code_split(j, m, e, k);
                const unsigned q = code_grid_index(psc, before, psym, Ps, Pt, T, e);
                AFT_DEV_ASSERT(q <= a.elems && k < (unsigned)m);
                const unsigned w = (unsigned)(frame_word(kt, kStreamDataBits, q) >> (63 - k)) & 1u;
                const unsigned cbit = (unsigned)(sent[col] >> lane) & 1u;
                Z[col * kWave + lane] = (short)(Z[col * kWave + lane] + code_quantise(llr[(size_t)q * m + k], (w ^ cbit) != 0, a.qgain));
                j += a.stride64;
                j -= j >= a.used ? a.used : 0;
                col = col + 1 == nb ? 0 : col + 1;
            }
            for (int cc = 0; cc < nb; ++cc) L[cc * kWave + lane] = Z[cc * kWave + lane];
            for (int e = 0; e < edges; ++e) R[e * kWave + lane] = 0;
            wave_sync();

            d = ldpc_min_sum(L, R, edge, first, mb, nb, a.offset, a.max_iters, lane);
            iterations += d.ran;
            unsigned long long wrong_any = 0;                   // wave-uniform, and in scalar registers: the branch below is too
            for (int cc = 0; cc < kb; ++cc) wrong_any |= lane_word(d.hard_lo, d.hard_hi, cc) ^ uniform_word(sent[cc]);
            if (wrong_any == 0) {                               // an ideal CRC: acknowledged iff the information bits are the sent ones
#pragma unroll
                for (int r = 0; r < AFT_LINK_HARQ_MAX_ROUNDS; ++r) acked[r] += r == t ? 1 : 0;
                delivered = true;
                break;
            }
        }
        for (int cc = 0; cc < kb; ++cc) {                       // the last attempt the block ran
            const unsigned long long got = lane_word(d.hard_lo, d.hard_hi, cc);
            if (!delivered) bit_errors += __popcll(got ^ sent[cc]);
            if (a.bits != nullptr) a.bits[(g * a.blocks + b) * (size_t)K + (unsigned)(cc * kWave + lane)] = (unsigned char)(got >> lane & 1ull);
        }
        failed += delivered ? 0 : 1;
        wave_sync();                                            // the next block's words go where these were read
    }
    if (lane == 0) {
        for (int t = 0; t < AFT_LINK_HARQ_MAX_ROUNDS; ++t) part[wave][t] = acked[t];
        part[wave][4] = bit_errors;
        part[wave][5] = failed;
        part[wave][6] = iterations;
    }
    __syncthreads();
    if (tid < AFT_LINK_HARQ_COUNTS) {
        int total = 0;
        for (int w = 0; w < waves; ++w) total += part[w][tid];
        a.counts[AFT_LINK_HARQ_COUNTS * g + tid] = total;
    }
}

size_t harq_state_bytes(int base_cols, int edges) {             // a block's soft buffer, posteriors and messages
    return 2 * (size_t)base_cols * kWave * sizeof(short) + (size_t)edges * kWave;
}

}  // namespace

int link_harq_waves(int base_cols, int edges, unsigned blocks) { return ldpc_waves(harq_state_bytes(base_cols, edges), blocks); }

hipError_t launch_link_harq(const aft_link &link, const float *llr, const unsigned long long *keys, int base_rows, int base_cols,
                            const int32_t *shifts, int tx_cols, int rounds, const int32_t *starts, unsigned blocks,
                            unsigned long long stride, float qgain, int offset, int max_iters, int32_t *counts, unsigned char *bits,
                            int batch, hipStream_t st) {
    static_assert(AFT_LINK_HARQ_MAX_ROUNDS == 4 && AFT_LINK_HARQ_COUNTS == AFT_LINK_HARQ_MAX_ROUNDS + 3, "the kernel's count columns");
    LinkHarqArgs a{};
    a.c = link;
    a.llr = llr; a.keys = keys; a.counts = counts; a.bits = bits;
    a.elems = (unsigned)((unsigned long long)link.num_scs * (unsigned long long)link.num_symbols - 1);
    a.blocks = blocks;
    a.tx_cols = tx_cols; a.rounds = rounds;
    for (int t = 0; t < rounds; ++t) a.starts[t] = starts[t];
    a.offset = offset; a.max_iters = max_iters; a.qgain = qgain;
    a.used = (unsigned long long)blocks * (unsigned long long)(tx_cols * kWave);
    a.stride = stride;
    a.stride64 = (unsigned long long)((unsigned __int128)stride * kWave % a.used);
    a.used_inverse = (unsigned long long)(((unsigned __int128)1 << 64) / a.used);      // used >= 128
    if (!ldpc_edge_list(base_rows, base_cols, shifts, a.base)) return hipErrorInvalidValue;   // aft_link_harq_f32 has counted them
    const int waves = link_harq_waves(base_cols, a.base.edges, blocks);
    const size_t lds = (size_t)waves * harq_state_bytes(base_cols, a.base.edges);
    static PerDeviceOnce lds_attr;
    const hipError_t e = ensure_dynamic_lds(lds_attr, reinterpret_cast<const void *>(link_harq_kernel), kLdpcLdsBudget);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(link_harq_kernel, dim3((unsigned)(batch / rounds)), dim3((unsigned)(waves * kWave)), lds, st, a);
    return hipGetLastError();
}

}  // namespace aft
