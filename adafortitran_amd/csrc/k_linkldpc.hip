// The LDPC-coded link: a quasi-cyclic LDPC code of lifting 64 rides on the link's sent bits in the convolutional code's place, and a
// layered offset min-sum decoder reads the LLR tensor aft_link_soft_f32 writes (include/adafortitran_amd.h "LDPC-coded link";
// adafortitran_amd/linksim.py is the definition and the integer NumPy twin).  One workgroup per frame, one launch per batch; a frame's
// three counts and its decoded bits are a function of its own key and LLRs only.
//
//   1. the pilot positions go to LDS as in k_linkcode.hip, and so does the base matrix as a list of edges in layer order (column and
//      shift in one 16-bit word) with the first edge of every layer;
//   2. a wave takes the frame's code blocks b = wave, wave + W, ...; ONE LANE PER ROW OF A CIRCULANT.  A block column of hard bits is
//      one 64-bit ballot word and rot(x, s) a 64-bit rotate, so encoding the information words taken from the hash is one rotate and
//      XOR per information edge on wave-uniform words, and the syndrome check after an iteration is the same over all edges plus a
//      zero test;
//   3. lane l loads coded bits l, 64 + l, ...: position j = (b n + i) stride mod U by one multiply-high modulo and then steps of
//      64 stride mod U, the grid element by code_grid_index, the sent bit from the hash, the codeword bit from the column's word; the
//      quantised z is the posterior's start, an int16 in LDS;
//   4. a layer: lane l is row l of the layer's circulants and, for l below the row's degree, also holds the layer's l-th edge, so
//      an edge's word is a lane read (wave-uniform, no LDS round trip).  Edge (column j, shift s) reads L[64 j + ((l + s) & 63)],
//      contiguous across the wave with a wrap: no bank conflict.  Two passes over the layer's edges, four edges at a time so that
//      their reads of L and R are in flight together -- the first finds the two smallest |Q|, where the smallest sits and the sign
//      product; the second forms Q again and writes R (int8 [edges][64]) and L.  Rows of a layer share no variable, so no lane
//      reads in a layer what another writes in it; LDS serves a wave's requests in order, so between layers a compiler fence is
//      all that is needed.  After an iteration lane c holds the hard word of block column c; the syndrome is lane reads only;
//   5. a wave's three counts are sums over its blocks; the W waves' counts meet in LDS and three threads store the frame's triple.
//
// Steps 2 and 4 -- the edge list, the codeword and the decoder -- are written once in linkldpc_device.h and shared with the HARQ link
// (k_linkharq.hip).  No atomics, no workspace: everything is integer after the quantiser, whose one float32 product and
// round-to-nearest-even are the definition's.
//
//   link_ldpc_kernel<LinkLdpcArgs>        (aft_link_ldpc_f32)         every frame is decoded
//   link_ldpc_kernel<LinkLdpcMaskedArgs>  (aft_link_ldpc_masked_f32)  the same body; a frame whose mask word is 0 stores zeros and leaves first
#include "linkldpc_device.h"

namespace aft {
namespace {

struct LinkLdpcArgs {
    aft_link c;
    const float *llr;
    const unsigned long long *keys;
    int *counts;
    unsigned char *bits;                                        // may be NULL
    unsigned long long used, stride, used_inverse, stride64;    // U, the interleaver's stride, floor(2^64 / U), 64 stride mod U
    unsigned elems;                                             // S T - 1, as in k_link.hip
    unsigned blocks;                                            // B
    int offset, max_iters;
    float qgain;
    LdpcEdges base;                                             // mb, nb and the entries of the base matrix, layer by layer
};

// what the masked launch adds: one word per frame, mask[f mask_stride]; a frame whose word is 0 is not decoded.  Its own struct: the
// unmasked kernel's arguments stay as they are
struct LinkLdpcMaskedArgs : LinkLdpcArgs {
    const int *mask;
    int mask_stride;
};

// The kernel, once: Args = LinkLdpcArgs is aft_link_ldpc_f32's, Args = LinkLdpcMaskedArgs aft_link_ldpc_masked_f32's, whose workgroups
// read their frame's mask word first -- wave-uniform -- and, where it is 0, store the frame's zeros (three counts, and B K bits when
// asked for) and leave before any barrier and before any LLR is read.
template <class Args>
__global__ __launch_bounds__(kLdpcMaxWaves *kWave) void link_ldpc_kernel(const Args a) {
    constexpr bool Masked = std::is_same<Args, LinkLdpcMaskedArgs>::value;
    extern __shared__ __attribute__((aligned(16))) unsigned char state_all[];    // [waves]: posteriors int16 [n], messages int8 [edges][64]
    __shared__ int psc[AFT_CHANSIM_MAX_PILOT_SCS], psym[AFT_CHANSIM_MAX_PILOT_SYMBOLS];
    __shared__ unsigned before[AFT_CHANSIM_MAX_PILOT_SCS];
    __shared__ unsigned short edge[AFT_LINK_LDPC_MAX_EDGES];
    __shared__ int first[kLdpcMaxRows + 1];
    __shared__ unsigned long long sent_all[kLdpcMaxWaves][kLdpcMaxCols], hard_all[kLdpcMaxWaves][kLdpcMaxCols];
    __shared__ int part[kLdpcMaxWaves][3];
    const aft_link &c = a.c;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), waves = blockDim.x / kWave;
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const size_t f = blockIdx.x;
    const int Ps = c.pilot_scs, Pt = c.pilot_symbols, m = c.bits_per_symbol;
    const int mb = a.base.rows, nb = a.base.cols, kb = nb - mb, edges = a.base.edges;
    const unsigned T = (unsigned)c.num_symbols, n = (unsigned)nb * kWave, K = (unsigned)kb * kWave;
    AFT_DEV_ASSERT(Ps >= 1 && Ps <= AFT_CHANSIM_MAX_PILOT_SCS && Pt >= 1 && Pt <= AFT_CHANSIM_MAX_PILOT_SYMBOLS && (unsigned)Pt <= T);
    AFT_DEV_ASSERT(waves >= 1 && waves <= kLdpcMaxWaves);
    if constexpr (Masked) {
        AFT_DEV_ASSERT(a.mask_stride >= 1);
        if (__builtin_amdgcn_readfirstlane(a.mask[f * (size_t)a.mask_stride]) == 0) {      // the whole workgroup: no barrier has been met
            if (tid < 3) a.counts[3 * f + tid] = 0;
            if (a.bits != nullptr) {
                const size_t per_frame = (size_t)a.blocks * K;  // B K <= 2^31
                for (size_t i = (size_t)tid; i < per_frame; i += blockDim.x) a.bits[f * per_frame + i] = 0;
            }
            return;
        }
    }
    code_pilot_tables(c, tid, psc, before, psym);
    ldpc_edge_tables(a.base, tid, (int)blockDim.x, edge, first);
    __syncthreads();
    const unsigned long long kf = a.keys[f];
    const float *llr = a.llr + f * ((size_t)a.elems + 1) * (size_t)m;
    const size_t per_wave = (size_t)n * sizeof(short) + (size_t)edges * kWave;
    short *L = reinterpret_cast<short *>(state_all + (size_t)wave * per_wave);
    signed char *R = reinterpret_cast<signed char *>(L + n);
    unsigned long long *sent = sent_all[wave], *hard = hard_all[wave];

    int bit_errors = 0, block_errors = 0, iterations = 0;
    for (unsigned b = (unsigned)wave; b < a.blocks; b += (unsigned)waves) {
        // the codeword: the information words from the hash, then the parity words.  B K <= 2^31: the hash's index does not wrap
        ldpc_codeword(kf, b * K, edge, first, mb, nb, sent, hard, lane);

        // the inputs: coded bit i = 64 col + lane of the block sits at j = (b n + i) stride mod U
        unsigned long long j = code_mulmod((unsigned long long)b * n + (unsigned)lane, a.stride, a.used, a.used_inverse);
        for (int col = 0; col < nb; ++col) {
            AFT_DEV_ASSERT(j < a.used);
            unsigned e, k;
            code_split(j, m, e, k);
            const unsigned q = code_grid_index(psc, before, psym, Ps, Pt, T, e);
            AFT_DEV_ASSERT(q <= a.elems && k < (unsigned)m);
            const unsigned w = (unsigned)(frame_word(kf, kStreamDataBits, q) >> (63 - k)) & 1u;
            const unsigned cbit = (unsigned)(sent[col] >> lane) & 1u;
            L[col * kWave + lane] = (short)code_quantise(llr[(size_t)q * m + k], (w ^ cbit) != 0, a.qgain);
            j += a.stride64;
            j -= j >= a.used ? a.used : 0;
        }
        for (int e = 0; e < edges; ++e) R[e * kWave + lane] = 0;
        wave_sync();

        const LdpcDecoded d = ldpc_min_sum(L, R, edge, first, mb, nb, a.offset, a.max_iters, lane);

        unsigned long long wrong_any = 0;
        for (int col = 0; col < kb; ++col) {
            const unsigned long long got = lane_word(d.hard_lo, d.hard_hi, col), wrong = got ^ sent[col];
            bit_errors += __popcll(wrong);
            wrong_any |= wrong;
            if (a.bits != nullptr) a.bits[(f * a.blocks + b) * (size_t)K + (unsigned)(col * kWave + lane)] = (unsigned char)(got >> lane & 1ull);
        }
        block_errors += wrong_any != 0 ? 1 : 0;
        iterations += d.ran;
        wave_sync();                                            // the next block's words go where these were read
    }
    if (lane == 0) {
        part[wave][0] = bit_errors;
        part[wave][1] = block_errors;
        part[wave][2] = iterations;
    }
    __syncthreads();
    if (tid < 3) {                                              // bit errors, block errors, iterations
        int total = 0;
        for (int w = 0; w < waves; ++w) total += part[w][tid];
        a.counts[3 * f + tid] = total;
    }
}

size_t ldpc_state_bytes(int base_cols, int edges) {             // a block's posteriors and messages
    return (size_t)base_cols * kWave * sizeof(short) + (size_t)edges * kWave;
}

}  // namespace

int link_ldpc_waves(int base_cols, int edges, unsigned blocks) { return ldpc_waves(ldpc_state_bytes(base_cols, edges), blocks); }

hipError_t launch_link_ldpc(const aft_link &link, const float *llr, const unsigned long long *keys, int base_rows, int base_cols,
                            const int32_t *shifts, unsigned blocks, unsigned long long stride, float qgain, int offset, int max_iters,
                            int32_t *counts, unsigned char *bits, const int32_t *mask, int mask_stride, int batch, hipStream_t st) {
    LinkLdpcMaskedArgs a{};
    a.c = link;
    a.llr = llr; a.keys = keys; a.counts = counts; a.bits = bits;
    a.elems = (unsigned)((unsigned long long)link.num_scs * (unsigned long long)link.num_symbols - 1);
    a.blocks = blocks;
    a.offset = offset; a.max_iters = max_iters; a.qgain = qgain;
    a.used = (unsigned long long)blocks * (unsigned long long)(base_cols * kWave);
    a.stride = stride;
    a.stride64 = (unsigned long long)((unsigned __int128)stride * kWave % a.used);
    a.used_inverse = (unsigned long long)(((unsigned __int128)1 << 64) / a.used);      // used >= 256
    if (!ldpc_edge_list(base_rows, base_cols, shifts, a.base)) return hipErrorInvalidValue;   // aft_link_ldpc_f32 has counted them
    const int waves = link_ldpc_waves(base_cols, a.base.edges, blocks);
    const size_t lds = (size_t)waves * ldpc_state_bytes(base_cols, a.base.edges);
    if (mask == nullptr) {
        static PerDeviceOnce lds_attr;
        const hipError_t e = ensure_dynamic_lds(lds_attr, reinterpret_cast<const void *>(link_ldpc_kernel<LinkLdpcArgs>), kLdpcLdsBudget);
        if (e != hipSuccess) return e;
        const LinkLdpcArgs plain = a;
        hipLaunchKernelGGL(link_ldpc_kernel<LinkLdpcArgs>, dim3((unsigned)batch), dim3((unsigned)(waves * kWave)), lds, st, plain);
        return hipGetLastError();
    }
    a.mask = mask; a.mask_stride = mask_stride;                 // the masked instantiation of the same body
    static PerDeviceOnce masked_lds_attr;
    const hipError_t e = ensure_dynamic_lds(masked_lds_attr, reinterpret_cast<const void *>(link_ldpc_kernel<LinkLdpcMaskedArgs>), kLdpcLdsBudget);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(link_ldpc_kernel<LinkLdpcMaskedArgs>, dim3((unsigned)batch), dim3((unsigned)(waves * kWave)), lds, st, a);
    return hipGetLastError();
}

}  // namespace aft
