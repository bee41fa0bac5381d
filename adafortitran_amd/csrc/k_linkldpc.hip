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
// No atomics, no workspace: everything is integer after the quantiser, whose one float32 product and round-to-nearest-even are the
// definition's.
#include "linkcode_device.h"

namespace aft {
namespace {

constexpr int kLdpcMaxWaves = 16;                               // waves (code blocks in flight) per workgroup
constexpr int kLdpcMaxRows = 16, kLdpcMaxCols = 32;             // the base matrix
constexpr size_t kLdpcLdsBudget = 150 * 1024;                   // posteriors and messages per workgroup (160 KiB less the static arrays)
constexpr int kLdpcPosteriorMax = 8191, kLdpcMessageMax = 127;
constexpr int kLdpcChunk = 4;                                   // edges of a layer whose LDS reads are in flight together

struct LinkLdpcArgs {
    aft_link c;
    const float *llr;
    const unsigned long long *keys;
    int *counts;
    unsigned char *bits;                                        // may be NULL
    unsigned long long used, stride, used_inverse, stride64;    // U, the interleaver's stride, floor(2^64 / U), 64 stride mod U
    unsigned elems;                                             // S T - 1, as in k_link.hip
    unsigned blocks;                                            // B
    int rows, cols, edges;                                      // mb, nb, the entries of the base matrix
    int offset, max_iters;
    float qgain;
    unsigned short edge[AFT_LINK_LDPC_MAX_EDGES];               // layer by layer, columns increasing: column << 6 | shift
    unsigned char first[kLdpcMaxRows + 1];                      // layer i's edges are first[i] .. first[i + 1] - 1
};

__device__ __forceinline__ unsigned long long rot64(unsigned long long x, unsigned s) {       // rot(x, s)[r] = x[(r + s) mod 64]
    return x >> s | x << ((64u - s) & 63u);
}

// A wave's LDS writes become visible to its own later reads from other lanes: requests of one wave are served in order, so this
// only keeps the compiler from moving accesses across it.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A layer's edges, one per lane (a row has at most 32): a lane read makes an edge's word wave-uniform without an LDS round trip.
struct LayerEdges {
    int e0, deg, mine;
    __device__ __forceinline__ unsigned word(int e) const { return (unsigned)__builtin_amdgcn_readlane(mine, e); }
    // the variable of row `lane` on edge e: 64 column + ((lane + shift) mod 64)
    __device__ __forceinline__ unsigned variable(int e, int lane) const {
        const unsigned ed = word(e);
        return (ed & ~63u) | (((unsigned)lane + ed) & 63u);
    }
};
__device__ __forceinline__ LayerEdges layer_edges(const unsigned short *edge, const int *first, int i, int lane, int nb) {
    LayerEdges le;
    le.e0 = __builtin_amdgcn_readfirstlane(first[i]);
    le.deg = __builtin_amdgcn_readfirstlane(first[i + 1]) - le.e0;
    AFT_DEV_ASSERT(le.deg >= 2 && le.deg <= kLdpcMaxCols);
    le.mine = lane < le.deg ? (int)edge[le.e0 + lane] : 0;
    AFT_DEV_ASSERT((le.mine >> 6) < nb);                        // every variable it names lies inside the block's n posteriors
    return le;
}

// the 64-bit word lane `c` holds in (lo, hi), wave-uniform
__device__ __forceinline__ unsigned long long lane_word(int lo, int hi, int c) {
    return (unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, c) << 32 | (unsigned)__builtin_amdgcn_readlane(lo, c);
}

__global__ __launch_bounds__(kLdpcMaxWaves *kWave) void link_ldpc_kernel(const LinkLdpcArgs a) {
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
    const int mb = a.rows, nb = a.cols, kb = nb - mb, mid = mb / 2, edges = a.edges;
    const unsigned T = (unsigned)c.num_symbols, n = (unsigned)nb * kWave, K = (unsigned)kb * kWave;
    AFT_DEV_ASSERT(Ps >= 1 && Ps <= AFT_CHANSIM_MAX_PILOT_SCS && Pt >= 1 && Pt <= AFT_CHANSIM_MAX_PILOT_SYMBOLS && (unsigned)Pt <= T);
    AFT_DEV_ASSERT(waves >= 1 && waves <= kLdpcMaxWaves && mb >= 3 && mb <= kLdpcMaxRows && nb > mb && nb <= kLdpcMaxCols);
    AFT_DEV_ASSERT(edges >= 2 * mb && edges <= AFT_LINK_LDPC_MAX_EDGES && a.first[mb] == edges);
    code_pilot_tables(c, tid, psc, before, psym);
    for (int i = tid; i < edges; i += (int)blockDim.x) edge[i] = a.edge[i];
    if (tid <= mb) first[tid] = a.first[tid];
    __syncthreads();
    const unsigned long long kf = a.keys[f];
    const float *llr = a.llr + f * ((size_t)a.elems + 1) * (size_t)m;
    const size_t per_wave = (size_t)n * sizeof(short) + (size_t)edges * kWave;
    short *L = reinterpret_cast<short *>(state_all + (size_t)wave * per_wave);
    signed char *R = reinterpret_cast<signed char *>(L + n);
    unsigned long long *sent = sent_all[wave], *hard = hard_all[wave];

    int bit_errors = 0, block_errors = 0, iterations = 0;
    for (unsigned b = (unsigned)wave; b < a.blocks; b += (unsigned)waves) {
        // the codeword: the information words from the hash, lam_i into `hard` for the moment, then the parity words
        const unsigned info0 = b * K;                           // B K <= 2^31: the hash's index does not wrap
        for (int j = 0; j < kb; ++j) {
            const unsigned long long w = __ballot((frame_word(kf, kStreamCodeBits, info0 + (unsigned)(j * kWave + lane)) >> 63) != 0);
            if (lane == 0) sent[j] = w;
        }
        wave_sync();
        unsigned long long p0 = 0;
        for (int i = 0; i < mb; ++i) {
            unsigned long long lam = 0;
            for (int e = first[i]; e < first[i + 1]; ++e) {
                const unsigned ed = edge[e];
                if ((int)(ed >> 6) < kb) lam ^= rot64(sent[ed >> 6], ed & 63u);
            }
            if (lane == 0) hard[i] = lam;
            p0 ^= lam;
        }
        wave_sync();
        {
            unsigned long long p = hard[0] ^ rot64(p0, 1);      // p_1
            if (lane == 0) {
                sent[kb] = p0;
                sent[kb + 1] = p;
            }
            for (int i = 1; i < mb - 1; ++i) {
                p ^= hard[i] ^ (i == mid ? p0 : 0ull);
                if (lane == 0) sent[kb + i + 1] = p;
            }
        }
        wave_sync();

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

        int ran = 0, hard_lo = 0, hard_hi = 0;                  // lane c holds the hard bits of block column c after an iteration
        for (int it = 1; it <= a.max_iters; ++it) {
            for (int i = 0; i < mb; ++i) {
                const LayerEdges le = layer_edges(edge, first, i, lane, nb);
                signed char *Rl = R + le.e0 * kWave + lane;
                int m1 = 1 << 20, m2 = 1 << 20, at = -1;
                bool tot = false;
                for (int e = 0; e < le.deg; e += kLdpcChunk) {  // the chunk's loads are issued together: one LDS round trip, not four
                    int q[kLdpcChunk];
#pragma unroll
                    for (int k = 0; k < kLdpcChunk; ++k) {
                        const int ee = min(e + k, le.deg - 1);  // past the end: the last edge again, ignored below
                        q[k] = (int)L[le.variable(ee, lane)] - (int)Rl[ee * kWave];
                    }
#pragma unroll
                    for (int k = 0; k < kLdpcChunk; ++k) {
                        const bool valid = e + k < le.deg;
                        const int mag = valid ? (q[k] < 0 ? -q[k] : q[k]) : 1 << 20;
                        tot ^= valid && q[k] < 0;
                        if (mag < m1) {                         // the lowest e that attains the minimum
                            m2 = m1;
                            m1 = mag;
                            at = e + k;
                        } else if (mag < m2) {
                            m2 = mag;
                        }
                    }
                }
                const int out1 = min(max(m1 - a.offset, 0), kLdpcMessageMax), out2 = min(max(m2 - a.offset, 0), kLdpcMessageMax);
                for (int e = 0; e < le.deg; e += kLdpcChunk) {
                    int q[kLdpcChunk];
                    unsigned v[kLdpcChunk];
#pragma unroll
                    for (int k = 0; k < kLdpcChunk; ++k) {
                        const int ee = min(e + k, le.deg - 1);
                        v[k] = le.variable(ee, lane);
                        q[k] = (int)L[v[k]] - (int)Rl[ee * kWave];
                    }
#pragma unroll
                    for (int k = 0; k < kLdpcChunk; ++k) {
                        if (e + k >= le.deg) break;             // wave-uniform
                        const int mag = e + k == at ? out2 : out1;
                        const int r = (tot != (q[k] < 0)) ? -mag : mag;
                        Rl[(e + k) * kWave] = (signed char)r;
                        L[v[k]] = (short)min(max(q[k] + r, -kLdpcPosteriorMax), kLdpcPosteriorMax);
                    }
                }
                wave_sync();                                    // the next layer reads what other lanes wrote
            }
            ran = it;
            for (int col = 0; col < nb; col += kLdpcChunk) {
                short l[kLdpcChunk];
#pragma unroll
                for (int k = 0; k < kLdpcChunk; ++k) l[k] = L[min(col + k, nb - 1) * kWave + lane];
#pragma unroll
                for (int k = 0; k < kLdpcChunk; ++k) {          // past the last column: a lane whose word is never read
                    const unsigned long long w = __ballot(l[k] < 0);
                    if (lane == col + k) {
                        hard_lo = (int)(unsigned)w;
                        hard_hi = (int)(unsigned)(w >> 32);
                    }
                }
            }
            unsigned long long unsatisfied = 0;                 // wave-uniform: lane reads of the edges and of the hard words
            for (int i = 0; i < mb; ++i) {
                const LayerEdges le = layer_edges(edge, first, i, lane, nb);
                unsigned long long s = 0;
                for (int e = 0; e < le.deg; ++e) {
                    const unsigned ed = le.word(e);
                    s ^= rot64(lane_word(hard_lo, hard_hi, (int)(ed >> 6)), ed & 63u);
                }
                unsatisfied |= s;
            }
            if (unsatisfied == 0) break;
        }

        unsigned long long wrong_any = 0;
        for (int col = 0; col < kb; ++col) {
            const unsigned long long got = lane_word(hard_lo, hard_hi, col), wrong = got ^ sent[col];
            bit_errors += __popcll(wrong);
            wrong_any |= wrong;
            if (a.bits != nullptr) a.bits[(f * a.blocks + b) * (size_t)K + (unsigned)(col * kWave + lane)] = (unsigned char)(got >> lane & 1ull);
        }
        block_errors += wrong_any != 0 ? 1 : 0;
        iterations += ran;
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

}  // namespace

int link_ldpc_waves(int base_cols, int edges, unsigned blocks) {
    const size_t per_wave = (size_t)base_cols * kWave * sizeof(short) + (size_t)edges * kWave;
    return (int)std::min<size_t>({(size_t)kLdpcMaxWaves, (size_t)blocks, std::max<size_t>(kLdpcLdsBudget / per_wave, 1)});
}

hipError_t launch_link_ldpc(const aft_link &link, const float *llr, const unsigned long long *keys, int base_rows, int base_cols,
                            const int32_t *shifts, unsigned blocks, unsigned long long stride, float qgain, int offset, int max_iters,
                            int32_t *counts, unsigned char *bits, int batch, hipStream_t st) {
    LinkLdpcArgs a{};
    a.c = link;
    a.llr = llr; a.keys = keys; a.counts = counts; a.bits = bits;
    a.elems = (unsigned)((unsigned long long)link.num_scs * (unsigned long long)link.num_symbols - 1);
    a.blocks = blocks;
    a.rows = base_rows; a.cols = base_cols; a.offset = offset; a.max_iters = max_iters; a.qgain = qgain;
    a.used = (unsigned long long)blocks * (unsigned long long)(base_cols * kWave);
    a.stride = stride;
    a.stride64 = (unsigned long long)((unsigned __int128)stride * kWave % a.used);
    a.used_inverse = (unsigned long long)(((unsigned __int128)1 << 64) / a.used);      // used >= 256
    // the edges layer by layer: the information part from the table, then the parity part (linksim.py "parity part")
    const int kb = base_cols - base_rows, mid = base_rows / 2;
    int edges = 0;
    for (int i = 0; i < base_rows; ++i) {
        a.first[i] = (unsigned char)edges;
        for (int j = 0; j < base_cols; ++j) {
            int s = -1;
            if (j < kb) s = shifts[i * kb + j];
            else if (j == kb) s = (i == 0 || i == base_rows - 1) ? 1 : i == mid ? 0 : -1;
            else if (j - kb - 1 == i || j - kb == i) s = 0;     // column kb + 1 + t holds rows t and t + 1
            if (s < 0) continue;
            if (edges == AFT_LINK_LDPC_MAX_EDGES) return hipErrorInvalidValue;         // aft_link_ldpc_f32 has counted them
            a.edge[edges++] = (unsigned short)(j << 6 | s);
        }
    }
    a.first[base_rows] = (unsigned char)edges;
    a.edges = edges;
    const int waves = link_ldpc_waves(base_cols, edges, blocks);
    const size_t lds = (size_t)waves * ((size_t)base_cols * kWave * sizeof(short) + (size_t)edges * kWave);
    static PerDeviceOnce lds_attr;
    const hipError_t e = ensure_dynamic_lds(lds_attr, reinterpret_cast<const void *>(link_ldpc_kernel), kLdpcLdsBudget);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(link_ldpc_kernel, dim3((unsigned)batch), dim3((unsigned)(waves * kWave)), lds, st, a);
    return hipGetLastError();
}

}  // namespace aft
