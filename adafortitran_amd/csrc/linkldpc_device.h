// What the two kernels with the QC-LDPC code in them share (k_linkldpc.hip, k_linkharq.hip), each written once: the base matrix as a
// list of edges, the codeword of a block from the hash's information words, and the layered offset min-sum decoder with its syndrome
// stop rule (adafortitran_amd/linksim.py "the LDPC-coded link" is the definition).  One wave per code block, ONE LANE PER ROW OF A
// CIRCULANT; k_linkldpc.hip's header comment says how a layer runs.  Everything here is force-inlined into its caller.
#pragma once

#include <algorithm>

#include "linkcode_device.h"

namespace aft {

constexpr int kLdpcMaxWaves = 16;                               // waves (code blocks in flight) per workgroup
constexpr int kLdpcMaxRows = 16, kLdpcMaxCols = 32;             // the base matrix
constexpr size_t kLdpcLdsBudget = 150 * 1024;                   // posteriors and messages per workgroup (160 KiB less the static arrays)
constexpr int kLdpcPosteriorMax = 8191, kLdpcMessageMax = 127;
constexpr int kLdpcChunk = 4;                                   // edges of a layer whose LDS reads are in flight together

// The base matrix as the kernels take it, by value: its entries layer by layer, columns increasing (column << 6 | shift), and the first
// entry of every layer.
struct LdpcEdges {
    int rows, cols, edges;                                      // mb, nb, the entries of the base matrix
    unsigned short edge[AFT_LINK_LDPC_MAX_EDGES];
    unsigned char first[kLdpcMaxRows + 1];                      // layer i's edges are first[i] .. first[i + 1] - 1
};

// the information part from the host table, then the parity part (linksim.py "parity part"); false: more than AFT_LINK_LDPC_MAX_EDGES,
// which the entry points have counted and refused
inline bool ldpc_edge_list(int base_rows, int base_cols, const int32_t *shifts, LdpcEdges &out) {
    const int kb = base_cols - base_rows, mid = base_rows / 2;
    int edges = 0;
    for (int i = 0; i < base_rows; ++i) {
        out.first[i] = (unsigned char)edges;
        for (int j = 0; j < base_cols; ++j) {
            int s = -1;
            if (j < kb) s = shifts[i * kb + j];
            else if (j == kb) s = (i == 0 || i == base_rows - 1) ? 1 : i == mid ? 0 : -1;
            else if (j - kb - 1 == i || j - kb == i) s = 0;     // column kb + 1 + t holds rows t and t + 1
            if (s < 0) continue;
            if (edges == AFT_LINK_LDPC_MAX_EDGES) return false;
            out.edge[edges++] = (unsigned short)(j << 6 | s);
        }
    }
    out.first[base_rows] = (unsigned char)edges;
    out.rows = base_rows; out.cols = base_cols; out.edges = edges;
    return true;
}

// the code blocks a workgroup holds at once when a block's state takes `per_wave` bytes of LDS
inline int ldpc_waves(size_t per_wave, unsigned blocks) {
    return (int)std::min<size_t>({(size_t)kLdpcMaxWaves, (size_t)blocks, std::max<size_t>(kLdpcLdsBudget / per_wave, 1)});
}

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

// The tables every workgroup keeps in LDS: the edges and the first edge of every layer.  All threads call it; the caller's barrier
// follows.
__device__ __forceinline__ void ldpc_edge_tables(const LdpcEdges &m, int tid, int threads, unsigned short *edge, int *first) {
    AFT_DEV_ASSERT(m.rows >= 3 && m.rows <= kLdpcMaxRows && m.cols > m.rows && m.cols <= kLdpcMaxCols);
    AFT_DEV_ASSERT(m.edges >= 2 * m.rows && m.edges <= AFT_LINK_LDPC_MAX_EDGES && m.first[m.rows] == m.edges);
    for (int i = tid; i < m.edges; i += threads) edge[i] = m.edge[i];
    if (tid <= m.rows) first[tid] = m.first[tid];
}

// The codeword of the block whose information bits are the hash's stream 8 of key kf from index info0 on: its nb block columns as
// 64-bit words in sent[0 .. nb).  `hard` [mb] holds lam_i for the moment.  edge / first / sent / hard are LDS; ends with a wave_sync.
__device__ __forceinline__ void ldpc_codeword(unsigned long long kf, unsigned info0, const unsigned short *edge, const int *first, int mb,
                                              int nb, unsigned long long *sent, unsigned long long *hard, int lane) {
    const int kb = nb - mb, mid = mb / 2;
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
        unsigned long long p = hard[0] ^ rot64(p0, 1);          // p_1
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
}

// What a decoding attempt leaves: the iterations it ran and, in lane c, the hard bits of block column c (lane_word reads them).
struct LdpcDecoded {
    int ran, hard_lo, hard_hi;
};

// Layered offset min-sum on the posteriors L (int16 [64 nb], the quantised inputs on entry) and the messages R (int8 [edges][64], zero
// on entry), both this wave's LDS and visible to it (a wave_sync has followed their last write): up to max_iters iterations, stopping
// after the first whose hard bits satisfy all 64 mb checks.
__device__ __forceinline__ LdpcDecoded ldpc_min_sum(short *L, signed char *R, const unsigned short *edge, const int *first, int mb, int nb,
                                                    int offset, int max_iters, int lane) {
    LdpcDecoded d{0, 0, 0};
    for (int it = 1; it <= max_iters; ++it) {
        for (int i = 0; i < mb; ++i) {
            const LayerEdges le = layer_edges(edge, first, i, lane, nb);
            signed char *Rl = R + le.e0 * kWave + lane;
            int m1 = 1 << 20, m2 = 1 << 20, at = -1;
            bool tot = false;
            for (int e = 0; e < le.deg; e += kLdpcChunk) {      // the chunk's loads are issued together: one LDS round trip, not four
                int q[kLdpcChunk];
#pragma unroll
                for (int k = 0; k < kLdpcChunk; ++k) {
                    const int ee = min(e + k, le.deg - 1);      // past the end: the last edge again, ignored below
                    q[k] = (int)L[le.variable(ee, lane)] - (int)Rl[ee * kWave];
                }
#pragma unroll
                for (int k = 0; k < kLdpcChunk; ++k) {
                    const bool valid = e + k < le.deg;
                    const int mag = valid ? (q[k] < 0 ? -q[k] : q[k]) : 1 << 20;
                    tot ^= valid && q[k] < 0;
                    if (mag < m1) {                             // the lowest e that attains the minimum
                        m2 = m1;
                        m1 = mag;
                        at = e + k;
                    } else if (mag < m2) {
                        m2 = mag;
                    }
                }
            }
            const int out1 = min(max(m1 - offset, 0), kLdpcMessageMax), out2 = min(max(m2 - offset, 0), kLdpcMessageMax);
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
                    if (e + k >= le.deg) break;                 // wave-uniform
                    const int mag = e + k == at ? out2 : out1;
                    const int r = (tot != (q[k] < 0)) ? -mag : mag;
                    Rl[(e + k) * kWave] = (signed char)r;
                    L[v[k]] = (short)min(max(q[k] + r, -kLdpcPosteriorMax), kLdpcPosteriorMax);
                }
            }
            wave_sync();                                        // the next layer reads what other lanes wrote
        }
        d.ran = it;
        for (int col = 0; col < nb; col += kLdpcChunk) {
            short l[kLdpcChunk];
#pragma unroll
            for (int k = 0; k < kLdpcChunk; ++k) l[k] = L[min(col + k, nb - 1) * kWave + lane];
#pragma unroll
            for (int k = 0; k < kLdpcChunk; ++k) {              // past the last column: a lane whose word is never read
                const unsigned long long w = __ballot(l[k] < 0);
                if (lane == col + k) {
                    d.hard_lo = (int)(unsigned)w;
                    d.hard_hi = (int)(unsigned)(w >> 32);
                }
            }
        }
        unsigned long long unsatisfied = 0;                     // wave-uniform: lane reads of the edges and of the hard words
        for (int i = 0; i < mb; ++i) {
            const LayerEdges le = layer_edges(edge, first, i, lane, nb);
            unsigned long long s = 0;
            for (int e = 0; e < le.deg; ++e) {
                const unsigned ed = le.word(e);
                s ^= rot64(lane_word(d.hard_lo, d.hard_hi, (int)(ed >> 6)), ed & 63u);
            }
            unsatisfied |= s;
        }
        if (unsatisfied == 0) break;
    }
    return d;
}

}  // namespace aft
