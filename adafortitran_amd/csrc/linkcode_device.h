// What the coded links' kernels share (k_linkcode.hip, k_linkldpc.hip), each written once: the interleaver's modulo without a division,
// the walk from a data-bit index to the grid element and the bit that carry it, and the quantiser.  Both codes sit on the link in the
// same place (adafortitran_amd/linksim.py "the coded link").
#pragma once

#include "frame_device.h"

namespace aft {

// x mod u without a division: inv = floor(2^64 / u), so mulhi(x, inv) is the quotient or up to two below it
__device__ __forceinline__ unsigned long long code_mod(unsigned long long x, unsigned long long u, unsigned long long inv) {
    unsigned long long r = x - __umul64hi(x, inv) * u;
    r -= r >= u ? u : 0;
    r -= r >= u ? u : 0;
    AFT_DEV_ASSERT(r < u);
    return r;
}

// p a mod u for p, a < u < 2^35: the product fits 64 bits below 2^32, else in three pieces of 17 bits
__device__ __forceinline__ unsigned long long code_mulmod(unsigned long long p, unsigned long long a, unsigned long long u,
                                                          unsigned long long inv) {
    if (u <= (1ull << 32)) return code_mod(p * a, u, inv);
    const unsigned long long hi = code_mod((p >> 17) * a, u, inv);
    return code_mod(code_mod(hi << 17, u, inv) + code_mod((p & 0x1FFFF) * a, u, inv), u, inv);
}

// grid index of the e-th data element: before[i] data elements lie before pilot row psc[i]
__device__ __forceinline__ unsigned code_grid_index(const int *psc, const unsigned *before, const int *psym, int Ps, int Pt, unsigned T,
                                                    unsigned e) {
    int lo = 0, hi = Ps;
    while (lo < hi) {                                           // lo = #{i : before[i] <= e}
        const int mid = (lo + hi) >> 1;
        if (before[mid] <= e) lo = mid + 1;
        else hi = mid;
    }
    if (lo > 0) {
        const unsigned l = e - before[lo - 1];
        if (l < T - (unsigned)Pt) {                             // inside pilot row lo - 1: the l-th column that is no pilot
            unsigned t = l;
            for (int i = 0; i < Pt; ++i) t += (unsigned)psym[i] <= t ? 1u : 0u;
            return (unsigned)psc[lo - 1] * T + t;
        }
    }
    return e + (unsigned)lo * (unsigned)Pt;                     // as if the lo pilot rows before it were whole
}

// The pilot positions in LDS with, per pilot row, the number of data elements before it (what code_grid_index searches): threads
// 0 .. max(Ps, Pt) - 1 write; the caller's barrier follows.
__device__ __forceinline__ void code_pilot_tables(const aft_link &c, int tid, int *psc, unsigned *before, int *psym) {
    if (tid < c.pilot_scs) {
        psc[tid] = c.pilot_sc_index[tid];
        before[tid] = (unsigned)c.pilot_sc_index[tid] * (unsigned)c.num_symbols - (unsigned)tid * (unsigned)c.pilot_symbols;
    }
    if (tid < c.pilot_symbols) psym[tid] = c.pilot_symbol_index[tid];
}

// data-bit index j = m e + k: bit k of the word of the e-th data element
__device__ __forceinline__ void code_split(unsigned long long j, int m, unsigned &e, unsigned &k) {
    switch (m) {
        case 2: e = (unsigned)(j >> 1); k = (unsigned)j & 1u; break;
        case 4: e = (unsigned)(j >> 2); k = (unsigned)j & 3u; break;
        case 8: e = (unsigned)(j >> 3); k = (unsigned)j & 7u; break;
        default: e = (unsigned)((j >> 1) / 3); k = (unsigned)(j - 6ull * e); break;
    }
}

// the descrambled LLR, quantised: one float32 product, to nearest with ties to even, NaN gives 0
__device__ __forceinline__ int code_quantise(float l, bool turn, float qgain) {
    const float v = (turn ? -l : l) * qgain;
    if (v != v) return 0;
    return (int)fminf(fmaxf(rintf(v), -127.f), 127.f);
}

}  // namespace aft
