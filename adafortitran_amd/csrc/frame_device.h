// What the one-workgroup-per-frame kernels share (k_chansim.hip, k_lmmse.hip, k_link.hip), each written once: the counter-based hash and
// its stream numbers, the Box-Muller noise, and the row-tile pass that writes a row-major [S, T] plane of complex values.  A frame's bits
// are a function of these (adafortitran_amd/chansim.py and linksim.py hold the definitions and the float64 twins).
#pragma once

#include "aft_internal.h"

namespace aft {

// word(kf, stream, index) = splitmix64(kf ^ (stream << 32 | index)): one 64-bit word per (frame key, stream, index)
enum FrameStream : unsigned {
    kStreamCondition = 0,                                       // the frame's conditions (index 0 snr, 1 delay spread, 2 doppler)
    kStreamRayAngle = 1, kStreamRayPhase = 2,                   // a sinusoid's angle of arrival and phase (index 16 tap + ray)
    kStreamPilotNoiseRadius = 3, kStreamPilotNoiseAngle = 4,    // noise on the pilots (index i pilot_symbols + j)
    kStreamDataBits = 5,                                        // the link's sent bits (index q = s T + t)
    kStreamDataNoiseRadius = 6, kStreamDataNoiseAngle = 7,      // ... and the noise on its data symbols
    kStreamCodeBits = 8,                                        // the coded links' information bits (index b K + t, the top bit)
};

__host__ __device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ unsigned long long frame_word(unsigned long long kf, FrameStream stream, unsigned index) {
    return splitmix64(kf ^ ((unsigned long long)stream << 32 | index));
}

// (k + 0.5) 2^-23 from a word's top 23 bits: exact in fp32, never 0, never 1
__device__ __forceinline__ float unit23(unsigned long long word) {
    return ((float)(unsigned)(word >> 41) + 0.5f) * 0x1p-23f;
}

// exp(j 2 pi x) for x in turns, any size: reduced to [0, 1] first
__device__ __forceinline__ float2 cis_turns(float x) {
    float s, c;
    sincospif(2.f * (x - floorf(x)), &s, &c);
    return make_float2(c, s);
}

// Box-Muller: the sample is r (c + j s), r = sigma sqrt(-ln u1), c + j s = exp(j 2 pi u2); the caller adds it with two fused multiply-adds
struct FrameNoise {
    float r, c, s;
};
__device__ __forceinline__ FrameNoise frame_noise(unsigned long long kf, FrameStream radius, FrameStream angle, unsigned index, float sigma) {
    const float u1 = unit23(frame_word(kf, radius, index)), u2 = unit23(frame_word(kf, angle, index));
    const float r = sigma * sqrtf(-logf(u1));
    const float2 z = cis_turns(u2);
    return FrameNoise{r, z.x, z.y};
}

// acc += a b, complex, as two chains of two fused multiply-adds: the one sequence the row-tile pass uses
__device__ __forceinline__ void cfma(float2 &acc, float2 a, float2 b) {
    acc.x = fmaf(a.x, b.x, fmaf(-a.y, b.y, acc.x));
    acc.y = fmaf(a.x, b.y, fmaf(a.y, b.x, acc.y));
}

// ---- the row-tile pass: per time tile of kFrameTile symbols a thread takes one row and kFrameCols of the tile's columns ----
constexpr int kFrameThreads = 256, kFrameTile = 16, kFrameCols = 8;     // tile: symbols; columns: 64 bytes of a row per thread

// A thread's results acc[0 .. n) leave for `row`, their place in the plane: 16-byte stores when `wide` (wide_ok: n is even then), 8-byte
// stores otherwise.  Consecutive lanes hold consecutive rows: a wave's store instruction is a comb of pieces at the rows' pitch.
__device__ __forceinline__ void store_row_piece(float2 *row, const float2 *acc, int n, int wide) {
    AFT_DEV_ASSERT(n >= 1 && n <= kFrameCols);
    if (wide) {
#pragma unroll
        for (int j = 0; j < kFrameCols; j += 2)
            if (j < n) *reinterpret_cast<f32x4 *>(row + j) = f32x4{acc[j].x, acc[j].y, acc[j + 1].x, acc[j + 1].y};
    } else {
#pragma unroll
        for (int j = 0; j < kFrameCols; ++j)
            if (j < n) row[j] = acc[j];
    }
}

// the launchers' decision for 16-byte accesses to row-major [.., T] complex planes: no pair straddles a row, every base is aligned
template <class... Plane>
inline int wide_ok(int T, const Plane *...base) {
    return T % 2 == 0 && (... | reinterpret_cast<uintptr_t>(base)) % 16 == 0 ? 1 : 0;
}

}  // namespace aft
