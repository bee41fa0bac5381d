// The OFDM channel simulator (include/adafortitran_amd.h "training data made on the device"; adafortitran_amd/chansim.py is the
// definition and the float64 twin).  One workgroup per frame, one launch per batch; a frame is a pure function of (seed, g).
//
//   1. every thread hashes the frame's key and its three conditions (wave-uniform integer arithmetic, no hand-over needed);
//   2. the taps x rays sinusoids -- (turns per symbol, phase in turns) -- go to LDS once;
//   3. per time tile of 16 symbols: the tap gains h_p(t) go to LDS (one thread per (p, t), `rays` sincos each); then a thread takes one
//      subcarrier and 8 of the tile's columns: the tap's delay phasor is formed once per tap in registers and multiplied into the 8
//      gains, which every lane of the wave reads from the same LDS address (a broadcast: no bank conflicts).  A thread's 8 results are
//      64 contiguous bytes of the row-major [S, T] plane and leave as four 16-byte stores (T even, base 16-byte aligned; 8-byte stores
//      otherwise); consecutive lanes hold consecutive rows, so one store instruction of a wave is a comb of 16-byte pieces at the
//      rows' pitch (112 bytes on the default grid) and a cache line is completed by several partial stores, merged in L2.
//      The tile loop is what lets T be anything: LDS holds one tile whatever the grid's length.
//   4. the pilots ride in the first tile: the gains at the pilot symbols are extra items of its gain pass, the Ps x Pt pilot values
//      (channel + Box-Muller noise) extra items of its main pass.
//
// Phases are formed in TURNS and reduced with x - floor(x) (exact in floating point) before sincospi, so the evaluation error of the
// sine does not grow with the argument; what does grow is the rounding of the turn count itself (2^-24 relative), which is what the
// bound of tests/test_chansim_gpu.py is made of.  No atomics, no reads of device buffers (lane-indexed table entries are read from the kernel-argument segment), every output element written exactly once.
//
// The grouped instantiation (aft_channel_sim_group_f32; chansim.py "antenna correlation"): still one workgroup per output frame, member
// a of a group of G = rx * tx frames.  The conditions are hashed from the LEADER's key; the gain pass of a tile (pilot-symbol gains
// included) runs once per source j = 0 .. a -- a wave-uniform loop that stops at a, `mix` being lower triangular --: the ray table of
// frame lead + j is re-staged into the one `ray` array, and a thread adds L[a][j] z_j to the SAME (p, t) items it owns in every pass, so
// the accumulation in `gain` / `pgain` needs no atomics and no barrier of its own (two barriers per source fence the ray table).  The
// main pass and the pilots' noise (the frame's OWN key) are the ungrouped kernel's.  L[a][j] comes from the kernel-argument segment by a
// wave-uniform index.  LDS is 12 KB in every instantiation -- ray 4 KB, gain 4 KB, pgain 4 KB -- whatever T, G and K are.
//
// The sequence instantiation (aft_channel_sim_seq_f32; chansim.py "time continuity"): the grouped kernel on K G frames per sequence,
// slot-major.  Output frame b is member b % G of slot (b / G) % K of its sequence; the conditions and the sources' keys come from the
// SEQUENCE's leader, and the slot enters in one place only: stage_rays_slot moves every ray's phase to the slot's first symbol,
// phi_k = frac(fma(rate, float(k L), phi)) -- one fused multiply-add and one floor per ray, k L exact in float32 -- so tap_gain and
// everything after it are untouched and the float32 error of a phase does not grow with the slot's distance.  With k = 0 the phase is
// the grouped kernel's bit for bit (phi is in [0, 1)).
#include "frame_device.h"

namespace aft {
namespace {

struct ChanSimArgs {
    aft_chansim c;
    float delay_turns[AFT_CHANSIM_MAX_VALUES];     // float(subcarrier_spacing_hz * delay_spread_ns * 1e-9): turns per subcarrier per unit delay
    float doppler_turns[AFT_CHANSIM_MAX_VALUES];   // float(doppler_hz * symbol_period_s): turns per symbol at cos = 1
    unsigned long long seed_key;                   // splitmix64(seed)
    unsigned long long base, start, stride, modulo;
    float2 *ideal, *pilots;
    float *meta;
    int wide;                                      // 1: 16-byte stores into ideal
    static constexpr bool kGrouped = false;
    static constexpr bool kSeq = false;
};

// The grouped launch: the ungrouped arguments (base, start, stride and modulo count GROUPS here) and the packed lower triangle of `mix`,
// row a at a (a + 1) / 2: 136 complex values for the largest group
constexpr int kMixPacked = AFT_CHANSIM_MAX_GROUP * (AFT_CHANSIM_MAX_GROUP + 1) / 2;
struct ChanSimGroupArgs : ChanSimArgs {
    int group;                                     // G = rx * tx
    float2 mix[kMixPacked];
    static constexpr bool kGrouped = true;
};
// The sequence launch: the grouped arguments (base, start, stride and modulo count SEQUENCES here), the slots of a sequence and the
// symbols from one slot's start to the next
struct ChanSimSeqArgs : ChanSimGroupArgs {
    int slots, slot_symbols;
    static constexpr bool kSeq = true;
};
static_assert(sizeof(ChanSimSeqArgs) <= 4096, "kernel arguments travel by value: HIP's limit is 4 KB");

__device__ __forceinline__ int sim_pick(unsigned long long kf, unsigned which, int n) {
    return (int)(((unsigned)(frame_word(kf, kStreamCondition, which) >> 40) * (unsigned)n) >> 24);    // 24-bit word x n <= 16: fits 32 bits
}

__device__ __forceinline__ float2 tap_gain(const aft_chansim &c, const float2 *ray, int p, int t) {
    float re = 0.f, im = 0.f;
    const float ft = (float)t;
    for (int m = 0; m < c.rays; ++m) {
        const float2 r = ray[p * c.rays + m];
        const float2 z = cis_turns(fmaf(r.x, ft, r.y));
        re += z.x;
        im += z.y;
    }
    const float amp = c.tap_amp[p];
    return make_float2(amp * re, amp * im);
}

// conj(exp(j 2 pi s c_p)): the tap's delay phasor at subcarrier s
__device__ __forceinline__ float2 delay_phasor(const aft_chansim &c, float tau, int p, int s) {
    const float2 z = cis_turns((float)s * (tau * c.tap_delay[p]));
    return make_float2(z.x, -z.y);
}

// the frame's ray table: (turns per symbol, phase in turns) per (tap, ray), from the angle and phase streams of key `kf`
__device__ __forceinline__ void stage_rays(float2 *ray, unsigned long long kf, float dop, int P, int M, int tid) {
    for (int i = tid; i < P * M; i += kFrameThreads) {
        const int p = i / M, m = i - p * M;
        const unsigned idx = 16u * p + m;
        const float u = (float)(unsigned)(frame_word(kf, kStreamRayAngle, idx) >> 44) * 0x1p-20f;        // m + u is exact: 4 + 20 bits
        const float turn = ((float)m + u) / (float)M;
        const float phase = (float)(unsigned)(frame_word(kf, kStreamRayPhase, idx) >> 40) * 0x1p-24f;
        ray[i] = make_float2(dop * cospif(2.f * turn), phase);
    }
}

// ... and the table of a later slot of the same rays: the phase moved to the slot's first symbol `first` = float(k L), reduced to [0, 1)
__device__ __forceinline__ void stage_rays_slot(float2 *ray, unsigned long long kf, float dop, float first, int P, int M, int tid) {
    for (int i = tid; i < P * M; i += kFrameThreads) {
        const int p = i / M, m = i - p * M;
        const unsigned idx = 16u * p + m;
        const float u = (float)(unsigned)(frame_word(kf, kStreamRayAngle, idx) >> 44) * 0x1p-20f;        // m + u is exact: 4 + 20 bits
        const float turn = ((float)m + u) / (float)M;
        const float phase = (float)(unsigned)(frame_word(kf, kStreamRayPhase, idx) >> 40) * 0x1p-24f;
        const float rate = dop * cospif(2.f * turn);
        const float x = fmaf(rate, first, phase);
        ray[i] = make_float2(rate, x - floorf(x));
    }
}

template <class Args>
__global__ __launch_bounds__(kFrameThreads) void channel_sim_kernel(const Args a) {
    constexpr bool kGrouped = Args::kGrouped, kSeq = Args::kSeq;
    __shared__ float2 ray[AFT_CHANSIM_MAX_TAPS * AFT_CHANSIM_MAX_RAYS];
    __shared__ float2 gain[AFT_CHANSIM_MAX_TAPS][kFrameTile];
    __shared__ float2 pgain[AFT_CHANSIM_MAX_TAPS][AFT_CHANSIM_MAX_PILOT_SYMBOLS];
    const aft_chansim &c = a.c;
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int S = c.num_scs, T = c.num_symbols, P = c.taps, M = c.rays, Ps = c.pilot_scs, Pt = c.pilot_symbols;
    // ungrouped: g the frame, kc = kf its key.  Grouped: output frame b is member `member` of group base + (start + (b / G) stride) %
    // modulo; kc, the LEADER's key, picks the conditions and kf, the frame's own, draws the pilots' noise
    unsigned long long g, lead = 0;
    int member = 0;
    [[maybe_unused]] float first_symbol = 0.f;                 // the sequence kernel: float(k L), the slot's first absolute symbol
    if constexpr (kSeq) {
        // output frame b is member b % G of group `unit` = b / G of the batch, slot unit % K of the batch's sequence unit / K
        const size_t unit = b / (size_t)a.group, seq = unit / (size_t)a.slots;
        const int slot = (int)(unit - seq * (size_t)a.slots);
        AFT_DEV_ASSERT(a.slots >= 1 && a.slot_symbols >= c.num_symbols && (long long)a.slots * a.slot_symbols <= AFT_CHANSIM_MAX_SLOTS);
        member = (int)(b % (size_t)a.group);
        lead = (a.base + (a.start + seq * a.stride) % a.modulo) * (unsigned long long)(a.group * a.slots);
        g = lead + (unsigned long long)(slot * a.group + member);
        first_symbol = (float)(slot * a.slot_symbols);
    } else if constexpr (kGrouped) {
        member = (int)(b % (size_t)a.group);
        lead = (a.base + (a.start + (b / (size_t)a.group) * a.stride) % a.modulo) * (unsigned long long)a.group;
        g = lead + (unsigned long long)member;
    } else {
        g = a.base + (a.start + b * a.stride) % a.modulo;
    }
    const unsigned long long kf = splitmix64(a.seed_key ^ g);
    const unsigned long long kc = kGrouped ? splitmix64(a.seed_key ^ lead) : kf;
    const int i_snr = sim_pick(kc, 0, c.n_snr), i_ds = sim_pick(kc, 1, c.n_ds), i_dop = sim_pick(kc, 2, c.n_dop);
    AFT_DEV_ASSERT(i_snr < c.n_snr && i_ds < c.n_ds && i_dop < c.n_dop);
    if (tid < 3) a.meta[3 * b + tid] = tid == 0 ? c.snr_db[i_snr] : tid == 1 ? c.delay_spread_ns[i_ds] : c.doppler_hz[i_dop];
    const float dop = a.doppler_turns[i_dop], tau = a.delay_turns[i_ds], sigma = c.noise_sigma[i_snr];

    if constexpr (!kGrouped) {                                  // written out, not stage_rays(): the ungrouped instruction stream stays as it was
        for (int i = tid; i < P * M; i += kFrameThreads) {
            const int p = i / M, m = i - p * M;
            const unsigned idx = 16u * p + m;
            const float u = (float)(unsigned)(frame_word(kf, kStreamRayAngle, idx) >> 44) * 0x1p-20f;    // m + u is exact: 4 + 20 bits
            const float turn = ((float)m + u) / (float)M;
            const float phase = (float)(unsigned)(frame_word(kf, kStreamRayPhase, idx) >> 40) * 0x1p-24f;
            ray[i] = make_float2(dop * cospif(2.f * turn), phase);
        }
        __syncthreads();
    }

    for (int t0 = 0; t0 < T; t0 += kFrameTile) {
        const bool first = t0 == 0;
        if constexpr (kGrouped) {
            AFT_DEV_ASSERT(member < a.group && a.group <= AFT_CHANSIM_MAX_GROUP);
            for (int j = 0; j <= member; ++j) {
                if (!first || j > 0) __syncthreads();                   // the readers of `ray` (and the previous tile's of `gain`) are done
                if constexpr (kSeq)
                    stage_rays_slot(ray, splitmix64(a.seed_key ^ (lead + (unsigned long long)j)), dop, first_symbol, P, M, tid);
                else
                    stage_rays(ray, splitmix64(a.seed_key ^ (lead + (unsigned long long)j)), dop, P, M, tid);
                __syncthreads();
                const float2 l = a.mix[member * (member + 1) / 2 + j];
                for (int i = tid; i < P * kFrameTile + (first ? P * Pt : 0); i += kFrameThreads) {    // item i has one owner in every pass
                    if (i < P * kFrameTile) {
                        const int p = i / kFrameTile, tt = i - p * kFrameTile;
                        float2 h = j == 0 ? make_float2(0.f, 0.f) : gain[p][tt];
                        cfma(h, l, t0 + tt < T ? tap_gain(c, ray, p, t0 + tt) : make_float2(0.f, 0.f));
                        gain[p][tt] = h;
                    } else {
                        const int q = i - P * kFrameTile, p = q / Pt, k = q - p * Pt;
                        AFT_DEV_ASSERT(p < P && c.pilot_symbol_index[k] >= 0 && c.pilot_symbol_index[k] < T);
                        float2 h = j == 0 ? make_float2(0.f, 0.f) : pgain[p][k];
                        cfma(h, l, tap_gain(c, ray, p, c.pilot_symbol_index[k]));
                        pgain[p][k] = h;
                    }
                }
            }
        } else {
            if (!first) __syncthreads();                                // the previous tile's readers are done with `gain`
            for (int i = tid; i < P * kFrameTile + (first ? P * Pt : 0); i += kFrameThreads) {
                if (i < P * kFrameTile) {
                    const int p = i / kFrameTile, tt = i - p * kFrameTile;
                    gain[p][tt] = t0 + tt < T ? tap_gain(c, ray, p, t0 + tt) : make_float2(0.f, 0.f);
                } else {
                    const int q = i - P * kFrameTile, p = q / Pt, j = q - p * Pt;
                    AFT_DEV_ASSERT(p < P && c.pilot_symbol_index[j] >= 0 && c.pilot_symbol_index[j] < T);
                    pgain[p][j] = tap_gain(c, ray, p, c.pilot_symbol_index[j]);
                }
            }
        }
        __syncthreads();

        const int groups = (min(T - t0, kFrameTile) + kFrameCols - 1) / kFrameCols;
        for (int i = tid; i < S * groups + (first ? Ps * Pt : 0); i += kFrameThreads) {
            if (i < S * groups) {
                const int hg = i / S, s = i - hg * S, col = kFrameCols * hg;
                float2 acc[kFrameCols];
#pragma unroll
                for (int j = 0; j < kFrameCols; ++j) acc[j] = make_float2(0.f, 0.f);
                for (int p = 0; p < P; ++p) {
                    const float2 e = delay_phasor(c, tau, p, s);
#pragma unroll
                    for (int j = 0; j < kFrameCols; ++j) cfma(acc[j], gain[p][col + j], e);
                }
                const int n = min(kFrameCols, T - t0 - col);           // valid columns; even when T is
                AFT_DEV_ASSERT(s < S && t0 + col + n <= T);
                store_row_piece(a.ideal + (b * S + s) * (size_t)T + t0 + col, acc, n, a.wide);
            } else {
                const int q = i - S * groups, pi = q / Pt, pj = q - pi * Pt, s = c.pilot_sc_index[pi];
                AFT_DEV_ASSERT(pi < Ps && s >= 0 && s < S);
                float re = 0.f, im = 0.f;
                for (int p = 0; p < P; ++p) {
                    const float2 e = delay_phasor(c, tau, p, s), h = pgain[p][pj];
                    re = fmaf(h.x, e.x, fmaf(-h.y, e.y, re));
                    im = fmaf(h.x, e.y, fmaf(h.y, e.x, im));
                }
                const FrameNoise nz = frame_noise(kf, kStreamPilotNoiseRadius, kStreamPilotNoiseAngle, (unsigned)q, sigma);
                a.pilots[b * (size_t)(Ps * Pt) + q] = make_float2(fmaf(nz.r, nz.c, re), fmaf(nz.r, nz.s, im));
            }
        }
    }
}

}  // namespace

namespace {

void fill_args(ChanSimArgs &a, const aft_chansim &sim, unsigned long long seed, long long base, long long start, long long stride,
               long long modulo, float *ideal, float *pilots, float *meta) {
    a.c = sim;
    for (int i = 0; i < AFT_CHANSIM_MAX_VALUES; ++i) {
        a.delay_turns[i] = i < sim.n_ds ? (float)(sim.subcarrier_spacing_hz * (double)sim.delay_spread_ns[i] * 1e-9) : 0.f;
        a.doppler_turns[i] = i < sim.n_dop ? (float)((double)sim.doppler_hz[i] * sim.symbol_period_s) : 0.f;
    }
    a.seed_key = splitmix64(seed);
    a.base = (unsigned long long)base; a.start = (unsigned long long)start;
    a.stride = (unsigned long long)stride; a.modulo = (unsigned long long)modulo;
    a.ideal = reinterpret_cast<float2 *>(ideal); a.pilots = reinterpret_cast<float2 *>(pilots); a.meta = meta;
    a.wide = wide_ok(sim.num_symbols, ideal);
}

}  // namespace

hipError_t launch_channel_sim(const aft_chansim &sim, unsigned long long seed, long long base, long long start, long long stride,
                              long long modulo, int batch, float *ideal, float *pilots, float *meta, hipStream_t st) {
    ChanSimArgs a{};
    fill_args(a, sim, seed, base, start, stride, modulo, ideal, pilots, meta);
    hipLaunchKernelGGL(channel_sim_kernel<ChanSimArgs>, dim3((unsigned)batch), dim3(kFrameThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_channel_sim_group(const aft_chansim &sim, int group, const float *mix_packed, unsigned long long seed, long long base,
                                    long long start, long long stride, long long modulo, int batch, float *ideal, float *pilots,
                                    float *meta, hipStream_t st) {
    ChanSimGroupArgs a{};
    fill_args(a, sim, seed, base, start, stride, modulo, ideal, pilots, meta);
    a.group = group;
    for (int i = 0; i < group * (group + 1) / 2; ++i) a.mix[i] = make_float2(mix_packed[2 * i], mix_packed[2 * i + 1]);
    hipLaunchKernelGGL(channel_sim_kernel<ChanSimGroupArgs>, dim3((unsigned)batch), dim3(kFrameThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_channel_sim_seq(const aft_chansim &sim, int group, const float *mix_packed, int slots, int slot_symbols,
                                  unsigned long long seed, long long base, long long start, long long stride, long long modulo,
                                  int batch, float *ideal, float *pilots, float *meta, hipStream_t st) {
    ChanSimSeqArgs a{};
    fill_args(a, sim, seed, base, start, stride, modulo, ideal, pilots, meta);
    a.group = group;
    for (int i = 0; i < group * (group + 1) / 2; ++i) a.mix[i] = make_float2(mix_packed[2 * i], mix_packed[2 * i + 1]);
    a.slots = slots;
    a.slot_symbols = slot_symbols;
    hipLaunchKernelGGL(channel_sim_kernel<ChanSimSeqArgs>, dim3((unsigned)batch), dim3(kFrameThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace aft
