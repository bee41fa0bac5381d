// stamp_report.h -- the diagnostic build's reports (-DAFT_DIAG_STAMPS, switch AFT_STAMPS) as plain host C++: no HIP, so that a host
// compiler builds them for tests/test_stamp_report.py.  Each function takes the stamp table of ONE launch as StampRun::collect()
// returns it -- h[row * kStampSlots + slot], an unwritten slot is 0 -- and the few launch facts it prints.  Which slot holds what:
// at the AFT_STAMP sites of the kernel.  s_memtime counts shader cycles, s_memrealtime 100 MHz ticks (hence "/ 100.0" = us).
#pragma once

#include <algorithm>
#include <cstdio>
#include <vector>

#include "stamps.h"

namespace aft {

constexpr int kStampRows = 16384;   // rows of a device's stamp buffer (aft_stamps.hip)
// The capacity rule: a launch is stamped only when every row it can write lies inside the buffer.
inline bool stamp_rows_fit(long long rows) { return rows > 0 && rows <= kStampRows; }

using StampWord = unsigned long long;
constexpr int kSl = kStampSlots;

// (xcc, hw cu id) of a chain tile's slot 14 = HW_ID << 32 | XCC_ID, as an index below 8 * 4096: cu_id, se_id, sh_id
inline unsigned stamp_cu_index(StampWord id) {
    const unsigned hw = (unsigned)(id >> 32), xcc = (unsigned)id & 7;
    return xcc * 4096 + (((hw >> 8) & 0xf) | (((hw >> 13) & 0x7) << 4) | (((hw >> 12) & 1) << 7));
}

// chain_kernel<D, MLP, QKV>: one row per 32-row tile (`nblk`), walked by `blocks` persistent workgroups; per_cu = the occupancy query
inline void report_chain(FILE *f, const StampWord *h, int nblk, int blocks, int D, int mlp, int qkv, int per_cu, size_t lds) {
    double sum[12] = {0};
    for (int b = 0; b < nblk; ++b)
        for (int i = 1; i < 12; ++i) {
            int k = i - 1;
            while (k > 0 && h[b * kSl + k] == 0) --k;   // a phase this variant does not run leaves its slot unwritten
            if (h[b * kSl + i]) sum[i] += (double)(h[b * kSl + i] - h[b * kSl + k]);
        }
    fprintf(f, "chain<%d,mlp=%d,qkv=%d> %d blocks/CU at %zu B LDS; mean cycles per phase:", D, mlp, qkv, per_cu, lds);
    for (int i = 1; i < 12; ++i) fprintf(f, " [%d]=%.0f", i, sum[i] / nblk);
    fprintf(f, "\n");
    // residency: busy tile-time per (xcc, hw cu id) / kernel span
    StampWord t0 = ~0ull, t1 = 0;
    std::vector<double> busy(8 * 4096, 0.0);
    std::vector<int> cnt(8 * 4096, 0);
    for (int b = 0; b < nblk; ++b) {
        const StampWord s0 = h[b * kSl + 12], s1 = h[b * kSl + 13];
        t0 = std::min(t0, s0); t1 = std::max(t1, s1);
        busy[stamp_cu_index(h[b * kSl + 14])] += (double)(s1 - s0);
        cnt[stamp_cu_index(h[b * kSl + 14])]++;
    }
    int ncu = 0, mn = 1 << 30, mx = 0; double tot = 0;
    for (size_t i = 0; i < busy.size(); ++i) if (cnt[i]) { ++ncu; tot += busy[i]; mn = std::min(mn, cnt[i]); mx = std::max(mx, cnt[i]); }
    fprintf(f, "  span %.1f us; %d distinct CUs; tiles/CU min %d max %d; mean concurrent workgroups per CU %.2f; mean tile time %.1f us\n",
            (t1 - t0) / 100.0, ncu, mn, mx, tot / ncu / (double)(t1 - t0), tot / nblk / 100.0);
    {   // is the spread of finish times WITHIN a CU (arbitration between its workgroups) or ACROSS CUs / XCDs?
        std::vector<double> first(8 * 4096, 1e30), last(8 * 4096, 0.0);
        double xlast[8] = {0}; int xn[8] = {0};
        for (int b = std::max(nblk - blocks, 0); b < nblk; ++b) {   // every workgroup's last tile
            const unsigned cu = stamp_cu_index(h[b * kSl + 14]);
            const double en = (h[b * kSl + 13] - t0) / 100.0;
            first[cu] = std::min(first[cu], en); last[cu] = std::max(last[cu], en);
        }
        double fmin = 1e30, fmax = 0, fsum = 0, lmin = 1e30, lmax = 0, lsum = 0; int n = 0;
        for (size_t i = 0; i < last.size(); ++i) if (last[i] > 0) {
            ++n; fmin = std::min(fmin, first[i]); fmax = std::max(fmax, first[i]); fsum += first[i];
            lmin = std::min(lmin, last[i]); lmax = std::max(lmax, last[i]); lsum += last[i];
            xlast[i / 4096] += last[i]; xn[i / 4096]++;
        }
        fprintf(f, "  per CU, last-round tiles: first workgroup done %.1f / %.1f / %.1f us, last workgroup done %.1f / %.1f / %.1f us (min/mean/max over %d CUs)\n",
                fmin, fsum / n, fmax, lmin, lsum / n, lmax, n);
        fprintf(f, "  mean finish per XCD:");
        for (int x = 0; x < 8; ++x) fprintf(f, " %.1f", xn[x] ? xlast[x] / xn[x] : 0.0);
        fprintf(f, "\n");
    }
    for (int r0 = 0; r0 < nblk; r0 += blocks) {   // persistent rounds: when do their tiles start / end
        double smin = 1e30, smax = 0, ssum = 0, emin = 1e30, emax = 0, esum = 0;
        const int r1 = std::min(nblk, r0 + blocks);
        for (int b = r0; b < r1; ++b) {
            const double st = (h[b * kSl + 12] - t0) / 100.0, en = (h[b * kSl + 13] - t0) / 100.0;
            smin = std::min(smin, st); smax = std::max(smax, st); ssum += st;
            emin = std::min(emin, en); emax = std::max(emax, en); esum += en;
        }
        fprintf(f, "  round %d (%d tiles): start %.1f / %.1f / %.1f us (min/mean/max), end %.1f / %.1f / %.1f us\n", r0 / blocks, r1 - r0,
                smin, ssum / (r1 - r0), smax, emin, esum / (r1 - r0), emax);
    }
    fflush(f);
}

// attn_kernel: one row per task (`n`), four tasks per round of each of `blocks` workgroups; slots 0 .. 4 cycles, 6 / 5 = start / end ticks
inline void report_attn(FILE *f, const StampWord *h, int n, int blocks, int tokpad) {
    double sum[5] = {0};
    for (int t = 0; t < n; ++t)
        for (int i = 1; i < 5; ++i) sum[i] += (double)(h[t * kSl + i] - h[t * kSl + i - 1]);
    double clk = 0;
    for (int t = 0; t < n; ++t) clk += (double)(h[t * kSl + 4] - h[t * kSl + 0]) / (double)(h[t * kSl + 5] - h[t * kSl + 6]) * 100e6;
    fprintf(f, "in-kernel shader clock: %.3f GHz\n", clk / n / 1e9);
    fprintf(f, "attn stamps: mean per task: prologue=%.0f loop=%.0f store=%.0f (cycles); MFMA ideal %d\n", sum[1] / n, sum[2] / n,
            sum[4] / n, 32 * (tokpad / 32) * 64);
    // schedule: when do the tasks of each persistent round start / end
    StampWord t0 = ~0ull, t1 = 0;
    for (int t = 0; t < n; ++t) { t0 = std::min(t0, h[t * kSl + 6]); t1 = std::max(t1, h[t * kSl + 5]); }
    const int per_round = blocks * 4;
    double busy = 0;
    for (int t = 0; t < n; ++t) busy += (double)(h[t * kSl + 5] - h[t * kSl + 6]);
    fprintf(f, "  span %.1f us, %d tasks in rounds of %d; mean concurrent waves per SIMD %.2f\n", (t1 - t0) / 100.0, n, per_round,
            busy / (double)(t1 - t0) / 1024.0);
    for (int r0 = 0; r0 < n; r0 += per_round) {
        double smin = 1e30, smax = 0, ssum = 0, emin = 1e30, emax = 0, esum = 0;
        const int r1 = std::min(n, r0 + per_round);
        for (int t = r0; t < r1; ++t) {
            const double st = (h[t * kSl + 6] - t0) / 100.0, en = (h[t * kSl + 5] - t0) / 100.0;
            smin = std::min(smin, st); smax = std::max(smax, st); ssum += st;
            emin = std::min(emin, en); emax = std::max(emax, en); esum += en;
        }
        fprintf(f, "  round %d: start %.1f / %.1f / %.1f us (min/mean/max), end %.1f / %.1f / %.1f us\n", r0 / per_round, smin,
                ssum / (r1 - r0), smax, emin, esum / (r1 - r0), emax);
    }
    fflush(f);
}

// conv_stack_kernel (banded conv, inference): one row per workgroup (`nb` = planes x bands x column tiles), thread 0
inline void report_conv(FILE *f, const StampWord *h, int nb, int mode) {
    double sum[9] = {0};
    for (int b = 0; b < nb; ++b)
        for (int i = 1; i < 9; ++i) sum[i] += (double)(h[b * kSl + i] - h[b * kSl + i - 1]);
    fprintf(f, "conv mode %d stamps (mean cycles, thread 0): weights=%.0f zero=%.0f input=%.0f conv1=%.0f mfma(wave0)=%.0f "
            "wait=%.0f fixup=%.0f conv4=%.0f total=%.0f\n", mode, sum[1] / nb, sum[2] / nb, sum[3] / nb, sum[4] / nb, sum[5] / nb,
            sum[6] / nb, sum[7] / nb, sum[8] / nb, (sum[1] + sum[2] + sum[3] + sum[4] + sum[5] + sum[6] + sum[7] + sum[8]) / nb);
    fflush(f);
}

// conv_stream16_kernel: one row per workgroup of the stamped launch (`nb` = its planes x `nsplit` column ranges; a remainder launch
// behind it is not stamped: `launches` says how many there were); matrix wave in slots 0 .. 6, helper wave in 8 .. 15
inline void report_conv_stream(FILE *f, const StampWord *h, int nb, int mode, int nsplit, int launches) {
    double m[7] = {0}, hsum[7] = {0}, in_lds = 0;
    for (int b = 0; b < nb; ++b) {
        for (int i = 1; i < 7; ++i) {
            m[i] += (double)(h[b * kSl + i] - h[b * kSl + i - 1]);
            hsum[i] += (double)(h[b * kSl + 8 + i] - h[b * kSl + 8 + i - 1]);
        }
        in_lds += (double)(h[b * kSl + 15] - h[b * kSl + 8]);
    }
    fprintf(f, "conv stream16: input plane in LDS %.0f cycles after the kernel's start (helper wave)\n", in_lds / nb);
    fprintf(f, "conv stream mode %d (mean cycles): matrix wave: stage=%.0f gather=%.0f wait=%.0f sweeps=%.0f wait=%.0f store=%.0f | "
            "helper wave: stage=%.0f zero+input+conv1=%.0f wait=%.0f conv4=%.0f wait=%.0f store=%.0f\n", mode, m[1] / nb, m[2] / nb,
            m[3] / nb, m[4] / nb, m[5] / nb, m[6] / nb, hsum[1] / nb, hsum[2] / nb, hsum[3] / nb, hsum[4] / nb, hsum[5] / nb, hsum[6] / nb);
    fprintf(f, "  stamped: launch 1 of %d, %d workgroups, %d column range(s) per plane\n", launches, nb, nsplit);
    fflush(f);
}

// chain_fwd_train_kernel<QKV>: one row per 32-row tile (`ntiles`), `blocks` persistent workgroups; slots 0 .. 8 cycles, 9 = start tick
inline void report_chain_train(FILE *f, const StampWord *h, int ntiles, int blocks, int qkv) {
    const int nb = std::min(blocks, ntiles);
    StampWord t0 = ~0ull, tend = 0;
    for (int t = 0; t < nb; ++t) t0 = std::min(t0, h[t * kSl + 9]);
    for (int t = 0; t < ntiles; ++t) tend = std::max(tend, h[t * kSl + 9]);
    int late = 0;
    double mean = 0, mx = 0;
    for (int t = 0; t < nb; ++t) {
        const double us = (double)(h[t * kSl + 9] - t0) * 0.01;
        mean += us; mx = std::max(mx, us); late += us > 20.0;
    }
    fprintf(f, "chain_fwd_train<QKV=%d>: %d workgroups, first tile starts %.1f us (mean) / %.1f us (max) after the earliest, %d later than 20 us; "
            "the launch's last tile starts at %.1f us\n", qkv, nb, mean / nb, mx, late, (double)(tend - t0) * 0.01);
    double sum[9] = {0};
    for (int t = 0; t < ntiles; ++t)
        for (int i = 1; i < 9; ++i) sum[i] += (double)(h[t * kSl + i] - h[t * kSl + i - 1]);
    fprintf(f, "  mean cycles per tile: outproj=%.0f s1+LN1+x1+barrier=%.0f ffn_up=%.0f act+a+hd+barrier=%.0f ffn_down=%.0f s2+LN2+out=%.0f "
            "qkv=%.0f end_barrier=%.0f total=%.0f\n", sum[1] / ntiles, sum[2] / ntiles, sum[3] / ntiles, sum[4] / ntiles, sum[5] / ntiles,
            sum[6] / ntiles, sum[7] / ntiles, sum[8] / ntiles,
            (sum[1] + sum[2] + sum[3] + sum[4] + sum[5] + sum[6] + sum[7] + sum[8]) / ntiles);
    fflush(f);
}

}  // namespace aft
