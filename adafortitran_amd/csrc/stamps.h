// stamps.h -- the diagnostic build's phase stamps (-DAFT_DIAG_STAMPS, switch AFT_STAMPS), device side: the one definition of the
// stamp store.  A kernel that carries a `stamps` pointer writes clock values into row `row` (a tile, a task, a workgroup) of a
// [rows][kStampSlots] table; launchers hand the table in through StampRun (aft_internal.h) and stamp_report.h prints it.  Without
// the flag every macro expands to nothing: the product's kernels carry the pointer (NULL) and no store.
#pragma once

namespace aft {
constexpr int kStampSlots = 16;   // 64-bit words per row, every kernel
}

#ifdef AFT_DIAG_STAMPS
#define AFT_STAMP_VALUE(cond, buf, row, slot, value) \
    do { if ((buf) && (cond)) (buf)[(size_t)(row) * aft::kStampSlots + (slot)] = (value); } while (0)
#else
#define AFT_STAMP_VALUE(cond, buf, row, slot, value) do { } while (0)
#endif
// the shader clock (cycles) / the chip's 100 MHz wall clock (one clock for all XCDs)
#define AFT_STAMP(cond, buf, row, slot) AFT_STAMP_VALUE(cond, buf, row, slot, __builtin_amdgcn_s_memtime())
#define AFT_STAMP_WALL(cond, buf, row, slot) AFT_STAMP_VALUE(cond, buf, row, slot, __builtin_amdgcn_s_memrealtime())
