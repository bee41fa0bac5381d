"""The diagnostic build's reports (csrc/stamp_report.h: plain host C++, no HIP) and its capacity rule, without a GPU.

tests/stamp_report_driver.cpp is compiled with the host compiler and run on stamp tables written here: known cycle counts per phase,
rows with unwritten (zero) slots, two persistent rounds, two XCDs and three hardware CU ids, distinct matrix- and helper-wave rows.
Every printed line is compared with the line formatted here from means, spans and per-round min / mean / max that numpy computes from
the same numbers -- as text: the inputs are chosen so that every printed field is exact at its precision."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SLOTS = 16


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stamp_report") / "driver")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "stamp_report_driver.cpp"), "-o", exe],
                   check=True)
    return exe


def _run(driver, tmp_path, what, table, *facts):
    path = str(tmp_path / (what + ".bin"))
    np.ascontiguousarray(table, dtype="<u8").tofile(path)
    out = subprocess.run([driver, what, path, str(table.shape[0]), *map(str, facts)], check=True, capture_output=True, text=True).stdout
    return out.splitlines()


def _cumulative(start, durations):
    """Clock values at the phase boundaries: `start` [rows] and `durations` [rows][phases] -> [rows][phases + 1]."""
    return np.concatenate([start[:, None], start[:, None] + np.cumsum(durations, axis=1)], axis=1)


def _mmm(v):
    return f"{v.min():.1f} / {v.mean():.1f} / {v.max():.1f}"


def test_capacity_rule(driver):
    """stamp_rows_fit: the buffer holds 16 384 rows.  The default model's 2 240 chain tiles and 9 216 attention tasks at 128 frames fit
    (and its 4 480 tiles at 256 frames, which the old 4 096-row chain buffer did not hold); 18 432 tasks, 4 480 x 4 rows and one row
    past the end do not; no rows or a negative count never do."""
    rows = [18432, 4480 * 4, 16385, 16384, 4480, 2240, 9216, 1, 0, -1, -(2 ** 40), 2 ** 40]
    out = subprocess.run([driver, "fit", *map(str, rows)], check=True, capture_output=True, text=True).stdout.split()
    assert dict(zip(out[::2], out[1::2])) == {str(r): str(int(0 < r <= 16384)) for r in rows}
    assert [int(v) for v in out[1::2]] == [0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0]


def test_chain_report(driver, tmp_path):
    """Six tiles on four persistent workgroups (rounds of 4 and 2), on three CUs of two XCDs; tile 1 skips phase 3 and the second round
    skips phases 9 and 10 (the report charges the next written slot from the last written one)."""
    nblk, blocks = 6, 4
    b = np.arange(nblk)
    dur = 1000 * np.arange(1, 12)[None, :] + 12 * b[:, None]
    cyc = _cumulative(1_000_000 + 5000 * b, dur)                  # slots 0 .. 11
    written = np.ones_like(cyc, dtype=bool)
    written[1, 3] = False
    written[4:, 9:11] = False
    start = np.array([0, 10, 20, 30, 0, 0]) + 5_000_000           # slot 12 / 13: 100 MHz ticks
    end = start + 2000 + 100 * b
    start[4:] = end[:2] + 10
    end[4:] = start[4:] + 2000
    xcc, cu, se, sh = np.array([0, 1, 0, 1, 0, 1]), np.array([1, 1, 1, 2, 1, 2]), np.array([0, 2, 0, 2, 0, 2]), np.array([0, 0, 0, 1, 0, 1])
    hw = 0x37 | (cu << 8) | (sh << 12) | (se << 13) | (1 << 20)   # HW_ID: wave / SIMD ids below, other fields above the ones used
    table = np.zeros((nblk, SLOTS), dtype=np.uint64)
    table[:, :12] = np.where(written, cyc, 0)
    table[:, 12], table[:, 13], table[:, 14] = start, end, (hw.astype(np.uint64) << np.uint64(32)) | (xcc | 8).astype(np.uint64)
    lines = _run(driver, tmp_path, "chain", table, blocks, 128, 1, 0, 3, 53248)

    sums = np.zeros(12)
    for row in range(nblk):
        last = cyc[row, 0]
        for i in range(1, 12):
            if written[row, i]:
                sums[i] += cyc[row, i] - last
                last = cyc[row, i]
    # (phase i is dur[:, i - 1]) tile 1's phase 3 is charged to phase 4; the second round's phases 9 and 10 to phase 11
    assert sums[3] == dur[:, 2].sum() - dur[1, 2] and sums[4] == dur[:, 3].sum() + dur[1, 2]
    assert sums[9] == dur[:4, 8].sum() and sums[11] == dur[:, 10].sum() + dur[4:, 8:10].sum()
    want = ["chain<128,mlp=1,qkv=0> 3 blocks/CU at 53248 B LDS; mean cycles per phase:" + "".join(f" [{i}]={sums[i] / nblk:.0f}" for i in range(1, 12))]
    t0, t1 = start.min(), end.max()
    cus = sorted(set(zip(xcc, cu, se, sh)))
    tiles_on = {c: [r for r in range(nblk) if (xcc[r], cu[r], se[r], sh[r]) == c] for c in cus}
    busy = sum(float((end - start)[rows].sum()) for rows in tiles_on.values())
    counts = [len(rows) for rows in tiles_on.values()]
    assert len(cus) == 3 and counts == [3, 1, 2]
    want.append(f"  span {(t1 - t0) / 100:.1f} us; 3 distinct CUs; tiles/CU min 1 max 3; mean concurrent workgroups per CU "
                f"{busy / 3 / (t1 - t0):.2f}; mean tile time {busy / nblk / 100:.1f} us")
    us_end = (end - t0) / 100.0
    last_round = {c: us_end[[r for r in rows if r >= nblk - blocks]] for c, rows in tiles_on.items() if any(r >= nblk - blocks for r in rows)}
    first, last = np.array([v.min() for v in last_round.values()]), np.array([v.max() for v in last_round.values()])
    want.append(f"  per CU, last-round tiles: first workgroup done {_mmm(first)} us, last workgroup done {_mmm(last)} us (min/mean/max over 2 CUs)")
    per_xcd = [np.mean([v.max() for c, v in last_round.items() if c[0] == x]) if any(c[0] == x for c in last_round) else 0.0 for x in range(8)]
    want.append("  mean finish per XCD:" + "".join(f" {v:.1f}" for v in per_xcd))
    for r, (lo, hi) in enumerate([(0, 4), (4, 6)]):
        want.append(f"  round {r} ({hi - lo} tiles): start {_mmm((start[lo:hi] - t0) / 100.0)} us (min/mean/max), end {_mmm(us_end[lo:hi])} us")
    assert lines == want


def test_attention_report(driver, tmp_path):
    """Twelve tasks on two workgroups (rounds of 8 and 4) at 21 cycles per 100 MHz tick: the in-kernel clock reads 2.100 GHz."""
    n, blocks, tokpad = 12, 2, 288
    t = np.arange(n)
    dur = np.stack([420 + 21 * t, 21000 + 0 * t, 0 * t, 210 + 0 * t], axis=1)   # prologue, loop, (slot 3 = slot 2), store
    cyc = _cumulative(10_000 + 777 * t, dur)
    ticks = (cyc[:, 4] - cyc[:, 0]) // 21
    assert ((cyc[:, 4] - cyc[:, 0]) == 21 * ticks).all()
    start = 7_000_000 + 2 * t
    start[8:] = start[:4] + ticks[:4] + 1
    end = start + ticks
    table = np.zeros((n, SLOTS), dtype=np.uint64)
    table[:, :5], table[:, 6], table[:, 5] = cyc, start, end
    lines = _run(driver, tmp_path, "attn", table, blocks, tokpad)
    t0, t1 = start.min(), end.max()
    want = ["in-kernel shader clock: 2.100 GHz",
            f"attn stamps: mean per task: prologue={dur[:, 0].mean():.0f} loop=21000 store=210 (cycles); MFMA ideal {32 * 9 * 64}",
            f"  span {(t1 - t0) / 100:.1f} us, 12 tasks in rounds of 8; mean concurrent waves per SIMD {ticks.sum() / (t1 - t0) / 1024:.2f}"]
    for r, (lo, hi) in enumerate([(0, 8), (8, 12)]):
        want.append(f"  round {r}: start {_mmm((start[lo:hi] - t0) / 100.0)} us (min/mean/max), end {_mmm((end[lo:hi] - t0) / 100.0)} us")
    assert lines == want


def test_banded_conv_report(driver, tmp_path):
    nb = 5
    b = np.arange(nb)
    dur = 100 * np.arange(1, 9)[None, :] + 5 * b[:, None]
    table = np.zeros((nb, SLOTS), dtype=np.uint64)
    table[:, :9] = _cumulative(123_456 + 999 * b, dur)
    m = dur.mean(axis=0)
    assert (m == 100 * np.arange(1, 9) + 10).all()
    names = ["weights", "zero", "input", "conv1", "mfma(wave0)", "wait", "fixup", "conv4"]
    assert _run(driver, tmp_path, "conv", table, 1) == [
        "conv mode 1 stamps (mean cycles, thread 0): " + " ".join(f"{k}={v:.0f}" for k, v in zip(names, m)) + f" total={m.sum():.0f}"]


def test_streaming_conv_report(driver, tmp_path):
    """Matrix-wave rows (slots 0 .. 6) and helper-wave rows (slots 8 .. 14, slot 15 = input plane in LDS) with different durations."""
    nb = 4
    b = np.arange(nb)
    mat = 200 * np.arange(1, 7)[None, :] + 4 * b[:, None]
    hlp = 300 * np.arange(1, 7)[None, :] + 8 * b[:, None]
    table = np.zeros((nb, SLOTS), dtype=np.uint64)
    table[:, :7] = _cumulative(50_000 + 11 * b, mat)
    table[:, 8:15] = _cumulative(50_040 + 13 * b, hlp)
    table[:, 15] = table[:, 8] + (1500 + 2 * b).astype(np.uint64)
    mm, hm = mat.mean(axis=0), hlp.mean(axis=0)
    assert (mm == 200 * np.arange(1, 7) + 6).all() and (hm == 300 * np.arange(1, 7) + 12).all()
    assert _run(driver, tmp_path, "stream", table, 0, 1, 2) == [
        "conv stream16: input plane in LDS 1503 cycles after the kernel's start (helper wave)",
        "conv stream mode 0 (mean cycles): matrix wave: " + " ".join(f"{k}={v:.0f}" for k, v in zip(["stage", "gather", "wait", "sweeps", "wait", "store"], mm))
        + " | helper wave: " + " ".join(f"{k}={v:.0f}" for k, v in zip(["stage", "zero+input+conv1", "wait", "conv4", "wait", "store"], hm)),
        "  stamped: launch 1 of 2, 4 workgroups, 1 column range(s) per plane"]


def test_training_chain_report(driver, tmp_path):
    """Seven tiles on four workgroups: the first tiles start 0 / 5 / 25 / 10 us after the earliest (one later than 20 us), the launch's
    last tile at 350 us."""
    ntiles, blocks = 7, 4
    b = np.arange(ntiles)
    dur = 1000 * np.arange(1, 9)[None, :] + 7 * b[:, None]
    table = np.zeros((ntiles, SLOTS), dtype=np.uint64)
    table[:, :9] = _cumulative(2_000_000 + 31 * b, dur)
    table[:, 9] = 9_000_000 + np.array([0, 500, 2500, 1000, 30_000, 31_000, 35_000])
    m = dur.mean(axis=0)
    assert (m == 1000 * np.arange(1, 9) + 21).all()
    names = ["outproj", "s1+LN1+x1+barrier", "ffn_up", "act+a+hd+barrier", "ffn_down", "s2+LN2+out", "qkv", "end_barrier"]
    assert _run(driver, tmp_path, "train", table, blocks, 1) == [
        "chain_fwd_train<QKV=1>: 4 workgroups, first tile starts 10.0 us (mean) / 25.0 us (max) after the earliest, 1 later than 20 us; "
        "the launch's last tile starts at 350.0 us",
        "  mean cycles per tile: " + " ".join(f"{k}={v:.0f}" for k, v in zip(names, m)) + f" total={m.sum():.0f}"]
