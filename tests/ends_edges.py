"""The training step's thin ends, dense layers and channel adapter at the sizes where their kernels' geometry changes (helper module:
no tests here).

Holds the matrix (ENDS_CASES, DENSE_CASES, ADAPTER_CASES, REFUSALS, the accumulate cases), a Python restatement of the planners of
csrc/k_ends_train.hip and csrc/k_gemm.hip with the CU count as a parameter (the matrix is written for 256), the float64 references as
plain tensor formulas (index by the patch map, ``@``, sums), the float32 yardsticks (the same formulas in float32), the bounds, the
judge, and the defects that tests/test_ends_dense_edges.py plants to show that the bounds see them.
tools/debug/ends_edges_vs_fp64.py prints every figure; profiles/ends_edges_vs_fp64.json holds them.

Tensors.  Embed: x0 = (in W1^T + b1) + pos, d_in = dx0 W1 -> d_conv | d_tok6, dW1 = dx0^T in, db1 = sum dx0, dpos = sum over planes.
Tail: out = resid + unpatch(x W2^T + b2), d6 = patch(d_out), dx = d6 W2, dW2 = d6^T x, db2 = sum d6.  Dense: y = x W^T + b, dx = dy W,
dW = dy^T x, db = sum dy.  Adapter: three MLPs 1 -> h0 -> h1 -> h2 with ReLU; its backward reference is "tape style": it takes the
float32 activations a0, a1 the forward KERNEL wrote as data, so no ReLU decision crosses a precision boundary.
"""
import ctypes as C
from types import SimpleNamespace

import torch

# ---------------------------------------------------------------- the planners, restated
ENDS_TILE, EMB_TOK, EMB_PASS, EMB_MAX_OUT, EMB_MAX_PIECES, TAIL_MAX_F = 32, 8, 4, 80, 4, 32     # csrc/k_ends_train.hip
GBM, GBN, GBK, GEMM_MAX_SLICES, COLSUM_MAX_SLICES = 128, 128, 16, 256, 1024                      # csrc/k_gemm.hip, aft_internal.h


def cdiv(a, b):
    return -(-a // b)


def al64(n):
    return cdiv(n, 64) * 64


def make_dims(planes, S, T, p0, p1, d, adapter):
    """make_dims of k_ends_train.hip: the geometry, or None where the ends refuse the shape."""
    if planes <= 0 or S <= 0 or T <= 0 or p0 <= 0 or p1 <= 0 or S % p0 or T % p1 or d < 4 or d % 4 or d > 1024:
        return None
    tw = T // p1
    g = SimpleNamespace(planes=planes, S=S, T=T, p0=p0, p1=p1, d=d, tw=tw, tokens=(S // p0) * tw, p=p0 * p1)
    g.din = g.p + (6 if adapter else 0)
    g.rows = planes * g.tokens
    ok = d <= 512 and g.p <= TAIL_MAX_F and d * g.din <= 256 * EMB_MAX_OUT and EMB_TOK * (d // 4) <= 256 * EMB_MAX_PIECES
    return g if ok else None


def ends_grid(g, cus):
    return min(cdiv(g.rows, ENDS_TILE), 4 * cus)


def embed_bwd_chunks(g, cus):
    """(tb token blocks, ch planned plane chunks, planes_per_chunk, chunks launched)."""
    tb = cdiv(g.tokens, EMB_TOK)
    ch = max(1, min(g.planes, (4 * cus + tb - 1) // tb))
    ppc = cdiv(g.planes, ch)
    return tb, ch, ppc, cdiv(g.planes, ppc)


def embed_bwd_class(g, generic=False):
    """The kernel launch_embed_train_bwd picks: "mfma128", or the <NOUT, NPIECE> instantiation of the vector kernel."""
    nout, npiece = cdiv(g.d * g.din, 256), cdiv(EMB_TOK * (g.d // 4), 256)
    if g.d == 128 and g.din <= 16 and not generic:
        return "mfma128"
    if nout <= 8 and npiece <= 1:
        return (8, 1)
    return (24, 4) if nout <= 24 else (EMB_MAX_OUT, EMB_MAX_PIECES)


def tail_nf(g):
    """(fg_n, nf, NF): feature groups of tail_rows_bwd_kernel, patch elements per thread, the instantiation."""
    fg_n = 256 // (g.d // 4)
    nf = cdiv(g.p, fg_n)
    return fg_n, nf, 1 if nf <= 1 else 4 if nf <= 4 else 16


def embed_bwd_slice_floats(g, cus):
    tb, ch, _, _ = embed_bwd_chunks(g, cus)
    return al64(tb * ch * g.d * g.din) + al64(tb * ch * g.d) + al64(ch * g.tokens * g.d)


def tail_bwd_slice_floats(g, cus):
    wgs = ends_grid(g, cus)
    return al64(wgs * g.p * g.d) + al64(wgs * g.p)


def ends_props(case, cus=256):
    """Everything the matrix names about one ends case."""
    S, T, p0, p1, d, adapter, planes, sw, _ = case
    g = make_dims(planes, S, T, p0, p1, d, adapter)
    q = SimpleNamespace(**vars(g))
    q.ntiles, q.grid = cdiv(g.rows, ENDS_TILE), ends_grid(g, cus)
    q.qn = d // 4
    q.row_groups = 256 // q.qn
    q.idle = 256 - q.row_groups * q.qn
    q.straddle = any((t * ENDS_TILE) // g.tokens != (min(g.rows, (t + 1) * ENDS_TILE) - 1) // g.tokens for t in range(q.ntiles))
    q.embed_class = embed_bwd_class(g, ("AFT_EMBED_BWD_GENERIC", "1") in sw)
    q.nout, q.npiece = cdiv(d * g.din, 256), cdiv(EMB_TOK * q.qn, 256)
    q.tb, q.ch, q.ppc, q.chunks = embed_bwd_chunks(g, cus)
    q.passes = [min(EMB_PASS, q.ppc - nb) for nb in range(0, q.ppc, EMB_PASS)]           # of a full chunk
    q.last_chunk = planes - (q.chunks - 1) * q.ppc
    q.last_block = g.tokens - (q.tb - 1) * EMB_TOK
    q.fg_n, q.nf, q.NF = tail_nf(make_dims(planes, S, T, p0, p1, d, False))
    return q


def gemm_fast_ok(op, M, N, K, lda, ldb, ldc):
    a_bytes, b_bytes = 4 * (K if op == 2 else M) * lda, 4 * (N if op == 0 else K) * ldb
    return (not (lda & 3 or ldb & 3 or ldc & 3 or N & 3 or K % GBK) and (op != 2 or not M & 3)
            and a_bytes < 0x7ffffff0 and b_bytes < 0x7ffffff0)


def gemm_vec_ok(op, M, N, K, lda, ldb):
    return not (lda & 3 or (M if op == 2 else K) & 3) and not (ldb & 3 or (K if op == 0 else N) & 3)


def gemm_path(op, M, N, K, lda, ldb, ldc):
    return "fast" if gemm_fast_ok(op, M, N, K, lda, ldb, ldc) else "vec" if gemm_vec_ok(op, M, N, K, lda, ldb) else "scalar"


def gemm_rows(op, M, N, K, lda, ldb, ldc, cus, forced=0):
    """launch_gemm's 64 / 96-row choice: 96 where it saves a round of tiles over the resident workgroups (aligned path, N <= 128)."""
    if not (gemm_fast_ok(op, M, N, K, lda, ldb, ldc) and (N <= GBN or forced == 96)):
        return 64
    ntn = cdiv(N, GBN)
    cost = lambda bm, per: cdiv(cdiv(M, bm) * ntn, cus * per) * bm * per  # noqa: E731
    return forced if forced in (64, 96) else 96 if cost(96, 3) < cost(64, 4) else 64


def gemm_split_slices(rows, tiles):
    return max(1, min(GEMM_MAX_SLICES, cdiv(512, tiles), rows // 128))


def colsum_slices(rows):
    return max(1, min(COLSUM_MAX_SLICES, rows // 64))


def dense_scratch_floats(rows, in_f, out_f):
    tiles = cdiv(in_f, 128) * cdiv(out_f, 128)
    return al64(gemm_split_slices(rows, tiles) * in_f * out_f) + al64(colsum_slices(rows) * out_f)   # aft_internal.h: Layout::take


def dense_props(case, cus=256):
    rows, in_f, out_f, _, _, sw = case
    forced = int(dict(sw).get("AFT_GEMM_BM", 0))
    q = SimpleNamespace(rows=rows, in_f=in_f, out_f=out_f)
    fwd, dgrad = (0, rows, out_f, in_f, in_f, in_f, out_f), (1, rows, in_f, out_f, out_f, in_f, in_f)
    q.fwd, q.dgrad, q.wgrad = gemm_path(*fwd), gemm_path(*dgrad), gemm_path(2, out_f, in_f, rows, out_f, in_f, in_f)
    q.fwd_bm, q.dgrad_bm = gemm_rows(*fwd, cus, forced), gemm_rows(*dgrad, cus, forced)
    q.fwd_tiles, q.dgrad_tiles = cdiv(rows, q.fwd_bm) * cdiv(out_f, GBN), cdiv(rows, q.dgrad_bm) * cdiv(in_f, GBN)
    per = {128: 2, 96: 3, 64: 4}
    q.fwd_grid, q.dgrad_grid = min(q.fwd_tiles, cus * per[q.fwd_bm]), min(q.dgrad_tiles, cus * per[q.dgrad_bm])
    q.nz = gemm_split_slices(rows, cdiv(in_f, GBN) * cdiv(out_f, GBM))
    q.chunk = cdiv(cdiv(rows, q.nz), GBK) * GBK
    q.used = cdiv(rows, q.chunk)
    q.cs_nz = colsum_slices(rows)
    q.cs_chunk = cdiv(rows, q.cs_nz)
    q.cs_used = cdiv(rows, q.cs_chunk)
    return q


# ---------------------------------------------------------------- the matrix
GEN = (("AFT_EMBED_BWD_GENERIC", "1"),)
# An ends case: (S, T, p0, p1, d, adapter features, planes, switches, dpos wanted).  Every case runs embed forward + backward and
# tail forward + backward (the tail has no adapter features).  ENDS_EDGE names the property each is in the matrix for.
ENDS_CASES = [
    (3, 1, 1, 1, 4, False, 2, (), True),            # 6 rows: one partial tile; d = 4: 256 row groups; din = 1; a 3-token block
    (4, 2, 1, 1, 8, False, 4, (), True),            # 32 rows: the tile boundary; a full 8-token block
    (3, 1, 1, 1, 8, True, 11, (), True),            # 33 rows; din = 7
    (28, 4, 2, 2, 128, True, 3, (), True),          # 28 tokens: tiles straddle plane boundaries; the MFMA embed backward
    (28, 4, 2, 2, 128, True, 3, (), False),         # dpos = NULL
    (30, 3, 3, 1, 200, False, 3, (), True),         # 30 tokens; d = 200: 6 idle threads
    (9, 2, 1, 2, 260, True, 5, (), True),           # 9 tokens: a block of one token; d = 260: 61 idle threads
    (16, 16, 4, 8, 512, True, 3, (), True),         # d = 512: 2 row groups; din = 38: <80,4> at 76 accumulators; nf = 16
    (20, 6, 1, 1, 8, False, 276, (), True),         # 33 120 rows, 1 035 tiles: the persistent loop's second trip
    (20, 6, 1, 1, 8, True, 276, (), True),          # ... with adapter features
    (10, 6, 5, 2, 128, True, 5, (), True),          # d = 128, din = 16: nout = 8, the MFMA kernel
    (10, 6, 5, 2, 128, True, 5, GEN, True),         # ... and <8,1>
    (22, 3, 11, 1, 128, True, 5, (), True),         # din = 17: nout = 9, <24,4>; tail p = 11
    (8, 12, 4, 6, 256, False, 9, (), True),         # d = 256, din = 24: nout = 24, <24,4>
    (10, 10, 5, 5, 256, False, 9, (), True),        # din = 25: <80,4>
    (64, 32, 1, 1, 8, False, 18, (), True),         # tb = 256, ch = 4, ppc = 5: passes 4 + 1
    (20, 14, 1, 1, 8, False, 256, GEN, True),       # 280 tokens: ch = 30, ppc = 9, 29 chunks, passes 4 + 4 + 1, last chunk 4 planes
    (20, 14, 1, 1, 128, False, 256, (), True),      # ... on the MFMA kernel
    (8, 4, 4, 2, 128, False, 9, (), True),          # tail d = 128, p = 8: nf = 1
    (6, 6, 3, 3, 128, False, 9, (), True),          # p = 9: nf = 2
    (16, 8, 8, 4, 128, False, 9, (), True),         # p = 32: nf = 4
    (8, 10, 4, 5, 256, False, 9, (), True),         # d = 256, p = 20: nf = 5
    (8, 12, 4, 6, 200, False, 9, (), True),         # d = 200, p = 24: fg_n = 5
]
PERSISTENT, STRADDLE, ONE_TOKEN_BLOCK, FIVE_PLANES, NF_1_2 = ENDS_CASES[8], ENDS_CASES[3], ENDS_CASES[6], ENDS_CASES[15], ENDS_CASES[19]
ENDS_EDGE = {
    0: lambda q: (q.rows, q.ntiles, q.row_groups, q.din, q.tokens, q.embed_class) == (6, 1, 256, 1, 3, (8, 1)),
    1: lambda q: (q.rows, q.ntiles, q.tokens, q.last_block) == (32, 1, 8, 8),
    2: lambda q: (q.rows, q.ntiles, q.din) == (33, 2, 7),
    3: lambda q: q.tokens == 28 and q.straddle and q.embed_class == "mfma128" and q.idle == 0,
    4: lambda q: q.tokens == 28 and q.embed_class == "mfma128",
    5: lambda q: q.tokens == 30 and q.straddle and (q.row_groups, q.idle, q.embed_class) == (5, 6, (24, 4)),
    6: lambda q: (q.tokens, q.tb, q.last_block, q.row_groups, q.idle) == (9, 2, 1, 3, 61),
    7: lambda q: (q.row_groups, q.din, q.p, q.embed_class, q.nf, q.NF) == (2, 38, 32, (80, 4), 16, 16) and q.d * q.din == 256 * 76,
    8: lambda q: (q.rows, q.ntiles) == (33120, 1035) and q.ntiles > q.grid and q.din == 1,
    9: lambda q: (q.rows, q.ntiles) == (33120, 1035) and q.ntiles > q.grid and q.din == 7,
    10: lambda q: (q.d, q.din, q.nout, q.embed_class) == (128, 16, 8, "mfma128"),
    11: lambda q: (q.d, q.din, q.nout, q.embed_class) == (128, 16, 8, (8, 1)),
    12: lambda q: (q.din, q.nout, q.embed_class, q.nf) == (17, 9, (24, 4), 2),
    13: lambda q: (q.d, q.din, q.nout, q.embed_class) == (256, 24, 24, (24, 4)),
    14: lambda q: (q.d, q.din, q.nout, q.embed_class) == (256, 25, 25, (80, 4)),
    15: lambda q: q.ppc > 4 and q.passes[-1] < 4 and q.tb == 256,
    16: lambda q: q.chunks < q.ch and len(q.passes) == 3 and q.passes[-1] < 4 and q.embed_class == (8, 1) and q.tokens == 280,
    17: lambda q: q.chunks < q.ch and len(q.passes) == 3 and q.passes[-1] < 4 and q.embed_class == "mfma128",
    18: lambda q: (q.fg_n, q.nf, q.NF) == (8, 1, 1),
    19: lambda q: (q.fg_n, q.nf, q.NF) == (8, 2, 4),
    20: lambda q: (q.fg_n, q.nf, q.NF) == (8, 4, 4),
    21: lambda q: (q.fg_n, q.nf, q.NF) == (4, 5, 16),
    22: lambda q: (q.fg_n, q.nf, q.NF, q.idle) == (5, 5, 16, 6),
}
# (planes, S, T, p0, p1, d): a patch of 33 elements, d = 516, d = 6, S % p0 != 0
REFUSALS = [(2, 33, 2, 33, 1, 8), (2, 4, 2, 1, 1, 516), (2, 4, 2, 1, 1, 6), (2, 7, 2, 2, 1, 8)]

G64 = (("AFT_GEMM_BM", "64"),)
G96 = (("AFT_GEMM_BM", "96"),)
# A dense case: (rows, in, out, bias, dx wanted, switches).  Paths (forward | dgrad | wgrad) in DENSE_EDGE.
DENSE_CASES = [
    (64, 16, 16, True, True, ()),                   # fast | fast | fast; K = 16 in all three
    (63, 16, 128, True, True, ()),                  # fast | fast | vec; 63 rows: colsum's one slice
    (64, 16, 128, True, True, ()),
    (65, 16, 128, True, True, ()),
    (64, 16, 127, True, True, ()),                  # fast needs out % 4: vec | scalar | scalar
    (64, 16, 129, True, True, ()),
    (64, 16, 132, True, True, ()),                  # fast | vec | fast; a second column tile of 4 columns
    (65, 12, 132, True, True, ()),                  # vec | vec | vec
    (64, 1, 128, True, True, ()),                   # K = 1 forward (scalar)
    (64, 17, 128, True, True, ()),                  # K = 17 forward (scalar): a last partial 16-step
    (65, 17, 129, True, True, ()),                  # scalar everywhere, ragged everywhere
    (64, 8, 1, True, True, ()),                     # K = 1 dgrad
    (64, 8, 17, True, True, ()),                    # K = 17 dgrad
    (1, 16, 4, True, True, ()),                     # K = 1 wgrad
    (16, 16, 4, True, True, ()),                    # K = 16 wgrad (fast)
    (17, 16, 4, True, True, ()),                    # K = 17 wgrad (vec)
    (65600, 16, 4, True, True, ()),                 # 64 * 4 * 256 + 64 rows: the forward picks 96-row tiles, the dgrad walks 1 025 64-row tiles
    (65600, 16, 4, True, True, G64),                # ... the aligned forward walks 1 025 64-row tiles
    (73824, 16, 4, True, True, G96),                # 96 * 3 * 256 + 96 rows: a second trip over 96-row tiles
    (127, 16, 8, True, True, ()),                   # nz = 1
    (255, 16, 8, True, True, ()),                   # nz = 1
    (256, 16, 8, True, True, ()),                   # nz = 2
    (32776, 16, 8, True, True, ()),                 # chunk 144, 228 of 256 slices used (vec: 32 776 % 16 = 8)
    (32777, 16, 8, True, True, ()),                 # the same, one odd row
    (32784, 16, 8, True, True, ()),                 # the same on the fast path
    (32777, 15, 8, True, True, ()),                 # the same on the scalar path
    (66561, 4, 8, True, True, ()),                  # 65 * 1024 + 1 rows: colsum chunk 66, 1 009 of 1 024 slices used
    (128, 4, 63, True, True, ()),                   # colsum column blocks of 64
    (128, 4, 64, True, True, ()),
    (128, 4, 65, True, True, ()),
    (65, 12, 132, True, False, ()),                 # dx = NULL
    (65, 12, 132, False, True, ()),                 # bias = NULL, dbias = NULL
]
EMPTY_SLICES = [c for c in DENSE_CASES if c[0] in (32776, 32777, 32784)]
DENSE_EDGE = {
    0: lambda q: (q.fwd, q.dgrad, q.wgrad) == ("fast", "fast", "fast"),
    1: lambda q: (q.fwd, q.dgrad, q.wgrad, q.cs_nz) == ("fast", "fast", "vec", 1),
    2: lambda q: (q.fwd, q.dgrad, q.wgrad, q.cs_nz, q.fwd_tiles) == ("fast", "fast", "fast", 1, 1),
    3: lambda q: (q.fwd, q.dgrad, q.wgrad, q.fwd_tiles) == ("fast", "fast", "vec", 2),
    4: lambda q: (q.fwd, q.dgrad, q.wgrad) == ("vec", "scalar", "scalar"),
    5: lambda q: (q.fwd, q.dgrad, q.wgrad, q.fwd_tiles) == ("vec", "scalar", "scalar", 2),
    6: lambda q: (q.fwd, q.dgrad, q.wgrad, q.fwd_tiles) == ("fast", "vec", "fast", 2),
    7: lambda q: (q.fwd, q.dgrad, q.wgrad) == ("vec", "vec", "vec"),
    8: lambda q: (q.fwd, q.in_f) == ("scalar", 1),
    9: lambda q: (q.fwd, q.in_f, q.dgrad) == ("scalar", 17, "scalar"),
    10: lambda q: (q.fwd, q.dgrad, q.wgrad) == ("scalar", "scalar", "scalar"),
    11: lambda q: (q.dgrad, q.out_f) == ("scalar", 1),
    12: lambda q: (q.dgrad, q.out_f) == ("scalar", 17),
    13: lambda q: (q.wgrad, q.rows, q.nz) == ("vec", 1, 1),
    14: lambda q: (q.wgrad, q.rows) == ("fast", 16),
    15: lambda q: (q.wgrad, q.rows) == ("vec", 17),
    16: lambda q: q.fwd == "fast" and q.fwd_bm == 96 and q.dgrad == "vec" and q.dgrad_tiles > q.dgrad_grid,
    17: lambda q: q.fwd == "fast" and q.fwd_bm == 64 and q.fwd_tiles > q.fwd_grid,
    18: lambda q: q.fwd == "fast" and q.fwd_bm == 96 and q.fwd_tiles > q.fwd_grid,
    19: lambda q: q.nz == 1,
    20: lambda q: q.nz == 1,
    21: lambda q: q.nz == 2,
    22: lambda q: (q.wgrad, q.nz, q.chunk, q.used) == ("vec", 256, 144, 228),
    23: lambda q: (q.wgrad, q.nz, q.chunk, q.used) == ("vec", 256, 144, 228),
    24: lambda q: (q.wgrad, q.nz, q.chunk, q.used) == ("fast", 256, 144, 228),
    25: lambda q: (q.wgrad, q.nz, q.chunk, q.used) == ("scalar", 256, 144, 228),
    26: lambda q: (q.cs_nz, q.cs_chunk, q.cs_used) == (1024, 66, 1009),
    27: lambda q: q.cs_nz == 2 and q.out_f == 63,
    28: lambda q: q.cs_nz == 2 and q.out_f == 64,
    29: lambda q: q.cs_nz == 2 and q.out_f == 65,
    30: lambda q: True,
    31: lambda q: True,
}
COLSUM_TAIL, K17, STALE_SLICE = DENSE_CASES[26], DENSE_CASES[9], DENSE_CASES[22]

# (hidden sizes, frames); the fused backward refuses hidden[1] = 65
ADAPTER_CASES = [((1, 1, 2), 1), ((1, 1, 2), 13), ((256, 64, 560), 1), ((256, 64, 560), 13), ((7, 42, 560), 1), ((7, 42, 560), 13),
                 ((5, 9, 82), 1), ((5, 9, 82), 13)]
ADAPTER_REFUSED = (7, 65, 560)
ACCUMULATE = dict(ends=ENDS_CASES[5], dense=DENSE_CASES[7], adapter=ADAPTER_CASES[7])


def ends_id(c):
    S, T, p0, p1, d, ad, n, sw, dpos = c
    return f"{S}x{T}_p{p0}x{p1}_d{d}_n{n}" + ("_ad" if ad else "") + ("_generic" if sw else "") + ("" if dpos else "_nodpos")


def dense_id(c):
    rows, in_f, out_f, bias, dx, sw = c
    return f"{rows}x{in_f}x{out_f}" + ("" if bias else "_nobias") + ("" if dx else "_nodx") + "".join(f"_bm{v}" for _, v in sw)


def adapter_id(c):
    return "h" + "-".join(map(str, c[0])) + f"_f{c[1]}"


# ---------------------------------------------------------------- bounds
ENDS_TOL = dict(x0=2e-6, out=2e-6, d_conv=2e-5, d_tok6=2e-5, dx=2e-5, dW1=2e-5, db1=2e-5, dpos=2e-5, dW2=2e-5, db2=2e-5)
DENSE_TOL = dict(y=1e-5, dx=1e-5, dW=1e-4, db=1e-4)          # tests/test_train_hip.py's bounds for these tensors
ADAPTER_ELEMENT_TOL, ADAPTER_SUM_TOL = 1e-5, 1e-4
EDGE_FACTOR = 4.0                                            # as conv_edges.py
SUM_FLOOR = 2.0 ** -22
FACTOR = {}                                                  # (family, tensor) -> a raised factor, with its figure in the JSON (none)
EMBED_SUMS, TAIL_SUMS, DENSE_SUMS = ("dW1", "db1", "dpos"), ("dW2", "db2"), ("dW", "db")


def rel_err(a, ref):
    """max |a - ref| / max |ref| (float64 CPU tensors)."""
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def sum_err(a, ref, mag):
    """max_i |a_i - ref_i| / A_i: a sum's error against the sum of its terms' magnitudes."""
    return float(((a.double().cpu() - ref).abs() / mag.clamp_min(1e-300)).max())


def judge(family, names, got, ref, y32, mag, tol):
    """One row per tensor: dict(name, hip, e32, bound, project, ok, ratio [, hip_max, e32_max]); ratio = the error over the tighter
    bound.  Elementwise tensors: ``hip`` and ``bound`` relative to the float64 tensor's max, held to BOTH the project bound and
    EDGE_FACTOR e32 + 1e-6.  Summed gradients (the names in ``mag``): per element relative to A_i, err_i / A_i <= EDGE_FACTOR e32' +
    2^-22, and hip_max (relative to the max) within the project bound.  The HIP result enters ``hip`` / ``hip_max`` only."""
    rows = []
    for n in names:
        factor, project = FACTOR.get((family, n), EDGE_FACTOR), tol[n] if isinstance(tol, dict) else tol
        assert bool(torch.isfinite(got[n]).all()), f"{family} {n}: unwritten or non-finite elements"
        if n in mag:
            e32, e32_max = sum_err(y32[n], ref[n], mag[n]), rel_err(y32[n], ref[n])
            bound = factor * e32 + SUM_FLOOR
            hip, hip_max = sum_err(got[n], ref[n], mag[n]), rel_err(got[n], ref[n])
            rows.append(dict(name=n, hip=hip, e32=e32, bound=bound, hip_max=hip_max, e32_max=e32_max, project=project,
                             ok=hip <= bound and hip_max <= project, ratio=max(hip / bound, hip_max / project)))
        else:
            e32 = rel_err(y32[n], ref[n])
            bound, hip = factor * e32 + 1e-6, rel_err(got[n], ref[n])
            rows.append(dict(name=n, hip=hip, e32=e32, bound=bound, project=project, ok=hip <= bound and hip <= project,
                             ratio=hip / min(bound, project)))
    return rows


def show(label, rows):
    for r in rows:
        extra = f" | of max: hip {r['hip_max']:.2e} torch32 {r['e32_max']:.2e}" if "hip_max" in r else ""
        print(f"{label} {r['name']}: hip {r['hip']:.2e} torch32 {r['e32']:.2e} bound {r['bound']:.2e} project {r['project']:.2e}{extra}")
    return [f"{r['name']}: hip {r['hip']:.2e} > bound {r['bound']:.2e} or project {r['project']:.2e}" for r in rows if not r["ok"]]


# ---------------------------------------------------------------- inputs (float32 CPU tensors, the same bits on every device)
def _seeded(seed, shapes):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return [torch.randn(*s) for s in shapes]


def make_ends(case):
    S, T, p0, p1, d, adapter, planes = case[:7]
    g = make_dims(planes, S, T, p0, p1, d, adapter)
    n, t, p, din = planes, g.tokens, g.p, g.din
    names = ("conv", "tok6", "w1", "b1", "pos", "dx0", "x", "w2", "b2", "resid", "d_out")
    shapes = ((n, S, T), (n, t, 6), (d, din), (d,), (t, d), (n, t, d), (n, t, d), (p, d), (p,), (n, S, T), (n, S, T))
    inp = dict(zip(names, _seeded(4100 + 131 * S + 17 * T + 7 * d + planes + din, shapes)))
    inp["w1"] /= din ** 0.5
    inp["w2"] /= d ** 0.5
    if not adapter:
        inp["tok6"] = None
    return inp


def make_dense(case):
    rows, in_f, out_f = case[:3]
    x, w, b, dy = _seeded(5200 + rows + 37 * in_f + 101 * out_f, ((rows, in_f), (out_f, in_f), (out_f,), (rows, out_f)))
    return dict(x=x, w=w / in_f ** 0.5, b=b if case[3] else None, dy=dy)


ADAPTER_GRADS = tuple(f"d{k}{j}_{e}" for e in range(3) for j in (1, 2, 3) for k in ("W", "b"))


def make_adapter(case):
    """The 18 parameters of blocks.ChannelAdapter(hidden) under a fixed seed ({snr, ds, dop} x {0, 2, 4} x {weight, bias}), raw
    conditions of the data set's ranges (snr 0 .. 30, delay spread 50 .. 350, doppler 200 .. 1400) and d(tokens) [frames, tokens, 6]."""
    import adafortitran_amd.blocks as blocks
    hidden, frames = case
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(6300 + hidden[0] + 3 * hidden[1] + frames)
        params = [p.detach().clone() for p in blocks.ChannelAdapter(hidden).parameters()]
        conds = [torch.randint(0, 7, (frames,)).float() * 5, torch.randint(1, 8, (frames,)).float() * 50,
                 torch.randint(1, 8, (frames,)).float() * 200]
        dtok = torch.randn(frames, hidden[2] // 2, 6)
    return dict(params=params, conds=conds, dtok=dtok)


# ---------------------------------------------------------------- references
def patch_index(S, T, p0, p1):
    """[tokens, p] pixel offsets inside a plane: token t = (s / p0) * (T / p1) + t' / p1, element f = (s % p0) * p1 + t' % p1."""
    tw = T // p1
    t, f = torch.arange((S // p0) * tw)[:, None], torch.arange(p0 * p1)[None, :]
    return ((t // tw) * p0 + f // p1) * T + (t % tw) * p1 + f % p1


def patch(img, idx, stray=False):
    """[n, S, T] -> [n, tokens, p] by the patch map.  ``stray`` (a defect): the rows of a 32-row tile that lie past a plane boundary
    read the previous plane's pixels."""
    n, tokens = img.shape[0], idx.shape[0]
    flat = img.reshape(n, -1)
    if not stray:
        return flat[:, idx]
    row = torch.arange(n * tokens, device=img.device).view(n, tokens)
    first = (row // ENDS_TILE * ENDS_TILE) // tokens                                   # the plane of the tile's first row
    src = torch.where(first < row // tokens, row // tokens - 1, row // tokens)
    return flat[src[:, :, None], idx[None]]


def unpatch(vals, idx, S, T):
    n = vals.shape[0]
    out = torch.zeros(n, S * T, dtype=vals.dtype, device=vals.device)
    out[:, idx.reshape(-1)] = vals.reshape(n, -1)
    return out.view(n, S, T)


def _r(t):
    return t.reshape(-1, t.shape[-1])


def _out(d):
    return {k: v.double().cpu() for k, v in d.items() if v is not None}


def embed(case, inp, dtype=torch.float64, device="cpu", defect=None, cus=256, magnitudes=False):
    """{"x0", "d_conv", "d_tok6", "dW1", "db1", "dpos"} as float64 CPU tensors.  ``magnitudes``: A = sum |terms| of the three summed
    gradients (the same routine on |dx0| and |in|).  Defects: stray_plane, last_block (the one-token last block is missing from dpos /
    d_conv), fifth_plane (the fifth plane of every chunk is missing from dW1 / db1 / dpos)."""
    S, T, p0, p1, d, adapter, planes = case[:7]
    to = lambda t: None if t is None else t.to(device=device, dtype=dtype)  # noqa: E731
    conv, tok6, w1, b1, pos, dx0 = [to(inp[k]) for k in ("conv", "tok6", "w1", "b1", "pos", "dx0")]
    idx = patch_index(S, T, p0, p1).to(device)
    tokens, p = idx.shape
    tin = patch(conv, idx, defect == "stray_plane")
    if tok6 is not None:
        tin = torch.cat((tin, tok6), dim=2)
    x0 = ((_r(tin) @ w1.T).view(planes, tokens, d) + b1) + pos
    d_in = (_r(dx0) @ w1).view(planes, tokens, -1)
    d_conv = unpatch(d_in[:, :, :p], idx, S, T)
    g, a = (dx0.abs(), tin.abs()) if magnitudes else (dx0, tin)
    if defect == "fifth_plane":
        ppc = embed_bwd_chunks(make_dims(planes, S, T, p0, p1, d, adapter), cus)[2]
        keep = [n for n in range(planes) if n % ppc != 4]
        g, a = g[keep], a[keep]
    out = dict(x0=x0, d_conv=d_conv, d_tok6=d_in[:, :, p:] if adapter else None, dW1=_r(g).T @ _r(a), db1=_r(g).sum(0), dpos=g.sum(0))
    if defect == "last_block":
        assert tokens % EMB_TOK == 1
        out["dpos"] = out["dpos"].clone()
        out["dpos"][tokens - 1] = 0
        out["d_conv"] = unpatch(torch.cat((d_in[:, :-1, :p], torch.zeros_like(d_in[:, -1:, :p])), dim=1), idx, S, T)
    return _out(out)


def tail(case, inp, dtype=torch.float64, device="cpu", defect=None, cus=256, magnitudes=False):
    """{"out", "dx", "dW2", "db2"}.  Defects: stray_plane, second_tile (the rows of every workgroup's second tile are missing from
    dW2 / db2), fgn (patch elements f >= fg_n are missing from dW2)."""
    S, T, p0, p1, d, _, planes = case[:7]
    to = lambda t: t.to(device=device, dtype=dtype)  # noqa: E731
    x, w2, b2, resid, d_out = [to(inp[k]) for k in ("x", "w2", "b2", "resid", "d_out")]
    idx = patch_index(S, T, p0, p1).to(device)
    tokens, p = idx.shape
    out = resid + unpatch((_r(x) @ w2.T + b2).view(planes, tokens, p), idx, S, T)
    d6 = _r(patch(d_out, idx, defect == "stray_plane"))
    dx = (d6 @ w2).view(planes, tokens, d)
    g, a = (d6.abs(), _r(x).abs()) if magnitudes else (d6, _r(x))
    geo = make_dims(planes, S, T, p0, p1, d, False)
    if defect == "second_tile":
        kept = ENDS_TILE * ends_grid(geo, cus)
        assert kept < geo.rows
        g, a = g[:kept], a[:kept]
    dW2 = g.T @ a
    if defect == "fgn":
        dW2 = dW2.clone()
        dW2[tail_nf(geo)[0]:] = 0
    return _out(dict(out=out, dx=dx, dW2=dW2, db2=g.sum(0)))


def dense(case, inp, dtype=torch.float64, device="cpu", defect=None, magnitudes=False):
    """{"y", "dx", "dW", "db"}.  Defects: stale_slice (one trailing slice of the weight gradient's split holds an earlier call's
    partial product: here the first slice's, added once more), k17 (the forward's last partial 16-step is dropped), colsum_tail (the
    rows a column-sum chunk leaves to the kernel's tail loop are dropped)."""
    rows, in_f, out_f = case[:3]
    to = lambda t: None if t is None else t.to(device=device, dtype=dtype)  # noqa: E731
    x, w, b, dy = [to(inp[k]) for k in ("x", "w", "b", "dy")]
    kk = in_f // GBK * GBK if defect == "k17" else in_f
    y = x[:, :kk] @ w[:, :kk].T
    if b is not None:
        y = y + b
    g, a = (dy.abs(), x.abs()) if magnitudes else (dy, x)
    dW, db = g.T @ a, g.sum(0)
    q = dense_props(case)
    if defect == "stale_slice":
        assert q.used < q.nz
        dW = dW + g[:q.chunk].T @ a[:q.chunk]
    if defect == "colsum_tail":
        local = torch.arange(rows, device=device) % q.cs_chunk
        assert q.cs_chunk % 16 and q.cs_chunk > 64
        db = g[local < q.cs_chunk // 16 * 16].sum(0)
    return _out(dict(y=y, dx=dy @ w, dW=dW, db=db))


def adapter_forward(inp, dtype=torch.float64, device="cpu"):
    """{"tok6" [frames, tokens, 6], "a0" [frames, 3, h0], "a1" [frames, 3, h1]}."""
    to = lambda t: t.to(device=device, dtype=dtype)  # noqa: E731
    P, outs, a0s, a1s = [to(p) for p in inp["params"]], [], [], []
    for e in range(3):
        W1, b1, W2, b2, W3, b3 = P[6 * e:6 * e + 6]
        x = to(inp["conds"][e])
        a0 = torch.relu(x[:, None] * W1[:, 0] + b1)
        a1 = torch.relu(a0 @ W2.T + b2)
        outs.append((a1 @ W3.T + b3).view(x.shape[0], -1, 2))
        a0s.append(a0)
        a1s.append(a1)
    return _out(dict(tok6=torch.cat(outs, dim=2), a0=torch.stack(a0s, dim=1), a1=torch.stack(a1s, dim=1)))


def adapter_backward(inp, a0, a1, dtype=torch.float64, device="cpu", magnitudes=False):
    """{"da0", "da1", "dW1_e", "db1_e", ... "db3_e" (e = 0, 1, 2)} from the float32 activations a0, a1 the forward kernel wrote.
    ``magnitudes``: the whole chain on absolute values (|dtok|, |W|, |a|, |x|; the masks stay a > 0): A of the 18 gradients."""
    ab = (lambda t: t.abs()) if magnitudes else (lambda t: t)
    to = lambda t: ab(t.to(device=device, dtype=dtype))  # noqa: E731
    P, dtok, out, da0s, da1s = [to(p) for p in inp["params"]], to(inp["dtok"]), {}, [], []
    a0, a1 = to(a0), to(a1)
    for e in range(3):
        _, _, W2, _, W3, _ = P[6 * e:6 * e + 6]
        x, frames = to(inp["conds"][e]), dtok.shape[0]
        dout = dtok[:, :, 2 * e:2 * e + 2].reshape(frames, -1)
        da1 = (dout @ W3) * (a1[:, e] > 0).to(dtype)
        da0 = (da1 @ W2) * (a0[:, e] > 0).to(dtype)
        out[f"dW3_{e}"], out[f"db3_{e}"] = dout.T @ a1[:, e], dout.sum(0)
        out[f"dW2_{e}"], out[f"db2_{e}"] = da1.T @ a0[:, e], da1.sum(0)
        out[f"dW1_{e}"], out[f"db1_{e}"] = da0.T @ x[:, None], da0.sum(0)
        da0s.append(da0)
        da1s.append(da1)
    out["da0"], out["da1"] = torch.stack(da0s, dim=1), torch.stack(da1s, dim=1)
    return _out(out)


# ---------------------------------------------------------------- the library calls (GPU)
def _lib():
    from adafortitran_amd import _lib as L
    return L, L.load()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _scratch(nbytes, fill):
    assert nbytes > 0 and nbytes % 4 == 0
    return torch.full((nbytes // 4,), fill, dtype=torch.float32, device="cuda"), nbytes


def _cuda(inp):
    return {k: None if v is None else v.cuda() for k, v in inp.items()}


def hip_embed(case, dev, prefill=None, fill=float("nan"), check=True):
    """aft_embed_fwd_train_f32 + aft_embed_bwd_f32 on CUDA tensors; outputs and scratch start as NaN (scratch: ``fill``).
    ``prefill``: {"dW1", "db1", "dpos"} the call adds onto (accumulate = 1).  ``check`` False: returns (rc forward, rc backward, outputs)."""
    L, lib = _lib()
    S, T, p0, p1, d, adapter, planes, _, want_pos = case
    tokens, dims, st = (S // p0) * (T // p1) if p0 and p1 else 0, (planes, S, T, p0, p1, d), L.current_stream_ptr("cuda")
    o = dict(x0=_nan(planes, tokens, d), d_conv=_nan(planes, S, T), d_tok6=_nan(planes, tokens, 6) if adapter else None,
             dW1=_nan(*dev["w1"].shape), db1=_nan(d), dpos=_nan(tokens, d) if want_pos else None)
    if prefill is not None:
        o.update({k: v.clone() for k, v in prefill.items()})
    rc_f = lib.aft_embed_fwd_train_f32(dev["conv"].data_ptr(), _ptr(dev["tok6"]), dev["w1"].data_ptr(), dev["b1"].data_ptr(),
                                       dev["pos"].data_ptr(), o["x0"].data_ptr(), *dims, st)
    nbytes = lib.aft_embed_bwd_scratch_bytes(*dims, int(adapter))
    buf, nbytes = _scratch(nbytes, fill) if check else (_nan(64), 256)
    rc_b = lib.aft_embed_bwd_f32(dev["conv"].data_ptr(), _ptr(dev["tok6"]), dev["w1"].data_ptr(), dev["dx0"].data_ptr(),
                                 o["d_conv"].data_ptr(), _ptr(o["d_tok6"]), o["dW1"].data_ptr(), o["db1"].data_ptr(), _ptr(o["dpos"]),
                                 int(prefill is not None), buf.data_ptr(), nbytes, *dims, st)
    torch.cuda.synchronize()
    if not check:
        return rc_f, rc_b, o
    L.check(rc_f)
    L.check(rc_b)
    return {k: v for k, v in o.items() if v is not None}


def hip_tail(case, dev, prefill=None, fill=float("nan"), check=True):
    """aft_tail_fwd_train_f32 + aft_tail_bwd_f32; as hip_embed."""
    L, lib = _lib()
    S, T, p0, p1, d, _, planes = case[:7]
    tokens, dims, st = (S // p0) * (T // p1) if p0 and p1 else 0, (planes, S, T, p0, p1, d), L.current_stream_ptr("cuda")
    o = dict(out=_nan(planes, S, T), dx=_nan(planes, tokens, d), dW2=_nan(*dev["w2"].shape), db2=_nan(dev["w2"].shape[0]))
    if prefill is not None:
        o.update({k: v.clone() for k, v in prefill.items()})
    rc_f = lib.aft_tail_fwd_train_f32(dev["x"].data_ptr(), dev["w2"].data_ptr(), dev["b2"].data_ptr(), dev["resid"].data_ptr(),
                                      o["out"].data_ptr(), *dims, st)
    nbytes = lib.aft_tail_bwd_scratch_bytes(*dims)
    buf, nbytes = _scratch(nbytes, fill) if check else (_nan(64), 256)
    rc_b = lib.aft_tail_bwd_f32(dev["x"].data_ptr(), dev["w2"].data_ptr(), dev["d_out"].data_ptr(), o["dx"].data_ptr(), o["dW2"].data_ptr(),
                                o["db2"].data_ptr(), int(prefill is not None), buf.data_ptr(), nbytes, *dims, st)
    torch.cuda.synchronize()
    if not check:
        return rc_f, rc_b, o
    L.check(rc_f)
    L.check(rc_b)
    return o


def hip_dense(case, dev, prefill=None, fill=float("nan")):
    """aft_dense_fwd_f32 + aft_dense_bwd_f32: {"y", "dW" [, "dx", "db"]}."""
    L, lib = _lib()
    rows, in_f, out_f, bias, want_dx, _ = case
    st = L.current_stream_ptr("cuda")
    o = dict(y=_nan(rows, out_f), dx=_nan(rows, in_f) if want_dx else None, dW=_nan(out_f, in_f), db=_nan(out_f) if bias else None)
    if prefill is not None:
        o.update({k: v.clone() for k, v in prefill.items()})
    L.check(lib.aft_dense_fwd_f32(dev["x"].data_ptr(), dev["w"].data_ptr(), _ptr(dev["b"]), o["y"].data_ptr(), rows, in_f, out_f, st))
    buf, nbytes = _scratch(lib.aft_dense_bwd_scratch_bytes(rows, in_f, out_f), fill)
    L.check(lib.aft_dense_bwd_f32(dev["x"].data_ptr(), dev["w"].data_ptr(), dev["dy"].data_ptr(), _ptr(o["dx"]), o["dW"].data_ptr(),
                                  _ptr(o["db"]), int(prefill is not None), buf.data_ptr(), nbytes, rows, in_f, out_f, st))
    torch.cuda.synchronize()
    return {k: v for k, v in o.items() if v is not None}


def _ptrs(tensors, n):
    arr = (C.c_void_p * n)()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def hip_adapter(case, dev, prefill=None, check=True):
    """aft_adapter_fwd_train_f32 + aft_adapter_bwd_f32 (on the a0, a1 the forward just wrote): {"tok6", "a0", "a1", "da0", "da1",
    the 18 gradients}.  ``prefill``: the 18 gradients in ADAPTER_GRADS' order, added onto."""
    L, lib = _lib()
    (h0, h1, h2), frames = case
    tokens, st = h2 // 2, L.current_stream_ptr("cuda")
    params, conds = dev["params"], dev["conds"]
    ws, bs, hid = params[0::2], params[1::2], (C.c_int32 * 3)(h0, h1, h2)
    o = dict(tok6=_nan(frames, tokens, 6), a0=_nan(frames, 3, h0), a1=_nan(frames, 3, h1), da0=_nan(frames, 3, h0), da1=_nan(frames, 3, h1))
    grads = [torch.full_like(p, float("nan")) for p in params] if prefill is None else [t.clone() for t in prefill]
    rc_f = lib.aft_adapter_fwd_train_f32(C.byref(_ptrs(conds, 3)), C.byref(_ptrs(ws, 9)), C.byref(_ptrs(bs, 9)), C.byref(hid), tokens,
                                         frames, o["tok6"].data_ptr(), o["a0"].data_ptr(), o["a1"].data_ptr(), st)
    rc_b = lib.aft_adapter_bwd_f32(C.byref(_ptrs(conds, 3)), C.byref(_ptrs(ws, 9)), C.byref(_ptrs(bs, 9)), C.byref(hid), tokens, frames,
                                   o["a0"].data_ptr(), o["a1"].data_ptr(), dev["dtok"].data_ptr(), o["da0"].data_ptr(), o["da1"].data_ptr(),
                                   C.byref(_ptrs(grads[0::2], 9)), C.byref(_ptrs(grads[1::2], 9)), int(prefill is not None), st)
    torch.cuda.synchronize()
    o.update(zip(ADAPTER_GRADS, grads))
    if not check:
        return rc_f, rc_b, o
    L.check(rc_f)
    L.check(rc_b)
    return o


def _set(switches, sw):
    for name, value in sw:
        switches.set(name, value)


def gpu_ends(case, switches=None, fill=float("nan")):
    """One ends case on the GPU: (embed rows, tail rows) of ``judge``."""
    _set(switches, case[7])
    inp = make_ends(case)
    dev = _cuda(inp)
    got_e, got_t = hip_embed(case, dev, fill=fill), hip_tail(case, dev, fill=fill)
    names_e = [n for n in ("x0", "d_conv", "d_tok6", "dW1", "db1", "dpos") if n in got_e]
    mag_e = {k: v for k, v in embed(case, inp, magnitudes=True).items() if k in EMBED_SUMS}
    rows_e = judge("ends", names_e, got_e, embed(case, inp), embed(case, inp, torch.float32, "cuda"), mag_e, ENDS_TOL)
    mag_t = {k: v for k, v in tail(case, inp, magnitudes=True).items() if k in TAIL_SUMS}
    rows_t = judge("ends", ("out", "dx", "dW2", "db2"), got_t, tail(case, inp), tail(case, inp, torch.float32, "cuda"), mag_t, ENDS_TOL)
    return rows_e, rows_t


def gpu_dense(case, switches=None, fill=float("nan")):
    _set(switches, case[5])
    inp = make_dense(case)
    got = hip_dense(case, _cuda(inp), fill=fill)
    mag = {k: v for k, v in dense(case, inp, magnitudes=True).items() if k in DENSE_SUMS}
    return judge("dense", [n for n in ("y", "dx", "dW", "db") if n in got], got, dense(case, inp), dense(case, inp, torch.float32, "cuda"),
                 mag, DENSE_TOL)


def gpu_adapter(case):
    """(forward rows, backward rows)."""
    inp = make_adapter(case)
    dev = dict(params=[p.cuda() for p in inp["params"]], conds=[c.cuda() for c in inp["conds"]], dtok=inp["dtok"].cuda())
    got = hip_adapter(case, dev)
    rows_f = judge("adapter", ("tok6", "a0", "a1"), got, adapter_forward(inp), adapter_forward(inp, torch.float32, "cuda"), {},
                   ADAPTER_ELEMENT_TOL)
    a0, a1 = got["a0"].cpu(), got["a1"].cpu()
    ref = adapter_backward(inp, a0, a1)
    y32 = adapter_backward(inp, a0, a1, torch.float32, "cuda")
    mag = {k: v for k, v in adapter_backward(inp, a0, a1, magnitudes=True).items() if k in ADAPTER_GRADS}
    tol = {**{n: ADAPTER_SUM_TOL for n in ADAPTER_GRADS}, "da0": ADAPTER_ELEMENT_TOL, "da1": ADAPTER_ELEMENT_TOL}
    return rows_f, judge("adapter", ("da0", "da1") + ADAPTER_GRADS, got, ref, y32, mag, tol)
