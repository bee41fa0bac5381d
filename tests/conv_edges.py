"""The ConvEnhancer training kernels at the grids where their geometry changes (helper module: no tests here).

Holds the matrix (ONE_BAND .. MANY_PLANES, CASES), a Python restatement of the two planners of csrc/k_conv.hip, the float64 references of
the training forward and of the backward, the bounds, and the defects that tests/test_conv_train_edges.py plants to show that the
bounds see them.  tools/debug/conv_edges_vs_fp64.py prints every figure; profiles/conv_edges_vs_fp64.json holds them.

Backward reference ("tape style", as check (a) of tests/test_train_token_edges.py): it takes the float32 activations c1, c2, c3 the forward KERNEL wrote
as data -- masks are c_k > 0, activations are c_k.double() -- so no ReLU decision crosses a precision boundary:
    g4 = dy,  g_k = conv-transpose(g_{k+1}, w_{k+1}) * (c_k > 0),  dx = conv-transpose(g_1, w_1),
    dW_k = the correlation of g_k with a_{k-1} (a_0 = x),  db_k = sum g_k.
"""
import torch
import torch.nn.functional as F

# ---------------------------------------------------------------- the planners, restated
# csrc/conv_device.h:83-86: kConvThreads = 512 -> kConvWaves = 8; kTileRows = 30; kWStage = 72 * 33 + 96 * 33.
TILE_ROWS, CONV_WAVES, WSTAGE, LDS_BYTES = 30, 8, 72 * 33 + 96 * 33, 160 * 1024


def _band(S, nb):
    """csrc/k_conv.hip:705-708 (= 750-754): rows per band, row tiles over the band and its two halo rows, the row pitch."""
    br = S // nb
    ntiles = -(-(br if nb == 1 else br + 2) // TILE_ROWS)
    return br, ntiles, max(br + 8, 4 + TILE_ROWS * ntiles + 2)


def plan_bands(S, T):
    """csrc/k_conv.hip:701-737 with train = true and extra_floats = 0: the fewest row bands (a divisor of S) whose 17 channel planes
    of T + 2 columns fit the LDS; two column segments from T = 8.  None: no band plan."""
    for nb in range(1, S + 1):
        if S % nb:
            continue
        br, ntiles, sp = _band(S, nb)
        arena = (max(17 * (T + 2) * sp, WSTAGE) + 3) & ~3
        lds = 4 * (arena + 32 + 80)
        if lds <= LDS_BYTES:
            return dict(kind="bands", nbands=nb, band_rows=br, ntiles=ntiles, nseg=2 if T >= 8 else 1, sp=sp, lds=lds, nctiles=1,
                        tcols=T)
    return None


def plan_tiles(S, T, min_tiles=1):
    """csrc/k_conv.hip:744-780 with extra_floats = 0: row bands x column tiles of tcols owned columns (window tcols + 8); of the
    bands with room for an owned column, the first with the fewest computed pixels per owned pixel."""
    best, plan = 0.0, None
    for nb in range(1, S + 1):
        if S % nb:
            continue
        br, ntiles, sp = _band(S, nb)
        if ntiles > CONV_WAVES:
            continue
        room = LDS_BYTES // 4 - 32 - 80 - 4
        wmax = min(room // (17 * sp) - 2, T + 8)
        if wmax < 9 or room < WSTAGE:
            continue
        nct = max((T + wmax - 9) // (wmax - 8), min(min_tiles, T))
        tcols = -(-T // nct)
        nct = -(-T // tcols)
        win = min(tcols + 8, T)
        cost = nb * (br + 8) * nct * win / (S * T)
        if plan is not None and cost >= best:
            continue
        best = cost
        arena = (max(17 * (win + 2) * sp, WSTAGE) + 3) & ~3
        plan = dict(kind="tiles", nbands=nb, band_rows=br, ntiles=ntiles, nseg=max(1, min(CONV_WAVES // ntiles, win // 6)), sp=sp,
                    lds=4 * (arena + 32 + 80), nctiles=nct, tcols=tcols)
    return plan


def plan(S, T, column_tiles=None):
    """csrc/k_conv.hip:810-814 (launch_conv): AFT_CONV_COLUMN_TILES=v forces at least max(2, v) column tiles; else bands, else tiles."""
    if column_tiles is not None:
        return plan_tiles(S, T, max(2, column_tiles))
    return plan_bands(S, T) or plan_tiles(S, T)


def tile_widths(p, T):
    return [min(p["tcols"], T - i * p["tcols"]) for i in range(p["nctiles"])]


def wgrad_chunks(planes, S, T):
    """csrc/k_conv_train.hip:39-40, 261-262: 64-row chunks of wgrad32x8_kernel and its grid (four waves per workgroup)."""
    chunks = planes * T * (-(-S // 64))
    return chunks, max(1, min(512, -(-chunks // 4)))


# ---------------------------------------------------------------- the matrix
# (S, T): the property test_every_grid_reaches_its_plan_edge_cpu asserts for it.  2 planes.  (120, 16) is the largest one-band plan at
# 120 rows (157 120 bytes of LDS; 17 columns need two bands).
ONE_BAND = [(1, 1), (2, 3), (3, 8), (29, 7), (30, 8), (31, 9), (60, 14), (61, 14), (63, 4), (64, 4), (65, 4), (128, 2), (129, 2),
            (120, 16), (120, 14)]
# (S, T): (bands, rows per band)
SEVERAL_BANDS = {(118, 20): (2, 59), (122, 15): (2, 61), (122, 28): (61, 2), (59, 40): (59, 1), (232, 33): (4, 58), (30, 64): (2, 15),
                 (62, 64): (31, 2)}
# (S, T): (bands, widths of the column tiles); (16, 70) and (37, 66) have no band plan and take what plan_tiles gives
COLUMN_TILES = {(30, 65): (1, [33, 32]), (62, 65): (2, [22, 22, 21]), (16, 70): None, (37, 66): None}
FORCED_TILES = [((31, 9), 2), ((31, 9), 7), ((118, 20), 2), ((118, 20), 7)]          # AFT_CONV_COLUMN_TILES
MANY_PLANES = [((8, 8), 600), ((65, 3), 350), ((24, 4), 9), ((24, 4), 17)]
DEFAULT_GRID = (120, 14)
NSPLITS = ["1", "2", "4"]                                                            # AFT_CONV_NSPLIT on the default grid; + unset
ACCUMULATE_GRID = (65, 4)
END_TO_END = [(61, 14), (118, 20), (62, 65), (120, 14)]                              # 2 planes
END_TO_END_PLANES = [((65, 3), 350), ((24, 4), 9)]

# A case: (S, T, planes, switches as a tuple of (name, value), scratch) -- scratch False: the forward call gets scratch = NULL
PLAIN_CASES = ([(S, T, 2, (), True) for S, T in ONE_BAND + list(SEVERAL_BANDS) + list(COLUMN_TILES)]
               + [(S, T, n, (), True) for (S, T), n in MANY_PLANES])
VARIANT_CASES = ([(*DEFAULT_GRID, 2, (("AFT_CONV_NSPLIT", v),), True) for v in NSPLITS]
                 + [(*DEFAULT_GRID, 2, (), False)]
                 + [(S, T, 2, (("AFT_CONV_COLUMN_TILES", str(v)),), True) for (S, T), v in FORCED_TILES])
CASES = PLAIN_CASES + VARIANT_CASES


def case_id(c):
    S, T, n, sw, scratch = c
    return f"{S}x{T}x{n}" + "".join(f"_{k[4:].lower()}{v}" for k, v in sw) + ("" if scratch else "_noscratch")


def all_grids():
    """Every (planes, S, T) the GPU tests run."""
    return sorted({(c[2], c[0], c[1]) for c in CASES} | {(2, *ACCUMULATE_GRID)} | {(2, S, T) for S, T in END_TO_END}
                  | {(n, S, T) for (S, T), n in END_TO_END_PLANES})


# ---------------------------------------------------------------- inputs
PARAM_NAMES = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias", "conv4.weight", "conv4.bias")
GRAD_NAMES = ("dW1", "db1", "dW2", "db2", "dW3", "db3", "dW4", "db4")


def make_case(S, T, planes):
    """Float32 CPU tensors, the same bits on every device: the eight parameters of blocks.ConvEnhancer() under a fixed seed (conv1's
    weight and bias, ...), x and dy [planes, 1, S, T]."""
    import adafortitran_amd.blocks as blocks
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(20250 + 1009 * S + 31 * T + planes)
        params = [p.detach().clone() for p in blocks.ConvEnhancer().parameters()]
        x, dy = torch.randn(planes, 1, S, T), torch.randn(planes, 1, S, T)
    return params, x, dy


def to_ts(t):
    """[n, C, S, T] -> the kernels' [n, C, T, S]; its own inverse."""
    return t.transpose(2, 3).contiguous()


# ---------------------------------------------------------------- seams (the planted defects' tool)
def _split(t, dim, size):
    return t.split(size, dim=dim) if size else (t,)


def conv_seamed(conv, inp, dim, size):
    """``conv`` (a 3x3, padding 1 map [n, C, S, T] -> [n, C', S, T]) run separately on consecutive slabs of ``size`` rows (dim 2) or
    columns (dim 3): every slab seam is taken as zero padding, which is what a band or a column tile without its halo computes."""
    return torch.cat([conv(s) for s in _split(inp, dim, size)], dim=dim)


# ---------------------------------------------------------------- forward
def _taps(x):
    S, T = x.shape[2], x.shape[3]
    pad = F.pad(x, (1, 1, 1, 1))
    return [(ky, kx, pad[:, :, ky:ky + S, kx:kx + T]) for ky in range(3) for kx in range(3)]


def conv_taps(x, w, b=None):
    """conv2d(x, w, b, padding=1) as nine shifted channel products: plain matrix products on every device (the GPU yardstick does not
    depend on a convolution library's choice of algorithm)."""
    out = sum(torch.einsum("oc,ncst->nost", w[:, :, ky, kx], xs) for ky, kx, xs in _taps(x))
    return out if b is None else out + b.view(1, -1, 1, 1)


def dgrad_taps(g, w):
    return conv_taps(g, w.transpose(0, 1).flip(2, 3))


def wgrad_taps(a, g):
    return torch.stack([torch.einsum("nost,ncst->oc", g, xs) for _, _, xs in _taps(a)], dim=-1).reshape(g.shape[1], a.shape[1], 3, 3)


def conv_ops(device):
    """(conv, dgrad, wgrad): torch's own convolutions on the CPU -- F.conv2d, torch.nn.grad.conv2d_input / conv2d_weight, the float64
    reference -- and the shifted products above elsewhere (test_conv_train_edges.py holds the two to each other in float64)."""
    if str(device) == "cpu":
        return (lambda x, w, b: F.conv2d(x, w, b, padding=1),
                lambda g, w: torch.nn.grad.conv2d_input((g.shape[0], w.shape[1], g.shape[2], g.shape[3]), w, g, padding=1),
                lambda a, g: torch.nn.grad.conv2d_weight(a, (g.shape[1], a.shape[1], 3, 3), g, padding=1))
    return conv_taps, dgrad_taps, wgrad_taps


def forward(params, x, dtype=torch.float64, device="cpu", seam3=None):
    """y [n, 1, S, T] and c1, c2, c3 in the kernels' [n, C, T, S], float64 CPU tensors.  float64 on the CPU is the reference, float32
    on the GPU the yardstick.  ``seam3`` = (dim, size): defects (a) / (d), conv3 takes the band (dim 2) or column-tile (dim 3) seams as
    zero padding."""
    w1, b1, w2, b2, w3, b3, w4, b4 = [p.to(device=device, dtype=dtype) for p in params]
    conv = conv_ops(device)[0]
    c1 = F.relu(conv(x.to(device=device, dtype=dtype), w1, b1))
    c2 = F.relu(conv(c1, w2, b2))
    conv3 = lambda t: conv(t, w3, b3)  # noqa: E731
    c3 = F.relu(conv3(c2) if seam3 is None else conv_seamed(conv3, c2, *seam3))
    y = conv(c3, w4, b4)
    return [y.double().cpu()] + [to_ts(c).double().cpu() for c in (c1, c2, c3)]


FWD_NAMES = ("y", "c1", "c2", "c3")

# ---------------------------------------------------------------- backward
BWD_ELEMENT_NAMES = ("dx", "g1", "g2", "g3")


def backward(params, x, dy, c_ts, dtype=torch.float64, device="cpu", defect=None, geo=None, magnitudes=False):
    """The tape-style backward from the float32 activations ``c_ts`` = (c1, c2, c3) in [n, C, T, S] that the forward kernel wrote.
    Returns {"dx", "g1", "g2", "g3" (g* in [n, C, T, S]), "dW1", "db1", ... "db4"} as float64 CPU tensors.

    ``magnitudes``: A = sum |terms| of every parameter gradient -- the same routine on |g_k| and |a_{k-1}| with the g_k of the
    plain run (the elementwise tensors are those of the plain run).

    ``defect`` (with ``geo`` = the grid's plan, or what the defect needs) plants one of DEFECTS:
      seam_dgrad2       (b) conv2^T of the data gradient takes the band seams as zero padding
      halo_mask         (c) a band's halo rows of g2 pass unmasked into its conv2^T (g2 as saved stays masked)
      tail_dropped      (e) wgrad32x8_kernel's tail value at row s0 + 64 is zero: dW2 loses g2[s0 + 63] * a1[s0 + 64] in its three
                            ky = 2 taps, dW3 loses g3[s0 + 64] * a2[s0 + 63] in its three ky = 0 taps (the kernel's shift is -1 there)
      plane9_missing    (f) wgrad8x1_kernel's second plane group (planes 8 ..) never reaches dW1 / dW4
      second_chunk      (g) wave 0 of workgroup 0 skips its second chunk (chunk 4 x grid) in dW2
    """
    to = lambda t: t.to(device=device, dtype=dtype)  # noqa: E731
    _, _dgrad, _wgrad = conv_ops(device)
    w1, _, w2, _, w3, _, w4, _ = [to(p) for p in params]
    a0, g4 = to(x), to(dy)
    c1, c2, c3 = [to(to_ts(c)) for c in c_ts]                     # [n, C, S, T]
    m1, m2, m3 = [(c > 0).to(dtype) for c in (c1, c2, c3)]
    g3 = _dgrad(g4, w4) * m3
    g2 = _dgrad(g3, w3) * m2
    conv2t = lambda t: _dgrad(t, w2)  # noqa: E731
    if defect == "seam_dgrad2":
        g1 = conv_seamed(conv2t, g2, 2, geo["band_rows"]) * m1
    elif defect == "halo_mask":
        u2, br, S = _dgrad(g3, w3), geo["band_rows"], g2.shape[2]
        parts = []
        for lo in range(0, S, br):
            m = m2.clone()
            m[:, :, [r for r in (lo - 1, lo + br) if 0 <= r < S], :] = 1.0
            parts.append(conv2t(u2 * m)[:, :, lo:lo + br, :])
        g1 = torch.cat(parts, dim=2) * m1
    else:
        g1 = conv2t(g2) * m1
    dx = _dgrad(g1, w1)
    acts, gs = [a0, c1, c2, c3], [g1, g2, g3, g4]
    if magnitudes:
        acts, gs = [t.abs() for t in acts], [t.abs() for t in gs]
    out = {"dx": dx, "g1": to_ts(g1), "g2": to_ts(g2), "g3": to_ts(g3)}
    for k, (a, g) in enumerate(zip(acts, gs)):
        out[f"dW{k + 1}"], out[f"db{k + 1}"] = _wgrad(a, g), g.sum(dim=(0, 2, 3))
    S = x.shape[2]
    if defect == "tail_dropped":
        lost2, lost3 = torch.zeros_like(gs[1]), torch.zeros_like(gs[2])
        rows = [r for r in range(64, S, 64)]                      # s0 + 64 inside the plane
        lost2[:, :, [r - 1 for r in rows], :] = gs[1][:, :, [r - 1 for r in rows], :]
        lost3[:, :, rows, :] = gs[2][:, :, rows, :]
        out["dW2"] = out["dW2"].clone()
        out["dW3"] = out["dW3"].clone()
        out["dW2"][:, :, 2, :] -= _wgrad(acts[1], lost2)[:, :, 2, :]
        out["dW3"][:, :, 0, :] -= _wgrad(acts[2], lost3)[:, :, 0, :]
    elif defect == "plane9_missing":
        out["dW1"] = _wgrad(acts[0][:8], gs[0][:8])
        out["dW4"] = _wgrad(acts[3][:8], gs[3][:8])
    elif defect == "second_chunk":
        n_, T = x.shape[0], x.shape[3]
        schunks = -(-S // 64)
        c = 4 * wgrad_chunks(n_, S, T)[1]
        sc, t, n = c % schunks, (c // schunks) % T, c // (schunks * T)
        lost = torch.zeros_like(gs[1])
        lost[n, :, 64 * sc:64 * sc + 64, t] = gs[1][n, :, 64 * sc:64 * sc + 64, t]
        out["dW2"] = out["dW2"] - _wgrad(acts[1], lost)
    return {k: v.double().cpu() for k, v in out.items()}


DEFECTS = ("seam_fwd3", "seam_dgrad2", "halo_mask", "tile_seam_fwd3", "tail_dropped", "plane9_missing", "second_chunk")

# ---------------------------------------------------------------- bounds
TOL_FWD, TOL_DGRAD, TOL_WGRAD = 2e-5, 1e-4, 2e-4      # the project's bounds for these kernels (tests/test_train_hip.py)
EDGE_FACTOR = 4.0                                     # as the token-edge tests; not measured for these kernels
SUM_FLOOR = 2.0 ** -22
FACTOR = {}                                           # tensor name -> a raised factor, with its figure in the JSON (none so far)


def rel_err(a, ref):
    """max |a - ref| / max |ref| (float64 CPU tensors)."""
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def sum_err(a, ref, mag):
    """max_i |a_i - ref_i| / A_i: a sum's error against the sum of its terms' magnitudes."""
    return float(((a.double().cpu() - ref).abs() / mag.clamp_min(1e-300)).max())


def element_limit(name, ref, y32):
    """(e32, project bound, edge bound) of an elementwise tensor, relative to the float64 tensor's max; both bounds must hold."""
    e32 = rel_err(y32, ref)
    return e32, (TOL_FWD if name in FWD_NAMES else TOL_DGRAD), FACTOR.get(name, EDGE_FACTOR) * e32 + 1e-6


def sum_limit(name, ref, mag, g32):
    """(e32', bound on err_i / A_i, e32 relative to the max, project bound relative to the max) of a parameter gradient."""
    e32 = sum_err(g32, ref, mag)
    return e32, FACTOR.get(name, EDGE_FACTOR) * e32 + SUM_FLOOR, rel_err(g32, ref), TOL_WGRAD


def judge(names, got, ref, y32, mag=None):
    """One row per tensor: dict(name, hip, e32, bound, project, ok, ratio [, hip_max, e32_max]); ratio = the error over the tighter bound.  ``hip`` and ``bound`` are relative to the
    tensor's max for elementwise tensors and per element relative to A_i for parameter gradients (then hip_max is the error relative
    to the max, held to ``project``).  The HIP result enters ``hip`` / ``hip_max`` only."""
    rows = []
    for n in names:
        if mag is not None and n in mag:
            e32, bound, e32_max, project = sum_limit(n, ref[n], mag[n], y32[n])
            hip, hip_max = sum_err(got[n], ref[n], mag[n]), rel_err(got[n], ref[n])
            rows.append(dict(name=n, hip=hip, e32=e32, bound=bound, hip_max=hip_max, e32_max=e32_max, project=project,
                             ok=hip <= bound and hip_max <= project, ratio=max(hip / bound, hip_max / project)))
        else:
            e32, project, bound = element_limit(n, ref[n], y32[n])
            hip = rel_err(got[n], ref[n])
            rows.append(dict(name=n, hip=hip, e32=e32, bound=bound, project=project, ok=hip <= bound and hip <= project,
                             ratio=hip / min(bound, project)))
    return rows


def show(label, rows):
    for r in rows:
        extra = f" | of max: hip {r['hip_max']:.2e} torch32 {r['e32_max']:.2e}" if "hip_max" in r else ""
        print(f"{label} {r['name']}: hip {r['hip']:.2e} torch32 {r['e32']:.2e} bound {r['bound']:.2e} project {r['project']:.2e}{extra}")
    return [f"{r['name']}: hip {r['hip']:.2e} > bound {r['bound']:.2e} or project {r['project']:.2e}" for r in rows if not r["ok"]]


# ---------------------------------------------------------------- the library calls (GPU)
def _ptr4(tensors):
    import ctypes as C
    arr = (C.c_void_p * 4)()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def hip_forward(params, x, scratch=True):
    """aft_conv_enhancer_fwd_train_f32 on CUDA float32 tensors: [y, c1, c2, c3], the c_k [n, C, T, S] as the kernel wrote them."""
    import ctypes as C
    from adafortitran_amd import _lib
    lib = _lib.load()
    n, _, S, T = x.shape
    y = torch.empty_like(x)
    saved = [torch.empty((n, ch, T, S), dtype=torch.float32, device=x.device) for ch in (8, 32, 8)]
    nbytes = lib.aft_conv_enhancer_fwd_scratch_bytes(n, S, T) if scratch else 0
    buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    _lib.check(lib.aft_conv_enhancer_fwd_train_f32(C.byref(_ptr4(params[0::2])), C.byref(_ptr4(params[1::2])), x.data_ptr(), y.data_ptr(),
                                                   *[t.data_ptr() for t in saved], buf.data_ptr() if scratch else None, nbytes, n, S, T,
                                                   _lib.current_stream_ptr(x.device)))
    torch.cuda.synchronize()
    return [y] + saved


def hip_backward(params, x, dy, cs, prefill=None):
    """aft_conv_enhancer_bwd_f32: {"dx", "dW1" .. "db4", "g1", "g2", "g3"}.  The g_k are read from the call's scratch, whose first
    region holds g3 [n, 8, T, S] | g2 [n, 32, T, S] | g1 [n, 8, T, S] (csrc/aft_train.hip: plan_conv_scratch; one launch while the
    planes' conv2 activations stay under 2 GiB).  ``prefill``: eight tensors the call adds onto (accumulate = 1)."""
    import ctypes as C
    from adafortitran_amd import _lib
    lib = _lib.load()
    n, _, S, T = x.shape
    assert n * 32 * S * T * 4 < 2 ** 31
    grads = [torch.full_like(p, float("nan")) for p in params] if prefill is None else [t.clone() for t in prefill]
    dx = torch.empty_like(x)
    nbytes = lib.aft_conv_enhancer_scratch_bytes(n, S, T)
    assert nbytes > 0 and nbytes % 4 == 0
    buf = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    _lib.check(lib.aft_conv_enhancer_bwd_f32(C.byref(_ptr4(params[0::2])), x.data_ptr(), *[c.data_ptr() for c in cs], dy.data_ptr(),
                                             dx.data_ptr(), C.byref(_ptr4(grads[0::2])), C.byref(_ptr4(grads[1::2])),
                                             int(prefill is not None), buf.data_ptr(), nbytes, n, S, T, _lib.current_stream_ptr(x.device)))
    torch.cuda.synchronize()
    st8 = n * 8 * S * T
    out = dict(zip(GRAD_NAMES, grads), dx=dx)
    out["g3"], out["g2"], out["g1"] = (buf[:st8].view(n, 8, T, S), buf[st8:5 * st8].view(n, 32, T, S), buf[5 * st8:6 * st8].view(n, 8, T, S))
    return out


def gpu_case(case, switches=None):
    """Run one case of the matrix on the GPU: (forward rows, backward rows) of ``judge``.  ``switches``: the tests' fixture, or any
    object with set(name, value)."""
    S, T, n, sw, scratch = case
    params, x, dy = make_case(S, T, n)
    for name, value in sw:
        switches.set(name, value)
    dev = [t.cuda() for t in params], x.cuda(), dy.cuda()
    fwd = hip_forward(dev[0], dev[1], scratch)
    hip = hip_backward(dev[0], dev[1], dev[2], fwd[1:])
    ref_f = dict(zip(FWD_NAMES, forward(params, x)))
    y32_f = dict(zip(FWD_NAMES, forward(params, x, torch.float32, "cuda")))
    rows_f = judge(FWD_NAMES, dict(zip(FWD_NAMES, fwd)), ref_f, y32_f)
    cs = [c.cpu() for c in fwd[1:]]
    ref = backward(params, x, dy, cs)
    rows_b = judge(BWD_ELEMENT_NAMES + GRAD_NAMES, hip, ref, backward(params, x, dy, cs, torch.float32, "cuda"),
                   {k: v for k, v in backward(params, x, dy, cs, magnitudes=True).items() if k in GRAD_NAMES})
    return rows_f, rows_b
