"""Float64 reference of one training-mode encoder layer WITH the library's own dropout masks (helper module: no tests here).

The masks of the training kernels are a pure function of (seed, site, row, column): ``site_seed`` of csrc/aft_train.hip turns the
call's 64-bit seed into one 32-bit seed per site, and ``dropmask_row_word`` / ``dropmask_col_word`` / ``dropmask_keep`` of
csrc/aft_internal.h decide every element.  Restated here in Python integers and numpy, so that a plain torch composite can be run
with exactly the masks the kernels use, and the comparison with float64 is as sharp with dropout on as it is at p = 0.

Sites: 0 = attention probabilities (rows / columns = query / key, both indexed (plane * heads + head) * tokens + token),
1 = out_proj output, 2 = FFN hidden layer, 3 = linear2 output (rows = plane * tokens + token, columns = feature).

Two test matrices live at the end: LAYER_CASES (one case per kernel family) and EDGE_CASES (token counts on and around the 32-row
tiles), each with a table of the kernels its rows reach.
"""
import math

import numpy as np
import torch

M64 = (1 << 64) - 1
M32 = 0xFFFFFFFF
GOLD = 0x9E3779B1


def site_seed(seed, site):
    """csrc/aft_train.hip::site_seed (a splitmix64 step of seed + golden * (site + 1)), low 32 bits."""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (site + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return (z ^ (z >> 31)) & M32


def mix32(x):
    """murmur3 finaliser on uint64 arrays holding 32-bit values."""
    x = x.astype(np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & M32
    x ^= x >> np.uint64(16)
    return x


def row_word(seed32, idx):
    idx = np.asarray(idx, dtype=np.uint64) & M32
    return (mix32(((idx * np.uint64(GOLD)) & M32) ^ np.uint64(seed32)) >> np.uint64(8)) | np.uint64(1)


def col_word(seed32, idx):
    idx = np.asarray(idx, dtype=np.uint64) & M32
    cseed = ((~int(seed32) & M32) * 0x632BE5AB + 0x7F4A7C15) & M32
    return (mix32(((idx * np.uint64(GOLD)) & M32) ^ np.uint64(cseed)) >> np.uint64(8)) | np.uint64(1)


def threshold(p):
    """The library computes it from the float32 p: (uint32_t)((double)p * 2^32)."""
    return int(float(np.float32(p)) * 2 ** 32)


def keep_scale(p):
    """1 / (1 - p) in float32, as the library computes it (a numpy float32)."""
    return np.float32(1) / (np.float32(1) - np.float32(p))


def keep_mask(seed32, row_idx, col_idx, p):
    """bool [len(row_idx), len(col_idx)]: element kept when the low 32 bits of the product of its two odd 24-bit words reach
    the threshold."""
    prod = (row_word(seed32, row_idx)[:, None] * col_word(seed32, col_idx)[None, :]) & M32
    return prod >= np.uint64(threshold(p))


def layer_masks(seed, p, planes, heads, tokens, d, sites=(0, 1, 2, 3), row_of=None, key_of=None):
    """The four masks of one layer call: [planes, heads, T, T], [rows, d], [rows, 2d], [rows, d] (bool).  ``sites``, ``row_of`` and
    ``key_of`` exist for the planted-defect tests: which site's seed each mask takes, a map applied to the global row index, and
    ``key_of(problem, keys)``: the index the attention mask hashes for each key of one (plane, head) in place of
    problem * tokens + key."""
    rows = np.arange(planes * tokens, dtype=np.uint64)
    if row_of is not None:
        rows = row_of(rows)
    s = [site_seed(seed, k) for k in sites]
    m0 = np.empty((planes, heads, tokens, tokens), dtype=bool)
    for ph in range(planes * heads):
        idx = np.arange(tokens, dtype=np.uint64) + np.uint64(ph * tokens)
        keys = idx if key_of is None else key_of(ph, np.arange(tokens, dtype=np.uint64))
        m0[ph // heads, ph % heads] = keep_mask(s[0], idx, keys, p)
    return [m0, keep_mask(s[1], rows, np.arange(d), p), keep_mask(s[2], rows, np.arange(2 * d), p),
            keep_mask(s[3], rows, np.arange(d), p)]


def ones_masks(planes, heads, tokens, d):
    rows = planes * tokens
    return [np.ones((planes, heads, tokens, tokens), bool), np.ones((rows, d), bool), np.ones((rows, 2 * d), bool),
            np.ones((rows, d), bool)]


def _ln(s, w, b):
    mu = s.mean(-1, keepdim=True)
    var = ((s - mu) ** 2).mean(-1, keepdim=True)          # biased variance, eps inside the root
    return (s - mu) / torch.sqrt(var + 1e-5) * w + b


DEFECTS = ("last_key_left_out", "phantom_key", "last_query_detached_kv")


def attention(q, k, v, m0, ks0, defect=None):
    """O = (softmax(q k^T / sqrt(dh)) * M0 * ks) v per (plane, head); q, k, v [planes, heads, T, dh].  ``defect`` plants what a
    kernel can get wrong at the last key or query of a plane (the tests of the token-edge bounds): ``last_key_left_out`` -- the
    softmax runs over every key but the last; ``phantom_key`` -- one more key with score 0 and value 0, what a range mask one key
    too long produces; ``last_query_detached_kv`` -- the last query row reads detached k and v (its q stays live), so it
    contributes nothing to dK and dV; ``last_value_zeroed`` (the inference matrix, tests/infer_edges.py; not in DEFECTS) -- the last key
    keeps its softmax weight but contributes a zero value, what a V^T padding mask one column too long produces."""
    scale = 1.0 / math.sqrt(q.shape[-1])
    if defect == "last_value_zeroed":
        v = torch.cat([v[..., :-1, :], torch.zeros_like(v[..., -1:, :])], dim=-2)
    s = q @ k.transpose(-1, -2) * scale if defect != "last_query_detached_kv" else torch.cat(
        [q[..., :-1, :] @ k.transpose(-1, -2), q[..., -1:, :] @ k.detach().transpose(-1, -2)], dim=-2) * scale
    if defect == "last_key_left_out":
        P = torch.cat([torch.softmax(s[..., :-1], dim=-1), torch.zeros_like(s[..., -1:])], dim=-1)
    elif defect == "phantom_key":
        P = torch.softmax(torch.cat([s, torch.zeros_like(s[..., -1:])], dim=-1), dim=-1)[..., :-1]
    else:
        P = torch.softmax(s, dim=-1)
    Pm = P * m0 * ks0
    if defect == "last_query_detached_kv":
        return torch.cat([Pm[..., :-1, :] @ v, Pm[..., -1:, :] @ v.detach()], dim=-2)
    return Pm @ v


def attention_lse(q, k, defect=None):
    """Natural-log log-sum-exp of the scaled scores, [planes, heads, T], under the same planted defects."""
    s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
    if defect == "last_key_left_out":
        s = s[..., :-1]
    elif defect == "phantom_key":
        s = torch.cat([s, torch.zeros_like(s[..., -1:])], dim=-1)
    return torch.logsumexp(s, dim=-1)


def attention_tape(qkv, m0, ks0, planes, heads, dtype, device, defect=None):
    """What the attention kernel leaves in the tape, from the float32 ``qkv`` block it read ([planes * T, 3 d]): the natural-log
    LSE [planes, heads, T] and the attention output [planes, T, d], as float64 CPU tensors.  float64 on the CPU is the reference,
    float32 on the GPU the yardstick."""
    qkv = torch.as_tensor(np.asarray(qkv)).to(device=device, dtype=dtype)
    d = qkv.shape[-1] // 3
    T = qkv.shape[0] // planes
    q, k, v = [t.reshape(planes, T, heads, d // heads).transpose(1, 2) for t in qkv.split(d, dim=-1)]
    m0 = torch.as_tensor(np.asarray(m0)).to(device=device, dtype=dtype)
    O = attention(q, k, v, m0, float(ks0), defect).transpose(1, 2).reshape(planes, T, d)
    return attention_lse(q, k, defect).double().cpu(), O.double().cpu()


def reference_layer(x, params, masks, keep_scale, heads, act, dtype, device, bias_outside=(), probe=None, defect=None):
    """The post-LN layer in plain torch ops with explicit masks; differentiable in ``x`` and ``params`` (twelve tensors in
    _abi.LAYER_PARAM_NAMES order).  x [planes, T, d].  The bias is inside drop(...) at sites 1 and 3, as in
    nn.TransformerEncoderLayer.  ``keep_scale``: one number, or one per site.  float64 on the CPU is the reference; float32 on
    the GPU is the rounding yardstick.  ``bias_outside`` (sites whose bias is added after the dropout) is a planted defect for
    the tests of the check itself, ``defect`` another (one of DEFECTS, see ``attention``); ``probe`` receives the linear1
    pre-activation and the in-projection's output."""
    to = lambda t: t.to(device=device, dtype=dtype)  # noqa: E731
    x = to(x)
    wqkv, bqkv, wo, bo, w1, b1, w2, b2, g1, be1, g2, be2 = [to(q) for q in params]
    m0, m1, m2, m3 = [to(torch.as_tensor(np.asarray(m))) for m in masks]
    ks = [float(k) for k in (keep_scale if isinstance(keep_scale, (tuple, list)) else (keep_scale,) * 4)]
    planes, T, d = x.shape
    dh = d // heads
    qkv = x @ wqkv.t() + bqkv
    q, k, v = [t.reshape(planes, T, heads, dh).transpose(1, 2) for t in qkv.split(d, dim=-1)]
    if probe is not None:
        probe["qkv"] = qkv.detach()
    if defect is None:
        P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1)
        O = ((P * m0 * ks[0]) @ v).transpose(1, 2).reshape(planes, T, d)
    else:
        O = attention(q, k, v, m0, ks[0], defect).transpose(1, 2).reshape(planes, T, d)
    m1, m2, m3 = m1.reshape(planes, T, d), m2.reshape(planes, T, 2 * d), m3.reshape(planes, T, d)
    if 1 in bias_outside:
        s1 = x + (O @ wo.t()) * m1 * ks[1] + bo
    else:
        s1 = x + (O @ wo.t() + bo) * m1 * ks[1]
    x1 = _ln(s1, g1, be1)
    a = x1 @ w1.t() + b1
    if probe is not None:
        probe["a"] = a.detach()
    hd = (torch.nn.functional.gelu(a) if act == "gelu" else torch.relu(a)) * m2 * ks[2]
    if 3 in bias_outside:
        s2 = x1 + (hd @ w2.t()) * m3 * ks[3] + b2
    else:
        s2 = x1 + (hd @ w2.t() + b2) * m3 * ks[3]
    return _ln(s2, g2, be2)


GRAD_NAMES = ("dx", "self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
              "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
              "norm2.bias")


def make_case(d, heads, tokens, planes, seed, layers=1):
    """Deterministic float32 inputs, made on the CPU so that every device sees the same bits: x, gout [planes, T, d] and
    ``layers`` parameter sets (ABI order) with non-trivial biases and LayerNorm parameters."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
    x, gout = rn(planes, tokens, d), rn(planes, tokens, d)
    sets = []
    for _ in range(layers):
        sets.append([rn(3 * d, d) / math.sqrt(d), 0.1 * rn(3 * d), rn(d, d) / math.sqrt(d), 0.1 * rn(d),
                     rn(2 * d, d) / math.sqrt(d), 0.1 * rn(2 * d), rn(d, 2 * d) / math.sqrt(2 * d), 0.1 * rn(d),
                     1 + 0.1 * rn(d), 0.1 * rn(d), 1 + 0.1 * rn(d), 0.1 * rn(d)])
    return x, gout, (sets[0] if layers == 1 else sets)


def reference_grads(x, gout, param_sets, mask_sets, keep_scale, heads, act, dtype=torch.float64, device="cpu", **kw):
    """Run ``reference_layer`` over one or more layers (``param_sets`` / ``mask_sets``: one entry per layer) and differentiate:
    returns (out, [dx, then every layer's twelve parameter gradients]) as float64 CPU tensors."""
    xl = x.detach().to(device=device, dtype=dtype).requires_grad_(True)
    leaves = [[q.detach().to(device=device, dtype=dtype).requires_grad_(True) for q in ps] for ps in param_sets]
    h = xl
    for ps, ms in zip(leaves, mask_sets):
        h = reference_layer(h, ps, ms, keep_scale, heads, act, dtype, device, **kw)
    h.backward(gout.to(device=device, dtype=dtype))
    grads = [xl.grad] + [q.grad for ps in leaves for q in ps]
    return h.detach().double().cpu(), [t.double().cpu() for t in grads]


def rel_err(a, ref):
    """max |a - ref| / max |ref| (float64 CPU tensors)."""
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


# ---- the GPU test matrix (tests/test_train_dropout.py, tools/debug/dropout_vs_fp64.py) ----
# (d, heads, ofdm grid at patch 3x2, planes, act, p, input seed).  The relu cases' input seeds are ones whose float64 forward keeps
# every linear1 pre-activation at least 1e-5 |a|max away from zero (test_relu_cases_have_a_margin_cpu).
LAYER_CASES = [
    (128, 4, (120, 14), 2, "gelu", 0.1, 1),     # fused chains, attn_bwd_kernel<280,1>
    (128, 4, (24, 14), 2, "relu", 0.25, 102),     # ragged tiles, attn_bwd_kernel<0,1>
    (128, 4, (12, 14), 2, "gelu", 0.5, 3),      # one masked key tile
    (128, 4, (240, 28), 2, "gelu", 0.1, 4),     # 35 key tiles
    (128, 2, (24, 14), 2, "gelu", 0.1, 5),      # head dim 64 kernels
    (128, 8, (24, 14), 6, "relu", 0.1, 131),      # head dim 16 padded to 32
    (192, 4, (24, 14), 2, "gelu", 0.1, 7),      # head dim 48 padded to 64, NPL 3
    (256, 8, (48, 14), 2, "gelu", 0.1, 8),      # add_ln NPL 4 + gemm_act at N = 512
    (96, 3, (24, 14), 2, "relu", 0.25, 100),      # HALF row-wise variants
    (512, 4, (24, 14), 2, "gelu", 0.1, 10),     # wide<4> attention, stand-alone act fwd/bwd (ff 1024)
    (384, 4, (24, 14), 2, "relu", 0.1, 117),     # wide<3> attention
    (448, 8, (12, 14), 2, "gelu", 0.1, 12),     # head dim 56 padded to 64
    (200, 8, (24, 14), 2, "gelu", 0.1, 13),     # model_dim off the multiples of 32, head dim 25
    (8, 1, (12, 14), 2, "gelu", 0.5, 14),       # smallest
]
DROP_SEED = 3_000_000_000_000_000_007           # above 2^32, below 2^62 (the stack draws seeds up to 2^62)
TOL_FWD, TOL_GRAD, TOL_STACK_GRAD = 5e-5, 2e-4, 3e-4     # the project's bounds for these kernels at p = 0


def tokens_of(ofdm, patch=(3, 2)):
    return (ofdm[0] // patch[0]) * (ofdm[1] // patch[1])


def bound(project, e_torch32):
    """max(project bound, 2 x the float32 composite's own error + 1e-6): the HIP result never enters it."""
    return max(project, 2.0 * e_torch32 + 1e-6)


# ---- the token-edge matrix (tests/test_train_token_edges.py, tools/debug/token_edges_vs_fp64.py) ----
# Every training kernel of the layer works in 32-row tiles (attention: 32-token key and query tiles, three waves per workgroup; the
# row-local chains: 32-row tiles of rows = planes * tokens, with a ``ragged`` instantiation; GEMM epilogues: 64-row tiles; sliced
# reductions: rows / 32, / 64, / 128), and LAYER_CASES only knows token counts that are multiples of 7.  Token count N is the grid
# (3 N, 2) at patch 3x2.  All gelu, 2 planes, rows = 2 N.
#
#   tokens        why
#   31            one ragged tile, the last key the only one masked; 62 rows: the chains' last tile holds 30 rows
#   32, 64, 96    full last tile: no masked key; 96 = three tiles, a whole three-wave round on attn_bwd_kernel<0, *>
#   33, 65, 97    a tail of one token; 66, 130 and 194 rows: the chains' last tile holds 2 rows
#   160           five tiles: a round of three and a round of two
#   193           seven tiles (192 + 1): two whole rounds and a tail of one token in a round of one
#   320, 321      the twelve-wave workgroup's fit: 4 * group_lds <= 160 KiB holds up to 10 tiles
#   2368, 2369    group_lds <= 64 KiB holds up to 74 tiles: one-pass attn_bwd_kernel / attn_bwd_q_kernel + attn_bwd_kv_kernel
#
#   (d, heads)    kernels the row reaches                                                        tokens        p
#   (128, 4)      fused chains (chain_fwd_train / chain_bwd, ragged), attn_train_fwd_kernel,     EDGE_TOKENS   0, 0.1
#                 attn_bwd_kernel<0, 1>; at 321 the same kernels past the twelve-wave fit
#   (128, 2)      head dim 64: attn_train_fwd64_kernel, attn_bwd_q64_kernel, attn_bwd_kv64_kernel EDGE_TOKENS   0.1 (0 at 32, 33, 97)
#   (256, 8)      gemm_add_ln, gemm_act, gemm_actbwd, ln_bwd: 64-row tiles                        EDGE_TOKENS   0.1 (0 at 32, 33, 97)
#   (384, 4)      attn_train_fwd_wide_kernel<3>, attn_bwd_q_wide / attn_bwd_kv_wide<3>            EDGE_TOKENS_4 0.1
#   (512, 4)      the same at <4>, stand-alone activation forward / backward                      EDGE_TOKENS_4 0.1
#   (128, 8)      head dim 16 padded to 32 (pad_heads / unpad_heads around the 32-feature kernels) EDGE_TOKENS_4 0.1
#   (96, 3)       HALF row-wise variants                                                          EDGE_TOKENS_4 0.1
#   (200, 8)      head dim 25, the _any kernels                                                   EDGE_TOKENS_4 0.1
#   (32, 1)       attn_bwd_kernel<0, 1> at 2368, attn_bwd_q_kernel + attn_bwd_kv_kernel at 2369   2368, 2369    0, 0.1
#   variants      (128, 4) p 0.1 at EDGE_VARIANT_TOKENS: unfused forward + backward, AFT_TRAIN_ATTN_BWD_SPLIT, AFT_ATTN_BWD_GROUPS=4
#                 (8 problems; 320 tokens is the largest count the twelve-wave shape takes)
#   stacks        two layers through encoder_stack_train, p 0.1: (128, 4) at 33 and 97 tokens (the chained in-projection on a ragged
#                 last tile), (256, 8) at 33 (the link's GEMM fallback)
EDGE_TOKENS = [31, 32, 33, 64, 65, 96, 97, 160, 193, 320, 321]
EDGE_TOKENS_4 = [32, 33, 96, 97]
EDGE_VARIANT_TOKENS = [32, 33, 96, 97, 320]
EDGE_LDS_TOKENS = [2368, 2369]
EDGE_STACKS = [(128, 4, 33), (128, 4, 97), (256, 8, 33)]     # (d, heads, tokens): two layers, 2 planes, gelu, p = 0.1


def edge_grid(tokens):
    return (3 * tokens, 2)


def edge_case(d, heads, tokens, p):
    """A case in LAYER_CASES' form; the input seed is fixed by the shape."""
    return (d, heads, edge_grid(tokens), 2, "gelu", p, 7000 + 8 * d + heads + 100003 * tokens)


EDGE_CASES = (
    [edge_case(128, 4, n, p) for n in EDGE_TOKENS for p in (0.0, 0.1)]
    + [edge_case(d, h, n, p) for d, h in ((128, 2), (256, 8)) for n in EDGE_TOKENS for p in (0.0, 0.1) if p or n in (32, 33, 97)]
    + [edge_case(d, h, n, 0.1) for d, h in ((384, 4), (512, 4), (128, 8), (96, 3), (200, 8)) for n in EDGE_TOKENS_4]
    + [edge_case(32, 1, n, p) for n in EDGE_LDS_TOKENS for p in (0.0, 0.1)])
EDGE_VARIANT_CASES = [edge_case(128, 4, n, 0.1) for n in EDGE_VARIANT_TOKENS]

# The factor over the float32 composite's own error: the recorded worst e_hip / e_torch32 is 2.38 over LAYER_CASES
# (profiles/dropout_vs_fp64.json) and 3.52 over the edge matrix (profiles/token_edges_vs_fp64.json: dx, d 128, 4 heads, 160 tokens).
# The phantom-key defect still has to move its tensor by more than 10 x the bound at every token count
# (test_train_token_edges.py), which is what limits the factor and LSE_SPACINGS.
EDGE_FACTOR = 4.0
LSE_SPACINGS = 4


def edge_bound(e_torch32):
    """EDGE_FACTOR x the float32 composite's own error + 1e-6, relative to the tensor's max: the HIP result never enters it."""
    return EDGE_FACTOR * e_torch32 + 1e-6


def lse_bound(e_torch32_abs, lse_max):
    """Absolute: EDGE_FACTOR x the float32 LSE's own error + LSE_SPACINGS float32 spacings at max |lse|."""
    return EDGE_FACTOR * e_torch32_abs + LSE_SPACINGS * float(np.spacing(np.float32(lse_max)))


def case_masks(case, seed=DROP_SEED):
    """(masks, keep scale) of one case: all ones and 1 at p = 0."""
    d, heads, ofdm, planes, _, p, _ = case
    tokens = tokens_of(ofdm)
    if p > 0:
        return layer_masks(seed, p, planes, heads, tokens, d), float(keep_scale(p))
    return ones_masks(planes, heads, tokens, d), 1.0


def tape_figures(qkv, m0, ks, planes, heads, yardstick_device):
    """Check (a)'s reference, yardstick and bounds from one float32 qkv block: (lse64, o64, lse bound, attn bound, e32 of each)."""
    lse64, o64 = attention_tape(qkv, m0, ks, planes, heads, torch.float64, "cpu")
    lse32, o32 = attention_tape(qkv, m0, ks, planes, heads, torch.float32, yardstick_device)
    e_lse, e_o = float((lse32 - lse64).abs().max()), rel_err(o32, o64)
    return lse64, o64, lse_bound(e_lse, float(lse64.abs().max())), edge_bound(e_o), e_lse, e_o


def layer_limits(out64, g64, out32, g32, tol_grad=TOL_GRAD):
    """Check (b)'s bounds per tensor: (e_torch32, project bound, edge bound), output first."""
    tols = [TOL_FWD] + [tol_grad] * len(g64)
    e32 = [rel_err(out32, out64)] + [rel_err(t, r) for t, r in zip(g32, g64)]
    return [(e, bound(tol, e), edge_bound(e)) for e, tol in zip(e32, tols)]


def case_id(c):
    return f"d{c[0]}h{c[1]}_{tokens_of(c[2])}tok_p{c[5]}"
