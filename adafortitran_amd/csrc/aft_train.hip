// aft_train.hip -- C-ABI of the encoder layer's training forward / backward.
//
// One nn.TransformerEncoderLayer (post-LN, reference src/models/blocks/encoders.py:44-55) in
// train() mode as two calls: the forward keeps what the backward needs in a caller-owned "tape",
// the backward turns d(loss)/d(x_out) into d(loss)/d(x_in) and the gradients of the layer's twelve
// parameter tensors.  Everything row-major fp32, rows = 2B * tokens.  The caller (PyTorch autograd,
// adafortitran_amd/training.py) owns x_in, the tape and the gradient tensors.
#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdlib>

#include "aft_internal.h"

namespace aft {

namespace {

struct Tape : Layout { size_t qkv, attn, lse, s1, st1, x1, a, hd, s2, st2; };   // offsets in floats
// sl_*: slice storage per producer of the backward (every gradient kernel of the layer keeps its partial slices until the single
// reduction launch at the end): LayerNorm-2 / linear2's weight / activation / linear1's weight / LayerNorm-1 / out_proj's weight /
// in_proj's weight / in_proj's bias
struct Scratch : Layout {
    size_t g1, g2, g2b, gff, dqkv, dsum, sl_ln2, sl_w2, sl_act, sl_w1, sl_ln1, sl_wo, sl_wq, sl_bq, packed_t, lnp, attn_pad;
};

Tape plan_tape(const aft_config &c, int batch) {
    const size_t rows = (size_t)2 * batch * tokens_of(c), d = c.model_dim, ff = 2 * d;
    Tape t{};
    t.qkv = t.take(rows * 3 * d);
    t.attn = t.take(rows * d);
    t.lse = t.take(rows * c.num_head);
    t.s1 = t.take(rows * d);
    t.st1 = t.take(rows * 2);
    t.x1 = t.take(rows * d);
    t.a = t.take(rows * ff);
    t.hd = t.take(rows * ff);   // drop(act(a)): kept so the backward does not recompute it (24 us per layer)
    t.s2 = t.take(rows * d);
    t.st2 = t.take(rows * 2);
    return t;
}

Scratch plan_scratch(const aft_config &c, int batch) {
    const size_t rows = (size_t)2 * batch * tokens_of(c), d = c.model_dim, ff = 2 * d;
    const int r = (int)rows;
    Scratch s{};
    s.g1 = s.take(rows * d);
    s.g2 = s.take(rows * d);
    s.g2b = s.take(rows * d);   // d(out_proj output): g2 stays alive for linear2's weight gradient (batched at the end)
    s.gff = s.take(rows * ff);
    s.dqkv = s.take(rows * 3 * d);
    s.dsum = s.take(rows * c.num_head);
    s.sl_ln2 = s.take((size_t)ln_bwd_blocks(r) * 3 * d);
    s.sl_w2 = s.take(gemm_tn_slice_floats(d, ff, r));
    s.sl_act = s.take((size_t)ln_bwd_blocks(r) * ff);
    s.sl_w1 = s.take(gemm_tn_slice_floats(ff, d, r));
    s.sl_ln1 = s.take((size_t)ln_bwd_blocks(r) * 3 * d);
    s.sl_wo = s.take(gemm_tn_slice_floats(d, d, r));
    s.sl_wq = s.take(gemm_tn_slice_floats(3 * d, d, r));
    s.sl_bq = s.take((size_t)colsum_slices(r) * 3 * d);
    // fused row-local backward (k_chain_bwd.hip): transposed fragment-packed weights, per-tile LayerNorm parameter sums
    s.packed_t = s.take(std::max(chain_bwd_packed_floats((int)d), packed_layer_floats((int)d)));   // also the forward chain's fp32 image
    s.lnp = s.take(chain_bwd_lnp_floats(r, (int)d));
    s.attn_pad = s.take(attn_train_pad_floats(c, rows));    // head dim 16: padded-head images of qkv, o, d_o, dqkv
    return s;
}

// dense layer's backward: the weight gradient's split slices, the bias gradient's column-sum slices
struct DenseScratch : Layout { size_t wgrad, colsum; };
DenseScratch plan_dense_scratch(int rows, int in_f, int out_f) {
    const int tiles = ((in_f + 127) / 128) * ((out_f + 127) / 128);
    DenseScratch s{};
    s.wgrad = s.take((size_t)gemm_split_slices(rows, tiles) * in_f * out_f);
    s.colsum = s.take((size_t)colsum_slices(rows) * out_f);
    return s;
}

// The training conv kernels address the saved activations and masks ([planes][32][T][S] for conv2) through buffer resources with
// 32-bit byte offsets (conv_device.h): a launch takes at most this many planes, a call of more runs as consecutive launches
// (0: not even one plane fits -- refused)
int conv_train_chunk(int S, int T) {
    const size_t per = (size_t)32 * S * T * sizeof(float);
    return (int)std::min<size_t>((size_t)INT_MAX, (size_t)0x7fffffff / per);
}
// ConvEnhancer backward: the masked stage outputs g3 [8] | g2 [32] | g1 [8 channels] of one chunk of planes, back to back inside one
// region sized for all planes' 48 channels, then the weight-gradient slices, the transposed weights and their 16x16x4 operand
// fragments (default grid).  The forward's scratch is the fragment image alone.
struct ConvScratch : Layout { size_t g3, g2, g1, slices, flip, frag; };
ConvScratch plan_conv_scratch(int planes, int S, int T) {
    const size_t st1 = (size_t)S * T, chunk8 = (size_t)std::min(conv_train_chunk(S, T), planes) * 8 * st1;
    ConvScratch s{};
    s.g3 = s.take((size_t)planes * 48 * st1);
    s.g2 = s.g3 + chunk8;
    s.g1 = s.g2 + 4 * chunk8;
    s.slices = s.take(conv_wgrad_slice_floats(planes, S, T));
    s.flip = s.take(kConvFlipFloats);
    s.frag = s.take(kConvFragFloats);
    return s;
}

uint32_t site_seed(uint64_t seed, uint32_t site) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (site + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)(z ^ (z >> 31));
}

int check_train(const aft_config *cfg, int batch, float dropout_p) {
    int rc = check_config(cfg);
    if (rc != AFT_OK) return rc;
    if (batch <= 0 || !(dropout_p >= 0.f && dropout_p < 1.f)) {
        set_error("bad batch %d or dropout %g", batch, (double)dropout_p);
        return AFT_ERR_ARG;
    }
    // head dim 32 is the kernels' own shape, 64 runs as two 32-feature blocks under one softmax (forward + the two-pass backward
    // instantiated for two blocks), every other multiple of 8 as zero-padded 32- or 64-feature heads (k_attn_train.hip); check_config
    // above has already refused what the inference engine does not take (head dims off the multiples of 8, 56, > 64)
    if ((size_t)2 * batch * tokens_of(*cfg) * 3 * cfg->model_dim >= ((size_t)1 << 32)) {
        set_error("batch %d: dropout counters are 32-bit", batch);
        return AFT_ERR_ARG;
    }
    return AFT_OK;
}

}  // namespace

}  // namespace aft

using namespace aft;

extern "C" {

size_t aft_encoder_tape_bytes(const aft_config *cfg, int batch) {
    if (check_config(cfg) != AFT_OK || batch <= 0) return 0;
    return plan_tape(*cfg, batch).total * sizeof(float);
}

size_t aft_encoder_train_scratch_bytes(const aft_config *cfg, int batch) {
    if (check_config(cfg) != AFT_OK || batch <= 0) return 0;
    return plan_scratch(*cfg, batch).total * sizeof(float);
}

int aft_encoder_layer_fwd_train_chained_f32(const aft_config *cfg, const aft_layer_weights *w, const float *x_in, float *x_out,
                                            void *tape, size_t tape_bytes, void *scratch, size_t scratch_bytes, int batch,
                                            float dropout_p, uint64_t seed, int qkv_ready, const aft_layer_weights *next_w,
                                            void *next_tape, size_t next_tape_bytes, int *next_qkv_written, void *stream) {
    if (next_qkv_written) *next_qkv_written = 0;
    int rc = check_train(cfg, batch, dropout_p);
    if (rc != AFT_OK) return rc;
    if (!w || !x_in || !x_out || !tape || !scratch) { set_error("NULL pointer argument"); return AFT_ERR_ARG; }
    const Tape t = plan_tape(*cfg, batch);
    const Scratch s = plan_scratch(*cfg, batch);
    if (tape_bytes < t.total * sizeof(float) || scratch_bytes < s.total * sizeof(float)) {
        set_error("tape or scratch too small");
        return AFT_ERR_ARG;
    }
    if (next_w && next_tape && next_tape_bytes < t.total * sizeof(float)) {   // this call writes rows x 3d floats into next_tape's qkv block
        set_error("next_tape too small: %zu < %zu bytes (the linked layers share cfg and batch)", next_tape_bytes, t.total * sizeof(float));
        return AFT_ERR_ARG;
    }
    AFT_HOST_ASSERT(check_layout(t, tape_bytes) && check_layout(s, scratch_bytes), "tape or scratch region outside its buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *tp = static_cast<float *>(tape), *sc = static_cast<float *>(scratch);
    const int tokens = tokens_of(*cfg), planes = 2 * batch, rows = planes * tokens, d = cfg->model_dim, ff = 2 * d;
    float *o = sc + s.g1;   // projection outputs before the residual joins

    if (!qkv_ready)   // (else the previous layer's row-local kernel already left this layer's in-projection in the tape)
        STEP("qkv", launch_gemm(0, x_in, w->in_proj_w, tp + t.qkv, w->in_proj_b, rows, 3 * d, d, d, d, 3 * d, false, st));
    STEP("attention", launch_attn_train_fwd(*cfg, tp + t.qkv, tp + t.attn, tp + t.lse, planes, tokens, dropout_p,
                                            site_seed(seed, 0), st, sc + s.attn_pad));
    const uint32_t drop_th = dropout_p > 0.f ? (uint32_t)((double)dropout_p * 4294967296.0) : 0u;
    const float drop_ks = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
    // the NEXT layer's in-projection as the tail of this layer's row-local kernel (same tape layout: the layers share cfg and batch)
    const bool chain_next = next_w && next_w->in_proj_w && next_w->in_proj_b && next_tape && next_qkv_written;
    if (chain_fwd_train_ok(*cfg, rows) && !switch_on(SW_TRAIN_UNFUSED_FWD)) {
        // everything row-local behind the attention in ONE launch, the tape written from its epilogues (k_chain_bwd.hip);
        // the packed weight image lives in the scratch's packed_t region (8 d^2 floats needed, see plan_scratch)
        STEP("row-local forward chain", launch_chain_fwd_train(*cfg, *w, tp + t.attn, x_in, sc + s.packed_t, tp + t.s1, tp + t.st1, tp + t.x1,
                                                              tp + t.a, tp + t.hd, tp + t.s2, tp + t.st2, x_out, rows, site_seed(seed, 1),
                                                              site_seed(seed, 2), site_seed(seed, 3), drop_th, drop_ks, st,
                                                              chain_next ? next_w->in_proj_w : nullptr, chain_next ? next_w->in_proj_b : nullptr,
                                                              chain_next ? static_cast<float *>(next_tape) + t.qkv : nullptr));
        if (chain_next && next_qkv_written) *next_qkv_written = 1;
        return AFT_OK;
    }
    // projection + residual + dropout + LayerNorm: one launch when the fused epilogue covers the shape (d = 128)
    if (gemm_add_ln_ok(rows, d, d, d, d)) {
        STEP("out_proj + norm1", launch_gemm_add_ln(tp + t.attn, w->out_proj_w, w->out_proj_b, x_in, w->norm1_w, w->norm1_b, tp + t.s1,
                                                    tp + t.st1, tp + t.x1, rows, d, d, d, d, 1e-5f, drop_ks, drop_th, site_seed(seed, 1), st));
    } else {
        STEP("out_proj", launch_gemm(0, tp + t.attn, w->out_proj_w, o, w->out_proj_b, rows, d, d, d, d, d, false, st));
        STEP("norm1", launch_add_ln_fwd(x_in, o, w->norm1_w, w->norm1_b, tp + t.s1, tp + t.st1, tp + t.x1, rows, d, 1e-5f,
                                        dropout_p, site_seed(seed, 1), st));
    }
    if (gemm_act_ok(rows, ff, d, d, d, ff)) {   // linear1 + activation + dropout: one launch
        STEP("linear1 + activation", launch_gemm_act(tp + t.x1, w->lin1_w, w->lin1_b, tp + t.a, tp + t.hd, rows, ff, d, d, d, ff,
                                                     cfg->activation, drop_ks, drop_th, site_seed(seed, 2), st));
    } else {
        STEP("linear1", launch_gemm(0, tp + t.x1, w->lin1_w, tp + t.a, w->lin1_b, rows, ff, d, d, d, ff, false, st));
        STEP("activation", launch_act_fwd(cfg->activation, tp + t.a, tp + t.hd, rows, ff, dropout_p, site_seed(seed, 2), st));
    }
    if (gemm_add_ln_ok(rows, d, ff, ff, ff)) {
        STEP("linear2 + norm2", launch_gemm_add_ln(tp + t.hd, w->lin2_w, w->lin2_b, tp + t.x1, w->norm2_w, w->norm2_b, tp + t.s2, tp + t.st2,
                                                   x_out, rows, d, ff, ff, ff, 1e-5f, drop_ks, drop_th, site_seed(seed, 3), st));
    } else {
        STEP("linear2", launch_gemm(0, tp + t.hd, w->lin2_w, o, w->lin2_b, rows, d, ff, ff, ff, d, false, st));
        STEP("norm2", launch_add_ln_fwd(tp + t.x1, o, w->norm2_w, w->norm2_b, tp + t.s2, tp + t.st2, x_out, rows, d, 1e-5f,
                                        dropout_p, site_seed(seed, 3), st));
    }
    return AFT_OK;
}

int aft_encoder_layer_fwd_train_f32(const aft_config *cfg, const aft_layer_weights *w, const float *x_in, float *x_out,
                                    void *tape, size_t tape_bytes, void *scratch, size_t scratch_bytes, int batch,
                                    float dropout_p, uint64_t seed, void *stream) {
    return aft_encoder_layer_fwd_train_chained_f32(cfg, w, x_in, x_out, tape, tape_bytes, scratch, scratch_bytes, batch, dropout_p, seed, 0,
                                                   nullptr, nullptr, 0, nullptr, stream);
}

int aft_encoder_layer_bwd_f32(const aft_config *cfg, const aft_layer_weights *w, const float *x_in, const void *tape,
                              size_t tape_bytes, const float *dx_out, float *dx_in, const aft_layer_grads *g,
                              int accumulate, void *scratch, size_t scratch_bytes, int batch, float dropout_p,
                              uint64_t seed, void *stream) {
    int rc = check_train(cfg, batch, dropout_p);
    if (rc != AFT_OK) return rc;
    if (!w || !x_in || !tape || !dx_out || !dx_in || !g || !scratch) { set_error("NULL pointer argument"); return AFT_ERR_ARG; }
    const Tape t = plan_tape(*cfg, batch);
    const Scratch s = plan_scratch(*cfg, batch);
    if (tape_bytes < t.total * sizeof(float) || scratch_bytes < s.total * sizeof(float)) {
        set_error("tape or scratch too small");
        return AFT_ERR_ARG;
    }
    AFT_HOST_ASSERT(check_layout(t, tape_bytes) && check_layout(s, scratch_bytes), "tape or scratch region outside its buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float *tp = static_cast<const float *>(tape);
    float *sc = static_cast<float *>(scratch);
    const int tokens = tokens_of(*cfg), planes = 2 * batch, rows = planes * tokens, d = cfg->model_dim, ff = 2 * d;
    const bool acc = accumulate != 0;
    float *g1 = sc + s.g1, *g2 = sc + s.g2, *g2b = sc + s.g2b, *gff = sc + s.gff, *dqkv = sc + s.dqkv;
    ReduceBatchScope reductions;
    const uint32_t drop_th = dropout_p > 0.f ? (uint32_t)((double)dropout_p * 4294967296.0) : 0u;
    const float drop_ks = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
    // the layer's four weight gradients in ONE launch (dW2 = g2^T hd, dW1 = gff^T x1, dWo = g2b^T attn, dWqkv = dqkv^T x_in), then the
    // single reduction launch.  bias_out[j] != NULL: + that bias gradient as the column sums of operand A_j, slices in bias_sl[j]
    auto weight_grads = [&](float *const bias_out[4], float *const bias_sl[4]) -> int {
        const float *A[4] = {g2, gff, g2b, dqkv}, *B[4] = {tp + t.hd, tp + t.x1, tp + t.attn, x_in};
        float *C[4] = {g->lin2_w, g->lin1_w, g->out_proj_w, g->in_proj_w}, *S[4] = {sc + s.sl_w2, sc + s.sl_w1, sc + s.sl_wo, sc + s.sl_wq};
        const int M[4] = {d, ff, d, 3 * d}, N[4] = {ff, d, d, d}, lda[4] = {d, ff, d, 3 * d}, ldb[4] = {ff, d, d, d};
        STEP("weight gradients", launch_gemm_tn_batch(A, B, C, S, M, N, lda, ldb, 4, rows, acc, st, bias_out, bias_sl));
        STEP("gradient reductions", reductions.flush(st));
        return AFT_OK;
    };
    if (chain_bwd_ok(*cfg, rows) && !switch_on(SW_TRAIN_UNFUSED_BWD)) {
        // everything row-local in ONE launch: dx_out -> g2, gff, g2b (operands of the weight gradients), g1 = d(attention
        // output), dx_in = the residual branch of dL/dx, per-tile LayerNorm parameter sums
        float *lnp = sc + s.lnp;
        STEP("row-local backward chain", launch_chain_bwd(*cfg, *w, dx_out, tp + t.s2, tp + t.st2, tp + t.a, tp + t.s1, tp + t.st1,
                                                          sc + s.packed_t, g2, gff, g2b, g1, dx_in, lnp, rows, site_seed(seed, 1),
                                                          site_seed(seed, 2), site_seed(seed, 3), drop_th, drop_ks, st));
        const int ntl = chain_bwd_blocks(rows);
        STEP("norm2 parameter gradients", launch_reduce_slices3(lnp, g->norm2_w, g->norm2_b, nullptr, d, 2, ntl, (size_t)4 * d, acc, st));
        STEP("norm1 parameter gradients", launch_reduce_slices3(lnp + 2 * d, g->norm1_w, g->norm1_b, nullptr, d, 2, ntl, (size_t)4 * d, acc, st));
        STEP("attention bwd", launch_attn_train_bwd(*cfg, tp + t.qkv, tp + t.attn, g1, tp + t.lse, sc + s.dsum, dqkv, planes, tokens,
                                                    dropout_p, site_seed(seed, 0), st, sc + s.attn_pad));
        STEP("in_proj dgrad", launch_gemm(1, dqkv, w->in_proj_w, dx_in, nullptr, rows, d, 3 * d, 3 * d, d, d, true, st));
        // all four bias gradients ride on the weight-gradient launch; the LayerNorm slice regions are free on this path
        float *bias_out[4] = {g->lin2_b, g->lin1_b, g->out_proj_b, g->in_proj_b};
        float *bias_sl[4] = {sc + s.sl_ln2, sc + s.sl_act, sc + s.sl_ln1, sc + s.sl_bq};
        return weight_grads(bias_out, bias_sl);
    }
    // LN2: g1 = d(x1) through the residual, g2 = d(linear2 output) (dropout 3 applied)
    STEP("norm2 bwd", launch_ln_bwd(dx_out, tp + t.s2, tp + t.st2, w->norm2_w, g1, g2, g->norm2_w, g->norm2_b, g->lin2_b, sc + s.sl_ln2,
                                    rows, d, dropout_p, site_seed(seed, 3), acc, st));
    // linear2's data gradient with the activation backward as its epilogue (gff = d(linear1 output)); linear1's bias gradient
    // then rides on the batched weight-gradient launch below (column sums of gff)
    const bool fused_act = gemm_actbwd_ok(rows, ff, d, d, ff, ff);
    if (fused_act) {
        STEP("linear2 dgrad + activation bwd", launch_gemm_actbwd(g2, w->lin2_w, tp + t.a, gff, rows, ff, d, d, ff, ff, cfg->activation,
                                                                  drop_ks, drop_th, site_seed(seed, 2), st));
    } else {
        STEP("linear2 dgrad", launch_gemm(1, g2, w->lin2_w, gff, nullptr, rows, ff, d, d, ff, ff, false, st));
        STEP("activation bwd", launch_act_bwd(cfg->activation, tp + t.a, gff, g->lin1_b, sc + s.sl_act, rows, ff, dropout_p, site_seed(seed, 2),
                                              acc, st));
    }
    STEP("linear1 dgrad", launch_gemm(1, gff, w->lin1_w, g1, nullptr, rows, d, ff, ff, d, d, true, st));
    // LN1: dx_in = d(x_in) through the residual, g2b = d(out_proj output) (dropout 1 applied)
    STEP("norm1 bwd", launch_ln_bwd(g1, tp + t.s1, tp + t.st1, w->norm1_w, dx_in, g2b, g->norm1_w, g->norm1_b, g->out_proj_b, sc + s.sl_ln1,
                                    rows, d, dropout_p, site_seed(seed, 1), acc, st));
    STEP("out_proj dgrad", launch_gemm(1, g2b, w->out_proj_w, g1, nullptr, rows, d, d, d, d, d, false, st));
    STEP("attention bwd", launch_attn_train_bwd(*cfg, tp + t.qkv, tp + t.attn, g1, tp + t.lse, sc + s.dsum, dqkv, planes, tokens,
                                                dropout_p, site_seed(seed, 0), st, sc + s.attn_pad));
    STEP("in_proj dgrad", launch_gemm(1, dqkv, w->in_proj_w, dx_in, nullptr, rows, d, 3 * d, 3 * d, d, d, true, st));
    float *bias_out[4] = {nullptr, fused_act ? g->lin1_b : nullptr, nullptr, g->in_proj_b};   // db1 = gff^T 1, db_qkv = dqkv^T 1
    float *bias_sl[4] = {nullptr, sc + s.sl_act, nullptr, sc + s.sl_bq};
    return weight_grads(bias_out, bias_sl);
}

size_t aft_dense_bwd_scratch_bytes(int rows, int in_features, int out_features) {
    if (rows <= 0 || in_features <= 0 || out_features <= 0) return 0;
    return plan_dense_scratch(rows, in_features, out_features).total * sizeof(float);
}

int aft_dense_fwd_f32(const float *x, const float *weight, const float *bias, float *y, int rows, int in_features,
                      int out_features, void *stream) {
    if (!x || !weight || !y || rows <= 0 || in_features <= 0 || out_features <= 0) { set_error("bad dense argument"); return AFT_ERR_ARG; }
    STEP("dense forward", launch_gemm(0, x, weight, y, bias, rows, out_features, in_features, in_features, in_features,
                                      out_features, false, static_cast<hipStream_t>(stream)));
    return AFT_OK;
}

int aft_dense_bwd_f32(const float *x, const float *weight, const float *dy, float *dx, float *dweight, float *dbias,
                      int accumulate, void *scratch, size_t scratch_bytes, int rows, int in_features, int out_features,
                      void *stream) {
    if (!x || !weight || !dy || !dweight || !scratch || rows <= 0 || in_features <= 0 || out_features <= 0) {
        set_error("bad dense argument");
        return AFT_ERR_ARG;
    }
    const DenseScratch s = plan_dense_scratch(rows, in_features, out_features);
    if (scratch_bytes < s.total * sizeof(float)) { set_error("dense scratch too small"); return AFT_ERR_ARG; }
    AFT_HOST_ASSERT(check_layout(s, scratch_bytes), "dense scratch region outside its buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *sc = static_cast<float *>(scratch);
    ReduceBatchScope reductions;
    if (dx) STEP("dense dgrad", launch_gemm(1, dy, weight, dx, nullptr, rows, in_features, out_features, out_features, in_features,
                                            in_features, false, st));
    STEP("dense wgrad", launch_gemm_tn(dy, x, dweight, sc + s.wgrad, out_features, in_features, rows, out_features, in_features,
                                       accumulate != 0, st));
    if (dbias) STEP("dense bgrad", launch_colsum(dy, dbias, sc + s.colsum, rows, out_features, out_features, accumulate != 0, st));
    STEP("gradient reductions", reductions.flush(st));
    return AFT_OK;
}

size_t aft_embed_bwd_scratch_bytes(int planes, int num_scs, int num_symbols, int patch_scs, int patch_symbols, int model_dim,
                                   int with_tokens6) {
    return sizeof(float) * embed_bwd_slice_floats(planes, num_scs, num_symbols, patch_scs, patch_symbols, model_dim, with_tokens6 != 0);
}

int aft_embed_fwd_train_f32(const float *conv_enhanced, const float *tokens6, const float *w1, const float *b1, const float *pos,
                            float *x0, int planes, int num_scs, int num_symbols, int patch_scs, int patch_symbols, int model_dim,
                            void *stream) {
    if (!conv_enhanced || !w1 || !b1 || !pos || !x0 ||
        !ends_train_ok(planes, num_scs, num_symbols, patch_scs, patch_symbols, model_dim, tokens6 != nullptr)) {
        set_error("bad embed argument (patch of at most 32 elements, model_dim a multiple of 4 up to 512)");
        return AFT_ERR_ARG;
    }
    STEP("embed forward", launch_embed_train_fwd(conv_enhanced, tokens6, w1, b1, pos, x0, planes, num_scs, num_symbols, patch_scs,
                                                 patch_symbols, model_dim, static_cast<hipStream_t>(stream)));
    return AFT_OK;
}

int aft_embed_bwd_f32(const float *conv_enhanced, const float *tokens6, const float *w1, const float *dx0, float *d_conv_enhanced,
                      float *d_tokens6, float *dw1, float *db1, float *dpos, int accumulate, void *scratch, size_t scratch_bytes,
                      int planes, int num_scs, int num_symbols, int patch_scs, int patch_symbols, int model_dim, void *stream) {
    if (!conv_enhanced || !w1 || !dx0 || !d_conv_enhanced || !dw1 || !scratch || (tokens6 != nullptr) != (d_tokens6 != nullptr) ||
        !ends_train_ok(planes, num_scs, num_symbols, patch_scs, patch_symbols, model_dim, tokens6 != nullptr)) {
        set_error("bad embed argument (patch of at most 32 elements, model_dim a multiple of 4 up to 512)");
        return AFT_ERR_ARG;
    }
    if (scratch_bytes < aft_embed_bwd_scratch_bytes(planes, num_scs, num_symbols, patch_scs, patch_symbols, model_dim, tokens6 != nullptr)) {
        set_error("embed scratch too small");
        return AFT_ERR_ARG;
    }
    STEP("embed backward", launch_embed_train_bwd(conv_enhanced, tokens6, w1, dx0, d_conv_enhanced, d_tokens6, dw1, db1, dpos,
                                                  accumulate != 0, static_cast<float *>(scratch), planes, num_scs, num_symbols, patch_scs,
                                                  patch_symbols, model_dim, static_cast<hipStream_t>(stream)));
    return AFT_OK;
}

size_t aft_tail_bwd_scratch_bytes(int planes, int num_scs, int num_symbols, int patch_scs, int patch_symbols, int model_dim) {
    return sizeof(float) * tail_bwd_slice_floats(planes, num_scs, num_symbols, patch_scs, patch_symbols, model_dim);
}

int aft_tail_fwd_train_f32(const float *x, const float *w2, const float *b2, const float *resid, float *out, int planes, int num_scs,
                           int num_symbols, int patch_scs, int patch_symbols, int model_dim, void *stream) {
    if (!x || !w2 || !b2 || !resid || !out || !ends_train_ok(planes, num_scs, num_symbols, patch_scs, patch_symbols, model_dim, false)) {
        set_error("bad tail argument (patch of at most 32 elements, model_dim a multiple of 4 up to 512)");
        return AFT_ERR_ARG;
    }
    STEP("tail forward", launch_tail_train_fwd(x, w2, b2, resid, out, planes, num_scs, num_symbols, patch_scs, patch_symbols, model_dim,
                                               static_cast<hipStream_t>(stream)));
    return AFT_OK;
}

int aft_tail_bwd_f32(const float *x, const float *w2, const float *d_out, float *dx, float *dw2, float *db2, int accumulate,
                     void *scratch, size_t scratch_bytes, int planes, int num_scs, int num_symbols, int patch_scs, int patch_symbols,
                     int model_dim, void *stream) {
    if (!x || !w2 || !d_out || !dx || !dw2 || !scratch ||
        !ends_train_ok(planes, num_scs, num_symbols, patch_scs, patch_symbols, model_dim, false)) {
        set_error("bad tail argument (patch of at most 32 elements, model_dim a multiple of 4 up to 512)");
        return AFT_ERR_ARG;
    }
    if (scratch_bytes < aft_tail_bwd_scratch_bytes(planes, num_scs, num_symbols, patch_scs, patch_symbols, model_dim)) {
        set_error("tail scratch too small");
        return AFT_ERR_ARG;
    }
    STEP("tail backward", launch_tail_train_bwd(x, w2, d_out, dx, dw2, db2, accumulate != 0, static_cast<float *>(scratch), planes, num_scs,
                                                num_symbols, patch_scs, patch_symbols, model_dim, static_cast<hipStream_t>(stream)));
    return AFT_OK;
}

size_t aft_conv_enhancer_scratch_bytes(int planes, int num_scs, int num_symbols) {
    if (planes <= 0 || num_scs <= 0 || num_symbols <= 0 || !conv_plan_ok(num_scs, num_symbols, 0)) return 0;
    if (conv_train_chunk(num_scs, num_symbols) < 1) return 0;
    return plan_conv_scratch(planes, num_scs, num_symbols).total * sizeof(float);
}

size_t aft_conv_enhancer_fwd_scratch_bytes(int planes, int num_scs, int num_symbols) {
    if (planes <= 0 || num_scs <= 0 || num_symbols <= 0 || !conv_plan_ok(num_scs, num_symbols, 0)) return 0;
    if (conv_train_chunk(num_scs, num_symbols) < 1) return 0;
    Layout s{};
    s.take(kConvFragFloats);
    return s.total * sizeof(float);
}

int aft_conv_enhancer_fwd_train_f32(const float *const weights[4], const float *const biases[4], const float *x, float *y,
                                    float *c1, float *c2, float *c3, void *scratch, size_t scratch_bytes, int planes, int num_scs,
                                    int num_symbols, void *stream) {
    if (!weights || !biases || !x || !y || !c1 || !c2 || !c3 || planes <= 0 || num_scs <= 0 || num_symbols <= 0) {
        set_error("bad ConvEnhancer argument");
        return AFT_ERR_ARG;
    }
    if (scratch != nullptr && scratch_bytes < aft_conv_enhancer_fwd_scratch_bytes(planes, num_scs, num_symbols)) {
        set_error("ConvEnhancer forward scratch too small");
        return AFT_ERR_ARG;
    }
    const int chunk = conv_train_chunk(num_scs, num_symbols);
    if (chunk < 1) { set_error("ConvEnhancer: one %dx%d plane's saved activations exceed 2 GiB", num_scs, num_symbols); return AFT_ERR_SHAPE; }
    const size_t st1 = (size_t)num_scs * num_symbols;
    for (int p0 = 0; p0 < planes; p0 += chunk) {
        const int n = std::min(chunk, planes - p0);
        float *const save[3] = {c1 + p0 * 8 * st1, c2 + p0 * 32 * st1, c3 + p0 * 8 * st1};
        STEP("conv forward", launch_conv_train(weights, biases, x + p0 * st1, y + p0 * st1, save, nullptr, n, num_scs, num_symbols,
                                               static_cast<hipStream_t>(stream), static_cast<float *>(scratch)));
    }
    return AFT_OK;
}

int aft_conv_enhancer_bwd_f32(const float *const weights[4], const float *x, const float *c1, const float *c2,
                              const float *c3, const float *dy, float *dx, float *const dweights[4], float *const dbiases[4],
                              int accumulate, void *scratch, size_t scratch_bytes, int planes, int num_scs, int num_symbols,
                              void *stream) {
    if (!weights || !x || !c1 || !c2 || !c3 || !dy || !dx || !dweights || !dbiases || !scratch || planes <= 0) {
        set_error("bad ConvEnhancer argument");
        return AFT_ERR_ARG;
    }
    if (scratch_bytes < aft_conv_enhancer_scratch_bytes(planes, num_scs, num_symbols)) {
        set_error("ConvEnhancer scratch too small");
        return AFT_ERR_ARG;
    }
    const ConvScratch s = plan_conv_scratch(planes, num_scs, num_symbols);
    AFT_HOST_ASSERT(check_layout(s, scratch_bytes), "ConvEnhancer scratch region outside its buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int chunk = conv_train_chunk(num_scs, num_symbols);    // (> 0: the scratch size says so)
    const size_t st1 = (size_t)num_scs * num_symbols;
    float *sc = static_cast<float *>(scratch);
    float *flip = sc + s.flip, *frag = sc + s.frag, *slices = sc + s.slices, *g3 = sc + s.g3, *g2 = sc + s.g2, *g1 = sc + s.g1;
    // dgrad: the stack run on dy with conv4^T (1->8), conv3^T (8->32), conv2^T (32->8), conv1^T (8->1);
    // stage outputs masked by the saved activations = g3, g2, g1
    STEP("conv weight transposition", launch_conv_flip_weights(weights, flip, st));
    const float *const flipped_weights[4] = {flip, flip + 72, flip + 72 + 2304, flip + 72 + 4608};
    float *const save[3] = {g3, g2, g1};
    for (int p0 = 0; p0 < planes; p0 += chunk) {   // one pass unless the planes' saved activations pass 2 GiB (conv_train_chunk)
        const int n = std::min(chunk, planes - p0);
        const float *cc1 = c1 + p0 * 8 * st1, *cc2 = c2 + p0 * 32 * st1, *cc3 = c3 + p0 * 8 * st1;
        const float *const mask[3] = {cc3, cc2, cc1};
        STEP("conv dgrad", launch_conv_train(flipped_weights, nullptr, dy + p0 * st1, dx + p0 * st1, save, mask, n, num_scs, num_symbols,
                                             st, frag));
        STEP("conv wgrad", launch_conv_wgrad(x + p0 * st1, cc1, cc2, cc3, g1, g2, g3, dy + p0 * st1, dweights, dbiases, slices, n,
                                             num_scs, num_symbols, accumulate != 0 || p0 > 0, st));
    }
    return AFT_OK;
}

int aft_adapter_fwd_train_f32(const float *const conditions[3], const float *const weights[9], const float *const biases[9],
                              const int32_t hidden[3], int tokens, int frames, float *tokens6, float *hidden0, float *hidden1,
                              void *stream) {
    if (!conditions || !weights || !biases || !hidden || !tokens6 || !hidden0 || !hidden1 || frames <= 0 || tokens <= 0 ||
        hidden[2] != 2 * tokens) {
        set_error("bad ChannelAdapter argument");
        return AFT_ERR_ARG;
    }
    const int h[3] = {hidden[0], hidden[1], hidden[2]};
    STEP("adapter forward", launch_adapter_train_fwd(conditions, weights, biases, h, tokens, frames, tokens6, hidden0, hidden1,
                                                     static_cast<hipStream_t>(stream)));
    return AFT_OK;
}

int aft_adapter_bwd_f32(const float *const conditions[3], const float *const weights[9], const float *const biases[9],
                        const int32_t hidden[3], int tokens, int frames, const float *hidden0, const float *hidden1,
                        const float *dtokens6, float *dhidden0, float *dhidden1, float *const dweights[9],
                        float *const dbiases[9], int accumulate, void *stream) {
    if (!conditions || !weights || !biases || !hidden || !hidden0 || !hidden1 || !dtokens6 || !dhidden0 || !dhidden1 ||
        !dweights || !dbiases || frames <= 0 || tokens <= 0 || hidden[2] != 2 * tokens) {
        set_error("bad ChannelAdapter argument");
        return AFT_ERR_ARG;
    }
    if (hidden[1] > 64 || hidden[0] > 256) {
        set_error("ChannelAdapter hidden sizes [%d, %d] not covered by the fused backward (<= 256, <= 64)", hidden[0], hidden[1]);
        return AFT_ERR_SHAPE;
    }
    const int h[3] = {hidden[0], hidden[1], hidden[2]};
    STEP("adapter backward", launch_adapter_train_bwd(conditions, weights, biases, h, tokens, frames, hidden0, hidden1, dtokens6,
                                                      dhidden0, dhidden1, dweights, dbiases, accumulate != 0,
                                                      static_cast<hipStream_t>(stream)));
    return AFT_OK;
}

int aft_adam_step_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n, float lr, float beta1,
                      float beta2, float eps, float weight_decay, float grad_scale, int step, void *stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || step < 1) { set_error("bad Adam argument"); return AFT_ERR_ARG; }
    if (n == 0) return AFT_OK;
    STEP("adam", launch_adam(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, grad_scale, step,
                             static_cast<hipStream_t>(stream)));
    return AFT_OK;
}

// scratch of the squared norm: [blocks] float64 partials, then [blocks] uint32 non-finite flags
size_t aft_grad_sumsq_scratch_bytes(size_t n) {
    if (n == 0 || n > ((size_t)1 << 40)) return 0;
    return (grad_sumsq_blocks(n) * 12 + 15) / 16 * 16;
}

int aft_grad_sumsq_f32(const float *grad, size_t n, void *scratch, size_t scratch_bytes, double *sumsq, float *nonfinite,
                       void *stream) {
    if (!grad || !scratch || !sumsq || !nonfinite || n == 0 || n > ((size_t)1 << 40)) {
        set_error("bad squared-norm argument (NULL pointer, or n = %zu outside 1 .. 2^40)", n);
        return AFT_ERR_ARG;
    }
    if (((uintptr_t)grad & 15) || ((uintptr_t)scratch & 7) || scratch_bytes < aft_grad_sumsq_scratch_bytes(n)) {
        set_error("squared norm: grad must be 16-byte aligned and scratch 8-byte aligned with at least %zu bytes (got %zu)",
                  aft_grad_sumsq_scratch_bytes(n), scratch_bytes);
        return AFT_ERR_ARG;
    }
    double *partial = static_cast<double *>(scratch);
    STEP("grad sumsq", launch_grad_sumsq(grad, n, partial, reinterpret_cast<uint32_t *>(partial + grad_sumsq_blocks(n)), sumsq,
                                         nonfinite, static_cast<hipStream_t>(stream)));
    return AFT_OK;
}

int aft_adam_prepare_f32(aft_step_control *ctrl, const double *sumsq, const float *found_inf, const float *grad_scale,
                         double host_scale, double max_norm, float beta1, float beta2, void *stream) {
    if (!ctrl || (sumsq && !(max_norm >= 0.0))) {
        set_error("bad Adam preparation argument (NULL control block, or max_norm %g with a squared norm)", max_norm);
        return AFT_ERR_ARG;
    }
    STEP("adam prepare", launch_adam_prepare(ctrl, sumsq, found_inf, grad_scale, host_scale, max_norm, beta1, beta2,
                                             static_cast<hipStream_t>(stream)));
    return AFT_OK;
}

int aft_adam_step_ctrl_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n, float lr, float beta1,
                           float beta2, float eps, float weight_decay, const aft_step_control *ctrl, void *stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !ctrl || n == 0) {
        set_error("bad Adam argument (NULL pointer or n = 0)");
        return AFT_ERR_ARG;
    }
    STEP("adam", launch_adam_ctrl(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, ctrl,
                                  static_cast<hipStream_t>(stream)));
    return AFT_OK;
}

int aft_grad_clip_f32(float *grad, size_t n, const double *sumsq, double pre_scale, double max_norm, float *norm_out,
                      void *stream) {
    if (!grad || !sumsq || !norm_out || n == 0 || (n & 3) || ((uintptr_t)grad & 15) || !(max_norm >= 0.0)) {
        set_error("bad gradient clipping argument (NULL pointer, n = %zu not a positive multiple of 4, grad not 16-byte aligned, "
                  "or max_norm %g)", n, max_norm);
        return AFT_ERR_ARG;
    }
    STEP("grad clip", launch_grad_clip(grad, n, sumsq, pre_scale, max_norm, norm_out, static_cast<hipStream_t>(stream)));
    return AFT_OK;
}

}  // extern "C"
