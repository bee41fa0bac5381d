/*
 * adafortitran_amd.h -- C ABI of the MI355X (gfx950) AdaFortiTran forward path.
 *
 * The reference (BerkIGuler/AdaFortiTran) has no native layer: its boundary is the
 * Python nn.Module surface in src/models/ (SURVEY.md 8b).  This header is the ABI
 * that sits directly *below* that surface; each entry point names the reference
 * interface it replaces.  The Python-side binding a maintainer adds is a ctypes
 * stub (adafortitran_amd/_lib.py is that stub).
 *
 * Conventions
 *   - plain C symbols, no C++/torch types; all tensors are raw DEVICE pointers owned
 *     by the caller (PyTorch allocates inputs, outputs, weights and the workspace);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*, NULL =
 *     default stream), never synchronises, allocates nothing and keeps no state that
 *     describes a call (hipGraph-capturable, also as the very first call of a process);
 *     what the library caches is per DEVICE and idempotent -- the CU count and the
 *     "kernel may use N bytes of dynamic LDS" attribute, in tables indexed by the
 *     current device ordinal -- so one process may drive several GPUs through this ABI;
 *     the caller's loss.item() is the sync point, as in reference
 *     src/main/trainer.py:229,253,344;
 *   - complex64 tensors are passed as float* to interleaved (re,im) pairs, i.e. the
 *     memory of torch.view_as_real(x);
 *   - return 0 on success; AFT_ERR_ARG / AFT_ERR_SHAPE -> the Python side raises
 *     ValueError, AFT_ERR_HIP -> RuntimeError; aft_last_error() gives the text
 *     (thread-local).
 *   - inside the library a "plane" is one real-valued pass of the reference's
 *     _forward_real_valued (fortitran.py:176-177): plane n = 2*frame + (0:Re | 1:Im).
 */
#ifndef ADAFORTITRAN_AMD_H
#define ADAFORTITRAN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AFT_ABI_VERSION 10   /* bump whenever an entry point's meaning, a struct or a scratch size changes */

#define AFT_OK 0
#define AFT_ERR_ARG 1   /* NULL pointer, bad batch, workspace too small ...          */
#define AFT_ERR_SHAPE 2 /* configuration the kernels do not cover                    */
#define AFT_ERR_HIP 3   /* a HIP runtime call or kernel launch failed                */

/* aft_config.encoder_path.  LAUNCHES: embedding+QKV, then [attention, chain] per layer (13 launches at 6 layers).
 * AUTO: the library chooses between the launches and the fused layer sequence (aft_layer_fused_of, below).
 * PLANE: retired, runs the launches (it selected a one-launch plane-resident encoder kernel, measured 1.5 % slower than
 * the launches and removed; the value stays accepted for existing callers).  Identical output bits whichever is set. */
#define AFT_ENCODER_AUTO 0
#define AFT_ENCODER_LAUNCHES 1
#define AFT_ENCODER_PLANE 2

/* aft_config.precision.  F32: every product on exact-fp32 MFMAs (v_mfma_f32_32x32x2_f32) -- the default, the parity
 * contract (5e-5 |y|max, |dMSE|/MSE <= 1e-4) and the only mode the headline benchmark runs.  BF16X3 (opt-in, reported
 * separately, SURVEY.md 8d "bf16-MFMA tier"): the encoder's GEMMs (in-projection, out-projection, FFN) and attention products split
 * each fp32 operand into bf16 hi + lo and accumulate hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_bf16 in fp32 (~2^-16
 * relative per product; stated tolerance max|d| <= 1e-3 |y|max, |dMSE|/MSE <= 1e-2, observed ~1e-5 / ~1e-6: tests/
 * test_hip_parity.py).  The softmax, LayerNorm, GELU, the conv stacks and every accumulator stay fp32.  model_dim 128 or 256;
 * inference only. */
#define AFT_PRECISION_F32 0
#define AFT_PRECISION_BF16X3 1

#define AFT_ACT_RELU 0
#define AFT_ACT_GELU 1 /* exact erf form, as activation="gelu" in encoders.py:44-51 */

/* Shape of one estimator: system_config.yaml + model yaml
 * (reference src/config/schemas.py:20-45,113-146; fortitran.py:52-81). */
typedef struct aft_config {
    int32_t num_scs, num_symbols;     /* OFDM grid S x T (120 x 14)                  */
    int32_t pilot_scs, pilot_symbols; /* pilot grid (12 x 2)                         */
    int32_t patch_scs, patch_symbols; /* patch (3 x 2): tokens = (S/p0)*(T/p1)       */
    int32_t num_layers, model_dim, num_head; /* covered (aft_check_config says why not otherwise): any layer count, model_dim a multiple
                                       * of 8 up to 512, model_dim / num_head up to 128, patches of <= 32 elements.  Two engines behind one
                                       * call (aft_engine_of): the fragment-packed launch sequence -- model_dim a multiple of 32 up to 256,
                                       * head dim a multiple of 8 up to 64 except 56, patches of <= 16 elements -- and the row-major
                                       * general sequence for everything else (slower) */
    int32_t activation;               /* AFT_ACT_*                                   */
    int32_t adaptive;                 /* 1 = AdaFortiTran (adapter tokens), 0 = FortiTran */
    int32_t hidden[3];                /* channel_adaptivity_hidden_sizes (adaptive only) */
    int32_t encoder_path;             /* AFT_ENCODER_*: how aft_forward_f32 runs the encoder (same bits either way) */
    int32_t precision;                /* AFT_PRECISION_*: 0 = exact fp32 everywhere (the default and the parity contract) */
} aft_config;

/* One nn.TransformerEncoderLayer (post-LN), PyTorch layouts
 * (reference blocks/encoders.py:44-55). */
typedef struct aft_layer_weights {
    const float *in_proj_w, *in_proj_b;   /* [3d,d] = [Wq;Wk;Wv], [3d]              */
    const float *out_proj_w, *out_proj_b; /* [d,d], [d]                              */
    const float *lin1_w, *lin1_b;         /* [2d,d], [2d]                            */
    const float *lin2_w, *lin2_b;         /* [d,2d], [d]                             */
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b; /* [d] each                  */
} aft_layer_weights;

/* Every tensor of the reference state_dict, as device pointers to the tensors
 * PyTorch already holds (no repacking, no ownership transfer). */
typedef struct aft_weights {
    const float *up_w, *up_b;        /* pilot_upsampler [S*T, Ps*Pt], [S*T]  (fortitran.py:86) */
    const float *enh_w[4], *enh_b[4];/* initial_enhancer.conv_block.{0,2,4,6} (enhancers.py:12-20) */
    const float *ref_w[4], *ref_b[4];/* final_refiner.conv_block.{0,2,4,6}                   */
    const float *ada_w[3][3], *ada_b[3][3]; /* channel_adapter.{snr,ds,dop}_encoder.{0,2,4}
                                               (channel_adaptivity.py:35-39); NULL if !adaptive */
    const float *lin1_w, *lin1_b;    /* transformer_encoder.linear_1 [d, p(+6)], [d]          */
    const float *pos;                /* positional table rows [>=tokens, d] (learnable or sinusoid) */
    const float *lin2_w, *lin2_b;    /* transformer_encoder.linear_2 [p, d], [p]              */
    const aft_layer_weights *layers; /* HOST array of cfg->num_layers entries (any layer count: nn.TransformerEncoder stacks
                                        whatever num_layers says, encoders.py:52-55); read during the call only            */
} aft_weights;

int aft_version(void);
const char *aft_last_error(void);

/* AFT_OK when the gfx950 kernels cover `cfg`; else AFT_ERR_SHAPE / AFT_ERR_ARG with the reason in
 * aft_last_error().  The estimator calls it at construction (the reference validates its config in
 * __init__, fortitran.py:52-81), so an uncovered shape is refused before any training starts. */
int aft_check_config(const aft_config *cfg);

/* Which launch sequence aft_forward_f32 runs for `cfg` (a property of the configuration alone -- never of the batch, so a frame's
 * output bits do not depend on the batch it travels in): AFT_ENGINE_PACKED = the tuned fragment-packed kernels (chain + attention,
 * DESIGN.md 4.1 / 4.2), AFT_ENGINE_GENERAL = the row-major sequence that covers every shape the reference builds within the bounds
 * above (GEMM / attention / LayerNorm kernels of the training path, dropout off); < 0 = not covered (aft_check_config says why). */
#define AFT_ENGINE_PACKED 0
#define AFT_ENGINE_GENERAL 1
int aft_engine_of(const aft_config *cfg);

/* Measurement / A-B switches (no reference counterpart).  Every switch is declared once, with its purpose, in the table of
 * adafortitran_amd/csrc/switches.h.  The library reads the environment variables of those names ONCE, when it is loaded (other AFT_*
 * variables are ignored); afterwards a switch changes only through aft_set_switch (value NULL = unset) -- no getenv() on any call
 * path, so forwards on several host threads never race a setenv() elsewhere in the process.  A switch set to anything is on; its
 * value is read as atoi() reads it.  aft_set_switch returns AFT_ERR_ARG for a name the table does not declare (aft_last_error names
 * it).  aft_get_switch copies the current value into buf (at most n bytes including the terminator) and returns 1, returns 0 when
 * the switch is unset and -1 when the name is not a switch.  None of them changes results beyond summation order, and the product
 * never sets one. */
int aft_set_switch(const char *name, const char *value);
int aft_get_switch(const char *name, char *buf, size_t n);

/* Largest `batch` one aft_forward_f32 call accepts for `cfg` (0 on a bad config): the kernels use 32-bit byte offsets
 * into each workspace region, so no region (q / k / v^T: 2*batch*tokpad*model_dim floats) may reach 2 GiB.  The reference
 * accepts any batch (fortitran.py:145-182); the module surface above this ABI splits larger batches into chunks. */
int aft_max_batch(const aft_config *cfg);

/* Bytes of scratch aft_forward_f32 needs for `batch` frames (0 on a bad config). */
size_t aft_workspace_bytes(const aft_config *cfg, int batch);

/* The fused layer sequence (no reference counterpart): one launch per encoder layer on plane-aligned row tiles instead
 * of the [attention, chain] launches.  Same bits either way.  It needs two more blocks of scratch than aft_workspace_bytes plans
 * (x on plane-aligned tiles, a second V^T buffer), which the forward lays BEHIND the planned slices of all lanes: a caller opts in
 * by passing a workspace of aft_workspace_bytes_layer_fused bytes (= aft_workspace_bytes where the sequence is not instantiated);
 * with less, the launches run.  Every offset aft_workspace_lanes / aft_workspace_region report holds in both cases.
 * aft_layer_fused_of: which sequence a forward of `batch` frames in ONE lane runs given such a workspace: 1 = fused (fp32, model_dim
 * 128, head dimension 32, >= 32 tokens, encoder_path AUTO, and a batch at which plane-aligned tiles take no more rounds of the
 * persistent grid than global ones), 0 = the launches.  The switch AFT_LAYER_FUSED (0 = never, 1 = wherever the shape is covered)
 * overrides the batch rule.  -1 on a bad config or batch. */
size_t aft_workspace_bytes_layer_fused(const aft_config *cfg, int batch);
int aft_layer_fused_of(const aft_config *cfg, int batch);

/* Lanes (no reference counterpart).  A forward whose launches do not fill whole rounds of the kernels' persistent grids -- more than
 * one row tile per CU, fewer than ~15, and not as well aligned as the default model's 127 / 128 frames (DESIGN.md section 5 has the
 * rule and the measurements) -- is run as TWO complete forwards over contiguous shares of the batch: share 0 on the
 * caller's stream, share 1 on a library-owned side stream that is forked from the caller's stream by an event when the call starts
 * and joined back into it by an event before the call returns -- the hardware fills the idle tail of one share's launch with the
 * other share's next launch.  To the caller the call is still asynchronous on ONE stream (everything the call enqueues is ordered
 * after the stream's earlier work and before its later work; capturable in a hipGraph: the side stream joins the capture).  Frames
 * are independent, so the output bits are those of the unsplit forward.  The side stream and its two events are created on the
 * first such call per (device, caller stream) and kept for the 16 most recently used caller streams of the process (the least
 * recently used idle entry is destroyed when a seventeenth stream arrives).  Should the side stream be unavailable (creation failed,
 * or all 16 entries are in use by calls in flight on other host threads) the shares run one after the other on the caller's stream
 * in the SAME workspace layout -- slower, same bits, and aft_workspace_lanes stays true.  The switch AFT_LANES=1 (aft_set_switch)
 * turns the split off.
 * aft_workspace_lanes reports the split a forward of `batch` frames uses: lanes (1 .. AFT_MAX_LANES), and per lane its
 * frame count and the byte offset of its slice of `workspace` (a lane's slice is laid out as the workspace of a forward of that many
 * frames).  `frames` and `offset_bytes` are arrays of AFT_MAX_LANES entries. */
#define AFT_MAX_LANES 4
int aft_workspace_lanes(const aft_config *cfg, int batch, int *lanes, int *frames, size_t *offset_bytes);

/* Where aft_forward_f32 LEAVES its intermediates in `workspace` (no reference counterpart; known-answer tests use it to pin
 * the kernels the forward itself launches -- the per-stage entry points further down do not always run the same kernels):
 * byte offset and byte size of one region of a lane of `batch` frames, relative to that lane's slice of the workspace
 * (aft_workspace_lanes; a forward that is not split has one lane at offset 0).  Regions stay valid until the next call on that workspace.
 *   AFT_REGION_CONV_ENHANCED  f32 [2B,S,T]            output of S1+S2 (fortitran.py:203-209), kept for the S7 residual
 *   AFT_REGION_TOKENS6        f32 [B,tokens,6]        ChannelAdapter output (channel_adaptivity.py:59-63); adaptive configs
 *   AFT_REGION_ENC_OUT        f32 [2B*tokens,stride]  linear_2's output (encoders.py:70), `stride` = the patch element count rounded
 *                                                     up to 8 / 16 / 24 / 32; columns [0, patch elements) are valid
 * Returns AFT_OK, or AFT_ERR_ARG / AFT_ERR_SHAPE (bad region, batch or config). */
#define AFT_REGION_CONV_ENHANCED 0
#define AFT_REGION_TOKENS6 1
#define AFT_REGION_ENC_OUT 2
int aft_workspace_region(const aft_config *cfg, int batch, int region, size_t *offset_bytes, size_t *size_bytes);

/* Replaces BaseFortiTranEstimator.forward (reference src/models/fortitran.py:145-182):
 * pilots complex64 [B,Ps,Pt] -> out complex64 [B,S,T].  snr/ds/dop are float32 [B]
 * raw (un-normalised) channel conditions, NULL for FortiTran (meta_data[1..3],
 * fortitran.py:166-170).
 * `pilots`, `snr`, `ds`, `dop` may be ANY device-addressable memory, pinned host memory (hipHostMalloc / torch's
 * pin_memory()) included: the conv head and the adapter read them directly, so the model-owned H2D transfer of
 * fortitran.py:167-173 needs no copy engine hop in front of the first launch -- the caller keeps the buffer unchanged until
 * the call's kernels have run (record an event behind the call).  `out`, `workspace` and the weights are device memory.
 * Launches: [adapter + weight re-lay] (one prologue launch), conv head, embedding + in-projection, L x (attention, row-local
 * chain), conv tail -- once, or once per lane when a short forward is split ("Lanes" above). */
int aft_forward_f32(const aft_config *cfg, const aft_weights *w, const float *pilots,
                    const float *snr, const float *ds, const float *dop, float *out,
                    void *workspace, size_t workspace_bytes, int batch, void *stream);

/* The same forward for a caller that knows when its parameters change (an nn.Module in eval mode does: reference
 * trainer.py:332 `model.eval()` ... the weights are constant across a whole evaluation sweep).  aft_forward_f32 re-lays
 * the encoder's GEMM weights into MFMA-fragment order on EVERY call (5 us, 3 MB: it is stateless and always reflects the
 * caller's current parameters); here the caller owns that image -- aft_packed_weights_bytes() of device memory, filled by
 * aft_pack_weights_f32 whenever in_proj / out_proj / linear1 / linear2 weights of any layer changed -- and every forward
 * reads it.  `w` is still needed (biases, LayerNorm vectors, conv / adapter / dense weights are read in place).
 * THE CALLER'S DUTY: the image must have been packed with the SAME cfg (model_dim, num_layers AND precision: the fp32 and
 * the split-precision layouts have the same size) from the CURRENT weights; the library cannot check either without a
 * device-to-host synchronisation, which this ABI never performs.  Since ABI 4 aft_forward_f32 packs in the same launch as
 * the channel adapter, so the stateless entry point costs no more than this one: prefer it unless the 3 MB of weight reads
 * per call matter. */
size_t aft_packed_weights_bytes(const aft_config *cfg);
int aft_pack_weights_f32(const aft_config *cfg, const aft_weights *w, void *packed, size_t packed_bytes, void *stream);
int aft_forward_prepacked_f32(const aft_config *cfg, const aft_weights *w, const void *packed, const float *pilots,
                              const float *snr, const float *ds, const float *dop, float *out, void *workspace,
                              size_t workspace_bytes, int batch, void *stream);

/* Replaces LinearEstimator.forward (reference src/models/linear.py:65-97), applied to
 * the Re and Im planes separately: out[b,:,c] = W x[b,:,c] + bias. */
int aft_linear_forward_f32(const float *weight, const float *bias, const float *pilots,
                           float *out, int batch, int in_features, int out_features,
                           void *stream);

/* Replaces the metric of reference src/utils.py:164-180 + trainer.py:338-347:
 * *sum_sq (device, float64) += sum |est-ref|^2 over n_complex complex elements.
 * MSE = sum_sq / n_complex; dB = 10 log10 (utils.py:233-245). */
int aft_mse_partial_f32(const float *est, const float *ref, double *sum_sq,
                        long long n_complex, void *stream);

/* ---- the data formats either side of the path ---- */

/* Replaces the boolean-mask pilot extraction of MatDataset._process_channel_data (reference
 * src/data/dataset.py:116-139): hzero_ls complex64 [B, grid_elems] is the LS estimate with zeros at
 * non-pilot positions; the non-zero entries (re != 0 or im != 0) of each frame are compacted in
 * row-major order into pilots complex64 [B, expected].  counts[b] (device int32) receives the number
 * of non-zero entries found, so the caller can raise the reference's ValueError when it differs from
 * `expected` (dataset.py:128-132); exactly `expected` values are written per frame (zeros behind the
 * entries found when there are fewer: the output needs no initialisation). */
int aft_pilot_gather_f32(const float *hzero_ls, float *pilots, int *counts, int batch, int grid_elems,
                         int expected, void *stream);

/* Replaces utils.mse (reference src/utils.py:248-261) as get_ls_mse_per_folder applies it per file
 * (:264-303): db[b] = 10 log10( mean_i |ls[b,i] - ideal[b,i]|^2 ), complex64 [B, grid_elems] inputs. */
int aft_ls_mse_db_f32(const float *ls, const float *ideal, float *db, int batch, int grid_elems, void *stream);

/* Replaces the per-sample collation of DataLoader(MatDataset(...), shuffle=True) (reference src/main/trainer.py:505-511) for a data
 * set that is resident: ideal_all complex64 [frames, grid_elems] and pilots_all complex64 [frames, pilot_elems] live in device memory
 * or in pinned (device-addressable) host memory and are read in place.  index int64 [batch], ideal_out complex64 [batch, grid_elems],
 * pilots_out complex64 [batch, pilot_elems] and flags int32 [batch] are device memory.  Output frame b of either array is a bit copy of
 * frame index[b]; repeated indices are legal.  Nothing outside the two arrays is read whatever index holds: for an entry outside
 * [0, frames) output frame b is zero-filled and flags[b] = 1, otherwise flags[b] = 0.  Every output element and every flag is written
 * (the outputs need no initialisation); no atomics; one launch moves both arrays, nothing is synchronised.
 * AFT_ERR_ARG (nothing launched): a NULL pointer, batch / frames / grid_elems / pilot_elems below 1, an array or the index not 8-byte
 * aligned.  16-byte accesses are used for an array whose grid_elems (pilot_elems) is even and whose two bases are 16-byte aligned. */
int aft_frame_gather_f32(const float *ideal_all, const float *pilots_all, const long long *index, float *ideal_out,
                         float *pilots_out, int *flags, int batch, long long frames, int grid_elems, int pilot_elems, void *stream);

/* ---- training data made on the device: the OFDM channel simulator (adafortitran_amd/chansim.py holds the definition) ----
 *
 * A frame is a pure function of (seed, g), g its global frame number: a doubly-selective multipath Rayleigh channel over the S x T
 * grid, its noisy LS estimate at the pilot positions, and the three conditions it was drawn with.
 *   word(stream, index) = splitmix64(kf ^ (stream << 32 | index)),   kf = splitmix64(splitmix64(seed) ^ g)
 *   conditions (stream 0; index 0 snr, 1 delay spread, 2 doppler):  value[((word >> 40) * n_values) >> 24]
 *   ray (p, m), index 16 p + m:  angle a = (m + (word(1) >> 44) 2^-20) / rays turns,  phase f = (word(2) >> 40) 2^-24 turns
 *   h_p(t) = tap_amp[p] sum_m exp(j 2 pi (doppler_hz symbol_period_s cos(2 pi a) t + f))
 *   H[s, t] = sum_p h_p(t) exp(-j 2 pi s subcarrier_spacing_hz tap_delay[p] delay_spread_ns 1e-9)
 *   pilots[i, j] = H[pilot_sc_index[i], pilot_symbol_index[j]] + noise_sigma sqrt(-ln u1) exp(j 2 pi u2),  index i pilot_symbols + j,
 *                  u1 = ((word(3) >> 41) + 0.5) 2^-23,  u2 = ((word(4) >> 41) + 0.5) 2^-23
 * Every phase is formed in turns and reduced to [0, 1) before its sine / cosine.  The two products of a spacing and a condition are
 * formed in double and rounded to float once, on the host (float(subcarrier_spacing_hz * delay_spread_ns[i] * 1e-9),
 * float(doppler_hz[i] * symbol_period_s)); everything per frame is float32.  The caller supplies what needs pow():
 * tap_amp[p] = sqrt(power_p / sum(power) / rays) (unit mean |H|^2) and noise_sigma[i] = 10^(-snr_db[i] / 20). */
#define AFT_CHANSIM_MAX_TAPS 32
#define AFT_CHANSIM_MAX_RAYS 16
#define AFT_CHANSIM_MAX_VALUES 16
#define AFT_CHANSIM_MAX_PILOT_SCS 64
#define AFT_CHANSIM_MAX_PILOT_SYMBOLS 16
typedef struct aft_chansim {
    int32_t num_scs, num_symbols;      /* OFDM grid S x T, any size (ideal is [batch, S, T])             */
    int32_t pilot_scs, pilot_symbols;  /* pilot grid, at most 64 x 16                                    */
    int32_t taps, rays;                /* at most 32 taps of at most 16 sinusoids each                   */
    int32_t n_snr, n_ds, n_dop;        /* values per condition, 1..16 each                               */
    int32_t reserved;
    double subcarrier_spacing_hz, symbol_period_s;
    float tap_delay[AFT_CHANSIM_MAX_TAPS];   /* in multiples of the RMS delay spread                     */
    float tap_amp[AFT_CHANSIM_MAX_TAPS];     /* linear, per sinusoid (see above)                         */
    float snr_db[AFT_CHANSIM_MAX_VALUES], noise_sigma[AFT_CHANSIM_MAX_VALUES];
    float delay_spread_ns[AFT_CHANSIM_MAX_VALUES], doppler_hz[AFT_CHANSIM_MAX_VALUES];
    int32_t pilot_sc_index[AFT_CHANSIM_MAX_PILOT_SCS], pilot_symbol_index[AFT_CHANSIM_MAX_PILOT_SYMBOLS];
} aft_chansim;

/* One launch, one workgroup per frame: output frame b is global frame g = base + ((start + b stride) mod modulo) -- a contiguous
 * run (stride 1, modulo large) or a rank's share of an epoch that wraps the way DistributedSampler pads.  ideal complex64
 * [batch, S, T], pilots complex64 [batch, pilot_scs, pilot_symbols] and meta float32 [batch, 3] = (snr_db, delay_spread_ns,
 * doppler_hz) are device memory.  `sim` is read during the call only and travels to the kernel by value: nothing is uploaded.
 * Every output element is written (no initialisation needed); no atomics; nothing is synchronised; a frame's bits do not depend on
 * batch, b or the other arguments.  16-byte stores when T is even and ideal is 16-byte aligned, 8-byte stores otherwise.
 * Nothing is launched on AFT_ERR_ARG (a NULL pointer; ideal / pilots not 8-byte or meta not 4-byte aligned; batch < 1; base or start
 * negative, stride or modulo below 1, or a frame number past 2^62) and AFT_ERR_SHAPE (a dimension below 1 or a table beyond its
 * bound, a pilot index outside the grid). */
int aft_channel_sim_f32(const aft_chansim *sim, unsigned long long seed, long long base, long long start, long long stride,
                        long long modulo, int batch, float *ideal, float *pilots, float *meta, void *stream);

/* Antenna correlation (chansim.py "antenna correlation: Kronecker frame groups"): G = rx * tx consecutive frames are the antennas of
 * one receiver, member a = r tx + s of group g / G.  `mix` is the lower-triangular complex G x G matrix L = chol(C_rx) (x) chol(C_tx),
 * host memory, PACKED by rows: row a holds L[a][0 .. a] as (re, im) pairs at float offset a (a + 1), G (G + 1) floats in all.  For
 * frame g with lead = G (g / G):
 *   the three conditions are picked from the LEADER's key kf(lead): a group shares snr, delay spread and doppler;
 *   z_j[p][t], j = 0 .. a, is h_p(t) above from the ray streams of kf(lead + j) at the group's doppler;
 *   h_a[p][t] = sum_{j <= a} L[a][j] z_j[p][t], in increasing j from +0, one term being two fused multiply-adds per component:
 *     re = fma(L.re, z.re, fma(-L.im, z.im, re)),  im = fma(L.re, z.im, fma(L.im, z.re, im));
 *   H and the pilots follow as above from h_a, the group's delay spread and noise_sigma, and frame g's OWN noise streams.
 * base, start, stride and modulo count GROUPS: output frame b is member b mod G of group base + ((start + (b / G) stride) mod modulo);
 * batch counts frames.  Everything else is aft_channel_sim_f32's: the outputs, the store forms, one workgroup per frame, one launch,
 * no atomics, nothing synchronised; `sim` and `mix` are read during the call only.  With rx = tx = 1 the frames are
 * aft_channel_sim_f32's scaled by mix[0] (one frame per group).
 * Nothing is launched on AFT_ERR_ARG (aft_channel_sim_f32's, where the bound on frame numbers is 2^62 / G for groups; a NULL or
 * 4-byte-misaligned mix; a non-finite entry of mix; batch not a multiple of G) and AFT_ERR_SHAPE (aft_channel_sim_f32's; rx or tx
 * below 1 or rx * tx above AFT_CHANSIM_MAX_GROUP). */
#define AFT_CHANSIM_MAX_GROUP 16   /* the link's 8 branches x 2 streams */
int aft_channel_sim_group_f32(const aft_chansim *sim, int rx, int tx, const float *mix, unsigned long long seed, long long base,
                              long long start, long long stride, long long modulo, int batch, float *ideal, float *pilots,
                              float *meta, void *stream);

/* Time continuity (chansim.py "time continuity: slot sequences"): K = slots consecutive groups are K consecutive SLOTS of one fading
 * process, L = slot_symbols symbols from one slot's start to the next (L >= T; L > T leaves a gap).  Every K G consecutive frames, G =
 * rx * tx, are one sequence, slot-major: for frame g, seq = g / (K G), lead = seq K G, slot k = (g - lead) / G, member a = g mod G.
 *   the three conditions are picked from the SEQUENCE leader's key kf(lead): a sequence shares snr, delay spread and doppler;
 *   z_j, j = 0 .. a, uses the ray streams of kf(lead + j), the same rays in every slot, evaluated at the absolute symbol k L + t: a ray
 *     (rate = doppler_hz symbol_period_s cos(2 pi a) turns per symbol, phase f) first gets the slot's start phase
 *     f_k = frac(fma(rate, float(k L), f)), frac(x) = x - floor(x), k L exact in float; the phase at symbol t of the slot is then
 *     fma(rate, t, f_k), reduced as above.  f_0 = f exactly;
 *   the mixing, H and the pilots follow as in aft_channel_sim_group_f32, with frame g's OWN noise streams.
 * base, start, stride and modulo count SEQUENCES: output frame b is member b mod G of slot (b / G) mod K of sequence
 * base + ((start + (b / (K G)) stride) mod modulo); batch counts frames.  mix is aft_channel_sim_group_f32's (two floats, 1 and 0, for
 * rx = tx = 1).  Everything else is aft_channel_sim_group_f32's: one workgroup per frame, one launch, no atomics; with slots = 1 the
 * outputs are that entry point's, bit for bit, and slot 0 of sequence q is its group q K.
 * Nothing is launched on AFT_ERR_ARG (aft_channel_sim_group_f32's, where the bound on frame numbers is 2^62 / (K G) for sequences; batch
 * not a multiple of K G) and AFT_ERR_SHAPE (aft_channel_sim_group_f32's; slots below 1, slot_symbols below T, or slots, slot_symbols or
 * slots * slot_symbols above AFT_CHANSIM_MAX_SLOTS). */
/* the symbols a sequence may span: k L is far inside float's exact integers, and the rounding of a start phase, 2^-24 (rate k L + 1)
 * turns, stays below 3e-5 turns at 0.1 turns per symbol */
#define AFT_CHANSIM_MAX_SLOTS 4096
int aft_channel_sim_seq_f32(const aft_chansim *sim, int rx, int tx, const float *mix, int slots, int slot_symbols,
                            unsigned long long seed, long long base, long long start, long long stride, long long modulo, int batch,
                            float *ideal, float *pilots, float *meta, void *stream);

/* ---- the LMMSE (Wiener) baseline estimator (adafortitran_amd/lmmse.py holds the definition) ----
 *
 * The best linear estimator of the simulator's channel from its pilots, for the second-order statistics the simulator is defined
 * with: E|H|^2 = 1, frequency correlation r_f(d) = sum_p pw_p exp(-j 2 pi d df d_p DS), time correlation r_t(k) = J0(2 pi f_D k T_sym).
 * The pilot covariance is a Kronecker product, R_pp = R_f (x) R_t, so the estimator runs in its eigenbasis and no inverse is formed:
 *   R_f = U_f diag(lf) U_f^H  (per delay spread, Ps x Ps Hermitian),   F' = r_f(s - sc_i) U_f   [S, Ps]
 *   R_t = U_t diag(lt) U_t^T  (per Doppler, Pt x Pt real symmetric),   T' = r_t(t - sym_j) U_t  [T, Pt]
 *   est = F' [ D o (U_f^H P U_t) ] T'^T,    D[k][l] = 1 / (lf[k] lt[l] + noise_var),    P the frame's [Ps, Pt] pilots.
 * The caller computes the tables (pow, J0 and the eigen-decompositions are the host's, in double) and passes ONE float32 image:
 *   per delay spread i (n_ds blocks of fblock = 2 Ps Ps + 2 Ps S + Ps + (Ps & 1) floats, block i at i fblock):
 *     U_f^H  complex [Ps(k)][Ps(i)]   (re, im pairs; entry (k, i) = conj(U_f[i][k]))
 *     F'     complex [Ps(k)][S]       (k-major: consecutive subcarriers of one eigen-direction are adjacent)
 *     lf     real    [Ps]             (eigenvalues, clamped at 0 from below; one float of padding when Ps is odd)
 *   then per Doppler i (n_dop blocks of tblock = Pt Pt + Pt T + Pt floats, block i at n_ds fblock + i tblock):
 *     U_t    real    [Pt(j)][Pt(l)]
 *     T'     real    [Pt(l)][T]       (l-major)
 *     lt     real    [Pt]
 * aft_lmmse_table_floats gives the image's length.  Which block a frame uses: per condition, the index of the table value nearest to
 * the frame's (|v - value[i]| in double, ties to the lower index, a NaN to index 0) -- a total function; fixed_* >= 0 pins a condition
 * to that index for every frame (the mismatched receiver) and its per-frame array is then not read. */
typedef struct aft_lmmse {
    int32_t num_scs, num_symbols;              /* OFDM grid S x T, any size (est is [batch, S, T])           */
    int32_t pilot_scs, pilot_symbols;          /* pilot grid Ps x Pt, at most 64 x 16 (the simulator's)      */
    int32_t n_snr, n_ds, n_dop;                /* values per condition, 1..16 each                           */
    int32_t fixed_snr, fixed_ds, fixed_dop;    /* an index below n_*, or -1: chosen per frame                */
    float snr_db[AFT_CHANSIM_MAX_VALUES], delay_spread_ns[AFT_CHANSIM_MAX_VALUES], doppler_hz[AFT_CHANSIM_MAX_VALUES];
    float noise_var[AFT_CHANSIM_MAX_VALUES];   /* 10^(-snr_db[i] / 10)                                       */
} aft_lmmse;

/* Floats in the table image of `plan` (0 on a plan aft_lmmse_f32 would refuse with AFT_ERR_SHAPE). */
size_t aft_lmmse_table_floats(const aft_lmmse *plan);

/* One launch, one workgroup per frame: est complex64 [batch, S, T] (device memory) from pilots complex64 [batch, Ps, Pt] and the
 * float32 [batch] conditions snr / ds / dop.  pilots and the three condition arrays may be any device-addressable memory, pinned host
 * memory included (as for aft_forward_f32); a condition pointer may be NULL only when its fixed_* is set.  `tables` is the image above
 * in device memory; `plan` is read during the call only and travels to the kernel by value.  Every output element is written (no
 * initialisation needed); no atomics; nothing is synchronised; a frame's bits do not depend on batch or on its position in it.
 * 16-byte stores when T is even and est is 16-byte aligned, 8-byte stores otherwise.
 * Nothing is launched on AFT_ERR_ARG (a NULL plan / tables / pilots / est, or a NULL condition whose fixed_* is -1; tables, pilots or
 * est not 8-byte or a condition array not 4-byte aligned; batch < 1) and AFT_ERR_SHAPE (a dimension below 1 or beyond its bound, a
 * pilot grid larger than the OFDM grid, a fixed_* outside -1 .. n_* - 1). */
int aft_lmmse_f32(const aft_lmmse *plan, const float *tables, const float *pilots, const float *snr, const float *ds,
                  const float *dop, float *est, int batch, void *stream);

/* The multi-slot form (lmmse.py "smoothing and prediction over slot sequences"): the batch is whole sequences of the simulator's,
 * `slots` = K slots of `group` = G frames each, slot-major (aft_channel_sim_seq_f32's order): frame (seq, k, a) is (seq K + k) G + a.
 * Target frame (seq, k, a) is estimated from the pilots of member a in the w = min(window, k - horizon + 1) slots that end at slot
 * k - horizon, oldest first, side by side along time: P is [Ps, w Pt], and with it
 *   R_t^(w) = r_t(q - q') = U_t^(w) diag(lt^(w)) U_t^(w)T over the window's w Pt pilot symbols q = (i - (w - 1) - horizon) L + sym_j
 *             (relative to the target slot's symbol 0; L the symbols from one slot's start to the next),  T'^(w) = r_t(t - q) U_t^(w),
 *   est = F' [ D o (U_f^H P U_t^(w)) ] T'^(w)T,    D[k][l] = 1 / (lf[k] lt^(w)[l] + noise_var).
 * With k < horizon there is nothing to look at: est is +0 in every component and nothing is read for that frame.  The design point is
 * the TARGET frame's (its own entries of snr / ds / dop).  L and horizon's effect on q live in the tables only.  The image: the n_ds
 * blocks of aft_lmmse_f32's image, then per Doppler i the `window` sub-blocks for w = 1 .. window, adjacent, sub-block w holding
 *     U_t^(w)  real  [w Pt(j)][w Pt(l)],    T'^(w)  real  [w Pt(l)][T],    lt^(w)  real  [w Pt]
 * (w Pt (w Pt + T + 1) floats); aft_lmmse_seq_table_floats gives the image's length.  With window = 1 and horizon = 0 image and
 * output are aft_lmmse_f32's, bit for bit: every product stage is the same chain of fused multiply-adds in increasing index from +0,
 * over w Pt terms where that has Pt.  A frame's bits depend on its window's pilots and its conditions only: not on batch, not on the
 * sequence's place in it, and on k only through w. */
#define AFT_LMMSE_MAX_WINDOW_PILOTS 32

/* Floats in the multi-slot image of `plan` for `window` (0 where aft_lmmse_seq_f32 would refuse plan or window with AFT_ERR_SHAPE). */
size_t aft_lmmse_seq_table_floats(const aft_lmmse *plan, int window);

/* One launch, one workgroup per target frame; everything else as aft_lmmse_f32 (the memory each pointer may name, the stores, no
 * atomics, nothing synchronised, every output element written).  40 KB of static LDS; 24 KB when window * pilot_symbols <= 16 (the same
 * body on narrower tiles: the bits do not depend on it).
 * Nothing is launched on AFT_ERR_ARG (aft_lmmse_f32's; batch not a multiple of slots * group) and AFT_ERR_SHAPE (aft_lmmse_f32's;
 * group outside 1 .. AFT_CHANSIM_MAX_GROUP, slots outside 1 .. AFT_CHANSIM_MAX_SLOTS, window below 1 or above slots,
 * window * pilot_symbols above AFT_LMMSE_MAX_WINDOW_PILOTS, horizon outside 0 .. slots - 1). */
int aft_lmmse_seq_f32(const aft_lmmse *plan, int group, int slots, int window, int horizon, const float *tables, const float *pilots,
                      const float *snr, const float *ds, const float *dop, float *est, int batch, void *stream);

/* The full-grid smoother (lmmse.py "the full-grid smoother"): the same estimator with EVERY grid position an observation -- what a
 * receiver that re-estimates the channel from its own decisions runs on aft_link_observe_f32's z.  With r_f over all S subcarriers and
 * r_t over all T symbols,
 *   R_f = U_g diag(lg) U_g^H, of which the kf = min(S, taps) largest eigenpairs are kept, descending (R_f has rank at most the number
 *         of taps: nothing is lost),   F_g = U_g diag(lg)  [S, kf]
 *   R_t = U_tg diag(ltg) U_tg^T  [T, T],   T_g = U_tg diag(ltg)
 *   est = F_g [ D o (U_g^H Z U_tg) ] T_g^T,    D[k][l] = 1 / (lg[k] ltg[l] + noise_var),    Z the frame's [S, T] observations,
 * one noise variance for the whole grid: the caller puts beta 10^(-snr_db[i] / 10) into noise_var[i], beta its average over pilot and
 * data positions (formed in double, rounded once).  The image, float32:
 *   per delay spread i (n_ds blocks of 4 S kf + kf + (kf & 1) floats):
 *     U_g^H  complex [S(s)][kf(k)]    (s-major: entry (s, k) = conj(U_g[s][k]); the rows a workgroup streams are one contiguous run)
 *     F_g    complex [kf(k)][S]       (k-major, as F')
 *     lg     real    [kf]             (one float of padding when kf is odd)
 *   then per Doppler i (n_dop blocks of 2 T T + T floats):
 *     U_tg   real    [T(j)][T(l)],    T_g^T  real  [T(l)][T],    ltg  real  [T]
 * The design point is chosen as aft_lmmse_f32 chooses it; pilot_scs / pilot_symbols of `plan` are checked and otherwise unused.
 * One launch, one workgroup per frame: est complex64 [batch, S, T] from z complex64 [batch, S, T] (both device memory; z is read
 * once, in chunks of 32 rows) and the float32 [batch] conditions (any device-addressable memory; NULL where fixed_* pins).  The first
 * product is an S-deep chain of fused multiply-adds in increasing s from +0; from there on the arithmetic is aft_lmmse_f32's own code
 * with (Ps, Pt) = (kf, T).  Every output element is written; no atomics, no workspace; nothing is synchronised; a frame's bits do not
 * depend on batch or on its position in it; stores as aft_lmmse_f32's.  28 KB of static LDS, any S.
 * Nothing is launched on AFT_ERR_ARG (aft_lmmse_f32's, with z for pilots) and AFT_ERR_SHAPE (aft_lmmse_f32's; num_symbols above
 * AFT_LMMSE_MAX_WINDOW_PILOTS: all T symbols are filtered at once; kf outside 1 .. min(S, AFT_CHANSIM_MAX_TAPS)). */
int aft_lmmse_grid_f32(const aft_lmmse *plan, int kf, const float *tables, const float *z, const float *snr, const float *ds,
                       const float *dop, float *est, int batch, void *stream);

/* Choosing the design point from the pilots (lmmse.py "choosing the design point from the pilots"): a maximum-likelihood classification
 * of a window's pilots over the table's candidates c = (s, d, e) = (i_snr, i_ds, i_dop), in the estimator's own eigenbasis.  The batch is
 * whole sequences as for aft_lmmse_seq_f32, and target frame (seq, k, a) looks at exactly the window that call estimates it from:
 * w = min(window, k - horizon + 1) slots ending at slot k - horizon, P_a [Ps, w Pt].  A UNIT is the `group` frames of one slot when
 * pool = 1 (the simulator defines a group's conditions as shared; m = group members), one frame when pool = 0 (m = 1):
 *   Z_a = U_f[d]^H P_a U_t^(w)[e],   E_kl = sum over the unit's members of |Z_a,kl|^2,   V_kl = lf[d]_k lt^(w)[e]_l + noise_var[s],
 *   score(c) = -( m logdet[d][e][w][s] + sum_kl E_kl / V_kl ),
 * the Gaussian log-likelihood of the window under candidate c.  `tables` is aft_lmmse_seq_f32's image for `window` (with slots = 1,
 * window = 1 that is aft_lmmse_f32's image); `logdet` is float32 [n_ds][n_dop][window][n_snr] = sum_kl log V_kl, computed by the host
 * in double (the device takes no logarithm); aft_lmmse_classify_table_floats gives its length.  The highest score wins, ties go to the
 * lowest flat index (s n_ds + d) n_dop + e, a NaN score never wins, and with every score NaN the choice is index 0: a total function.
 * fixed_* >= 0 pins a condition: only candidates with that index compete, the others' scores are -inf; with all three pinned, or with
 * no slot to look at (k < horizon), nothing is read, the choice is the pinned index or 0 and the competing scores are +0.
 * Outputs, per FRAME (every member of a unit gets the unit's choice): idx int32 [batch, 3] and the table values snr / ds / dop
 * float32 [batch], the form aft_lmmse_seq_f32 takes them in; scores, when not NULL, float32 [units, n_snr n_ds n_dop] in flat index order,
 * units = batch / group when pool = 1, batch otherwise.  A unit's bits depend on its window's pilots only. */
size_t aft_lmmse_classify_table_floats(const aft_lmmse *plan, int window);

/* One launch, one workgroup per unit, no atomics, nothing synchronised, every output element written.  pilots may be any
 * device-addressable memory, pinned host memory included; tables, logdet and the outputs are device memory.  Static LDS: 40 KB,
 * 24 KB when window * pilot_symbols <= 16 (the same body: the bits do not depend on it).
 * Nothing is launched on AFT_ERR_ARG (a NULL plan / tables / logdet / pilots / idx / snr / ds / dop; tables or pilots not 8-byte, another
 * array not 4-byte aligned; batch < 1 or not a multiple of slots * group; pool not 0 or 1) and AFT_ERR_SHAPE (aft_lmmse_seq_f32's). */
int aft_lmmse_classify_f32(const aft_lmmse *plan, int group, int slots, int window, int horizon, int pool, const float *tables,
                           const float *logdet, const float *pilots, int32_t *idx, float *snr, float *ds, float *dop, float *scores,
                           int batch, void *stream);

/* ---- link-level bit errors (adafortitran_amd/linksim.py holds the definition) ----
 *
 * What a channel estimate is for: data symbols go through the TRUE channel H plus noise, a one-tap equaliser uses the ESTIMATE E, a hard
 * demapper decides, and the wrong bits are counted.  Per frame, with key kf (for simulated frames the simulator's,
 * splitmix64(splitmix64(seed) ^ g)), noise scale sigma and m = bits_per_symbol in {2, 4, 6, 8} (square QAM, L = 2^(m/2) levels per
 * axis, d = sqrt(3 / (2 (L^2 - 1))): unit mean symbol energy), over every grid element (s, t) that is not a pilot position
 * (pilot_sc_index x pilot_symbol_index), q = s T + t:
 *   word(stream, q) = splitmix64(kf ^ (stream << 32 | q)); streams 5 data bits, 6 data-noise radius, 7 data-noise angle (0..4 are the
 *                     simulator's)
 *   sent bits   w = word(5, q) >> (64 - m);  Gray codes gi = w >> (m/2), gq = w & (L - 1);  level k of a Gray code g: k ^ (k >> 1) = g
 *   sent symbol x = d ((2 ki - (L-1)) + j (2 kq - (L-1)))
 *   received    y = H[s,t] x + sigma sqrt(-ln u1) exp(j 2 pi u2),  u1 = ((word(6,q) >> 41) + 0.5) 2^-23,  u2 likewise from word(7,q)
 *               (the simulator's Box-Muller; the angle is formed in turns and reduced before its sine and cosine)
 *   decision    c = y conj(E[s,t]),  p = |E[s,t]|^2;  per axis (Re c for I, Im c for Q) the level is
 *               k^ = #{b in 1..L-1 : component >= beta_b p},  beta_b = 2 d (b - L/2);  its Gray code is k^ ^ (k^ >> 1)
 *   counts      bit errors = sum popcount(gi ^ g^i) + popcount(gq ^ g^q);  symbol errors = elements with any bit wrong
 * Zero-forcing with a hard decision and without a division: a total function, no special case for p = 0.  Everything per element is
 * float32, products are fused multiply-add chains; d is formed in double and rounded to float once. */
typedef struct aft_link {
    int32_t num_scs, num_symbols;              /* OFDM grid S x T, any size with S T <= 2^31                 */
    int32_t pilot_scs, pilot_symbols;          /* pilot grid Ps x Pt, at most 64 x 16 (the simulator's)      */
    int32_t bits_per_symbol, reserved;         /* 2, 4, 6 or 8                                               */
    int32_t pilot_sc_index[AFT_CHANSIM_MAX_PILOT_SCS], pilot_symbol_index[AFT_CHANSIM_MAX_PILOT_SYMBOLS];   /* strictly increasing */
} aft_link;

/* One launch, one workgroup per frame: counts int32 [batch][2] = (bit errors, symbol errors) of each frame (device memory) from ideal
 * and est complex64 [batch, S, T] (device memory), keys uint64 [batch] and sigma float32 [batch]; keys and sigma may be any
 * device-addressable memory, pinned host memory included.  `link` is read during the call only and travels to the kernel by value.
 * Every element of counts is written (no initialisation needed; a grid whose every element is a pilot gives (0, 0)); no atomics; nothing
 * is synchronised; a frame's counts depend neither on batch, nor on its position in it, nor on the run.  16-byte loads when T is even
 * and ideal and est are 16-byte aligned, 8-byte loads otherwise.
 * Nothing is launched on AFT_ERR_ARG (a NULL pointer; ideal / est / keys not 8-byte or sigma / counts not 4-byte aligned; batch < 1) and
 * AFT_ERR_SHAPE (a dimension below 1; S T above 2^31; a pilot grid beyond its bounds or larger than the grid; pilot indices not strictly
 * increasing or outside the grid; bits_per_symbol not one of 2, 4, 6, 8). */
int aft_link_errors_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                        const float *sigma, int32_t *counts, int batch, void *stream);

/* The soft half of the same link: max-log LLRs of the sent bits and the loss the achievable rate (the bit-interleaved coded-modulation
 * rate, the GMI of the LLRs) is read from.  With w, gi, gq, x, y, c, p as above, per data element and axis (comp = Re c for I, Im c for Q):
 *   levels   a_k = d (2k - (L-1)) with Gray label g_k = k ^ (k >> 1), k = 0 .. L-1
 *   metric   mu_k = a_k (a_k p - 2 comp)              |y - E x|^2 up to a constant: separable per axis, no division
 *   Delta_j  = min{mu_k : bit_j(g_k) = 1} - min{mu_k : bit_j(g_k) = 0},  bit_j(g) = (g >> (m/2 - 1 - j)) & 1  (MSB first)
 *   LLR      Lambda_j = scale Delta_j                 positive favours bit 0; I-axis bits 0 .. m/2-1, Q-axis bits m/2 .. m-1 (the order of w)
 *   loss[f] += log2(1 + exp(-(1 - 2 b_j) factors[f] Lambda_j))      b_j the sent bit, for each of the n_factors factors
 * A frame's rate at factor f is m - loss[f] / data elements (it may be negative: over-confident LLRs under a mismatched channel), and
 * the best of a factor grid is the GMI's supremum taken on that grid.  scale float32 [batch] is the LLR scale of each frame
 * (1 / (noise variance + the estimate's error variance)); factors float32 [n_factors], 1 <= n_factors <= 8.
 * One launch, one workgroup per frame: loss float32 [batch][n_factors] and, when llr is not NULL, llr float32 [batch, S, T, m], an
 * element's m values contiguous and zeros at the pilot positions (both device memory).  keys, sigma, scale and factors may be any
 * device-addressable memory, pinned host memory included.  Every element of loss and llr is written (no initialisation needed); no
 * atomics; nothing is synchronised; the K sums are float32, added in a fixed order, so a frame's outputs depend neither on batch, nor on
 * its position in it, nor on the run, nor on whether llr is written.  Loads as aft_link_errors_f32; 16-byte stores of llr when it is
 * 16-byte aligned and m is 4 or 8 or S T is even, 8-byte stores when it is 8-byte aligned, 4-byte stores otherwise.  exp and log1p are
 * the device library's, no fast-math; every metric is one fused multiply-add and one product.
 * Nothing is launched on AFT_ERR_ARG (what aft_link_errors_f32 refuses; a NULL scale / factors / loss; n_factors outside 1..8; scale /
 * factors / loss / llr not 4-byte aligned) and AFT_ERR_SHAPE (as aft_link_errors_f32). */
int aft_link_soft_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                      const float *sigma, const float *scale, const float *factors, int n_factors,
                      float *loss /* [batch][n_factors] */, float *llr /* [batch,S,T,m] or NULL */, int batch, void *stream);

/* ---- coded link: a convolutional code and a Viterbi decoder on those LLRs (adafortitran_amd/linksim.py holds the definition) ----
 *
 * The link is unchanged: a frame still sends the words w of stream 5.  The code rides on it through a scrambler both ends know.
 *   code        rate 1/2, constraint length 7, zero-terminated: for inputs u_0 .. u_{K-1} (u_t = 0 for t < 0 and K <= t < K + 6) and
 *               t = 0 .. K + 5:  A_t = u_t ^ u_{t-2} ^ u_{t-3} ^ u_{t-5} ^ u_{t-6} (133 octal),
 *               B_t = u_t ^ u_{t-1} ^ u_{t-2} ^ u_{t-3} ^ u_{t-6} (171 octal)
 *   puncturing  by t mod P, the 802.11 patterns: rate 1/2 (P = 1) keeps A B, 2/3 (P = 2) keeps A0 B0 A1, 3/4 (P = 3) keeps A0 B0 A1 B2;
 *               the kept bits step-major, A before B, are the n coded bits of a block
 *   blocks      N = m (S T - Ps Pt) bits per frame, B = N / n blocks (integer division), U = B n used bits.  Data-bit index j is bit
 *               k = j % m (the last axis of llr; bit (w >> (m-1-k)) & 1 of the sent word) of the (j / m)-th grid element that is no
 *               pilot, in row-major order.  Bits j >= U are filler the decoder ignores; LLRs at pilot positions are never read
 *   interleaver coded bit i of block b, p = b n + i, sits at j = p stride mod U, gcd(stride, U) = 1
 *   information u[b][t] = word(8, b K + t) >> 63: stream 8 of the frame's hash
 *   input       scrambler s_p = w_j ^ c_p (c_p the coded bit); lambda_p = (1 - 2 s_p) llr_j;
 *               z_p = clamp(rint(float32(lambda_p qgain)), -127, 127): one float32 product, to nearest with ties to even, NaN gives 0
 *   Viterbi     state sigma = sum_{i=1..6} u_{t-i} 2^(6-i), successor (sigma >> 1) | (u_t << 5); int32 metrics, M[0] = 0 and -2^30
 *               elsewhere; a branch gains the sum over its kept outputs of (1 - 2 out) z.  State n has predecessors
 *               r0 = (n & 31) << 1 and r1 = r0 | 1 with input n >> 5; the survivor is the larger sum and A TIE TAKES r0 (the decision
 *               bit is 1 only when r1 is strictly larger).  Traceback from state 0 after K + 6 steps: u^_t = n >> 5, previous state
 *               ((n & 31) << 1) | decision
 *   counts      (information-bit errors over the B K bits, blocks with any error) per frame
 * Everything after the quantiser is integer: a host evaluation of this definition agrees bit for bit. */
#define AFT_LINK_RATE_1_2 0
#define AFT_LINK_RATE_2_3 1
#define AFT_LINK_RATE_3_4 2
#define AFT_LINK_CODE_MAX_INFO_BITS 4090   /* 4096 trellis steps: a block's survivor words are 32 KiB, no metric can overflow */

/* One launch, one workgroup per frame, one wave per code block and one lane per trellis state: counts int32 [batch][2] = (bit errors,
 * block errors) of each frame and, when bits is not NULL, the decoded information bits uint8 [batch, B, K] (both device memory) from
 * llr float32 [batch, S, T, m] (device memory; what aft_link_soft_f32 writes) and keys uint64 [batch] (any device-addressable memory,
 * pinned host memory included).  `link` is read during the call only and travels to the kernel by value.  Every element of counts and
 * bits is written (no initialisation needed); no atomics; no workspace; nothing is synchronised; a frame's outputs depend neither on
 * batch, nor on its position in it, nor on the run, nor on whether bits is written.
 * Nothing is launched on AFT_ERR_ARG (a NULL link / llr / keys / counts; keys not 8-byte or llr / counts not 4-byte aligned; batch < 1;
 * qgain not finite and positive) and AFT_ERR_SHAPE (what aft_link_errors_f32 refuses; info_bits outside 1 ..
 * AFT_LINK_CODE_MAX_INFO_BITS; a rate that is none of the three; B = 0; B K above 2^31, where the hash's index and the int32 counts end; a stride outside
 * [1, U) -- U is at least 10 -- or not coprime to U; a stride_inverse outside [1, U) or with stride stride_inverse mod U != 1). */
int aft_link_decode_f32(const aft_link *link, const float *llr /* [batch,S,T,m] */, const unsigned long long *keys, int info_bits,
                        int rate /* AFT_LINK_RATE_* */, unsigned long long stride, unsigned long long stride_inverse, float qgain,
                        int32_t *counts /* [batch][2] */, unsigned char *bits /* [batch,B,K] or NULL */, int batch, void *stream);

/* ---- LDPC-coded link: a quasi-cyclic LDPC code and a layered min-sum decoder on those LLRs (adafortitran_amd/linksim.py holds the
 * definition in full) ----
 *
 * The code sits on the link exactly where the convolutional code does, with its own n and K.
 *   code        quasi-cyclic, lifting Z = 64.  Base matrix of mb = base_rows rows and nb = base_cols columns, 3 <= mb <= 16,
 *               mb < nb <= 32, kb = nb - mb; n = 64 nb coded and K = 64 kb information bits.  An entry is -1 (no block) or a shift s in
 *               0 .. 63: block (i, j) with shift s has, in its row r, its one at column (r + s) mod 64, so check 64 i + r contains
 *               variable 64 j + ((r + s) mod 64)
 *   parity part columns kb .. nb-1, fixed by structure, mid = mb / 2: column kb has shift 1 in rows 0 and mb-1 and shift 0 in row mid;
 *               column kb + 1 + i (i = 0 .. mb-2) has shift 0 in rows i and i + 1
 *   shifts      the information part, int32 [mb][kb]: every entry in -1 .. 63, every column with at least one entry, at most
 *               AFT_LINK_LDPC_MAX_EDGES entries in the whole base matrix, parity part included
 *   encoding    u_j the 64 bits of block column j, rot(x, s)[r] = x[(r + s) mod 64]: lam_i = XOR_j rot(u_j, S[i][j]) over the row's
 *               information blocks; p_0 = XOR_i lam_i; p_1 = lam_0 ^ rot(p_0, 1); p_{i+1} = lam_i ^ p_i ^ (p_0 if i == mid else 0)
 *               for i = 1 .. mb-2; the codeword is u | p_0 | .. | p_{mb-1}
 *   position    blocks, filler, interleaver, information bits (stream 8), scrambler and quantiser as for the coded link above
 *   decoder     layered offset min-sum, integer: posterior L_v = z_v, messages R = 0.  For iteration 1 .. max_iters and layer
 *               i = 0 .. mb-1 (its edges e the base columns with an entry, increasing, parity included), each of its 64 rows on its own:
 *               Q_e = L_v(e) - R_e (all Q of a layer before any update); neg_e = Q_e < 0; tot = XOR_e neg_e; m1 = min_e |Q_e| at the
 *               lowest e that attains it, a; m2 = min_{e != a} |Q_e|; mag_e = min(max((m2 if e == a else m1) - offset, 0), 127);
 *               R_e = -mag_e if tot ^ neg_e else +mag_e; L_v(e) = clamp(Q_e + R_e, -8191, 8191).  After each whole iteration
 *               x_v = [L_v < 0]; the decoder stops when all 64 mb checks hold, or after max_iters.  The decoded bits are x_0 .. x_{K-1}
 *   counts      (information-bit errors over the B K bits, blocks with any error, iterations run summed over the B blocks) per frame
 * Everything after the quantiser is integer: a host evaluation of this definition agrees bit for bit. */
#define AFT_LINK_LDPC_Z 64
#define AFT_LINK_LDPC_MAX_EDGES 160   /* entries of a base matrix: their int8 messages are 10 KiB of LDS per code block */

/* One launch, one workgroup per frame, one wave per code block and one lane per row of a circulant: counts int32 [batch][3] and, when
 * bits is not NULL, the decoded information bits uint8 [batch, B, K] (both device memory) from llr float32 [batch, S, T, m] (device
 * memory; what aft_link_soft_f32 writes) and keys uint64 [batch] (any device-addressable memory, pinned host memory included).
 * `link` and `shifts` (HOST memory) are read during the call only; the base matrix travels to the kernel by value.  Every element of
 * counts and bits is written (no initialisation needed); no atomics; no workspace; nothing is synchronised; a frame's outputs depend
 * neither on batch, nor on its position in it, nor on the run, nor on whether bits is written.
 * Nothing is launched on AFT_ERR_ARG (a NULL link / llr / keys / shifts / counts; keys not 8-byte or llr / shifts / counts not 4-byte
 * aligned; batch < 1; qgain not finite and positive) and AFT_ERR_SHAPE (what aft_link_errors_f32 refuses; base_rows outside 3 .. 16;
 * base_cols outside base_rows + 1 .. 32; offset outside 0 .. 127; max_iters outside 1 .. 255; a shift outside -1 .. 63; an information
 * column without an entry; more than AFT_LINK_LDPC_MAX_EDGES entries; B = 0; B K above 2^31; a stride or stride_inverse that
 * aft_link_decode_f32 would refuse for this U). */
int aft_link_ldpc_f32(const aft_link *link, const float *llr /* [batch,S,T,m] */, const unsigned long long *keys, int base_rows,
                      int base_cols, const int32_t *shifts /* HOST, [base_rows][base_cols - base_rows] */, unsigned long long stride,
                      unsigned long long stride_inverse, float qgain, int offset, int max_iters, int32_t *counts /* [batch][3] */,
                      unsigned char *bits /* [batch,B,K] or NULL */, int batch, void *stream);

/* ---- receive diversity: maximum-ratio combining over R branches (adafortitran_amd/linksim.py "the diversity link") ----
 *
 * R uncorrelated receive antennas, each with its own channel and its own estimate: group g of a batch is the frames g R .. g R + R - 1,
 * its branches r = 0 .. R-1, branch 0 its leader.  One transmission per group: w, gi, gq, x as aft_link_errors_f32's, from the
 * LEADER's key (stream 5).
 *   received    y_r = H_r x + sigma_r sqrt(-ln u1) exp(j 2 pi u2), u1 and u2 from streams 6 and 7 of branch r's OWN key
 *   combined    c = sum_r rho_r y_r conj(E_r),  p = sum_r rho_r |E_r|^2, in increasing r: c = fma(rho_r, c_r, c), p = fma(rho_r, p_r, p)
 *               rho float32 [batch], one weight per frame: rho_r = scale_r / scale_leader with scale the frame's LLR scale, so
 *               rho_0 = 1; per-branch noise variances without a division on the device
 *   decision, counts, mu_k, Delta_j, Lambda_j = scale Delta_j and loss[f] as aft_link_errors_f32's and aft_link_soft_f32's on this c
 *               and p, with the LEADER's scale (one per group)
 * With branches = 1 and rho = 1 counts are aft_link_errors_f32's and loss and llr aft_link_soft_f32's, bit for bit.
 * One launch, one workgroup per group: counts int32 [batch / branches][2], loss float32 [batch / branches][n_factors] and, when llr
 * is not NULL, llr float32 [batch / branches, S, T, m] (all device memory) from ideal and est complex64 [batch, S, T] (device
 * memory), keys uint64 [batch], sigma and rho float32 [batch], scale float32 [batch / branches] and factors float32 [n_factors]
 * (any device-addressable memory, pinned host memory included).  Every element of the outputs is written; no atomics, no workspace;
 * nothing is synchronised; float sums run in a fixed order, so a group's outputs depend neither on batch, nor on its position in
 * it, nor on the run, nor on the load and store forms (aft_link_soft_f32's), nor on whether llr is written.  The decoders
 * (aft_link_decode_f32, aft_link_ldpc_f32) read this llr with the leaders' keys and batch / branches frames.
 * Nothing is launched on AFT_ERR_ARG (what aft_link_soft_f32 refuses; a NULL rho / counts; rho / counts not 4-byte aligned; batch
 * not a multiple of branches) and AFT_ERR_SHAPE (branches outside 1 .. AFT_LINK_MAX_BRANCHES; what aft_link_errors_f32 refuses). */
#define AFT_LINK_MAX_BRANCHES 8
int aft_link_mrc_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                     const float *sigma, const float *rho, const float *scale /* [batch / branches] */, const float *factors,
                     int n_factors, int branches, int32_t *counts /* [groups][2] */, float *loss /* [groups][n_factors] */,
                     float *llr /* [groups,S,T,m] or NULL */, int batch, void *stream);

/* ---- HARQ link: rate matching and soft combining on the LDPC-coded link (adafortitran_amd/linksim.py "The HARQ link" holds the
 * definition in full) ----
 *
 * A block that fails is sent again, the receiver adds the new soft bits to the old ones and decodes again.
 *   mother code   the LDPC-coded link's: base matrix mb x nb, kb = nb - mb, n = 64 nb, K = 64 kb; encoder and decoder unchanged
 *   rate matching tx_cols = C, kb < C <= nb: a round sends E = 64 C coded bits per block.  rounds = Q in 1 .. AFT_LINK_HARQ_MAX_ROUNDS;
 *                 starts[t] = s_t in 0 .. nb-1, the block column where round t's window begins.  Transmitted bit e = 0 .. E-1 of round
 *                 t is codeword bit v_t(e) = 64 ((s_t + e / 64) mod nb) + e % 64: a circular buffer in whole block columns
 *   position      N bits per frame as on the coded links, B = N / E blocks (integer division), U = B E; transmitted bit e of block b
 *                 sits at data-bit index j = ((b E + e) stride) mod U, gcd(stride, U) = 1; j maps to a grid element and a bit of its
 *                 word as on the coded links; filler and pilots are never read
 *   groups        LLR frames h Q .. h Q + Q - 1 with keys k_0 .. k_{Q-1} are rounds 0 .. Q-1 of group h, k_0 its leader.
 *                 u[b][i] = word(k_0, stream 8, b K + i) >> 63 and c = the codeword of u.  Round t uses its OWN frame's sent words
 *                 w (stream 5 of k_t): scrambler s = w_j ^ c[v_t(e)], z_{t,b,e} = the coded links' quantiser of (1 - 2 s) llr_t[j]
 *   soft buffer   Z_t[b][v] = sum over t' <= t and e with v_{t'}(e) = v of z_{t',b,e}: an integer, |Z| <= 127 Q, 0 where nothing was sent
 *   attempts      after round t every block not yet acknowledged is decoded from scratch (L = Z_t, R = 0; offset, max_iters, layer
 *                 order, clamps and stop rule the LDPC-coded link's).  A block is ACKNOWLEDGED iff its decoded information bits equal u
 *                 (an ideal CRC) and then runs no further attempt: later rounds' LLRs at its positions influence nothing
 *   counts        [0 .. 3] blocks first acknowledged after round t (0 for t >= Q); [4] information-bit errors of the blocks never
 *                 acknowledged, from their last attempt; [5] blocks never acknowledged; [6] iterations summed over all attempts run
 *   bits          each block's decoded information bits from the last attempt it ran
 * With Q = 1, C = nb, s_0 = 0 and the same stride: counts [0] = B - block errors, [4], [5], [6] = aft_link_ldpc_f32's three counts,
 * and the bits are equal bit for bit.  Everything after the quantiser is integer: a host evaluation agrees bit for bit. */
#define AFT_LINK_HARQ_MAX_ROUNDS 4
#define AFT_LINK_HARQ_COUNTS 7

/* One launch, one workgroup per group, one wave per code block and one lane per row of a circulant: counts int32
 * [batch / rounds][AFT_LINK_HARQ_COUNTS] and, when bits is not NULL, bits uint8 [batch / rounds, B, K] (both device memory) from llr
 * float32 [batch, S, T, m] (device memory) and keys uint64 [batch] (any device-addressable memory, pinned host memory included).
 * `link`, `shifts` and `starts` (HOST memory) are read during the call only.  Every element of counts and bits is written; no atomics;
 * no workspace; nothing is synchronised; a group's outputs depend on its own Q keys and LLR frames only: neither on batch, nor on its
 * position in it, nor on the run, nor on whether bits is written.
 * Nothing is launched on AFT_ERR_ARG (what aft_link_ldpc_f32 gives it for; a NULL or misaligned starts; batch not a multiple of
 * rounds) and AFT_ERR_SHAPE (what aft_link_ldpc_f32 refuses for the struct, the base matrix, offset and max_iters; rounds outside 1 ..
 * AFT_LINK_HARQ_MAX_ROUNDS; tx_cols outside kb + 1 .. nb; a start outside 0 .. nb-1; B = 0; B K above 2^31; a stride not coprime to U
 * or outside [1, U), or a stride_inverse that is not its inverse modulo U). */
int aft_link_harq_f32(const aft_link *link, const float *llr /* [batch,S,T,m] */, const unsigned long long *keys, int base_rows,
                      int base_cols, const int32_t *shifts /* HOST, [base_rows][base_cols - base_rows] */, int tx_cols, int rounds,
                      const int32_t *starts /* HOST, [rounds] */, unsigned long long stride, unsigned long long stride_inverse,
                      float qgain, int offset, int max_iters, int32_t *counts /* [batch / rounds][7] */,
                      unsigned char *bits /* [batch / rounds,B,K] or NULL */, int batch, void *stream);

/* ---- spatial multiplexing: two-stream ZF / MMSE detection on R antennas (adafortitran_amd/linksim.py "the spatial-multiplexing link") ----
 *
 * N = streams = 2 transmit streams on R = branches uncorrelated receive antennas, 2 <= R <= AFT_LINK_MAX_BRANCHES, every (antenna,
 * stream) pair with its own channel and its own estimate: group g of a batch is the frames g N R .. g N R + N R - 1, frame
 * g N R + r N + s the pair (antenna r, stream s), frame (0, 0) the group's leader.
 *   sent        stream s sends w_s, gi_s, gq_s, x_s as aft_link_errors_f32's, from stream 5 of the key of frame (0, s)
 *   received    y_r = H_r0 x_0 + H_r1 x_1 + sigma_r sqrt(-ln u1) exp(j 2 pi u2), u1 and u2 from streams 6 and 7 of the key of frame
 *               (r, 0), sigma_r that frame's.  Stream 0's product is aft_link_mrc_f32's own chain, stream 1's two products are added by
 *               fused multiply-adds, the noise last.  keys / sigma / rho of frames (r, 1) are not read beyond stream 5 of (0, 1)
 *   Gram        g00 = sum_r rho_r |E_r0|^2, g11 = sum_r rho_r |E_r1|^2, g01 = sum_r rho_r conj(E_r0) E_r1, rho_r = rho of frame (r, 0)
 *   matched     m_s = sum_r rho_r conj(E_rs) y_r: in increasing r, one fused multiply-add per term as the combiner's, sums start at -0
 *   regulariser reg float32 [groups]: 0 is zero forcing, 1 / scale is MMSE.  a00 = g00 + reg, a11 = g11 + reg
 *   detector    c_0 = a11 m_0 - g01 m_1,        p_0 = g00 a11 - |g01|^2     (the adjugate: no division; comp >= beta_b p_s is the
 *               c_1 = a00 m_1 - conj(g01) m_0,  p_1 = g11 a00 - |g01|^2      unbiased decision)
 *   decision, counts, mu_k, Delta_j and loss[f] as aft_link_errors_f32's and aft_link_soft_f32's on (c_s, p_s) against stream s's sent
 *               word; Lambda_j = eff_s Delta_j with eff_s = scale / a_other (a11 for stream 0, a00 for stream 1: one correctly
 *               rounded division; 0 where a_other <= 0) and the LEADER's scale (one per group)
 * With H_r1 = E_r1 = 0 and reg scale = 1 in powers of two, stream 0's outputs are aft_link_mrc_f32's on the frames (r, 0), bit for bit.
 * (aft_link_joint_f32 below is the same frame walk with a joint max-log demapper in the detector's place.)
 * One launch, one workgroup per group: counts int32 [groups][streams][2], loss float32 [groups][streams][n_factors] and, when llr is
 * not NULL, llr float32 [groups, streams, S, T, m] (all device memory; contiguous, so they read as groups * streams frames with the
 * keys of frames (0, s)) from ideal and est complex64 [batch, S, T] (device memory), keys uint64 [batch], sigma and rho float32
 * [batch], scale and reg float32 [groups] and factors float32 [n_factors] (any device-addressable memory, pinned host memory
 * included).  Every element of the outputs is written; no atomics, no workspace; nothing is synchronised; float sums run in a fixed
 * order, so a group's outputs depend neither on batch, nor on its position in it, nor on the run, nor on the load and store forms
 * (aft_link_soft_f32's), nor on whether llr is written.  The decoders read this llr with the keys of frames (0, s) and
 * groups * streams frames.
 * Nothing is launched on AFT_ERR_ARG (what aft_link_mrc_f32 refuses; a NULL reg; reg not 4-byte aligned; batch not a multiple of
 * branches * streams) and AFT_ERR_SHAPE (streams other than AFT_LINK_MAX_STREAMS; branches outside 2 .. AFT_LINK_MAX_BRANCHES; what
 * aft_link_errors_f32 refuses). */
#define AFT_LINK_MAX_STREAMS 2
int aft_link_sm_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                    const float *sigma, const float *rho /* [batch] */, const float *scale /* [groups] */,
                    const float *reg /* [groups] */, const float *factors, int n_factors, int branches, int streams,
                    int32_t *counts /* [groups][streams][2] */, float *loss /* [groups][streams][n_factors] */,
                    float *llr /* [groups,streams,S,T,m] or NULL */, int batch, void *stream);

/* ---- joint detection: exact max-log LLRs of both streams of that link (adafortitran_amd/linksim.py "the joint link") ----
 *
 * The layout, keys, sent words, received samples, weights and the eight sums m_0, m_1, g00, g11, g01 are aft_link_sm_f32's, formed by
 * the same code: one frame walk serves both entry points, and only what turns an element's eight sums into LLRs and decisions
 * differs.  There is no regulariser and no division.  For stream e with the other stream o,
 * g_oe = g01 for e = 1 and conj(g01) for e = 0, a_k the L levels and mu_k(comp, p) = a_k (a_k p - 2 comp) as aft_link_soft_f32's:
 *   candidates   x_e = a_ki + j a_kq over all M = 2^m words of stream e
 *   interference z(x_e) = m_o - g_oe x_e
 *   inner min    r(x_e) = min_k mu_k(Re z, g_oo) + min_k mu_k(Im z, g_oo)
 *   metric       f(x_e) = g_ee |x_e|^2 - 2 Re(conj(x_e) m_e) + r(x_e): the minimum over x_o of the weighted residual
 *                sum_r rho_r |y_r - E_r0 x_0 - E_r1 x_1|^2, less a constant
 *   Delta_j      = min{f(x_e) : bit j of the word is 1} - min{f(x_e) : bit j is 0}, bit order as aft_link_soft_f32's
 *   Lambda_j     = scale Delta_j with the LEADER's scale (one per group); pilots carry 0
 *   hard         bit j is decided 1 iff Lambda_j < 0; bit errors against the sent word, a symbol error where any bit is wrong
 *   loss[f]      as aft_link_soft_f32's on Lambda_j
 * The exact max-log LLR of every bit of both streams in 2 M candidate evaluations per element: for a fixed x_e the best x_o
 * separates per axis.  Finite operands give finite LLRs, all-zero estimates included (every LLR is 0 then).  Outputs, operands,
 * memory rules and invariants are aft_link_sm_f32's: one launch, one workgroup per group, every element of the outputs written, no
 * atomics, no workspace, nothing synchronised, a group's outputs a function of its own operands only.
 * Nothing is launched on AFT_ERR_ARG and AFT_ERR_SHAPE: what aft_link_sm_f32 refuses, less what it says of reg. */
int aft_link_joint_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                       const float *sigma, const float *rho /* [batch] */, const float *scale /* [groups] */,
                       const float *factors, int n_factors, int branches, int streams,
                       int32_t *counts /* [groups][streams][2] */, float *loss /* [groups][streams][n_factors] */,
                       float *llr /* [groups,streams,S,T,m] or NULL */, int batch, void *stream);

/* ---- transmit diversity: Alamouti pairs over time or frequency (adafortitran_amd/linksim.py "the transmit-diversity link") ----
 *
 * Two transmit antennas send ONE stream as Alamouti pairs, R = branches receive antennas combine, 1 <= R <= AFT_LINK_MAX_BRANCHES:
 * group g of a batch is the frames g 2 R .. g 2 R + 2 R - 1, frame g 2 R + r 2 + s the pair (receive antenna r, transmit antenna s) --
 * aft_link_sm_f32's order --, frame (0, 0) the group's leader.
 *   lines       pairing AFT_LINK_PAIR_TIME: a line is a subcarrier, its elements in increasing symbol; AFT_LINK_PAIR_FREQUENCY: a
 *               line is a symbol, its elements in increasing subcarrier.  The DATA elements of a line in increasing order are
 *               d_0, d_1, ...; (d_2i, d_2i+1) is a pair (a, b), whether or not pilots lie between them; the last data element of
 *               a line with an odd number of them is LONE
 *   sent        every data element sends w, gi, gq, x as aft_link_errors_f32's, from stream 5 of the LEADER's key: one transmission
 *               per group, m data_elements bits
 *   transmit    pair: antenna 0 sends x_a at a and -conj(x_b) at b, antenna 1 sends x_b at a and conj(x_a) at b; lone: antenna 0
 *               sends x, antenna 1 nothing
 *   received    y_r[e] = H_r0[e] t0[e] + H_r1[e] t1[e] + sigma_r sqrt(-ln u1) exp(j 2 pi u2), u1 and u2 from streams 6 and 7 of the
 *               key of frame (r, 0) at e, sigma_r that frame's (aft_link_sm_f32's sample); keys, sigma and rho of frames (r, 1) are
 *               not read
 *   combiner    c_a = sum_r rho_r (conj(E_r0[a]) y_r[a] + E_r1[b] conj(y_r[b])),  p_a = sum_r rho_r (|E_r0[a]|^2 + |E_r1[b]|^2)
 *               c_b = sum_r rho_r (conj(E_r1[a]) y_r[a] - E_r0[b] conj(y_r[b])),  p_b = sum_r rho_r (|E_r1[a]|^2 + |E_r0[b]|^2)
 *               lone: c = sum_r rho_r conj(E_r0) y_r, p = sum_r rho_r |E_r0|^2; rho_r = rho of frame (r, 0); increasing r, within r
 *               the term at a before the term at b, one fused multiply-add per term, sums start at -0
 *   decision, counts, mu_k, Delta_j, Lambda_j = scale Delta_j (the LEADER's scale, one per group) and loss[f] as aft_link_mrc_f32's
 *               on (c, p); pilots carry 0
 * The linear Alamouti combiner, which assumes the channel equal over a pair: what is measured is the cross-talk that channel variation
 * inside a pair and estimation errors leave.  With H_r1 = E_r1 = 0 the LLRs at first and lone elements are aft_link_mrc_f32's on the
 * frames (r, 0), bit for bit.
 * One launch, one workgroup per group: counts int32 [groups][2], loss float32 [groups][n_factors] and, when llr is not NULL, llr
 * float32 [groups, S, T, m] (all device memory) -- aft_link_mrc_f32's outputs, read by the decoders with the leaders' keys -- from
 * ideal and est complex64 [batch, S, T] (device memory), keys uint64 [batch], sigma and rho float32 [batch], scale float32 [groups]
 * and factors float32 [n_factors] (any device-addressable memory, pinned host memory included).  Every element of the outputs is
 * written; no atomics, no workspace; nothing is synchronised; float sums run in a fixed order, so a group's outputs depend neither on
 * batch, nor on its position in it, nor on the run, nor on the alignment of the bases, nor on whether llr is written.
 * Nothing is launched on AFT_ERR_ARG (what aft_link_mrc_f32 refuses; batch not a multiple of branches * 2) and AFT_ERR_SHAPE (branches
 * outside 1 .. AFT_LINK_MAX_BRANCHES; a pairing other than the two below; what aft_link_errors_f32 refuses). */
#define AFT_LINK_PAIR_TIME 0
#define AFT_LINK_PAIR_FREQUENCY 1
int aft_link_alamouti_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                          const float *sigma, const float *rho /* [batch] */, const float *scale /* [groups] */,
                          const float *factors, int n_factors, int branches, int pairing,
                          int32_t *counts /* [groups][2] */, float *loss /* [groups][n_factors] */,
                          float *llr /* [groups,S,T,m] or NULL */, int batch, void *stream);

/* ---- closed-loop precoding: a codebook precoder per subband (adafortitran_amd/linksim.py "the closed-loop link") ----
 *
 * Two transmit antennas send ONE stream co-phased by a rank-1 precoder that the receiver picks per subband from its own estimates (the
 * precoding matrix indicator, PMI), R = branches receive antennas combine, 1 <= R <= AFT_LINK_MAX_BRANCHES: group g of a batch is the
 * frames g 2 R .. g 2 R + 2 R - 1, frame g 2 R + r 2 + s the pair (receive antenna r, transmit antenna s) -- aft_link_sm_f32's and
 * aft_link_alamouti_f32's order --, frame (0, 0) the group's leader.  B = subband, 1 <= B <= S.
 *   subbands    subband b = subcarriers b B .. min(S, (b + 1) B) - 1, all T symbols; n_sub = ceil(S / B) (the last may be short; B = S
 *               is one wideband PMI); n_sub <= AFT_LINK_MAX_SUBBANDS
 *   codebook    q_0 .. q_3 = 1, -1, j, -j; the precoder of index i is (1, q_i): antenna 0 sends x, antenna 1 sends q_i x
 *   selection   g_b = sum over the subband's elements (pilot positions included) and over r of rho_r conj(E_r0) E_r1;
 *               v = (Re g_b, -Re g_b, -Im g_b, Im g_b) = Re(q_i g_b); pmi_b = the LOWEST i that attains max v (g_b = 0 gives 0);
 *               rho_r = rho of frame (r, 0).  One team of W threads per subband, W a power of two in 8 .. 256 fixed by S, T and B:
 *               thread l adds its elements l, l + W, ... in increasing order, within an element the antennas in increasing r, one
 *               fused multiply-add per component; the team's sums are added by shuffles, then wave by wave
 *   sent        every data element sends w, gi, gq, x as aft_link_errors_f32's, from stream 5 of the LEADER's key: one transmission
 *               per group
 *   received    y_r = H_r0 x + (q H_r1) x + sigma_r sqrt(-ln u1) exp(j 2 pi u2), q = q_pmi of the element's subband (q H_r1 is
 *               exact), u1 and u2 from streams 6 and 7 of the key of frame (r, 0), sigma_r that frame's (aft_link_sm_f32's sample);
 *               keys, sigma and rho of frames (r, 1) are not read
 *   effective   e_r = E_r0 + q E_r1, one rounding per component
 *   combiner    c = sum_r rho_r y_r conj(e_r), p = sum_r rho_r |e_r|^2; increasing r, one fused multiply-add per term, sums start at -0
 *   decision, counts, mu_k, Delta_j, Lambda_j = scale Delta_j (the LEADER's scale, one per group) and loss[f] as aft_link_mrc_f32's
 *               on (c, p); pilots carry 0
 * Feedback is instantaneous and free of errors: one PMI per subband, from the same estimates the combiner uses.  With H_r1 = E_r1 = 0
 * every PMI is 0 and the LLRs are aft_link_mrc_f32's on the frames (r, 0), bit for bit; turning H_r1 and E_r1 by a power of j permutes
 * the PMIs and leaves counts, losses and LLRs as they are, bit for bit.
 * One launch, one workgroup per group: counts int32 [groups][2], loss float32 [groups][n_factors], pmi int32 [groups][n_sub] (values
 * 0 .. 3) and, when llr is not NULL, llr float32 [groups, S, T, m] (all device memory) from ideal and est complex64 [batch, S, T]
 * (device memory), keys uint64 [batch], sigma and rho float32 [batch], scale float32 [groups] and factors float32 [n_factors] (any
 * device-addressable memory, pinned host memory included).  Every element of the outputs is written; no atomics, no workspace; nothing
 * is synchronised; float sums run in a fixed order, so a group's outputs depend neither on batch, nor on its position in it, nor on the
 * run, nor on the alignment of the bases, nor on whether llr is written.
 * Every refusal is AFT_ERR_ARG and launches nothing: a NULL pointer (llr excepted) or a misaligned one, batch < 1 or not a multiple of
 * branches * 2, branches outside 1 .. AFT_LINK_MAX_BRANCHES, subband outside 1 .. S, more than AFT_LINK_MAX_SUBBANDS subbands,
 * n_factors outside 1 .. 8, and what aft_link_errors_f32 refuses of the struct (bits_per_symbol among it). */
#define AFT_LINK_MAX_SUBBANDS 1024
int aft_link_precoded_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                          const float *sigma, const float *rho /* [batch] */, const float *scale /* [groups] */,
                          const float *factors, int n_factors, int branches, int subband,
                          int32_t *counts /* [groups][2] */, float *loss /* [groups][n_factors] */,
                          float *llr /* [groups,S,T,m] or NULL */, int32_t *pmi /* [groups][n_sub], not NULL */, int batch,
                          void *stream);

/* Delayed feedback (linksim.py "delayed feedback"): the batch is whole sequences of K = slots groups -- the slots of
 * aft_channel_sim_seq_f32 --, input group seq K + k slot k of sequence seq, and d = delay, 0 <= d < K.  Slots k < d are warm-up: not sent,
 * no output.  Slot k >= d is sent with, per subband, the PMI selected as above from est and rho of slot k - d of the same sequence; the
 * received samples, the effective estimates, the combiner, the decision, the LLRs and the losses use the sent slot's own ideal, est,
 * keys, sigma, rho and scale, exactly as above.  Outputs are compact: output group o = seq (K - d) + (k - d), groups_out =
 * (groups / K) (K - d); counts, loss, llr and pmi have groups_out rows and pmi is the APPLIED index.  Inputs are indexed by input frame
 * or group (scale by input group).  The same kernel body, one workgroup per output group, no workspace, no atomics, no copies; with
 * d = 0 the outputs are aft_link_precoded_f32's, bit for bit.
 * Every refusal is AFT_ERR_ARG and launches nothing: aft_link_precoded_f32's, slots < 1, delay outside 0 .. slots - 1, batch not a
 * multiple of slots * 2 * branches. */
int aft_link_precoded_delayed_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                                  const float *sigma, const float *rho /* [batch] */, const float *scale /* [groups] */,
                                  const float *factors, int n_factors, int branches, int subband, int slots, int delay,
                                  int32_t *counts /* [groups_out][2] */, float *loss /* [groups_out][n_factors] */,
                                  float *llr /* [groups_out,S,T,m] or NULL */, int32_t *pmi /* [groups_out][n_sub], not NULL */,
                                  int batch, void *stream);

/* ---- successive cancellation: ordered MMSE-SIC of the two streams (adafortitran_amd/linksim.py "the successive-cancellation link") ----
 *
 * The layout, keys, sent words, received samples, weights, the eight sums, reg and scale are aft_link_sm_f32's, formed by the same
 * code: the third detector of the one frame walk.  Per data element:
 *   order      f = 1 iff g11 > g00, else 0 (a tie and NaN give 0), o = 1 - f: the order of the linear detector's post-detection SINRs
 *              for every reg >= 0, because p_0 a00 - p_1 a11 = (g00 - g11) det(A)
 *   first      stream f: aft_link_sm_f32's c_f, p_f, eff_f, decision ki, kq, errors and LLRs for that (element, stream), bit for bit
 *   decided    x^ = a_ki + j a_kq, a_k = d (2 k - (L - 1)) formed as the sent symbol is: a correct decision is the float32 that was sent
 *   cancel     c_o = m_o - gx x^, gx = g01 for o = 0 and conj(g01) for o = 1; p_o = g_oo.  re = fma(-gx.re, x^.re, fma(gx.im, x^.im,
 *              m_o.re)), im = fma(-gx.re, x^.im, fma(-gx.im, x^.re, m_o.im))
 *   second     stream o: aft_link_mrc_f32's decision, errors, mu_k, Delta_j and Lambda_j = scale Delta_j on (c_o, p_o) with the LEADER's
 *              scale: no regulariser, no division
 * counts, loss and llr are aft_link_sm_f32's tensors, indexed BY STREAM, not by detection order.  stats int32 [groups][3] (device
 * memory; may be NULL, as llr may) holds per group the data elements with f = 1, the data elements whose first decision is a symbol
 * error and, of those, the elements where stream o has a symbol error too.  One launch, one workgroup per group, every element of
 * the outputs written, no atomics, no workspace, nothing synchronised; a group's outputs depend neither on batch, nor on its
 * position in it, nor on the run, nor on the load and store forms, nor on whether llr or stats is written.  With H_r1 = E_r1 = 0
 * stream 0 is detected first everywhere and stream 1's LLRs are 0.
 * Nothing is launched on AFT_ERR_ARG and AFT_ERR_SHAPE: what aft_link_sm_f32 refuses, and a stats that is not 4-byte aligned. */
int aft_link_sic_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                     const float *sigma, const float *rho /* [batch] */, const float *scale /* [groups] */,
                     const float *reg /* [groups] */, const float *factors, int n_factors, int branches, int streams,
                     int32_t *counts /* [groups][streams][2] */, float *loss /* [groups][streams][n_factors] */,
                     float *llr /* [groups,streams,S,T,m] or NULL */, int32_t *stats /* [groups][3] or NULL */, int batch,
                     void *stream);

/* ---- codeword-level cancellation: decode, cancel, detect again (adafortitran_amd/linksim.py "the codeword-cancellation link") ----
 *
 * A two-codeword receiver cancels a stream only after its decoder has acknowledged it (an ideal CRC: the decoded information bits
 * equal the sent ones), so nothing wrong is ever cancelled.  The receiver is four launches: aft_link_sm_f32 with the MMSE reg and
 * aft_link_ldpc_f32 on its llr (the first pass), then the two entry points below (the second pass).
 *
 * aft_link_cancel_f32: the layout, keys, sent words, received samples, weights, the eight sums and scale are aft_link_sm_f32's, formed
 * by the same code: the fourth detector of the one frame walk.  There is no reg.
 *   failed     int32, any device-addressable memory: failed[(g 2 + s) failed_stride] is the first pass's block-error count of stream s of
 *              group g, failed_stride >= 1 in int32 units (aft_link_ldpc_f32's counts + 1 with stride 3 reads them in place)
 *   redo       redo_s = failed_s != 0 and failed_(1-s) == 0: at most one stream per group; formed by the kernel, wave-uniform
 *   cancel     for the stream s with redo, o = 1 - s, per data element: c_s = m_s - gx x_o with x_o the SENT symbol of stream o (an
 *              acknowledged codeword re-encodes to the sent bits; filler bits are known) and gx = g01 for s = 0, conj(g01) for s = 1,
 *              by aft_link_sic_f32's four fused multiply-adds; p_s = g_ss
 *   detect     aft_link_mrc_f32's decision, errors, mu_k, Delta_j, Lambda_j = scale Delta_j and loss[f] on (c_s, p_s) with the LEADER's
 *              scale: no regulariser, no division.  The residual (H_ro - E_ro) x_o that an imperfect estimate leaves is not modelled in
 *              the scale, as in aft_link_sic_f32's second stage
 *   outputs    counts, loss and llr are aft_link_sm_f32's tensors; a stream without redo has zeros in all three.  state int32
 *              [groups][streams] (device memory; may be NULL, as llr may) holds redo_s as 0 / 1.  A group without a redo reads no
 *              channel and hashes nothing
 * One launch, one workgroup per group, every element of the outputs written, no atomics, no workspace, no division, nothing
 * synchronised; a group's outputs depend neither on batch, nor on its position in it, nor on the run, nor on the load and store forms,
 * nor on whether llr or state is written.  Where aft_link_sic_f32 detected stream s second after a correct first decision, the LLRs
 * here are its second-stage LLRs bit for bit; with H_r1 = E_r1 = 0 stream 0 is aft_link_mrc_f32's on the frames (r, 0), bit for bit.
 * Nothing is launched on AFT_ERR_ARG and AFT_ERR_SHAPE: what aft_link_sm_f32 refuses, less what it says of reg; a NULL or misaligned
 * failed; failed_stride < 1; a state that is not 4-byte aligned. */
int aft_link_cancel_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                        const float *sigma, const float *rho /* [batch] */, const float *scale /* [groups] */,
                        const float *factors, int n_factors, int branches, int streams,
                        const int32_t *failed /* [(groups * streams - 1) * failed_stride + 1] */, int failed_stride,
                        int32_t *counts /* [groups][streams][2] */, float *loss /* [groups][streams][n_factors] */,
                        float *llr /* [groups,streams,S,T,m] or NULL */, int32_t *state /* [groups][streams] or NULL */, int batch,
                        void *stream);

/* aft_link_ldpc_masked_f32: aft_link_ldpc_f32 on the frames a mask selects -- a second instantiation of the same kernel body.
 * mask int32 (any device-addressable memory): frame f is decoded iff mask[f mask_stride] != 0, mask_stride >= 1 in int32 units
 * (aft_link_cancel_f32's state with stride 1 selects the streams it detected again).  A selected frame gets exactly
 * aft_link_ldpc_f32's counts and bits, bit for bit; a frame that is not selected gets counts (0, 0, 0) and, when bits is not NULL,
 * zeros in its rows of bits: its workgroup leaves by a uniform branch before it reads an LLR.  Every element of counts and bits is
 * written; the memory rules and invariants are aft_link_ldpc_f32's.
 * Nothing is launched on AFT_ERR_ARG and AFT_ERR_SHAPE: what aft_link_ldpc_f32 refuses; a NULL or misaligned mask; mask_stride < 1. */
int aft_link_ldpc_masked_f32(const aft_link *link, const float *llr /* [batch,S,T,m] */, const unsigned long long *keys, int base_rows,
                             int base_cols, const int32_t *shifts /* HOST, [base_rows][base_cols - base_rows] */,
                             unsigned long long stride, unsigned long long stride_inverse, float qgain, int offset, int max_iters,
                             const int32_t *mask /* [(batch - 1) * mask_stride + 1] */, int mask_stride,
                             int32_t *counts /* [batch][3] */, unsigned char *bits /* [batch,B,K] or NULL */, int batch, void *stream);

/* ---- decision-directed observation: what the receiver's own decisions say about the channel (adafortitran_amd/linksim.py "the
 * decision-directed observation") ----
 *
 * The diversity link's groups, keys, received samples and combiner, unchanged: y_r, c and p as aft_link_mrc_f32's, so the hard decision
 * k_i, k_q (per axis the number of inner boundaries beta_b p at or below the component of c) is that entry point's, bit for bit.
 *   x^          = d (2 k_i - (L - 1)) + j d (2 k_q - (L - 1)), the decided symbol; with source = AFT_LINK_OBSERVE_SENT the sent x
 *                 (the genie bound: what a decoder that got every bit right would re-modulate)
 *   z_r         = y_r conj(x^) / |x^|^2 at a data element, for each of the group's R frames: |x^|^2 = fma(ar, ar, ai ai), each
 *                 component one product, one fused multiply-add and one correctly rounded division;
 *                 frame r's own pilot, bit for bit, at pilot position (sc_i, sym_j)
 *   decisions   uint8 [batch / branches, S, T]: k_i | k_q << 4 at a data element (the DECIDED indices, whatever `source`), 255 at a pilot
 *   symbol_errors int32 [batch / branches]: the data elements whose decided (k_i, k_q) is not the sent one
 * One launch, one workgroup per group: z complex64 [batch, S, T] from ideal and est complex64 [batch, S, T] and pilots complex64
 * [batch, Ps, Pt] (device memory), keys uint64 [batch], sigma and rho float32 [batch] (any device-addressable memory).  Every element
 * of the three outputs is written exactly once; no atomics, no workspace; nothing is synchronised; a group's outputs depend neither on
 * batch, nor on its position in it, nor on the run, nor on the load and store forms (16 bytes per pair when T is even and the plane's
 * base is 16-byte aligned, 8 bytes per element otherwise).
 * Nothing is launched on AFT_ERR_ARG (a NULL pointer; ideal, est, keys, pilots or z not 8-byte, sigma, rho or symbol_errors not 4-byte
 * aligned; batch < 1 or not a multiple of branches; source neither constant) and AFT_ERR_SHAPE (what aft_link_mrc_f32 refuses). */
#define AFT_LINK_OBSERVE_DECIDED 0
#define AFT_LINK_OBSERVE_SENT 1
int aft_link_observe_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                         const float *sigma, const float *rho, const float *pilots /* [batch,Ps,Pt] */, int source, int branches,
                         float *z /* [batch,S,T] */, unsigned char *decisions /* [groups,S,T] */, int32_t *symbol_errors /* [groups] */,
                         int batch, void *stream);

/* ---- training path of the encoder ---- */

/* Gradients of one nn.TransformerEncoderLayer: same fields and shapes as aft_layer_weights,
 * writable.  These are the .grad tensors autograd hands to the optimizer
 * (reference src/main/trainer.py:195-233, loss.backward()). */
typedef struct aft_layer_grads {
    float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b;
    float *lin1_w, *lin1_b, *lin2_w, *lin2_b;
    float *norm1_w, *norm1_b, *norm2_w, *norm2_b;
} aft_layer_grads;

/* Bytes of the per-layer activation tape the training forward fills and the backward reads, and
 * of the scratch either call needs (both 0 on a bad config). */
size_t aft_encoder_tape_bytes(const aft_config *cfg, int batch);
size_t aft_encoder_train_scratch_bytes(const aft_config *cfg, int batch);

/* Replaces nn.TransformerEncoderLayer.forward in train() mode (reference blocks/encoders.py:44-55,
 * called from encoders.py:69): x_in f32 [2B*tokens, d] -> x_out (may not alias x_in, which the
 * backward reads again).  Dropout with probability `dropout_p` at the layer's four sites (attention
 * probabilities, after out_proj, after the activation, after linear2) from a counter-based
 * generator keyed by `seed`; the backward must be given the same seed.  dropout_p = 0 reproduces
 * the eval-mode layer. */
int aft_encoder_layer_fwd_train_f32(const aft_config *cfg, const aft_layer_weights *w, const float *x_in, float *x_out,
                                    void *tape, size_t tape_bytes, void *scratch, size_t scratch_bytes, int batch,
                                    float dropout_p, uint64_t seed, void *stream);

/* The same layer inside a stack (reference blocks/encoders.py:69 loops over the layers): what changes is only WHERE the
 * in-projection of a layer runs.  `qkv_ready` != 0: the previous call already left this layer's q | k | v in `tape`
 * (skip the in-projection GEMM).  `next_w` + `next_tape` (the NEXT layer's parameters and its tape, same cfg and batch) +
 * `next_qkv_written`: when the fused row-local kernel covers the shape, the next layer's in-projection is computed as its
 * tail while the output tile is still in registers and written into `next_tape`; *next_qkv_written says whether that
 * happened (pass it as the next call's qkv_ready).  The backward is unchanged: each layer's aft_encoder_layer_bwd_f32
 * still produces its own in-projection gradients from its own tape. */
int aft_encoder_layer_fwd_train_chained_f32(const aft_config *cfg, const aft_layer_weights *w, const float *x_in, float *x_out,
                                            void *tape, size_t tape_bytes, void *scratch, size_t scratch_bytes, int batch,
                                            float dropout_p, uint64_t seed, int qkv_ready, const aft_layer_weights *next_w,
                                            void *next_tape, size_t next_tape_bytes, int *next_qkv_written, void *stream);

/* Replaces autograd's backward through that layer: dx_out = dL/dx_out [2B*tokens, d] ->
 * dx_in = dL/dx_in (may alias dx_out) and the twelve parameter gradients in `grads`
 * (overwritten, or added to when accumulate != 0). */
int aft_encoder_layer_bwd_f32(const aft_config *cfg, const aft_layer_weights *w, const float *x_in, const void *tape,
                              size_t tape_bytes, const float *dx_out, float *dx_in, const aft_layer_grads *grads,
                              int accumulate, void *scratch, size_t scratch_bytes, int batch, float dropout_p,
                              uint64_t seed, void *stream);

/* nn.Linear in the training path (pilot_upsampler fortitran.py:86, linear_1 / linear_2 encoders.py:33,56,
 * the adapter MLPs channel_adaptivity.py:35-39): y[rows,out] = x[rows,in] W[out,in]^T + b, and its
 * backward dx = dy W (skipped when dx is NULL), dW (+)= dy^T x, db (+)= column sums of dy (NULL: none).
 * Any sizes; the weight gradient's reduction over rows is split and summed in a fixed order. */
int aft_dense_fwd_f32(const float *x, const float *weight, const float *bias, float *y, int rows, int in_features,
                      int out_features, void *stream);
size_t aft_dense_bwd_scratch_bytes(int rows, int in_features, int out_features);
int aft_dense_bwd_f32(const float *x, const float *weight, const float *dy, float *dx, float *dweight, float *dbias,
                      int accumulate, void *scratch, size_t scratch_bytes, int rows, int in_features, int out_features,
                      void *stream);

/* ConvEnhancer (reference src/models/blocks/enhancers.py:5-31: conv 1->8->32->8->1, ReLU after the
 * first three) in train() mode on `planes` real planes x, y: f32 [planes, S, T].  weights[k] / biases[k]
 * are conv_block.{0,2,4,6}.{weight,bias} in PyTorch layout.  c1, c2, c3 receive the activations the
 * backward needs: f32 [planes, C, T, S] with C = 8, 32, 8 (an internal layout; treat as opaque).
 * `scratch`: aft_conv_enhancer_fwd_scratch_bytes() bytes the call may overwrite (the weights re-laid as MFMA operand fragments for the
 * default grid's kernel; ABI 7), or NULL = the kernels that read the weights in place (on the default grid: results that agree with
 * the scratch call's to rounding, not bit for bit). */
size_t aft_conv_enhancer_fwd_scratch_bytes(int planes, int num_scs, int num_symbols);
int aft_conv_enhancer_fwd_train_f32(const float *const weights[4], const float *const biases[4], const float *x, float *y,
                                    float *c1, float *c2, float *c3, void *scratch, size_t scratch_bytes, int planes, int num_scs,
                                    int num_symbols, void *stream);

/* Backward of that call: dy = dL/dy -> dx = dL/dx and the eight parameter gradients (PyTorch layouts;
 * overwritten, or added to when accumulate != 0).  weights[k] are the module's conv weights as in the forward call:
 * the data gradient of the stack is the stack itself run on dy with weights[3-k].transpose(0,1).flip(2,3), which the
 * call lays out in its scratch (one small kernel).
 * aft_conv_enhancer_scratch_bytes returns 0 for an empty grid and for one whose single plane's conv2 activations pass 2 GiB; every
 * other grid has a plan (row bands, and column tiles where a band cannot hold all of the grid's symbols). */
size_t aft_conv_enhancer_scratch_bytes(int planes, int num_scs, int num_symbols);
int aft_conv_enhancer_bwd_f32(const float *const weights[4], const float *x, const float *c1, const float *c2,
                              const float *c3, const float *dy, float *dx, float *const dweights[4], float *const dbiases[4],
                              int accumulate, void *scratch, size_t scratch_bytes, int planes, int num_scs, int num_symbols,
                              void *stream);

/* ChannelAdapter (reference src/models/blocks/channel_adaptivity.py:24-63) in train() mode: conditions[e] f32
 * [frames] (snr, delay spread, doppler), weights / biases in the order {snr,ds,dop}_encoder.{0,2,4}; tokens6 f32
 * [frames, tokens, 6]; hidden0 / hidden1 receive the post-ReLU activations [frames,3,h0] / [frames,3,h1] the
 * backward needs.  The backward turns dL/dtokens6 into the 18 parameter gradients (inputs carry no gradient);
 * dhidden0 / dhidden1 are scratch of the same shapes. */
int aft_adapter_fwd_train_f32(const float *const conditions[3], const float *const weights[9], const float *const biases[9],
                              const int32_t hidden[3], int tokens, int frames, float *tokens6, float *hidden0, float *hidden1,
                              void *stream);
int aft_adapter_bwd_f32(const float *const conditions[3], const float *const weights[9], const float *const biases[9],
                        const int32_t hidden[3], int tokens, int frames, const float *hidden0, const float *hidden1,
                        const float *dtokens6, float *dhidden0, float *dhidden1, float *const dweights[9],
                        float *const dbiases[9], int accumulate, void *stream);

/* The two thin ends of the encoder in the training path (ABI 8), each ONE streaming launch per direction instead of PyTorch's
 * unfold / cat / broadcast add around a 6- or 12-column GEMM.  `planes` = 2 x frames in the training composite's order
 * [real planes | imaginary planes]; grid = num_scs x num_symbols, tokens = (num_scs / patch_scs) (num_symbols / patch_symbols),
 * p = patch_scs patch_symbols <= 32, model_dim a multiple of 4 up to 512.
 *   embed  (fortitran.py:212-217, blocks/patch_processors.py:22,34-35, blocks/encoders.py:67-68):
 *     x0[planes*tokens, d] = cat(PatchEmbedding(conv_enhanced), tokens6) W1^T + b1 + pos[:tokens]
 *     conv_enhanced f32 [planes,S,T]; tokens6 f32 [planes,tokens,6] PER PLANE or NULL (then W1 is [d,p], else [d,p+6]); pos f32
 *     [>= tokens, d] (the learnable table's or the sinusoid buffer's first rows).
 *     backward: dx0 -> d_conv_enhanced [planes,S,T] (every element written), d_tokens6 (NULL with tokens6 NULL), dW1, db1, dpos
 *     [tokens,d] (NULL: no table gradient, e.g. the sinusoid); the parameter gradients are overwritten, or added to when
 *     accumulate != 0.
 *   tail   (blocks/encoders.py:70, blocks/patch_processors.py InversePatchEmbedding, fortitran.py:225-227):
 *     out[planes,S,T] = resid + InversePatchEmbedding(x W2^T + b2),  x f32 [planes*tokens, d], W2 [p,d]
 *     backward: d_out [planes,S,T] -> dx [planes*tokens,d], dW2, db2 (the residual's gradient IS d_out: nothing to compute). */
size_t aft_embed_bwd_scratch_bytes(int planes, int num_scs, int num_symbols, int patch_scs, int patch_symbols, int model_dim,
                                   int with_tokens6);
int aft_embed_fwd_train_f32(const float *conv_enhanced, const float *tokens6, const float *w1, const float *b1, const float *pos,
                            float *x0, int planes, int num_scs, int num_symbols, int patch_scs, int patch_symbols, int model_dim,
                            void *stream);
int aft_embed_bwd_f32(const float *conv_enhanced, const float *tokens6, const float *w1, const float *dx0, float *d_conv_enhanced,
                      float *d_tokens6, float *dw1, float *db1, float *dpos, int accumulate, void *scratch, size_t scratch_bytes,
                      int planes, int num_scs, int num_symbols, int patch_scs, int patch_symbols, int model_dim, void *stream);
size_t aft_tail_bwd_scratch_bytes(int planes, int num_scs, int num_symbols, int patch_scs, int patch_symbols, int model_dim);
int aft_tail_fwd_train_f32(const float *x, const float *w2, const float *b2, const float *resid, float *out, int planes, int num_scs,
                           int num_symbols, int patch_scs, int patch_symbols, int model_dim, void *stream);
int aft_tail_bwd_f32(const float *x, const float *w2, const float *d_out, float *dx, float *dw2, float *db2, int accumulate,
                     void *scratch, size_t scratch_bytes, int planes, int num_scs, int num_symbols, int patch_scs, int patch_symbols,
                     int model_dim, void *stream);

/* Replaces torch.optim.Adam.step (reference src/main/trainer.py:407-413; amsgrad off) on one flat
 * float32 shard of n elements: grad is first multiplied by grad_scale (1/world_size after a
 * sum-reduce-scatter), weight_decay is the L2 form Adam uses; `step` is the 1-based step count. */
int aft_adam_step_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n, float lr, float beta1,
                      float beta2, float eps, float weight_decay, float grad_scale, int step, void *stream);

/* ---- the optimizer step without a host read (ABI 9) ----
 * What torch decides on the host around optimizer.step() -- clip_grad_norm_ (reference src/main/trainer.py:214,222-224),
 * GradScaler's found_inf / grad_scale (trainer.py:207-217), the step count of the bias correction -- decided on the device:
 *
 *     aft_grad_sumsq_f32 -> [all-reduce of *sumsq over the ranks] -> aft_adam_prepare_f32 -> aft_adam_step_ctrl_f32
 *
 * The control block is 32 bytes of DEVICE memory owned by the caller, zeroed once (step = 0); the preparation launch rewrites
 * it every step and the Adam launch reads it.  `step` counts APPLIED steps: a skipped step leaves it, the parameters and both
 * moments untouched. */
typedef struct aft_step_control {
    int32_t skip;        /* 1: found_inf was > 0, the Adam launch stores nothing                                      */
    int32_t step;        /* applied steps so far, this one included when it is applied                               */
    float grad_scale;    /* host_scale / grad_scale * min(1, max_norm / (grad_norm + 1e-6))                          */
    float inv_bc1;       /* 1 / (1 - beta1^step)                                                                     */
    float inv_sqrt_bc2;  /* 1 / sqrt(1 - beta2^step)                                                                 */
    float grad_norm;     /* global norm of the unscaled gradient before clipping (written when sumsq is given)       */
    float clip_coef;     /* min(1, max_norm / (grad_norm + 1e-6))                (written when sumsq is given)       */
    int32_t reserved;
} aft_step_control;

/* Sum of squares of a flat float32 buffer (16-byte aligned) in float64: per-workgroup partials over fixed chunks of 4096
 * elements in `scratch` (aft_grad_sumsq_scratch_bytes(n) bytes; 0 for n = 0 or beyond 2^40), then one workgroup adds them in a
 * fixed order.  No atomics: the bits depend on the data and on n only, not on the device or on what else runs on it.
 * *nonfinite = 1 when an element is inf / nan, else 0.  Two launches. */
size_t aft_grad_sumsq_scratch_bytes(size_t n);
int aft_grad_sumsq_f32(const float *grad, size_t n, void *scratch, size_t scratch_bytes, double *sumsq, float *nonfinite,
                       void *stream);
/* One launch, one thread: fills *ctrl for the Adam launch that follows.  sumsq (NULL: no clipping; max_norm is then ignored) is
 * the squared norm of the gradient buffer BEFORE host_scale and 1/grad_scale are applied; found_inf / grad_scale are
 * torch.amp.GradScaler's device scalars (NULL: none).  A nan norm leaves the scale unclipped, an infinite one makes it 0. */
int aft_adam_prepare_f32(aft_step_control *ctrl, const double *sumsq, const float *found_inf, const float *grad_scale,
                         double host_scale, double max_norm, float beta1, float beta2, void *stream);
/* aft_adam_step_f32 with grad_scale and the bias corrections read from *ctrl; nothing is stored when ctrl->skip is set. */
int aft_adam_step_ctrl_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n, float lr, float beta1,
                           float beta2, float eps, float weight_decay, const aft_step_control *ctrl, void *stream);
/* torch.nn.utils.clip_grad_norm_ on a flat buffer (16-byte aligned, n a multiple of 4) whose squared norm is *sumsq:
 * norm = sqrt(sumsq) * pre_scale, grad *= min(1, max_norm / (norm + 1e-6)), *norm_out = norm.  One launch. */
int aft_grad_clip_f32(float *grad, size_t n, const double *sumsq, double pre_scale, double max_norm, float *norm_out,
                      void *stream);

/* ---- per-stage entry points (known-answer tests) ----
 * Same arithmetic as aft_forward_f32 stage by stage, but NOT always the same kernels: these calls own no scratch, so on the default
 * 120 x 14 grid S1+S2 and the tail run the banded conv kernel with the pilot_upsampler product inside it (k_conv.hip), while the
 * forward runs the product in its prologue launch and the column-streaming conv kernel (k_conv_stream.hip); the embedding stage is
 * its own kernel here and part of the first chain launch there.  The kernels the forward launches are pinned through
 * aft_workspace_region (tests/test_hip_parity.py::test_forward_intermediates_match_golden). */

/* S1+S2 (fortitran.py:203-209): pilots complex64 [B,Ps,Pt] -> conv_enhanced f32 [2B,S,T]. */
int aft_stage_upsample_f32(const aft_config *cfg, const aft_weights *w, const float *pilots,
                           float *conv_enhanced, int batch, void *stream);
/* S4 (channel_adaptivity.py:59-63): snr/ds/dop [B] -> adapter tokens f32 [B,tokens,6]. */
int aft_stage_adapter_f32(const aft_config *cfg, const aft_weights *w, const float *snr,
                          const float *ds, const float *dop, float *tokens6, int batch,
                          void *stream);
/* S3+S4-concat+linear_1+pos (fortitran.py:212-217, encoders.py:67-68):
 * conv_enhanced [2B,S,T] (+ tokens6 [B,tokens,6] or NULL) -> x f32 [2B*tokens, d]. */
int aft_stage_embed_f32(const aft_config *cfg, const aft_weights *w, const float *conv_enhanced,
                        const float *tokens6, float *x, int batch, void *stream);
/* One nn.TransformerEncoderLayer in eval mode, in place on x [2B*tokens, d]
 * (encoders.py:69).  `scratch` needs aft_workspace_bytes(cfg,batch) bytes.  Runs the engine aft_engine_of(cfg) names. */
int aft_stage_encoder_layer_f32(const aft_config *cfg, const aft_weights *w, int layer, float *x,
                                void *scratch, size_t scratch_bytes, int batch, void *stream);
/* linear_2 + S6 + S7 + S8 + complex recombination (encoders.py:70, fortitran.py:225-231,180):
 * x [2B*tokens, d], conv_enhanced [2B,S,T] -> out complex64 [B,S,T].  This call owns no scratch, so linear_2's weights must fit the
 * conv kernel's LDS beside the plane (AFT_ERR_SHAPE otherwise, e.g. 32-element patches at model_dim 512 on the default grid: only
 * aft_forward_f32 serves those). */
int aft_stage_tail_f32(const aft_config *cfg, const aft_weights *w, const float *x,
                       const float *conv_enhanced, float *out, int batch, void *stream);

/* ---- measurement hook (bench.py roofline leg; no reference counterpart) ----
 * Launch ONE kernel class `reps` times back to back on `stream`, on the activations a previous
 * aft_forward_f32 of the same (cfg, batch) left in `workspace`, so the caller can bracket it with
 * events on that stream.  Same kernels, grids and arguments as inside aft_forward_f32. */
#define AFT_KERNEL_UPSAMPLE 0   /* initial ConvEnhancer as the forward launches it (on the planes of the prologue's
                                   pilot_upsampler product where the forward does that; else product + ConvEnhancer fused) */
#define AFT_KERNEL_EMBED 1      /* patch gather + adapter concat + linear_1 + pos as its own kernel (the stage entry
                                   point's; aft_forward_f32 runs it inside AFT_KERNEL_QKV)                     */
#define AFT_KERNEL_QKV 2        /* chain kernel: embedding + in-projection of layer 0.  Where the forward folds layer 0's K / V
                                   (fp32 packed engine, switch AFT_L0_FOLD) so does this class: it reads the two tables the
                                   prologue leaves in the workspace, which a forward overwrites later on -- its K / V are
                                   meaningful only right behind AFT_KERNEL_PROLOGUE; its timing is the forward's launch's either way */
#define AFT_KERNEL_ATTENTION 3  /* MFMA attention                                            */
#define AFT_KERNEL_CHAIN 4      /* chain kernel: out-proj+LN1+FFN+LN2 (layer 0) + QKV (layer 1) */
#define AFT_KERNEL_TAIL 5       /* fold + residual + final ConvEnhancer (linear_2 done by AFT_KERNEL_CHAIN_LAST) */
#define AFT_KERNEL_CHAIN_LAST 6 /* chain kernel of the last layer: out-proj+LN1+FFN+LN2 + linear_2             */
/* (7 was the retired plane-resident encoder kernel: now an unknown kernel id) */
#define AFT_KERNEL_PROLOGUE 8   /* the forward's first launch: channel adapter + weight re-lay + pilot_upsampler product (+ the
                                   tables and folded matrices of layer 0's K / V where the forward folds them); `out` = one
                                   buffer [pilots: batch x Ps x Pt x 2 floats | snr: batch | ds: batch | dop: batch]        */
int aft_profile_kernel_f32(const aft_config *cfg, const aft_weights *w, int which, float *out,
                           void *workspace, size_t workspace_bytes, int batch, int reps, void *stream);

/* ---- test hook (no reference counterpart) ----
 * Fill the LDS of every CU of the current device with `value` (a NaN, 1e30 ...): what a kernel finds in its LDS at start is whatever
 * the previous kernel on that CU left there, and a kernel that multiplies a zero weight with an LDS word it never wrote computes
 * 0 x NaN (round 6: embed_any_kernel did; caught only because another test's kernels had run before).  The allocator-poisoning
 * tests cannot reach LDS; this can: workgroups of 160 KB each, enough of them that every CU runs at least one.  Asynchronous on
 * `stream`. */
int aft_debug_fill_lds_f32(float value, void *stream);
/* The other half of the hook: what a kernel that writes nothing finds in its LDS.  `workgroups` workgroups (256 threads, 40 KB of
 * LDS each) copy the first `n` (<= 10240) floats of their LDS to out[workgroup][n] (device memory). */
int aft_debug_peek_lds_f32(float *out, int workgroups, int n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ADAFORTITRAN_AMD_H */
