// k_layer.hip -- one launch per encoder layer: the attention of a 32-row tile and the row-local chain behind it in ONE kernel
// (device code: attn_device.h, chain_device.h).
//
// Row tiles are PLANE-ALIGNED (ChainArgs::tpp = ceil(tokens / 32) tiles per plane; tile t = plane t / tpp, query tile t % tpp), so the
// four attention tasks of a tile's 32 query rows -- one per head -- are one per WAVE of the chain workgroup that owns the tile: wave w
// runs task (plane, head w, query tile) through attn_body, leaves the normalised O^T fragments in the workgroup's LDS (they come out of
// attn_body in exactly the operand-fragment layout the out-projection wants as its B operand), one workgroup barrier, and chain_body
// runs out-projection + LN1 + FFN + LN2 + the next layer's in-projection on the same rows.  The attention output never leaves the CU,
// no tile straddles a plane (the q / k / v^T epilogue is always the in-plane form), and a layer is one launch instead of two.
//
// Nothing synchronises workgroups inside the kernel: every dependency between workgroups is a launch boundary.  A layer's attention
// reads the K and V^T of its WHOLE plane while other workgroups already write the next layer's, so K and V^T alternate between two
// buffers from layer to layer (the caller's business, aft_api.hip); Q is read and re-written by the same wave, x by the same workgroup.
//
// Per row, every product keeps its k order and every LayerNorm its merge order: the bits are those of the launch sequence.
#include <algorithm>

#include "attn_device.h"
#include "chain_device.h"

namespace aft {

struct LayerArgs {
    ChainArgs c;                           // the chain's arguments; q / k / vt there are the NEXT layer's (written)
    const float *aq, *ak, *avt, *qbias;    // this layer's q / k / v^T (read) and its in_proj_bias (the query bias)
    float scale_log2e;
    int planes;
};

// chain_body's `pre`: the tile's attention, wave w = head w, into the upper half of the hidden buffer (idle until the FFN), + the barrier
template <int D, int TOK>
struct LayerAttention {
    const LayerArgs &a;
    float *sink;   // [head][s][lane][4]
    __device__ __forceinline__ void operator()(int tile) const {
        const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int plane = tile / a.c.tpp, qt = tile - plane * a.c.tpp;
        const int task = (plane * (D / kHeadDim) + w) * a.c.tpp + qt;     // attn_body's numbering: (plane * heads + head) * key tiles + query tile
        // exactly one task: no stride reaches a second one, so the hand-over of the next task's operands (12 registers that would have
        // to live across the chain) is off
        attn_body<false, kHeadDim, TOK, true>(a.aq, a.ak, a.avt, a.qbias, nullptr, D / kHeadDim, a.c.tokens, a.c.tokpad, D, a.scale_log2e, task,
                                              1 << 30, task + 1, nullptr, -1, sink + w * 1024);
        __syncthreads();
    }
};

// The register bound is chain_kernel's: three workgroups per CU, three waves per SIMD.
template <int D, int ACT, bool QKV, int TOK>
__global__ __launch_bounds__(D * 2, 3) void layer_kernel(const LayerArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    using S = ChainShape<D>;
    // XCD-contiguous tile ranges, as attn_kernel deals its tasks: the tiles of a plane read its K / V^T through one L2
    int vblock = blockIdx.x;
    if ((gridDim.x & 7) == 0) vblock = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    chain_body<D, ACT, true, QKV, false, true>(a.c, smem, threadIdx.x, vblock, gridDim.x, a.planes * a.c.tpp,
                                               LayerAttention<D, TOK>{a, smem + S::XB + S::XB});
}

// The first launch of the fused sequence: embedding + layer 0's in-projection on plane-aligned tiles (chain_kernel<.., false, true>'s body)
template <int D>
__global__ __launch_bounds__(D * 2, 3) void chain_plane_tiles_kernel(const ChainArgs a, int planes) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int vblock = blockIdx.x;
    if ((gridDim.x & 7) == 0) vblock = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    chain_body<D, AFT_ACT_RELU, false, true, false, true>(a, smem, threadIdx.x, vblock, gridDim.x, planes * a.tpp);
}

template <class K, class A, class... Rest>
static hipError_t launch_plane_tiles(K kernel, const A &args, int planes, int tpp, hipStream_t st, PerDeviceOnce &lds_attr, Rest... rest) {
    using S = ChainShape<128>;
    hipError_t ea = ensure_dynamic_lds(lds_attr, reinterpret_cast<const void *>(kernel), S::LDS_BYTES);
    if (ea != hipSuccess) return ea;
    const int blocks = std::min(planes * tpp, current_device_cus() * 3);      // the co-resident count, as launch_chain
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(S::THREADS), S::LDS_BYTES, st, args, rest...);
    return hipGetLastError();
}

bool layer_fused_ok(const aft_config &c) {
    return packed_engine_ok(c) && c.precision == AFT_PRECISION_F32 && c.model_dim == 128 && c.num_head * kHeadDim == c.model_dim &&
           tokens_of(c) >= kTile;
}

hipError_t launch_chain_plane_tiles(const aft_config &c, const aft_layer_weights *qw, const float *q_packed, float *x, float *q, float *k,
                                    float *vt, int planes, int tokens, int tokpad, hipStream_t st, const ChainFusion *fuse) {
    if (!layer_fused_ok(c) || fuse == nullptr || fuse->conv_enhanced == nullptr) return hipErrorInvalidValue;
    ChainArgs a = make_chain_args(c, nullptr, nullptr, qw, q_packed, nullptr, x, q, k, vt, planes * tokens, tokens, tokpad, fuse);
    a.tpp = tokpad / kTile;
    static PerDeviceOnce once;
    return launch_plane_tiles(chain_plane_tiles_kernel<128>, a, planes, a.tpp, st, once, planes);
}

template <int ACT, bool QKV, int TOK>
static hipError_t launch_layer_v(const LayerArgs &a, hipStream_t st) {
    static PerDeviceOnce once;   // per instantiation x device
    return launch_plane_tiles(layer_kernel<128, ACT, QKV, TOK>, a, a.planes, a.c.tpp, st, once);
}
template <int ACT, bool QKV>
static hipError_t launch_layer_t(const LayerArgs &a, hipStream_t st) {
    // the benchmark grid's token count at compile time, as attn_kernel<32, 280> (k_attn.hip)
    return a.c.tokens == 280 ? launch_layer_v<ACT, QKV, 280>(a, st) : launch_layer_v<ACT, QKV, 0>(a, st);
}

hipError_t launch_layer(const aft_config &c, const aft_layer_weights *m, const float *m_packed, const aft_layer_weights *qw,
                        const float *q_packed, float *x, float *q, const float *k_in, const float *vt_in, float *k_out, float *vt_out,
                        int planes, int tokens, int tokpad, hipStream_t st, const ChainFusion *fuse) {
    if (!layer_fused_ok(c) || m == nullptr || k_in == k_out || vt_in == vt_out) return hipErrorInvalidValue;
    LayerArgs a{};
    a.c = make_chain_args(c, m, m_packed, qw, q_packed, nullptr, x, q, k_out, vt_out, planes * tokens, tokens, tokpad, fuse);
    a.c.tpp = tokpad / kTile;
    a.aq = q; a.ak = k_in; a.avt = vt_in;
    a.qbias = m->in_proj_b;
    a.scale_log2e = 1.4426950408889634f / sqrtf((float)kHeadDim);
    a.planes = planes;
    const bool gelu = c.activation == AFT_ACT_GELU;
    if (qw != nullptr) return gelu ? launch_layer_t<AFT_ACT_GELU, true>(a, st) : launch_layer_t<AFT_ACT_RELU, true>(a, st);
    return gelu ? launch_layer_t<AFT_ACT_GELU, false>(a, st) : launch_layer_t<AFT_ACT_RELU, false>(a, st);
}

}  // namespace aft
