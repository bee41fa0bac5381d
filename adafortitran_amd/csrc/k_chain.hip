// k_chain.hip -- launchers of the row-local chain kernel (device code: chain_device.h) and the weight re-packing kernel.
#include <algorithm>
#include <cstdlib>

#include "chain_device.h"
#include "pack_device.h"

#ifndef AFT_CHAIN_MANY_MAX_D
#define AFT_CHAIN_MANY_MAX_D 96
#endif

namespace aft {

// MLP / QKV select the three launch variants at compile time (distinct symbols in a profile), see chain_device.h
template <int D, int ACT, bool MLP, bool QKV>
__global__ __launch_bounds__(D * 2, D <= 128 ? 3 : 2) void chain_kernel(const ChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // persistent workgroups: the grid is sized to the co-resident count and each workgroup walks the row tiles with
    // stride gridDim.x (no dispatch gaps, no launch tail)
    chain_body<D, ACT, MLP, QKV>(a, smem, threadIdx.x, blockIdx.x, gridDim.x, (a.rows + 31) / 32);
}


// split-precision tier (aft_config.precision = AFT_PRECISION_BF16X3): the same body with its GEMMs on bf16 hi/lo terms
template <int D, int ACT, bool MLP, bool QKV>
__global__ __launch_bounds__(D * 2, D <= 128 ? 3 : 2) void chain_split_kernel(const ChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    chain_body<D, ACT, MLP, QKV, true>(a, smem, threadIdx.x, blockIdx.x, gridDim.x, (a.rows + 31) / 32);
}

template <int D, int ACT, bool MLP, bool QKV>
static hipError_t launch_chain_split_v(const ChainArgs &args, hipStream_t st) {
    using S = ChainShape<D>;
    static PerDeviceOnce lds_attr;
    hipError_t ea = ensure_dynamic_lds(lds_attr, reinterpret_cast<const void *>(chain_split_kernel<D, ACT, MLP, QKV>), S::LDS_BYTES);
    if (ea != hipSuccess) return ea;
    const int blocks = std::min((args.rows + 31) / 32, current_device_cus() * (D <= 128 ? 3 : 1));
    hipLaunchKernelGGL((chain_split_kernel<D, ACT, MLP, QKV>), dim3(blocks), dim3(S::THREADS), S::LDS_BYTES, st, args);
    return hipGetLastError();
}

template <int D, int ACT>
static hipError_t launch_chain_split_t(const ChainArgs &args, bool mlp, bool qkv, hipStream_t st) {
    if (mlp && qkv) return launch_chain_split_v<D, ACT, true, true>(args, st);
    if (mlp) return launch_chain_split_v<D, ACT, true, false>(args, st);
    return launch_chain_split_v<D, ACT, false, true>(args, st);
}

template <int D, int ACT, bool MLP, bool QKV>
static hipError_t launch_chain_v(const ChainArgs &args, hipStream_t st) {
    using S = ChainShape<D>;
    static PerDeviceOnce lds_attr;   // per instantiation x device
    hipError_t ea = ensure_dynamic_lds(lds_attr, reinterpret_cast<const void *>(chain_kernel<D, ACT, MLP, QKV>), S::LDS_BYTES);
    if (ea != hipSuccess) return ea;
    // co-resident workgroups: CUs x (3 at d = 128 | 1 above), see __launch_bounds__ / LDS.  The one-, two- and three-wave workgroups
    // of d = 32 / 64 / 96 would leave the SIMDs at 0.75 / 1.5 / 2.25 waves with three per CU: as many as give twelve waves per CU and
    // fit the LDS (1 280-byte granules, section 4.0 fact 8) -- round 5: d = 64 154 k -> 166 k frames/s, d = 96 chain 0.60 -> 0.67 of
    // the roof (bench `other_shapes`)
    constexpr int kGranules = (int)((S::LDS_BYTES + 1279) / 1280);
    constexpr int kPerCu = D <= AFT_CHAIN_MANY_MAX_D ? std::min(12 / S::WAVES, 128 / kGranules) : (D <= 128 ? 3 : 1);
    const int resident = current_device_cus() * kPerCu;
    const int blocks = std::min((args.rows + 31) / 32, resident);
    const size_t lds = S::LDS_BYTES;
#ifdef AFT_DIAG_STAMPS   // phase stamps of this launch, printed on the host (never in the product build)
    StampRun run(SW_STAMPS, MLP && QKV ? kStampChainMlpQkv : MLP ? kStampChainMlp : kStampChainQkv, (args.rows + 31) / 32, st);
    ChainArgs stamped = args;
    stamped.stamps = run.buffer();
    const ChainArgs &a = stamped;
#else
    const ChainArgs &a = args;
#endif
    hipLaunchKernelGGL((chain_kernel<D, ACT, MLP, QKV>), dim3(blocks), dim3(S::THREADS), lds, st, a);
    const hipError_t e = hipGetLastError();
#ifdef AFT_DIAG_STAMPS
    if (const unsigned long long *h = run.collect()) {
        int per_cu = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, chain_kernel<D, ACT, MLP, QKV>, S::THREADS, lds);
        report_chain(stdout, h, (args.rows + 31) / 32, blocks, D, (int)MLP, (int)QKV, per_cu, lds);
    }
#endif
    return e;
}

// Packed-weight block of one layer inside the workspace (floats): [in_proj 3D*D][out_proj D*D][lin1 2D*D][lin2 D*2D]
size_t packed_layer_floats(int d) { return (size_t)8 * d * d; }

__global__ __launch_bounds__(256) void pack_weights_kernel(const WeightsDev w, float *__restrict__ packed, int d,
                                                           int num_layers, int split) {
    pack_weights_vec(w, packed, d, 0, num_layers, split, (size_t)blockIdx.x * 256 + threadIdx.x);   // one float4 of the image
}

hipError_t launch_pack_weights(const aft_config &c, const aft_layer_weights *layers, float *packed, int count, hipStream_t st) {
    for (int first = 0; first < count; first += kLayerWindow) {   // the kernel takes a window of the layer table by value
        const int n = std::min(kLayerWindow, count - first);
        WeightsDev win{};
        for (int i = 0; i < n; ++i) win.layers[i] = layers[first + i];
        const size_t vecs = packed_layer_floats(c.model_dim) * n / 4;
        hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)((vecs + 255) / 256)), dim3(256), 0, st, win,
                           packed + packed_layer_floats(c.model_dim) * first, c.model_dim, n, c.precision == AFT_PRECISION_BF16X3 ? 1 : 0);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <int D, int ACT>
static hipError_t launch_chain_t(const ChainArgs &args, bool mlp, bool qkv, hipStream_t st) {
    if (mlp && qkv) return launch_chain_v<D, ACT, true, true>(args, st);
    if (mlp) return launch_chain_v<D, ACT, true, false>(args, st);
    return launch_chain_v<D, ACT, false, true>(args, st);
}

ChainArgs make_chain_args(const aft_config &c, const aft_layer_weights *m, const float *m_packed, const aft_layer_weights *qw,
                          const float *q_packed, const float *attn, float *x, float *q, float *k, float *vt, int rows, int tokens,
                          int tokpad, const ChainFusion *fuse) {
    const size_t dd = (size_t)c.model_dim * c.model_dim;
    ChainArgs a{};
    if (fuse != nullptr && fuse->out6 != nullptr && m != nullptr && qw == nullptr) {
        a.lin2_w = fuse->lin2_w; a.lin2_b = fuse->lin2_b; a.out6 = fuse->out6;
        a.out6_features = c.patch_scs * c.patch_symbols;
        a.out6_stride = out6_stride(c);
    }
    if (fuse != nullptr && fuse->conv_enhanced != nullptr && m == nullptr) {
        a.emb_conv = fuse->conv_enhanced; a.emb_tok6 = fuse->tokens6; a.emb_w1 = fuse->lin1_w; a.emb_b1 = fuse->lin1_b;
        a.emb_pos = fuse->pos;
        a.emb_S = c.num_scs; a.emb_T = c.num_symbols; a.emb_p0 = c.patch_scs; a.emb_p1 = c.patch_symbols;
        a.emb_K = c.patch_scs * c.patch_symbols + (fuse->tokens6 ? 6 : 0);
        if (fuse->fold_tk != nullptr && c.precision == AFT_PRECISION_F32) {   // (the split tier keeps the 128-deep product: l0_fold_selected)
            a.fold_tk = fuse->fold_tk; a.fold_tvt = fuse->fold_tvt; a.fold_w = fuse->fold_w;
        }
    }
    a.attn = attn;
    a.x = x;
    a.x_blocked = fuse != nullptr && fuse->x_blocked ? 1 : 0;
    if (m != nullptr) {
        a.wo = m_packed + 3 * dd; a.bo = m->out_proj_b;
        a.w1 = m_packed + 4 * dd; a.b1 = m->lin1_b;
        a.w2 = m_packed + 6 * dd; a.b2 = m->lin2_b;
        a.g1 = m->norm1_w; a.be1 = m->norm1_b;
        a.g2 = m->norm2_w; a.be2 = m->norm2_b;
    }
    if (qw != nullptr) {
        a.wqkv = q_packed;
        a.bv = qw->in_proj_b + 2 * c.model_dim;
    }
    a.q = q; a.k = k; a.vt = vt;
    a.rows = rows; a.tokens = tokens; a.tokpad = tokpad;
    a.heads = c.model_dim / kHeadDim;   // q / k / v^T are laid out per 32-feature block, whatever the head count (attn_device.h)
    return a;
}

hipError_t launch_chain(const aft_config &c, const aft_layer_weights *m, const float *m_packed,
                        const aft_layer_weights *qw, const float *q_packed,
                        const float *attn, float *x, float *q, float *k, float *vt, int rows, int tokens,
                        int tokpad, hipStream_t st, const ChainFusion *fuse) {
    const ChainArgs a = make_chain_args(c, m, m_packed, qw, q_packed, attn, x, q, k, vt, rows, tokens, tokpad, fuse);
    const bool gelu = c.activation == AFT_ACT_GELU;
    const bool mlp = m != nullptr, qkv = qw != nullptr;
    if (c.precision == AFT_PRECISION_BF16X3) {
        if (c.model_dim == 128)
            return gelu ? launch_chain_split_t<128, AFT_ACT_GELU>(a, mlp, qkv, st) : launch_chain_split_t<128, AFT_ACT_RELU>(a, mlp, qkv, st);
        if (c.model_dim == 256)
            return gelu ? launch_chain_split_t<256, AFT_ACT_GELU>(a, mlp, qkv, st) : launch_chain_split_t<256, AFT_ACT_RELU>(a, mlp, qkv, st);
        return hipErrorInvalidValue;    // refused earlier by check_config
    }
    // every multiple of 32 up to 256 (round 5: the body is generic in D = 32 x waves; 128 and 256 are the tuned shapes, the others are
    // covered -- odd wave counts leave SIMDs unevenly filled)
#define AFT_CHAIN_DIM(DD) \
    if (c.model_dim == DD) return gelu ? launch_chain_t<DD, AFT_ACT_GELU>(a, mlp, qkv, st) : launch_chain_t<DD, AFT_ACT_RELU>(a, mlp, qkv, st);
    AFT_CHAIN_DIM(32) AFT_CHAIN_DIM(96) AFT_CHAIN_DIM(160) AFT_CHAIN_DIM(224)
#undef AFT_CHAIN_DIM
    if (c.model_dim == 64)
        return gelu ? launch_chain_t<64, AFT_ACT_GELU>(a, mlp, qkv, st) : launch_chain_t<64, AFT_ACT_RELU>(a, mlp, qkv, st);
    if (c.model_dim == 192)
        return gelu ? launch_chain_t<192, AFT_ACT_GELU>(a, mlp, qkv, st) : launch_chain_t<192, AFT_ACT_RELU>(a, mlp, qkv, st);
    if (c.model_dim == 128)
        return gelu ? launch_chain_t<128, AFT_ACT_GELU>(a, mlp, qkv, st) : launch_chain_t<128, AFT_ACT_RELU>(a, mlp, qkv, st);
    if (c.model_dim == 256)
        return gelu ? launch_chain_t<256, AFT_ACT_GELU>(a, mlp, qkv, st) : launch_chain_t<256, AFT_ACT_RELU>(a, mlp, qkv, st);
    return hipErrorInvalidValue;
}

}  // namespace aft
