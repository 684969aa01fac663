// Launch record of the C ABI (include/cdseg.h: cdseg_route_enable / _clear / _read / _catalog): which kernel each host-side
// chooser picked, per host thread.  Host code only.  Off by default: a recording site then costs one thread-local test.
//
// ONE table names every kernel a chooser can launch; a kernel id is an index into it.  The recording sites take their ids
// from this table (the GEMM arms and the other template arms by a compile-time search on their template arguments, the rest by
// enumerator), and
// cdseg_route_catalog prints it: the catalogue cannot list a kernel the code does not name, nor the reverse.
#pragma once
#include <stdint.h>

#include "../../include/cdseg.h"

// record: 8 int32 (layout and flag bits: include/cdseg.h)
#define CDSEG_ROUTE_ID 0
#define CDSEG_ROUTE_BM 1
#define CDSEG_ROUTE_BN 2
#define CDSEG_ROUTE_SPLITS 3
#define CDSEG_ROUTE_FIX 4
#define CDSEG_ROUTE_XMODE 5
#define CDSEG_ROUTE_FLAGS 6
#define CDSEG_ROUTE_AUX 7

// gemm_kernel<CT, BN, NCH, GATHER, BM> instantiations of launch_bn: ct (b16 = the build's 16-bit type), column tile, K step class
// (kshort: the whole reduction is at most 64 long), plain / gather, row tile
#define CDSEG_RG_BN(X, ct, k, g, bm) X(ct, 32, k, g, bm) X(ct, 64, k, g, bm) X(ct, 128, k, g, bm)
#define CDSEG_RG_CT(X, ct)                                                                                    \
  CDSEG_RG_BN(X, ct, kshort, plain, 64) CDSEG_RG_BN(X, ct, kshort, gather, 64) CDSEG_RG_BN(X, ct, klong, plain, 64) \
  CDSEG_RG_BN(X, ct, klong, gather, 64) CDSEG_RG_BN(X, ct, klong, gather, 128)
#define CDSEG_ROUTE_GEMM_KERNELS(X)                                                          \
  CDSEG_RG_CT(X, b16) CDSEG_RG_CT(X, f32) CDSEG_RG_CT(X, x3)                                 \
  CDSEG_RG_BN(X, x3, kshort, plain, 128) CDSEG_RG_BN(X, x3, klong, plain, 128) X(b16, 128, klong, gather, 256)
// gemm_dma_kernel<BM, GATHER, BN, stages, SQ> instantiations: row tile, plain / gather, column tile, ring stages, the 8-wave
// square loop or not
#define CDSEG_ROUTE_DMA_KERNELS(Y)                                                                              \
  Y(64, plain, 128, 2, ring) Y(128, plain, 128, 2, ring) Y(256, plain, 128, 2, ring) Y(64, gather, 128, 2, ring) \
  Y(128, gather, 128, 2, ring) Y(256, gather, 128, 2, ring) Y(128, gather, 256, 3, ring) Y(256, gather, 256, 2, sq) \
  Y(256, gather, 128, 2, sq)
// every other chooser: enumerator, name
#define CDSEG_ROUTE_OTHER_KERNELS(Z)                                  \
  Z(MLP_32_64, "mlp_fused_kernel<32,64,mlp,64>")                      \
  Z(MLP_64_64, "mlp_fused_kernel<64,64,mlp,64>")                      \
  Z(MLP_128_64, "mlp_fused_kernel<128,64,mlp,64>")                    \
  Z(MLP_128_128, "mlp_fused_kernel<128,64,mlp,128>")                  \
  Z(TAIL_32_64, "mlp_fused_kernel<32,64,proj,64>")                    \
  Z(TAIL_64_64, "mlp_fused_kernel<64,64,proj,64>")                    \
  Z(HEAD_STREAM_32, "cpe_head_stream_kernel<32>")                     \
  Z(HEAD_STREAM_64, "cpe_head_stream_kernel<64>")                     \
  Z(HEAD_32_128, "cpe_head_fused_kernel<32,128>")                     \
  Z(HEAD_64_128, "cpe_head_fused_kernel<64,128>")                     \
  Z(HEAD_32_64, "cpe_head_fused_kernel<32,64>")                       \
  Z(HEAD_64_64, "cpe_head_fused_kernel<64,64>")                       \
  Z(DEEP_HEAD_128_128, "deep_head_kernel<128,128,1>")                 \
  Z(DEEP_HEAD_128_32, "deep_head_kernel<128,32,1>")                   \
  Z(DEEP_HEAD_256_128, "deep_head_kernel<256,128,1>")                 \
  Z(DEEP_HEAD_256_32, "deep_head_kernel<256,32,1>")                   \
  Z(DEEP_HEAD_512_64, "deep_head_kernel<512,64,2>")                   \
  Z(DEEP_HEAD_512_32, "deep_head_kernel<512,32,1>")                   \
  Z(DEEP_TAIL_128_128, "deep_tail_kernel<128,128,1>")                 \
  Z(DEEP_TAIL_128_32, "deep_tail_kernel<128,32,1>")                   \
  Z(DEEP_TAIL_256_128, "deep_tail_kernel<256,128,1>")                 \
  Z(DEEP_TAIL_256_32, "deep_tail_kernel<256,32,1>")                   \
  Z(DEEP_TAIL_512_64, "deep_tail_kernel<512,64,2>")                   \
  Z(DEEP_TAIL_512_32, "deep_tail_kernel<512,32,1>")                   \
  Z(HEAD_RR_32, "head_rr_kernel<32>")                                 \
  Z(HEAD_RR_64, "head_rr_kernel<64>")                                 \
  Z(TAIL_RR_32, "tail_rr_kernel<32>")                                 \
  Z(TAIL_RR_64, "tail_rr_kernel<64>")                                 \
  Z(CONV_LL_32, "conv_ll_kernel<32>")                                 \
  Z(CONV_LL_64, "conv_ll_kernel<64>")                                 \
  Z(CONV_LL_32_F32, "conv_ll_kernel<32>:f32out")                      \
  Z(CONV_LL_64_F32, "conv_ll_kernel<64>:f32out")                      \
  Z(ATTN_B16, "attn_bf16_kernel<narrow>")                             \
  Z(ATTN_B16_WIDE, "attn_bf16_kernel<16>")                            \
  Z(ATTN_X3, "attn_x3_kernel")                                        \
  Z(ATTN_F32, "attn_f32_kernel")                                      \
  Z(ATTN_DROP_F32, "attn_drop_f32_kernel")                            \
  Z(ATTN_DROP_B16, "attn_drop16_kernel")                              \
  Z(ATTN_BWD_Q_DROP, "attn_bwd_q_mfma_kernel<DropP>")                 \
  Z(ATTN_BWD_KV_DROP, "attn_bwd_kv_mfma_kernel<DropP>")               \
  Z(ATTN_BWD16_Q_DROP, "attn_bwd16_q_kernel<DropP>")                  \
  Z(ATTN_BWD16_KV_DROP, "attn_bwd16_kv_kernel<DropP>")                \
  Z(DROPOUT_F32, "dropout_kernel")                                    \
  Z(ATTN_BWD_Q, "attn_bwd_q_mfma_kernel<>")                           \
  Z(ATTN_BWD_KV, "attn_bwd_kv_mfma_kernel<>")                         \
  Z(ATTN_BWD16_Q, "attn_bwd16_q_kernel<>")                            \
  Z(ATTN_BWD16_KV, "attn_bwd16_kv_kernel<>")                          \
  Z(WGRAD, "wgrad_kernel")                                            \
  Z(WGRAD_DET, "wgrad_det_kernel")                                    \
  Z(LN_BWD, "layernorm_bwd_kernel")                                   \
  Z(LN_BWD_DET, "layernorm_bwd_det_kernel")                           \
  Z(GATHER_FIRST_B16, "gather_first_kernel<b16>")                     \
  Z(GATHER_FIRST_F32, "gather_first_kernel<f32>")                     \
  Z(SCATTER_FIRST_ACC, "scatter_first_kernel<acc>")                   \
  Z(SCATTER_FIRST_SET, "scatter_first_kernel<set>")                   \
  Z(SCALE_CAST_B16, "scale_cast_kernel<b16>")                         \
  Z(SCALE_CAST_F32, "scale_cast_kernel<f32>")                         \
  Z(GELU_FWD_B16, "gelu_fwd_kernel<b16>")                             \
  Z(GELU_FWD_F32, "gelu_fwd_kernel<f32>")                             \
  Z(GELU_BWD_CAST_B16, "gelu_bwd_cast_kernel<b16>")                   \
  Z(GELU_BWD_CAST_F32, "gelu_bwd_cast_kernel<f32>")                   \
  Z(SK_STATS_B16, "sk_stats_kernel<b16>")                             \
  Z(SK_STATS_F32, "sk_stats_kernel<f32>")                             \
  Z(SK_STATS_SCALAR_B16, "sk_stats_scalar_kernel<b16>")               \
  Z(SK_STATS_SCALAR_F32, "sk_stats_scalar_kernel<f32>")               \
  Z(SK_FOLD_B16, "sk_fold_kernel<b16>")                               \
  Z(SK_FOLD_F32, "sk_fold_kernel<f32>")                               \
  Z(SK_MERGE, "sk_merge_kernel")                                      \
  Z(SK_MERGE_SCALAR, "sk_merge_scalar_kernel")                        \
  Z(FG_FWD, "fg_fwd_kernel")                                          \
  Z(FG_FWD_SCALAR, "fg_fwd_scalar_kernel")                            \
  Z(FG_BWD, "fg_bwd_kernel")                                          \
  Z(FG_BWD_SCALAR, "fg_bwd_scalar_kernel")
// the choosers outside the GEMM whose arms are template arguments: family, up to three arguments, name.  Their recording sites
// find the id by a compile-time search on (family, arguments), like the GEMM arms
#define CDSEG_ROUTE_TEMPLATE_KERNELS(T)                                                                       \
  T(LN, 1, 0, 0, "layernorm_kernel<1>") T(LN, 2, 0, 0, "layernorm_kernel<2>")                                 \
  T(LN, 4, 0, 0, "layernorm_kernel<4>") T(LN, 8, 0, 0, "layernorm_kernel<8>")                                 \
  T(ADD_LN, 1, 1, 0, "add_layernorm_kernel<1,b16>") T(ADD_LN, 1, 0, 0, "add_layernorm_kernel<1,f32>")         \
  T(ADD_LN, 2, 1, 0, "add_layernorm_kernel<2,b16>") T(ADD_LN, 2, 0, 0, "add_layernorm_kernel<2,f32>")         \
  T(ADD_LN, 4, 1, 0, "add_layernorm_kernel<4,b16>") T(ADD_LN, 4, 0, 0, "add_layernorm_kernel<4,f32>")         \
  T(ADD_LN, 8, 1, 0, "add_layernorm_kernel<8,b16>") T(ADD_LN, 8, 0, 0, "add_layernorm_kernel<8,f32>")         \
  T(WGRAD16, 1, 1, 0, "wgrad16_kernel<1,1>") T(WGRAD16, 1, 2, 0, "wgrad16_kernel<1,2>")                       \
  T(WGRAD16, 1, 4, 0, "wgrad16_kernel<1,4>") T(WGRAD16, 2, 1, 0, "wgrad16_kernel<2,1>")                       \
  T(WGRAD16, 2, 2, 0, "wgrad16_kernel<2,2>") T(WGRAD16, 2, 4, 0, "wgrad16_kernel<2,4>")                       \
  T(WGRAD16, 4, 1, 0, "wgrad16_kernel<4,1>") T(WGRAD16, 4, 2, 0, "wgrad16_kernel<4,2>")                       \
  T(WGRAD16, 1, 1, 1, "wgrad16_det_kernel<1,1>") T(WGRAD16, 1, 2, 1, "wgrad16_det_kernel<1,2>")               \
  T(WGRAD16, 1, 4, 1, "wgrad16_det_kernel<1,4>") T(WGRAD16, 2, 1, 1, "wgrad16_det_kernel<2,1>")               \
  T(WGRAD16, 2, 2, 1, "wgrad16_det_kernel<2,2>") T(WGRAD16, 2, 4, 1, "wgrad16_det_kernel<2,4>")               \
  T(WGRAD16, 4, 1, 1, "wgrad16_det_kernel<4,1>") T(WGRAD16, 4, 2, 1, "wgrad16_det_kernel<4,2>")               \
  T(POOL, 32, 64, 0, "pool_fused_kernel<32,64,walk>") T(POOL, 32, 64, 1, "pool_fused_kernel<32,64,scan>")     \
  T(POOL, 64, 128, 0, "pool_fused_kernel<64,128,walk>") T(POOL, 64, 128, 1, "pool_fused_kernel<64,128,scan>") \
  T(UNPOOL, 32, 64, 0, "unpool_fused_kernel<32,64>") T(UNPOOL, 64, 128, 0, "unpool_fused_kernel<64,128>")     \
  T(LOSS, 16, 1, 0, "loss_rows_kernel<16,1>") T(LOSS, 16, 2, 0, "loss_rows_kernel<16,2>")                     \
  T(LOSS, 64, 1, 0, "loss_rows_kernel<64,1>") T(LOSS, 64, 2, 0, "loss_rows_kernel<64,2>")                     \
  T(LOSS, 64, 4, 0, "loss_rows_kernel<64,4>")                                                                 \
  T(LOSS, 16, 1, 1, "loss_bwd_kernel<16,1>") T(LOSS, 16, 2, 1, "loss_bwd_kernel<16,2>")                       \
  T(LOSS, 64, 1, 1, "loss_bwd_kernel<64,1>") T(LOSS, 64, 2, 1, "loss_bwd_kernel<64,2>")                       \
  T(LOSS, 64, 4, 1, "loss_bwd_kernel<64,4>")

enum {
  CDSEG_RT_b16 = 0, CDSEG_RT_f32 = 1, CDSEG_RT_x3 = 2,
  CDSEG_RT_kshort = 0, CDSEG_RT_klong = 1,
  CDSEG_RT_plain = 0, CDSEG_RT_gather = 1,
  CDSEG_RT_ring = 0, CDSEG_RT_sq = 1,
  // families of CDSEG_ROUTE_TEMPLATE_KERNELS
  CDSEG_RF_LN = 0, CDSEG_RF_ADD_LN = 1, CDSEG_RF_WGRAD16 = 2, CDSEG_RF_POOL = 3, CDSEG_RF_UNPOOL = 4, CDSEG_RF_LOSS = 5,
};

struct CdsegRouteEntry {
  const char* name;
  int key;  // GEMM and template arms: their template arguments, packed (0 for the kernels addressed by enumerator)
};

constexpr int cdseg_route_gemm_key(int ct, int bn, int klong, int gather, int bm) {
  return (1 << 28) | (ct << 24) | (klong << 23) | (gather << 22) | ((bn / 32) << 12) | (bm / 32);
}
constexpr int cdseg_route_dma_key(int bm, int gather, int bn, int stages, int sq) {
  return (2 << 28) | (stages << 24) | (sq << 23) | (gather << 22) | ((bn / 32) << 12) | (bm / 32);
}
constexpr int cdseg_route_template_key(int family, int a, int b, int c) {
  return (3 << 28) | (family << 24) | (a << 12) | (b << 4) | c;  // a <= 64, b <= 128, c <= 1
}

inline constexpr CdsegRouteEntry kCdsegRouteTable[] = {
#define CDSEG_RX(ct, bn, k, g, bm) \
  {"gemm_kernel<" #ct "," #bn "," #k "," #g "," #bm ">", cdseg_route_gemm_key(CDSEG_RT_##ct, bn, CDSEG_RT_##k, CDSEG_RT_##g, bm)},
    CDSEG_ROUTE_GEMM_KERNELS(CDSEG_RX)
#undef CDSEG_RX
#define CDSEG_RY(bm, g, bn, st, sq) \
  {"gemm_dma_kernel<" #bm "," #g "," #bn "," #st "," #sq ">", cdseg_route_dma_key(bm, CDSEG_RT_##g, bn, st, CDSEG_RT_##sq)},
    CDSEG_ROUTE_DMA_KERNELS(CDSEG_RY)
#undef CDSEG_RY
#define CDSEG_RZ(sym, name) {name, 0},
    CDSEG_ROUTE_OTHER_KERNELS(CDSEG_RZ)
#undef CDSEG_RZ
#define CDSEG_RT(fam, a, b, c, name) {name, cdseg_route_template_key(CDSEG_RF_##fam, a, b, c)},
    CDSEG_ROUTE_TEMPLATE_KERNELS(CDSEG_RT)
#undef CDSEG_RT
};
constexpr int kCdsegRouteCount = (int)(sizeof(kCdsegRouteTable) / sizeof(kCdsegRouteTable[0]));

constexpr int cdseg_route_find(int key) {
  for (int i = 0; i < kCdsegRouteCount; ++i)
    if (kCdsegRouteTable[i].key == key) return i;
  return -1;
}

// enumerators of the kernels addressed by name: CDSEG_RK_<sym> = their index in the table
enum {
#define CDSEG_RX(ct, bn, k, g, bm) CDSEG_RK_G_##ct##_##bn##_##k##_##g##_##bm,
  CDSEG_ROUTE_GEMM_KERNELS(CDSEG_RX)
#undef CDSEG_RX
#define CDSEG_RY(bm, g, bn, st, sq) CDSEG_RK_D_##bm##_##g##_##bn##_##st##_##sq,
  CDSEG_ROUTE_DMA_KERNELS(CDSEG_RY)
#undef CDSEG_RY
#define CDSEG_RZ(sym, name) CDSEG_RK_##sym,
  CDSEG_ROUTE_OTHER_KERNELS(CDSEG_RZ)
#undef CDSEG_RZ
#define CDSEG_RT(fam, a, b, c, name) CDSEG_RK_T_##fam##_##a##_##b##_##c,
  CDSEG_ROUTE_TEMPLATE_KERNELS(CDSEG_RT)
#undef CDSEG_RT
  CDSEG_RK_COUNT
};
static_assert(CDSEG_RK_COUNT == kCdsegRouteCount, "one table");

// ids of the GEMM arms from their template arguments; a launch arm whose instantiation the table lacks does not compile
template <int CT, int BN, bool KLONG, bool GATHER, int BM>
constexpr int cdseg_route_gemm_id() {
  constexpr int id = cdseg_route_find(cdseg_route_gemm_key(CT, BN, KLONG, GATHER, BM));
  static_assert(id >= 0, "gemm_kernel instantiation missing from CDSEG_ROUTE_GEMM_KERNELS");
  return id;
}
template <int BM, bool GATHER, int BN = 128, int STAGES = 2, bool SQ = false>
constexpr int cdseg_route_dma_id() {
  constexpr int id = cdseg_route_find(cdseg_route_dma_key(BM, GATHER, BN, STAGES, SQ));
  static_assert(id >= 0, "gemm_dma_kernel instantiation missing from CDSEG_ROUTE_DMA_KERNELS");
  return id;
}
// ids of the template arms outside the GEMM, the same way
template <int FAMILY, int A, int B = 0, int C = 0>
constexpr int cdseg_route_template_id() {
  constexpr int id = cdseg_route_find(cdseg_route_template_key(FAMILY, A, B, C));
  static_assert(id >= 0, "kernel instantiation missing from CDSEG_ROUTE_TEMPLATE_KERNELS");
  return id;
}

extern thread_local bool tl_cdseg_route_on;
void cdseg_route_push(int id, int bm, int bn, int splits, int fix, int xmode, int flags, int aux);
void cdseg_route_or_flags(int flags);  // into the newest record of this thread

// rows per split of a weight-gradient launch, for the xmode word of its record
constexpr int cdseg_route_rows(long rows) { return rows > 0x7fffffffL ? 0x7fffffff : (int)rows; }

// the recording site: immediately before the hipLaunchKernelGGL it describes
static inline void cdseg_route_rec(int id, int bm, int bn, int splits, int fix, int xmode, int flags, int aux) {
  if (tl_cdseg_route_on) cdseg_route_push(id, bm, bn, splits, fix, xmode, flags, aux);
}
