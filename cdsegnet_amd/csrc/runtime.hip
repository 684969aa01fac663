// Native executor for one PTv3 Block (ref: ptv3.py:399-428; big stages: conv, fused head, attention, fused tail;
// deep stages C = 128 / 256: conv, fused head, attention, fused tail (deep.hip); C = 512 and fp32: conv, cpe linear, qkv,
// attention, proj, fc1, fc2 + their second-pass kernels): issues all launches of the block
// from C++ so the Python binding pays one call instead of ~10 (the per-launch host cost of the
// binding, ~10 us, was the step's critical path once the kernels were fast).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "deep.h"
#include "tail_outputs.h"
#include "workspace.h"

namespace {

constexpr int FUSE_LN_MAX_C = 512;  // widest row one GEMM block finishes (LayerNorm fused into the epilogue)

// storage type of a descriptor's activations / weights: CDSEG_F32X3 is fp32 in memory (split-half arithmetic, gemm.hip)
inline int storage_dtype(int dtype) { return dtype == CDSEG_F32X3 ? CDSEG_F32 : dtype; }

struct Layout {
  void *y, *h, *qkv, *o, *u, *y2, *ws, *xs;
  size_t ws_bytes, total;
};

Layout carve(const cdseg_block_desc* d, long n, void* scratch) {
  Carver c{(char*)scratch, 0};
  const size_t e = esz(d->dtype);
  const size_t C = d->channels;
  Layout L;
  L.y = c.take(n * C * e);
  L.h = c.take(n * C * e);
  L.qkv = c.take(n * 3 * C * e);
  L.o = c.take(n * C * e);
  L.u = c.take(n * (size_t)d->hidden * e);
  L.y2 = d->channels > FUSE_LN_MAX_C ? c.take(n * C * 4) : nullptr;
  // one GEMM workspace for the whole Block (workspace.h): the plain and LayerNorm-fused products are gated by the narrowest
  // (N = C) and sized for the widest (qkv or fc1); the sparse conv (N = C, gathered) may want its deep-conv planes on top
  const long wide = std::max<long>(3 * C, d->hidden);
  L.ws_bytes = std::min(GEMM_WS_CAP, std::max(gemm_ws_rule(n, C, wide, false, true), gemm_ws_rule(n, C, C, true, false)));
  L.ws = L.ws_bytes ? c.take(L.ws_bytes) : nullptr;
  // deep stages: the residual rows between the fused head and the fused tail live here (head reads x, writes xs; tail reads
  // xs, writes x), which lets the few-row launches split a tile over several workgroups (deep.hip, cdseg_*_rr2)
  L.xs = (d->dtype == CDSEG_BF16 && C >= 128 && d->head_img && d->tail_img) ? c.take(n * C * 4) : nullptr;
  L.total = align_up(c.off, 256);
  return L;
}

cdseg_gemm_args base_args(const cdseg_block_desc* d, const Layout& L, long n) {
  cdseg_gemm_args a;
  std::memset(&a, 0, sizeof(a));
  a.M = n;
  a.kvol = 1;
  a.a_dtype = storage_dtype(d->dtype);
  a.compute_dtype = d->dtype;
  a.ws = L.ws;
  a.ws_bytes = L.ws_bytes;
  a.ln_eps = d->ln_eps;
  return a;
}

}  // namespace

extern "C" size_t cdseg_block_scratch_bytes(const cdseg_block_desc* d, long n) {
  if (!d || n <= 0) return 0;
  return carve(d, n, nullptr).total;
}

static int block_forward_impl(const cdseg_block_desc* d, const cdseg_block_io* io, void* stream);

extern "C" int cdseg_block_forward(const cdseg_block_desc* d, const cdseg_block_io* io, void* stream) {
  const int rc = block_forward_impl(d, io, stream);
  if (rc != CDSEG_OK || !io->sat_counter || io->n <= 0 || d->dtype != CDSEG_BF16) return rc;  // (16-bit trunks only)
  // diagnostic (IEEE-half build): clamped values in the Block's 16-bit buffers that reach memory - conv output, q and k
  // (v may be bfloat16), attention output, shadow copy of the residual stream.  LayerNorm outputs and the MLP's hidden
  // units live inside the fused kernels and are not seen.
  const Layout L = carve(d, io->n, io->scratch);
  const int C = d->channels;
  int r;
  if ((r = cdseg_count_saturated(L.y, io->n, C, C, io->sat_counter, stream)) != CDSEG_OK) return r;
  if ((r = cdseg_count_saturated(L.qkv, io->n, 2 * C, 3 * C, io->sat_counter, stream)) != CDSEG_OK) return r;
  if ((r = cdseg_count_saturated(L.o, io->n, C, C, io->sat_counter, stream)) != CDSEG_OK) return r;
  if ((const void*)io->xc_out != (const void*)io->x)
    if ((r = cdseg_count_saturated(io->xc_out, io->n, C, C, io->sat_counter, stream)) != CDSEG_OK) return r;
  return CDSEG_OK;
}

static int block_forward_impl(const cdseg_block_desc* d, const cdseg_block_io* io, void* stream) {
  if (!d || !io || !io->x || !io->xc_in || !io->xc_out || !io->nbr || !io->gidx || !io->widx || !io->patch_start)
    return CDSEG_ERR_ARG;
  const long n = io->n;
  if (n <= 0) return CDSEG_OK;
  const int C = d->channels, T = storage_dtype(d->dtype);  // T: what the buffers hold; d->dtype: how products are computed
  if (C != d->heads * CDSEG_HEAD_DIM) return CDSEG_ERR_UNSUPPORTED;
  const Layout L = carve(d, n, io->scratch);
  if (!io->scratch || io->scratch_bytes < L.total) return CDSEG_ERR_WORKSPACE;
  const bool fuse = C <= FUSE_LN_MAX_C;
  int rc;
  static const bool fused_tail = cdseg_knob("CDSEG_FUSED_TAIL", 1) != 0 && cdseg_knob("CDSEG_FUSED_MLP", 1) != 0;
  // the register-resident tail of the wide stages (blockrr.hip) is the one launch that honours the caller's word on which
  // outputs are read: X_DEAD is a permission, the logit fields are a request - refused here, before the Block's first
  // launch, when this call ends on another tail or the head does not fit (the saturation diagnostic reads xc_out)
  const bool tail_rr = fused_tail && T == CDSEG_BF16 && (C == 32 || C == 64) && d->hidden == 4 * C && d->tail_img;
  const bool want_logits = io->logits || io->head_w || io->head_b || io->out_idx || io->num_classes || io->ld_logits;
  if (io->flags & ~CDSEG_BLOCK_X_DEAD) return CDSEG_ERR_ARG;
  if (want_logits) {
    if (!tail_rr || io->sat_counter) return CDSEG_ERR_UNSUPPORTED;
    if ((rc = tail_logits_status(C, io->num_classes, io->ld_logits, io->logits, io->head_w, io->out_idx)) != CDSEG_OK) return rc;
  }
  // what the qkv producer of this Block has already done for the attention kernel (cdseg_attention_ex): the engine folds
  // scale * log2(e) into the q rows of the weights (desc), the fused heads write v as bfloat16
  // (the fp32 attention kernel honours Q_PRESCALED too - ADVICE r5: dropping the flag here applied the softmax scale twice
  // to a descriptor with folded q weights; V_BF16 is a 16-bit-build flag and is only ever set by the fused heads below)
  int attn_flags = d->attn_flags & CDSEG_ATTN_Q_PRESCALED;

  // ---- CPE: x += LN(Linear(SubMConv3d(xc)))  [+ t bias];  h = LN1(x)      (ptv3.py:401-413)
  // (the weight-stationary kernel addresses its buffers with 32-bit offsets: inputs past those limits - 16.7 M rows at
  // C = 64 - take the gathered GEMM below, which handled them before that kernel existed)
  const bool conv_fits = n * 27 * 4 < (1l << 31) && n * (long)C * 2 < (1l << 31) - 65536;
  // (the Block head that follows is deep.hip's - decided below with the same conditions -: it can take the conv's output as raw
  // split-K slices)
  const bool deep_head_next = cdseg_knob("CDSEG_DEEP_FUSED", 1) != 0 && T == CDSEG_BF16 && (C == 128 || C == 256) &&
                              d->hidden == 4 * C && d->head_img;
  int ysplits = 1;
  const float* ypart = nullptr;
  if (d->cpe_conv_wimg && T == CDSEG_BF16 && (C == 32 || C == 64) && conv_fits) {
    // wide stages: weight-stationary register-gather conv (conv.hip)
    rc = cdseg_subm_conv3(io->xc_in, C, d->cpe_conv_wimg, (const float*)d->cpe_conv_b, io->nbr, n, C, L.y, C, stream);
    if (rc != CDSEG_OK) return rc;
  } else {
    cdseg_gemm_args a = base_args(d, L, n);
    a.A = io->xc_in; a.lda = C; a.W = d->cpe_conv_w; a.bias = d->cpe_conv_b; a.nbr = io->nbr; a.nbr_kmajor = 1; a.kvol = 27;
    a.N = C; a.K = C; a.out = L.y; a.ldo = C; a.out_dtype = T;
    // few-row deep stages (a single scene): the conv runs split-K, and its second pass - sum the slices, add the bias, round -
    // is what the deep Block head's tile load can do on its way into LDS: the raw slices stay in the workspace, one launch and
    // one round trip of y fewer per Block (round 6; C = 128 / 256 - at C = 512 three workgroups per tile would each re-read
    // ~0.8 MB of slices; not with the saturation diagnostic, which reads y)
    static const bool partials_on = cdseg_knob("CDSEG_CONV_PARTIALS", 1) != 0;
    if (partials_on && deep_head_next && (C == 128 || C == 256) && !io->sat_counter && a.ws && a.bias) {
      if ((rc = gemm_leave_partials(&a, &ysplits, stream)) != CDSEG_OK) return rc;
      if (ysplits > 1) ypart = (const float*)a.ws;
    } else if ((rc = cdseg_gemm(&a, stream)) != CDSEG_OK) {
      return rc;
    }
  }
  static const bool fused_head = cdseg_knob("CDSEG_FUSED_HEAD", 1) != 0;
  // deep stages (C = 128 / 256) with weight-stream images: head and tail are one launch each (deep.hip)
  static const bool deep_on = cdseg_knob("CDSEG_DEEP_FUSED", 1) != 0;
  // C = 512: a workgroup streams the Block's whole weight set (2 + 4.7 MB) through ONE CU at ~85 GB/s, ~58 us whatever the
  // row count - a win from ~2.5 k rows (8 collated scenes: 6.2 k rows, head 51 -> 35 us, tail 85 -> 61 us), a loss on a single
  // scene's 800 rows (tail 42 -> 56 us; profiles/r05_deep512.txt).  Round 6: below that row count the tile's weight stream is
  // cut over 3 / 4 workgroups (cdseg_*_rr2, residual rows ping-ponged through the scratch arena), which needs L.xs
  static const long deep512_min = cdseg_knob("CDSEG_DEEP512_MIN_ROWS", CDSEG_DEEP512_MIN_ROWS);
  static const bool deep512_split = cdseg_knob("CDSEG_DEEP_SPLIT", 1) != 0;
  const bool deep = deep_on && T == CDSEG_BF16 &&
                    (C == 128 || C == 256 || (C == 512 && (n >= deep512_min || (deep512_split && L.xs)))) && d->hidden == 4 * C;
  const bool head = (fused_head && T == CDSEG_BF16 && (C == 32 || C == 64)) || (deep && d->head_img);
  const bool pingpong = deep && d->head_img && d->tail_img && L.xs;
  if (ypart) {  // (deep_head_next held: the head below is deep.hip's; x -> xs when the ping-pong buffer exists, else in place)
    float* xo = pingpong ? (float*)L.xs : (float*)io->x;
    if ((rc = deep_head(L.y, C, d->head_img, (const float*)d->cpe_lin_b, (const float*)d->cpe_ln_g, (const float*)d->cpe_ln_b,
                        (const float*)io->x, C, xo, C, (const float*)io->tbias, (const float*)d->norm1_g,
                        (const float*)d->norm1_b, d->ln_eps, (const float*)d->qkv_b, L.qkv, 3 * C, n, C, CDSEG_ATTN_V_BF16,
                        (hipStream_t)stream, ypart, ysplits, (const float*)d->cpe_conv_b)) != CDSEG_OK)
      return rc;
    attn_flags |= CDSEG_ATTN_V_BF16;
  } else if (pingpong) {
    if ((rc = cdseg_cpe_head_rr2(L.y, C, d->head_img, (const float*)d->cpe_lin_b, (const float*)d->cpe_ln_g,
                                 (const float*)d->cpe_ln_b, (const float*)io->x, C, (float*)L.xs, C, (const float*)io->tbias,
                                 (const float*)d->norm1_g, (const float*)d->norm1_b, d->ln_eps, (const float*)d->qkv_b, L.qkv,
                                 3 * C, n, C, CDSEG_ATTN_V_BF16, stream)) != CDSEG_OK)
      return rc;
    attn_flags |= CDSEG_ATTN_V_BF16;
  } else if (head && d->head_img) {
    // wide stages: weights resident in LDS, activations in registers (blockrr.hip)
    if ((rc = cdseg_cpe_head_rr(L.y, C, d->head_img, (const float*)d->cpe_lin_b, (const float*)d->cpe_ln_g,
                                (const float*)d->cpe_ln_b, (float*)io->x, C, (const float*)io->tbias,
                                (const float*)d->norm1_g, (const float*)d->norm1_b, d->ln_eps, (const float*)d->qkv_b, L.qkv,
                                3 * C, n, C, deep ? CDSEG_ATTN_V_BF16 : 0, stream)) != CDSEG_OK)
      return rc;
    if (deep) attn_flags |= CDSEG_ATTN_V_BF16;
  } else if (head) {
    // big stages: cpe linear + LN + residual (+ t bias) + LN1 + qkv in one launch (mlp.hip); h never leaves the CU
    if ((rc = cdseg_cpe_head_fused(L.y, C, d->cpe_lin_w, (const float*)d->cpe_lin_b, (const float*)d->cpe_ln_g,
                                   (const float*)d->cpe_ln_b, (float*)io->x, C, (const float*)io->tbias,
                                   (const float*)d->norm1_g, (const float*)d->norm1_b, d->ln_eps, d->qkv_w,
                                   (const float*)d->qkv_b, L.qkv, 3 * C, n, C, T, CDSEG_ATTN_V_BF16, stream)) != CDSEG_OK)
      return rc;
    attn_flags |= CDSEG_ATTN_V_BF16;
  } else if (fuse) {
    cdseg_gemm_args a = base_args(d, L, n);
    a.A = L.y; a.lda = C; a.W = d->cpe_lin_w; a.bias = d->cpe_lin_b; a.N = C; a.K = C;
    a.ln_pre_g = d->cpe_ln_g; a.ln_pre_b = d->cpe_ln_b; a.res = io->x; a.ldres = C; a.colbias = io->tbias;
    a.out = io->x; a.ldo = C; a.out_dtype = CDSEG_F32;
    a.ln_post_g = d->norm1_g; a.ln_post_b = d->norm1_b; a.ln_out = L.h; a.ldln = C; a.ln_out_dtype = T;
    if ((rc = cdseg_gemm(&a, stream)) != CDSEG_OK) return rc;
  } else {
    cdseg_gemm_args a = base_args(d, L, n);
    a.A = L.y; a.lda = C; a.W = d->cpe_lin_w; a.bias = d->cpe_lin_b; a.N = C; a.K = C;
    a.out = L.y2; a.ldo = C; a.out_dtype = CDSEG_F32;
    if ((rc = cdseg_gemm(&a, stream)) != CDSEG_OK) return rc;
    if ((rc = cdseg_layernorm(L.y2, CDSEG_F32, C, d->cpe_ln_g, d->cpe_ln_b, d->ln_eps, io->x, C, io->tbias, io->x,
                              CDSEG_F32, C, nullptr, 0, 0, n, C, stream)) != CDSEG_OK)
      return rc;
    if ((rc = cdseg_layernorm(io->x, CDSEG_F32, C, d->norm1_g, d->norm1_b, d->ln_eps, nullptr, 0, nullptr, L.h, T, C,
                              nullptr, 0, 0, n, C, stream)) != CDSEG_OK)
      return rc;
  }
  // ---- attention: x += proj(attn(qkv(h)));  h = LN2(x)                    (ptv3.py:413-421)
  if (!head) {
    cdseg_gemm_args a = base_args(d, L, n);
    a.A = L.h; a.lda = C; a.W = d->qkv_w; a.bias = d->qkv_b; a.N = 3 * C; a.K = C;
    a.out = L.qkv; a.ldo = 3 * C; a.out_dtype = T;
    if ((rc = cdseg_gemm(&a, stream)) != CDSEG_OK) return rc;
  }
  {
    const size_t e = esz(T);
    const char* q = (const char*)L.qkv;
    if ((rc = cdseg_attention_ex(q, q + (size_t)C * e, q + (size_t)2 * C * e, 3 * C, 3 * C, 3 * C, io->gidx, io->gidx,
                                 io->widx, io->patch_start, io->num_patches, d->heads, io->max_len, d->attn_scale, L.o, C,
                                 d->dtype, attn_flags, stream)) != CDSEG_OK)
      return rc;
  }
  if (pingpong) {
    void* xc = (const void*)io->xc_out != (const void*)io->x ? io->xc_out : nullptr;
    return cdseg_attn_tail_rr2(L.o, C, d->tail_img, (const float*)d->proj_b, (const float*)d->norm2_g, (const float*)d->norm2_b,
                               d->ln_eps, (const float*)d->fc1_b, (const float*)d->fc2_b, (const float*)L.xs, C, (float*)io->x,
                               C, xc, C, n, C, L.ws, L.ws_bytes, stream);
  }
  if (deep && d->tail_img) {
    void* xc = (const void*)io->xc_out != (const void*)io->x ? io->xc_out : nullptr;
    return cdseg_attn_tail_rr(L.o, C, d->tail_img, (const float*)d->proj_b, (const float*)d->norm2_g, (const float*)d->norm2_b,
                              d->ln_eps, (const float*)d->fc1_b, (const float*)d->fc2_b, (float*)io->x, C, xc, C, n, C, stream);
  }
  if (fused_tail && T == CDSEG_BF16 && (C == 32 || C == 64) && d->hidden == 4 * C) {
    // big stages: proj + residual + LN2 + MLP in one launch; h and the hidden activation never leave the CU
    void* xc = (const void*)io->xc_out != (const void*)io->x ? io->xc_out : nullptr;
    if (d->tail_img)  // weights resident in LDS, activations in registers (blockrr.hip); without a 16-bit copy x is all
                      // there is of the Block's output: the permission to leave it unwritten does not apply
      return cdseg_attn_tail_rr_ex(L.o, C, d->tail_img, (const float*)d->proj_b, (const float*)d->norm2_g,
                                   (const float*)d->norm2_b, d->ln_eps, (const float*)d->fc1_b, (const float*)d->fc2_b,
                                   (float*)io->x, C, xc, C, n, C, xc ? (io->flags & CDSEG_BLOCK_X_DEAD) : 0, io->logits,
                                   io->ld_logits, io->head_w, io->head_b, io->out_idx, io->num_classes, stream);
    return cdseg_attn_tail_fused(L.o, C, d->proj_w, (const float*)d->proj_b, (const float*)d->norm2_g,
                                 (const float*)d->norm2_b, d->ln_eps, d->fc1_w, (const float*)d->fc1_b, d->fc2_w,
                                 (const float*)d->fc2_b, (float*)io->x, C, xc, C, n, C, T, stream);
  }
  {
    cdseg_gemm_args a = base_args(d, L, n);
    a.A = L.o; a.lda = C; a.W = d->proj_w; a.bias = d->proj_b; a.N = C; a.K = C;
    a.res = io->x; a.ldres = C; a.out = io->x; a.ldo = C; a.out_dtype = CDSEG_F32;
    if (fuse) {
      a.ln_post_g = d->norm2_g; a.ln_post_b = d->norm2_b; a.ln_out = L.h; a.ldln = C; a.ln_out_dtype = T;
    }
    if ((rc = cdseg_gemm(&a, stream)) != CDSEG_OK) return rc;
    if (!fuse &&
        (rc = cdseg_layernorm(io->x, CDSEG_F32, C, d->norm2_g, d->norm2_b, d->ln_eps, nullptr, 0, nullptr, L.h, T, C,
                              nullptr, 0, 0, n, C, stream)) != CDSEG_OK)
      return rc;
  }
  // ---- MLP: x += fc2(GELU(fc1(h)));  xc = T(x)                            (ptv3.py:423-427)
  static const bool fused_mlp = cdseg_knob("CDSEG_FUSED_MLP", 1) != 0;
  static const int fused_maxc = cdseg_knob("CDSEG_FUSED_MLP_MAXC", 128);
  if (fused_mlp && T == CDSEG_BF16 && (C == 32 || C == 64 || C == 128) && C <= fused_maxc && d->hidden == 4 * C) {
    // big stages: one kernel, the 4C hidden activation stays in LDS (mlp.hip)
    void* xc = (const void*)io->xc_out != (const void*)io->x ? io->xc_out : nullptr;
    if ((rc = cdseg_mlp_fused(L.h, C, d->fc1_w, (const float*)d->fc1_b, d->fc2_w, (const float*)d->fc2_b, (float*)io->x, C,
                              xc, C, n, C, T, stream)) != CDSEG_OK)
      return rc;
    return CDSEG_OK;
  }
  {
    cdseg_gemm_args a = base_args(d, L, n);
    a.A = L.h; a.lda = C; a.W = d->fc1_w; a.bias = d->fc1_b; a.N = d->hidden; a.K = C; a.act = CDSEG_ACT_GELU;
    a.out = L.u; a.ldo = d->hidden; a.out_dtype = T;
    if ((rc = cdseg_gemm(&a, stream)) != CDSEG_OK) return rc;
  }
  {
    cdseg_gemm_args a = base_args(d, L, n);
    a.A = L.u; a.lda = d->hidden; a.W = d->fc2_w; a.bias = d->fc2_b; a.N = C; a.K = d->hidden;
    a.res = io->x; a.ldres = C; a.out = io->x; a.ldo = C; a.out_dtype = CDSEG_F32;
    if ((const void*)io->xc_out != (const void*)io->x) {
      a.out2 = io->xc_out; a.ldo2 = C; a.out2_dtype = T;
    }
    if ((rc = cdseg_gemm(&a, stream)) != CDSEG_OK) return rc;
  }
  return CDSEG_OK;
}
