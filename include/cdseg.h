/* cdseg.h - C ABI of libcdseg_hip.so: the MI355X (gfx950) kernels behind CDSegNet's
 * single-step-inference hot path.
 *
 * Drop-in boundary.  The reference (a Python program on PyTorch) reaches its fused
 * arithmetic through third-party Python ops; each entry point below is what a binding
 * for that call site would bind (plain device pointers + sizes, no torch types), and
 * cdsegnet_amd/ops.py is the ctypes binding the build ships (INTEGRATION.md shows the
 * equivalent stubs on the reference side).  "ref:" cites the reference interface
 * replaced, relative to /root/reference/pointcept/.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the name ends in _host;
 *  - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *  - every function is asynchronous on `stream`, returns CDSEG_OK (0) or a negative
 *    CDSEG_ERR_* code, and never allocates (callers own all buffers and workspaces);
 *  - dtypes: CDSEG_F32 = float32, CDSEG_BF16 = the build's 16-bit type as raw uint16 bits: bfloat16 in libcdseg_hip.so,
 *    IEEE half in libcdseg_hip_f16.so (the same sources compiled with -DCDSEG_LP_F16; float -> half conversions saturate
 *    at +-65504).  Same entry points, same signatures: a caller picks the library that matches its tensors' dtype;
 *  - index arrays are int32 unless stated; codes are int64 (non-negative).
 *  - attention head dimension is 16 (every stage of every shipped config: C/H = 16).
 */
#ifndef CDSEG_H
#define CDSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CDSEG_OK 0
#define CDSEG_ERR_ARG (-1)
#define CDSEG_ERR_LAUNCH (-2)
#define CDSEG_ERR_WORKSPACE (-3)
#define CDSEG_ERR_UNSUPPORTED (-4)

#define CDSEG_F32 0
#define CDSEG_BF16 1
/* compute type only (cdseg_gemm compute_dtype, cdseg_attention_ex dtype, cdseg_block_desc dtype): fp32 tensors in memory, every
 * product as three IEEE-half MFMAs on split operands (x ~= hi + lo' / 2048), fp32 accumulation - csrc/gemm.hip "fp32 x3" */
#define CDSEG_F32X3 2

#define CDSEG_ORDER_Z 0
#define CDSEG_ORDER_Z_TRANS 1
#define CDSEG_ORDER_HILBERT 2
#define CDSEG_ORDER_HILBERT_TRANS 3

#define CDSEG_ACT_NONE 0
#define CDSEG_ACT_GELU 1  /* exact erf GELU (nn.GELU()) */
#define CDSEG_ACT_SWISH 2 /* x * sigmoid(x), ref: models/point_transformer_v3/point_transformer_v3m1_base.py:30-31 */

#define CDSEG_HEAD_DIM 16
#ifndef CDSEG_DEEP512_MIN_ROWS
#define CDSEG_DEEP512_MIN_ROWS 2560 /* C = 512 Blocks with fewer rows keep the separate GEMM launches (csrc/runtime.hip) */
#endif
#define CDSEG_MAX_PATCH 1024

/* library / device identification (host-only helpers) */
int cdseg_abi_version(void);
const char* cdseg_build_info(void);

/* ------------------------------------------------------------------ serialization
 * ref: models/utils/structure.py:47-102 (Point.serialization),
 *      models/utils/serialization/default.py:8-24 (encode), z_order.py:66-101, hilbert.py:91-198 */

/* max over all grid coordinates -> *out_dev (int64); depth = bit_length(max).  ref: structure.py:66 */
int cdseg_grid_max(const void* grid, int elem_bytes, long n3, int64_t* out_dev, void* stream);
/* batch[i] = index of the batch element owning point i.  ref: models/utils/misc.py:18-23 (offset2batch) */
int cdseg_offset2batch(const int64_t* offset, int nb, long n, int32_t* batch, void* stream);
/* code[i] = (batch[i] << 3*depth) | curve_key(order_id, grid[i]).  grid (n,3) int32|int64,
 * batch int32|int64 or NULL.  ref: serialization/default.py:8-24 */
int cdseg_encode(const void* grid, int grid_elem_bytes, const void* batch, int batch_elem_bytes, long n, int depth,
                 int order_id, int64_t* code, void* stream);
/* all four curves, code4 is (4,n) row-major in CDSEG_ORDER_* order */
int cdseg_encode4(const int32_t* grid, const int32_t* batch, long n, int depth, int64_t* code4, void* stream);
/* stable radix sort of (code, value) pairs = torch.argsort(code) when vals_in == NULL (iota).
 * ref: structure.py:83 (torch.argsort), ptv3.py:493.  ws from cdseg_sort_ws_bytes(n). */
size_t cdseg_sort_ws_bytes(long n);
int cdseg_sort_pairs(const int64_t* keys_in, int64_t* keys_out, const int32_t* vals_in, int32_t* vals_out, long n,
                     int end_bit, void* ws, size_t ws_bytes, void* stream);
/* Orders of `count` (<= 4) curves of the same n points with ONE sort: codes (4, n) int64 (row r = curve r), rows[count] =
 * the curve rows wanted (host array), orders (count, n) int32 out (= count argsorts, ref: structure.py:83).  The curve
 * slot rides in the key bits above end_bit (end_bit + 2 <= 64).  ws from cdseg_sort_curves_ws_bytes(n, count). */
size_t cdseg_sort_curves_ws_bytes(long n, int count);
int cdseg_sort_curves(const int64_t* codes, const int* rows, int count, long n, int end_bit, int32_t* orders, void* ws,
                      size_t ws_bytes, void* stream);
/* inv[perm[i]] = i.  ref: structure.py:84-90 (scatter_ of arange) */
int cdseg_invert_perm(const int32_t* perm, long n, int32_t* inv, void* stream);
int cdseg_widen_i32(const int32_t* src, long n, int64_t* dst, void* stream);

/* row gathers / scatters (rows of row_bytes % 4 == 0 bytes); idx < 0 gathers zeros / skips.  cdseg_gather_i32 has NO sentinel:
 * every idx entry names an element of src (a negative one is read out of bounds). */
int cdseg_gather_rows(const void* src, const int32_t* idx, long n_out, int row_bytes, void* dst, void* stream);
int cdseg_scatter_rows(const void* src, const int32_t* idx, long n_in, int row_bytes, void* dst, void* stream);
int cdseg_gather_i32(const int32_t* src, const int32_t* idx, long n, int32_t* dst, void* stream);

/* engine plan, stage 0: int32 grid + batch in z-sorted ("physical") order */
int cdseg_plan_gather_grid(const void* grid, int grid_elem_bytes, const int32_t* perm, const int64_t* zcode_sorted,
                           long n, int depth, int32_t* grid_out, int32_t* batch_out, void* stream);

/* ------------------------------------------------------------------ pooling structure
 * ref: ptv3.py:477-492 (code >> 3*depth, torch.unique, sort(cluster), idx_ptr, head).
 * On z-sorted points a cluster is a contiguous run: cluster ids are an inclusive scan of the
 * run-start flags, seg_start (count+1 entries) are the run starts, *count_dev the number of runs.  What seg_start holds behind
 * those count+1 entries is undefined (cdseg_pool_levels: every row of seg_start likewise). */
int cdseg_pool_level(const int64_t* zcode_sorted, long n, int shift_bits, int32_t* cluster, int32_t* seg_start,
                     int32_t* count_dev, void* ws, size_t ws_bytes, void* stream);
/* All pooling levels of a scene in one flag / scan / finish pass (replaces one cdseg_pool_level per level).
 * shifts (host, nlev <= 8) = 3 * cumulative pooling depth; last_idx (nb, device) = last point of each batch element.
 * cluster (nlev, n), seg_start (nlev, n + 1) int32; meta: nlev * (1 + nb) + 1 int32 = per level [count, cluster of
 * last_idx[b] ...], then ONE trailing int = the number of points whose (batch, voxel) code repeats their predecessor's
 * (0 for a valid model input: one point per voxel - the host raises on anything else with the read it does anyway). */
size_t cdseg_pool_levels_ws_bytes(long n, int nlev);
int cdseg_pool_levels(const int64_t* zcode_sorted, long n, const int* shifts, int nlev, const int32_t* last_idx, int nb,
                      int32_t* cluster, int32_t* seg_start, int32_t* meta, void* ws, size_t ws_bytes, void* stream);
/* Link between two pooled levels a (finer, m_a points) and b (m_b) from their links to level 0:
 * cluster_ab (m_a), seg_ab (m_b + 1). */
int cdseg_link_derive(const int32_t* cluster_0a, const int32_t* seg_0a, long ma, const int32_t* cluster_0b,
                      const int32_t* seg_0b, long mb, int32_t* cluster_ab, int32_t* seg_ab, void* stream);
/* Curve orders of ALL pooled levels without sorting: z-order / Hilbert keys are hierarchical, so the coarse order on a
 * curve is the level-0 order with every point replaced by its cluster id and consecutive duplicates dropped
 * (replaces torch.argsort(code >> 3*depth) of SerializedPooling, ref ptv3.py:503-514).
 * clusters[l] (n0): level-0 point -> cluster id at pooled level l; orders[c] (n0): rank -> level-0 point on curve c.
 * out: level l / curve c at int32 offset ncurve * sum_{l'<l} m_l' + c * m_l. */
size_t cdseg_coarse_orders_ws_bytes(long n0, int nlev, int ncurve);
int cdseg_coarse_orders(const int32_t* const* clusters, int nlev, const int32_t* const* orders, int ncurve, long n0,
                        int32_t* out, void* ws, size_t ws_bytes, void* stream);
/* pooled grid / batch / codes from the first fine point of each run.  ref: ptv3.py:489-491, 519-525 */
int cdseg_pool_gather(const int32_t* seg_start, long m, long n_fine, int pooling_depth, const int32_t* grid_f,
                      const int32_t* batch_f, const int64_t* code4_f, int32_t* grid_c, int32_t* batch_c,
                      int64_t* code4_c, void* stream);

/* ------------------------------------------------------------------ sparse-conv kernel map
 * ref: spconv.SubMConv3d indice pairs (third party; call sites ptv3.py:356,647,1106,1118).
 * nbr (n, ksize^3): row index of the occupied voxel at grid + (a-r, b-r, c-r), column
 * a*k*k + b*k + c, or -1 (kmajor != 0: stored transposed, (ksize^3, n)).  Points must be sorted
 * by (batch | z-order) code. */
int cdseg_nbr_table(const int64_t* zcode_sorted, const int32_t* grid, const int32_t* batch, long n, int depth,
                    int ksize, int kmajor, int32_t* nbr, void* stream);

/* The same kernel map derived from the PARENT level's 3x3x3 map (pooling depth 1) instead of searching: a target
 * cell lies in one of the 27 parent cells around the point's parent; empty parent cell => empty target, else the target
 * is one of its <= 8 z-contiguous children.  cluster (n): point -> parent; parent_nbr3 (27, m) offset-major;
 * seg_start (m + 1): children runs of the parents. */
int cdseg_nbr_table_from_parent(const int64_t* zcode_sorted, const int32_t* grid, const int32_t* cluster,
                                const int32_t* parent_nbr3, const int32_t* seg_start, long n, long m, int depth, int ksize,
                                int kmajor, int32_t* nbr, void* stream);
/* ... and with the parents' child_info words (cdseg_child_info: first child row << 8 | octant occupancy) instead of the
 * children runs: target = first + popcount(occupancy below the target's octant). */
int cdseg_nbr_table_from_info(const int32_t* grid, const int32_t* cluster, const int32_t* parent_nbr3,
                              const int64_t* child_info, long n, long m, int depth, int ksize, int kmajor, int32_t* nbr,
                              void* stream);
/* ------------------------------------------------------------------ attention padding plan
 * ref: ptv3.py:188-244 (get_padding_and_inverse) in gather/scatter form: for every padded slot
 * the row to read (gidx) and the row to write (widx, -1 for the borrowed duplicates).
 * order: rank -> row for the curve of this block (NULL = identity); offs/offs_pad (nb+1). */
int cdseg_pad_plan(const int32_t* order, const int32_t* offs, const int32_t* offs_pad, int nb, int patch, long n_pad,
                   int32_t* gidx, int32_t* widx, void* stream);
/* every slot plan of a scene in ONE launch (count <= CDSEG_PAD_BATCH_MAX): plan j = (orders[j] or NULL, offs[j],
 * offs_pad[j], patch[j], n_pad[j]); gidx / widx of plan j start at sum_{i<j} n_pad[i]. Pointer arrays are host arrays. */
#define CDSEG_PAD_BATCH_MAX 48
int cdseg_pad_plan_batch(int count, const int32_t* const* orders, const int32_t* const* offs,
                         const int32_t* const* offs_pad, const int* patch, const long* n_pad, int nb, int32_t* gidx,
                         int32_t* widx, void* stream);
/* Slot plan of a collated batch whose elements read DIFFERENT curves (test-time voting with one order shuffle per
 * fragment): gidx[s] = gidx_src[choice[b]][s], widx[s] = widx_src[choice[b]][s] for every padded slot s of batch element b
 * (offs_pad[b] <= s < offs_pad[b + 1]).  gidx_src / widx_src: host arrays of nsrc (<= 4) device pointers, the slot plans of
 * ONE level and patch key on the curves in question, n_pad int32 each; an entry no element chooses may be NULL, a chosen
 * NULL entry (or choice >= nsrc) is CDSEG_ERR_ARG before any launch.  choice_host: nb bytes on the HOST, passed to the
 * kernel by value (no host-to-device copy); nb > CDSEG_SLOTS_SELECT_MAX is CDSEG_ERR_UNSUPPORTED.  No LDS, no atomics. */
#define CDSEG_SLOTS_SELECT_MAX 64
int cdseg_slots_select(const int32_t* const* gidx_src, const int32_t* const* widx_src, int nsrc, const int32_t* offs_pad,
                       int nb, const unsigned char* choice_host, long n_pad, int32_t* gidx, int32_t* widx, void* stream);

/* ------------------------------------------------------------------ dense / gathered GEMM
 * out = epilogue(A @ W^T): nn.Linear (ref: ptv3.py:170-171, 310-313, 463, 597-599, 1562) and,
 * with nbr != NULL, spconv.SubMConv3d as a gathered-A GEMM over kvol offsets
 * (W is the conv weight (N, kvol, K) flattened = (out, k0, k1, k2, in)).
 * epilogue: v = acc + bias; v = v*scale + shift (folded eval BatchNorm1d, ref: ptv3.py:1440);
 *           v = act(v); [out2 = v if out2_pre_add]; v += res; v += add_src[add_idx[m]];
 *           out[out_idx ? out_idx[m] : m] = v; [out2 = v otherwise]
 *         out_idx[m] < 0: row m is written nowhere (neither out nor out2).  add_idx has no sentinel: every entry names a row
 *         of add_src.
 * kvol <= 128 (k=5 stem: 125), K % 8 == 0. */
typedef struct cdseg_gemm_args {
  const void* A;          /* (M, lda) a_dtype; with nbr: the gather source (rows indexed by nbr) */
  const void* W;          /* (N, kvol*K) compute dtype, K contiguous */
  const float* bias;      /* (N) or NULL */
  const float* scale;     /* (N) or NULL */
  const float* shift;     /* (N) or NULL (required with scale) */
  const float* res;       /* (M, ldres) or NULL */
  const float* add_src;   /* (*, ldadd) or NULL */
  const int32_t* add_idx; /* (M) */
  const int32_t* nbr;     /* (M, kvol), or (kvol, M) when nbr_kmajor, or NULL */
  const int32_t* out_idx; /* (M) or NULL */
  void* out;              /* (M, ldo) out_dtype */
  void* out2;             /* (M, ldo2) out2_dtype or NULL */
  long M;
  int N, K, kvol;
  int lda, ldo, ldo2, ldres, ldadd;
  int a_dtype, compute_dtype, out_dtype, out2_dtype;
  int act;
  int out2_pre_add;
  void* ws;        /* fp32 partial tiles, 16-byte aligned, sized by cdseg_gemm_ws_bytes (0: pass NULL).  The workspace chooses */
  size_t ws_bytes; /*   the plan: without one there is no split-K (few-tile, long-K launches of the deep stages run unsplit),
                    *   and a fused LayerNorm over several column tiles (N > 128), which needs M * N * 4 bytes, is
                    *   CDSEG_ERR_WORKSPACE; a smaller ws_bytes is legal for split-K and lowers the slice count to the
                    *   (M, N) planes that fit.  Results are deterministic for a given ws_bytes. */
  /* fused row LayerNorm (N <= 128; ref: nn.LayerNorm eps 1e-5 at ptv3.py:365,367,381):
   *   v = act(acc + bias);  if ln_pre:  v = LN(v) * ln_pre_g + ln_pre_b      (CPE, ptv3.py:401-404)
   *   v += res + colbias (+ add_src);  out = v;  if ln_post: ln_out = LN(v) * ln_post_g + ln_post_b */
  const float* colbias;   /* (N) or NULL: timestep-embedding bias, ptv3.py:406-411 */
  const float* ln_pre_g;
  const float* ln_pre_b;
  const float* ln_post_g;
  const float* ln_post_b;
  void* ln_out;           /* (M, ldln) ln_out_dtype */
  int ldln, ln_out_dtype;
  float ln_eps;
  int nbr_kmajor;         /* neighbour table is offset-major (kvol, M): coalesced index loads, cheaper to build */
} cdseg_gemm_args;
int cdseg_gemm(const cdseg_gemm_args* args_host, void* stream);
/* The workspace cdseg_gemm's launch plan expects for M x N (gathered: nbr != NULL; fused_ln: ln_pre_g or ln_post_g set): the
 * split-K planes of a launch with few output tiles, or the one plane of a fused LayerNorm with N > 128; 0 = pass NULL.  A
 * function of the shape only (host code, no device needed). */
size_t cdseg_gemm_ws_bytes(long M, int N, int gathered, int fused_ln);

/* ------------------------------------------------------------------ LayerNorm
 * out = [res +] LayerNorm(x) * gamma + beta [+ colbias]; optional second copy out2.
 * ref: nn.LayerNorm(eps 1e-5) at ptv3.py:365, 367, 381 and the CPE residual ptv3.py:401-404,
 * t-embedding bias ptv3.py:406-411.
 * c % 4 == 0, c <= 2048; every row stride % 4 == 0; every access is a group of four elements, so x / out / out2 are 16-byte
 * aligned as fp32 and 8-byte aligned as the 16-bit type, gamma / beta / res / colbias 16-byte aligned (CDSEG_ERR_ARG otherwise,
 * nothing is launched).  res may be out (in place on the residual). */
int cdseg_layernorm(const void* x, int x_dtype, int ldx, const float* gamma, const float* beta, float eps,
                    const float* res, int ldres, const float* colbias, void* out, int out_dtype, int ldo,
                    void* out2, int out2_dtype, int ldo2, long m, int c, void* stream);

/* ------------------------------------------------------------------ serialized window attention
 * ref: ptv3.py:246-296 (SerializedAttention core; flash_attn_varlen_qkvpacked_func :282-288)
 *      ptv3.py:988-1055 (SerializedCrossAttention core; flash_attn_varlen_kvpacked_func :1038-1047)
 * For patch p (slots patch_start[p] .. patch_start[p+1], length <= 1024) and head h:
 *   O = softmax(scale * Q K^T) V over the full patch (no mask), head dim 16,
 *   Q row of slot s = q[q_gidx[s]*ldq + h*16 ..], K/V rows by kv_gidx, output row widx[s] (skip if -1).
 * The gather by serialized order, the padding duplicates and the scatter by inverse are fused. */
int cdseg_attention(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const int32_t* q_gidx,
                    const int32_t* kv_gidx, const int32_t* widx, const int32_t* patch_start, int num_patches,
                    int num_heads, int max_len, float scale, void* out, int ldo, int dtype, void* stream);
/* The same with producer-side preprocessing declared in `flags` (what the fused qkv epilogues of this library emit, so the
 * kernel - VALU-issue bound - does not redo per (head, query slice) what a producer does once per row):
 *   CDSEG_ATTN_Q_PRESCALED  q already carries softmax scale * log2(e) (folded into Wq / bq at load time); `scale` is ignored
 *   CDSEG_ATTN_V_BF16       v holds bfloat16 whatever the build's 16-bit type is (the IEEE-half build runs P V in bfloat16:
 *                           P = exp2(s - bound) needs fp32's exponent range); CDSEG_BF16 dtype only
 * q, k, v, out and every row (ld * element size) must be 16-byte aligned (CDSEG_ERR_ARG otherwise). */
#define CDSEG_ATTN_Q_PRESCALED 1
#define CDSEG_ATTN_V_BF16 2
int cdseg_attention_ex(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const int32_t* q_gidx,
                       const int32_t* kv_gidx, const int32_t* widx, const int32_t* patch_start, int num_patches,
                       int num_heads, int max_len, float scale, void* out, int ldo, int dtype, int flags, void* stream);

/* Diagnostic, host only: the block id -> (patch, head, query slice, slices of that patch-head) table of the launch
 * cdseg_attention_ex issues for this shape (the graded schedule of csrc/attention.hip: the last blocks an XCD runs cover a
 * half / a quarter of a patch-head's queries).  4 ints per block id, -1 x 4 for ids that exit at once.  Returns the number
 * of block ids (may exceed `capacity`; at most `capacity` rows are written), or a negative status. */
long cdseg_attention_schedule(int num_patches, int num_heads, int max_len, int dtype, int32_t* table, long capacity);

/* Launch record, host only: which kernel each host-side chooser of this library picked (csrc/route.h).  Almost every launch
 * is routed among template instantiations by row / column / reduction thresholds; with recording on, each chooser notes its
 * choice immediately before the launch it describes, per calling host thread, in a ring of the newest 64 launches (one
 * cdseg_block_forward leaves at most ten).  Off by default: a launch then pays one thread-local test.  Records of a call that
 * returns an error describe the launches attempted up to the error.
 *   record = 8 int32: [0] kernel id = line number in the catalogue; [1] row tile; [2] column tile (0: none); [3] split-K
 *   slices; [4] fix (0; 1 = split-K second pass; 2 = row finish of the fused LayerNorm); [5] xmode (cdseg_gemm's block id ->
 *   tile mapping, 0 / 1 / 2); [6] flags; [7] aux: the deep-stage head / tail: workgroups per row tile (the head, when it
 *   reads the conv's split-K partial planes: | their count << 8); attention: waves per block; fused MLP / tail / head: rows
 *   per workgroup; sparse conv: waves per block.
 *   The training, level and elementwise choosers: LayerNorm / add + LayerNorm: [1] rows per wave, [2] c, [7] lanes per row
 *   (tpr), the compute-type bits = the dtype of x / of h; weight gradients: [1] x [2] the dW tile, [3] row splits, [5] rows per
 *   split (not cdseg_gemm's xmode), [7] kernel offsets; attention backward: [3] slices of a patch-head, [7] waves per block;
 *   cdseg_pool_fused: [4] the fold taken (1 walk / 2 scan), [7] the fold asked for (0 = the rule decided); the segmentation
 *   loss: [2] c, [7] classes present; skip statistics: [3] row chunks; skip / fusion row kernels: F_VEC_OK = the 16-byte arm.
 * cdseg_route_enable: returns the previous state.  cdseg_route_clear: forget this thread's records.  cdseg_route_read: the
 * number of launches recorded since the last clear (may exceed both the ring and `capacity`); writes the newest
 * min(count, 64, capacity) records, oldest first (rec may be NULL with capacity 0).  cdseg_route_catalog: the names of every
 * kernel id compiled into this library, in id order, separated by '\n' and terminated by '\0' - the table the recording
 * sites take their ids from; returns the bytes needed (nothing is written if `bytes` is smaller).
 * TEST HOOK, not part of the product interface: cdseg_route_note appends one record as a chooser would (a no-op while
 * recording is off; CDSEG_ERR_ARG for an id outside the catalogue).  It exists so that the ring can be exercised on a machine
 * without a GPU (tests/test_cpu_routes.py); a record it appends describes no launch. */
#define CDSEG_ROUTE_WORDS 8
#define CDSEG_ROUTE_F_VEC_OK 1     /* every epilogue access of cdseg_gemm is a 16-byte group */
#define CDSEG_ROUTE_F_GATHER 2     /* rows gathered through a kernel map */
#define CDSEG_ROUTE_F_PARTIALS 4   /* split-K partial planes left in the workspace for the consuming kernel */
#define CDSEG_ROUTE_F_KDIV 8       /* K is no power of two: the gather locates a column by division */
#define CDSEG_ROUTE_F_KSHIFT_LT6 16 /* K is a power of two below 64 */
#define CDSEG_ROUTE_F_CT_SHIFT 5   /* bits 5-6: compute type (CDSEG_F32 / CDSEG_BF16 / CDSEG_F32X3) */
int cdseg_route_enable(int on);
void cdseg_route_clear(void);
int cdseg_route_read(int32_t* rec_host, int capacity);
int cdseg_route_catalog(char* buf_host, size_t bytes);
int cdseg_route_note(const int32_t* rec_host);

/* HIP-event timing of the attention launches on their own stream (bench.py's live roofline measurement):
 * enable(1) starts recording, summary() (after a device sync) returns the summed durations. */
int cdseg_prof_enable(int on);
int cdseg_prof_summary(double* total_ms, long* launches); /* class CDSEG_PROF_ATTENTION */
/* per kernel class: 0 = window attention, 1 = k = 3 sparse convs of the wide stages (cdseg_subm_conv3: HBM / gather bound),
 * 2 = k = 3 sparse convs on the gathered GEMM (cdseg_gemm with a 27-offset map: C >= 128, MFMA / LDS-DMA bound) */
#define CDSEG_PROF_ATTENTION 0
#define CDSEG_PROF_CONV 1
#define CDSEG_PROF_CONV_DEEP 2
int cdseg_prof_summary_class(int cls, double* total_ms, long* launches);

/* ------------------------------------------------------------------ pooling reduce
 * out[j] = act(max_{i in run j} y[i] * scale + shift), runs = seg_start (m+1).
 * ref: ptv3.py:510-515 (torch_scatter.segment_csr(..., "max")) + norm/act :548-551
 * c % 4 == 0, ldy / ldo / ldo2 % 4 == 0; out, scale and shift 16-byte aligned, y and out2 16-byte aligned as fp32 and 8-byte
 * aligned as the 16-bit type (CDSEG_ERR_ARG otherwise, nothing is launched).  Every run holds at least one row. */
int cdseg_segment_max(const void* y, int y_dtype, int ldy, const int32_t* seg_start, long m, int c,
                      const float* scale, const float* shift, int act, float* out, int ldo, void* out2,
                      int out2_dtype, int ldo2, void* stream);
/* The whole SerializedPooling feature path in one launch (16-bit trunk; ref: ptv3.py:506-515 proj + segment_csr("max"),
 * :548-551 norm + act):   out[j] = act(scale * max_{i in run j} round16(W x_i + bias) + shift),   out2 = 16-bit copy.
 * Bit-identical to cdseg_gemm (16-bit output) followed by cdseg_segment_max; the projected rows never reach HBM.
 * (cin, cout) = (32, 64) or (64, 128), else CDSEG_ERR_UNSUPPORTED (callers use the two-launch form).  wimg: fragment image
 * of W (cout, cin) built once by cdseg_pool_fused_pack (cdseg_pool_fused_img_bytes bytes).  act: NONE or GELU.
 * Every run holds at least one row, as for cdseg_segment_max.
 * The maximum of a run is folded in one of two ways that give the same bits: short runs (one octree step) through a strip
 * the lanes of a pooled row walk, long runs (two steps, ~8 children) by a segmented maximum across the 16 child lanes of a
 * step.  cdseg_pool_fused_n takes the rows of x, n_fine = seg_start[m], which only the device holds otherwise, and chooses
 * from the mean run length n_fine / m; cdseg_pool_fused, without it, walks.
 * TEST HOOK, not part of the product interface: cdseg_pool_fused_fold forces the fold of every later launch of the process
 * (0 = as above, 1 = walk, 2 = segmented maximum) and returns the previous setting; CDSEG_ERR_ARG otherwise. */
int cdseg_pool_fused_fold(int fold);
int cdseg_pool_fused_n(const void* x, int ldx, long n_fine, const void* wimg, const float* bias, const int32_t* seg_start, long m,
                       const float* scale, const float* shift, int act, float* out, int ldo, void* out2, int ldo2,
                       int cin, int cout, void* stream);
size_t cdseg_pool_fused_img_bytes(int cin, int cout);
int cdseg_pool_fused_pack(const void* w, int cin, int cout, void* wimg, void* stream);
int cdseg_pool_fused(const void* x, int ldx, const void* wimg, const float* bias, const int32_t* seg_start, long m,
                     const float* scale, const float* shift, int act, float* out, int ldo, void* out2, int ldo2,
                     int cin, int cout, void* stream);
/* SerializedUnpooling of the wide decoder stages, mode "add", in one launch (16-bit trunk; ref: ptv3.py:597-630):
 *   s = act(scale_skip * (W_skip skip_x[i] + bias_skip) + shift_skip),   out2[i] = round16(s)   (the pre-add skip),
 *   out[i] = s + act(scale_child * (W_child coarse_x[j] + bias_child) + shift_child)   for the rows i of run j,
 * runs = seg_start (m + 1 entries, every run holds at least one row; the rows of skip_x / out / out2 are seg_start[m]).
 * Bit-identical to cdseg_gemm of coarse_x into an fp32 buffer followed by cdseg_gemm of skip_x with add_src / add_idx (the
 * cluster of seg_start) / out2_pre_add; the projected coarse rows never reach HBM.  (k_skip, k_child, c) = (32, 64, 64) or
 * (64, 128, 64), else CDSEG_ERR_UNSUPPORTED (callers use the two launches).  wimg_*: fragment images of the (c, k) weights
 * built once by cdseg_unpool_fused_pack (cdseg_unpool_fused_img_bytes bytes; cin 32 / 64 / 128, cout 64).  act: NONE or GELU.
 * ld_skip / ld_coarse % 8 == 0, ldo / ldo2 % 4 == 0; skip_x, coarse_x, the images, out and the parameter vectors 16-byte
 * aligned, out2 8-byte aligned (CDSEG_ERR_ARG otherwise, nothing is launched).  No workspace. */
size_t cdseg_unpool_fused_img_bytes(int cin, int cout);
int cdseg_unpool_fused_pack(const void* w, int cin, int cout, void* wimg, void* stream);
int cdseg_unpool_fused(const void* skip_x, int ld_skip, const void* wimg_skip, const float* bias_skip,
                       const float* scale_skip, const float* shift_skip, const void* coarse_x, int ld_coarse,
                       const void* wimg_child, const float* bias_child, const float* scale_child,
                       const float* shift_child, const int32_t* seg_start, long m, int act, float* out, int ldo,
                       void* out2, int ldo2, int k_skip, int k_child, int c, void* stream);
/* segment mean of coord (ref: ptv3.py:513-515) */
int cdseg_segment_mean(const float* x, int ldx, const int32_t* seg_start, long m, int c, float* out, int ldo,
                       void* stream);

/* ------------------------------------------------------------------ small dense helpers */
/* y = act(W x + b), W (n,k) fp32: the timestep-embedding MLP, ref: ptv3.py:1772-1778, :406-411 */
int cdseg_gemv(const float* w, const float* b, const float* x, int n, int k, int act, float* y, void* stream);
/* standard normal draws (Philox4x32-10 + Box-Muller), the noise-branch input.  ref: default.py:393 */
int cdseg_randn(float* out, long n, uint64_t seed, uint64_t offset, void* stream);
int cdseg_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long n, void* stream);
/* dst[i, 0:cpad] = cast(src[idx[i], 0:cin]), zero padded (idx NULL = identity): stem input rows in the
 * engine's point order, padded to a 16-byte multiple so the stem conv runs on the gathered GEMM.  No sentinel: every idx entry
 * names a row of src. */
int cdseg_gather_pad_cast(const float* src, int ld_src, const int32_t* idx, long n, int cin, int cpad, void* dst,
                          int dst_dtype, void* stream);
/* DDIM update of the noise-branch input on a uniform timestep t (ref: default.py:192-214, dm_target="noise"):
 * x0 = (xt - sqrt(1-ab_t) eps) / sqrt(ab_t); out = final ? x0 : sqrt(ab_{t-1}) x0 + sqrt(1-ab_{t-1}) eps */
int cdseg_ddim_update(const float* xt, const float* eps, float sqrt_ab_prev, float sqrt_1m_ab, float sqrt_ab,
                      float sqrt_1m_ab_prev, int final_step, float* out, long n, void* stream);
/* Diagnostic of the IEEE-half build: *counter += the number of elements of the 16-bit buffer x (rows x cols, row stride ld
 * elements) that sit exactly at +-65504 - the value every float -> half conversion of that build clamps to.  The bfloat16
 * build never clamps and adds nothing.  cdseg_block_forward runs it over a Block's conv output, q / k, attention output and
 * shadow copy when cdseg_block_io.sat_counter is set. */
int cdseg_count_saturated(const void* x, long rows, int cols, int ld, unsigned long long* counter, void* stream);
/* x (rows, cols) fp32 -> hi = T(x) (saturating), lo = T((x - hi) * lo_scale) in the build's 16-bit type T (cols, ldx, ld16
 * multiples of 4).  The IEEE-half build with lo_scale = 2048 gives x ~= hi + lo / 2048 to 22 significant bits: the operand
 * pairs of precision "fp32x3"'s sparse convs (three 16-bit gathered GEMMs into one fp32 output). */
/* cdseg_subm_conv3 with an fp32 output: yf = (accumulate ? yf : 0) + (conv + bias) * out_scale (C = 32 / 64, 16-bit x and
 * weight image as above).  Three calls on IEEE-half operand pairs give a k = 3 conv to 22 significant bits ("fp32x3"). */
int cdseg_subm_conv3_f32(const void* x, int ldx, const void* wimg, const float* bias, const int32_t* nbr_kmajor, long n,
                         int channels, float* yf, int ldyf, float out_scale, int accumulate, void* stream);
int cdseg_split16(const float* x, int ldx, long rows, int cols, void* hi, void* lo, int ld16, float lo_scale, void* stream);
/* out = a + alpha * b (fp32).  ref: default.py:228-236 (add_gaussian_noise) */
int cdseg_axpy(const float* a, const float* b, float alpha, float* out, long n, void* stream);
/* The glue of one step of multi-step inference (MSAI / MSFI, ref: default.py:327-349) in one launch over both arrays:
 *   eps != NULL: c_xt[0..n_c) <- cdseg_ddim_update's result, IN PLACE
 *   acc != NULL: acc[0..n_l) <- logits (acc_mode 0) | acc + logits (1) | (acc + logits) * scale (2: the last step's mean)
 * Bit-equal to cdseg_ddim_update / cdseg_axpy.  16-byte accesses where a pair of arrays sits at the same offset from a 16-byte
 * boundary, scalar head / tail otherwise.  CDSEG_ERR_ARG before any launch: a negative count, a NULL array with a positive
 * count, an unknown acc_mode, a pointer that is not 4-byte aligned. */
int cdseg_msi_step(float* c_xt, const float* eps, long n_c, float sqrt_ab_prev, float sqrt_1m_ab, float sqrt_ab,
                   float sqrt_1m_ab_prev, int final_step, float* acc, const float* logits, long n_l, int acc_mode,
                   float scale, void* stream);

/* ------------------------------------------------------------------ test-time pipeline
 * ref: datasets/transform.py:821-897 (GridSample mode="test"), engines/test.py:261-278 (softmax vote, arg-max) */
/* grid = floor(coord / grid_size) - min (int32), key = one int64 per voxel; min3_dev (3 x int32) receives the min */
int cdseg_voxelize(const float* coord, double grid_size, long n, int32_t* grid, int64_t* key, int32_t* min3_dev,
                   void* stream);
int cdseg_voxelize_f64(const double* coord, double grid_size, long n, int32_t* grid, int64_t* key, int32_t* min3_dev,
                       void* stream); /* float64 coordinates: what GridSample sees after a test-time rotation */
/* pre-model transforms of the test pipeline (ref: configs/scannet/CDSegNet.py:253-398, datasets/transform.py):
 * CenterShift :142-155 on an (n,3) float32 / float64 array (ws12: 96 bytes of device scratch);
 * one test-time augmentation :259-328 - rot9_host (row-major R) given: out FLOAT64 (n,3) = (in R^T) [* scale]
 *   (RandomRotateTargetAngle about the origin, then RandomScale), else flip: out float32 = in with x and y negated;
 * NormalizeColor :113-117 as out = in / div + add;  Collect(feat_keys=(a, b)) :46-49 as feat = cat([a, float(b)], 1). */
int cdseg_center_shift(const void* xyz, int is_f64, long n, int apply_z, void* out, void* ws12, void* stream);
int cdseg_tta_apply(const float* in, long n, const double* rot9_host, double scale, int apply_scale, int flip, void* out,
                    void* stream);
int cdseg_div_add(const float* in, float div, float add, long n, float* out, void* stream);
int cdseg_collect_feat(const float* a, int ca, const void* b, int b_is_f64, int cb, long n, float* out, void* stream);
/* largest run length of a seg_start array (m runs) = number of test fragments (count.max()) */
int cdseg_max_run(const int32_t* seg_start, long m, int32_t* out_dev, void* stream);
/* fragment `frag`: idx_part[v] = idx_sort[seg_start[v] + frag % count_v].  ref: transform.py:862-864 */
int cdseg_fragment_select(const int32_t* idx_sort, const int32_t* seg_start, long m, int frag, int32_t* idx_part,
                          void* stream);
/* pred[idx[i], :] += softmax(logits[i, :]).  ref: engines/test.py:261-267.  No sentinel and no atomics: every idx entry names a
 * row of pred, no row twice (the members of one fragment). */
int cdseg_softmax_vote(const float* logits, int ldl, const int32_t* idx, long m, int c, float* pred, int ldp,
                       void* stream);
/* out[i] = first arg-max of row i.  ref: engines/test.py:278 */
int cdseg_argmax_rows(const float* x, int ldx, long n, int c, int32_t* out, void* stream);
/* ALL F fragments of one augmented scan as dense arrays, in a number of launches that does not depend on F
 * (ref: transform.py:867-895 + the post_transform CenterShift(apply_z=False) :142-155 and Collect :27-50).
 * idx_sort / seg_start: the stable voxel sort and its m runs over the n source rows; fragment f takes member f % count_v
 * of voxel v.  index (F,m) int32 = source rows; grid_out (F,m,3) = grid rows; feat_out (F,m,c) = feat rows (16-byte
 * accesses when c % 4 == 0 and both feature pointers are 16-byte aligned, 8-byte for even c, else 4-byte); coord_out (F,m,3)
 * float32 from coord (n,3) float32 (coord_f64 = 0) or float64.  center_shift != 0: fragment f's coordinates minus
 * [(xmin + xmax) / 2, (ymin + ymax) / 2, 0] of that fragment, computed in coord's precision (bounds by order-independent
 * integer min / max atomics), then rounded to float32 once - bit-equal to cdseg_fragment_select + cdseg_gather_rows +
 * cdseg_center_shift + a conversion.  ws: cdseg_fragments_build_ws_bytes(F) bytes (only read with center_shift).
 * F <= 65535.  Source rows outside [0, n) are skipped. */
size_t cdseg_fragments_build_ws_bytes(int F);
int cdseg_fragments_build(const int32_t* idx_sort, const int32_t* seg_start, long m, int F, long n, const int32_t* grid,
                          const float* feat, int c, const void* coord, int coord_f64, int center_shift, int32_t* index,
                          int32_t* grid_out, float* feat_out, float* coord_out, void* ws, size_t ws_bytes, void* stream);
/* the votes of k collated fragments in one launch: pred[index[f][v], :] += softmax(logits[f m + v, :]), f = 0 .. k-1 in
 * that order for every voxel v (logits (k m, c), index (k, m), pred n rows).  No float atomics; bit-equal to k successive
 * cdseg_softmax_vote calls when no row is named by two voxels (the fragments of cdseg_fragments_build). */
int cdseg_softmax_vote_fragments(const float* logits, int ldl, const int32_t* index, long m, int k, int c, float* pred,
                                 int ldp, long n, void* stream);
/* GridSample(return_inverse=True) :847-849: inverse[idx_sort[j]] = cluster[j], the voxel rank of every one of the n rows */
int cdseg_voxel_inverse(const int32_t* idx_sort, const int32_t* cluster, long n, int32_t* inverse, void* stream);

/* ------------------------------------------------------------------ train-time pipeline
 * ref: configs/{scannet,scannet200,nuscenes}/CDSegNet.py data.train / data.val transform lists, datasets/transform.py.
 * Coordinates and normals are FLOAT64 (n,3) between the first transform and GridSample; every float64 operation is one
 * correctly rounded add / multiply / divide in the documented order, never a fused multiply-add, so the results are
 * bit-equal to a numpy restatement of the same operations.  `*_host` arguments are read on the host at the call. */
#define CDSEG_TT_CENTER_NONE 0     /* no translation */
#define CDSEG_TT_CENTER_HOST 1     /* center3_host */
#define CDSEG_TT_CENTER_BBOX 2     /* ((min + max) / 2) of all three axes of bbox6_dev: RandomRotate(center=None) :245-247 */
#define CDSEG_TT_CENTER_SHIFT_Z 3  /* CenterShift(apply_z=True) :148-151: [(xmin+xmax)/2, (ymin+ymax)/2, zmin] */
#define CDSEG_TT_CENTER_SHIFT_XY 4 /* CenterShift(apply_z=False): [(xmin+xmax)/2, (ymin+ymax)/2, 0] */
/* bounding box of an (n,3) float32 / float64 array; ws12: 96 bytes of device memory, doubles ws12[6..11] receive
 * [min x y z, max x y z] (ws12 + 6 is the `bbox6_dev` of the calls below) */
int cdseg_tt_bbox(const void* xyz, int is_f64, long n, void* ws12, void* stream);
/* t = in - c ; rot9_host (row-major R) given: t_j = (t0 R[j][0] + t1 R[j][1]) + t2 R[j][2] ; add_back: t += c ;
 * apply_scale: t *= scale ; flipx / flipy: negate.  CenterShift :142-155, RandomRotate :230-255, RandomScale :303-309,
 * RandomFlip :317-328; normals use center = NONE.  in / out float32 or float64 (out may alias in when the types agree). */
int cdseg_tt_affine(const void* in, int in_f64, long n, int center, const double* center3_host, const double* bbox6_dev,
                    const double* rot9_host, int add_back, double scale, int apply_scale, int flipx, int flipy, void* out,
                    int out_f64, void* stream);
/* RandomJitter :338-346: coord[i] += min(max(sigma z[i], -clip), clip); z (n,3) float32 or float64 normals */
int cdseg_tt_jitter(double* coord, const void* z, int z_f64, double sigma, double clip, long n, void* stream);
/* ElasticDistortion :742-784.  blur3: one zero-padded 3-tap box pass along `axis` of a (d0,d1,d2,3) float32 grid
 * (float64 accumulation left to right with the float32 weight 1/3, rounded to float32); in != out.
 * elastic: coord += trilinear(noise, coord) * magnitude on the axes ax_a(k) = k < d_a - 1 ? k step_a + start_a : stop_a
 * (numpy.linspace), corner weights ((w_x w_y) w_z) summed in itertools.product order, fill value 0 outside the axes. */
int cdseg_tt_blur3(const float* in, int d0, int d1, int d2, int axis, float* out, void* stream);
int cdseg_tt_elastic(double* coord, long n, const float* noise, const int* dims3_host, const double* start3_host,
                     const double* step3_host, const double* stop3_host, double magnitude, void* stream);
/* colour chain on (n,3) float32 in place, each stage optional (:385-431): contrast - float32 blend with
 * (c - lo) * (255 / (hi - lo)), lo / hi from bbox6_dev; tr3_host - c = f32(clip(tr + c, 0, 255)) in float64;
 * noise (n,3) float32 / float64 - c = f32(clip(noise * noise_mul + c, 0, 255)) in float64.  contrast blends
 * f32(1 - blend) * c + f32(blend) * contrast in float32 */
int cdseg_tt_color(float* color, long n, const double* bbox6_dev, double blend, int contrast, const double* tr3_host,
                   const void* noise, int noise_f64, double noise_mul, void* stream);
/* GridSample(mode="train") :834-838: out[v] = idx_sort[seg_start[v] + r[v] % count_v], r (m) int64 >= 0 */
int cdseg_tt_voxel_pick(const int32_t* idx_sort, const int32_t* seg_start, long m, const int64_t* r, int32_t* out,
                        void* stream);
/* SphereCrop :1012: key[i] = bit image of the float64 (dx dx + dy dy) + dz dz to row `center` (sorts like the distance) */
int cdseg_tt_dist_key(const double* coord, long n, long center, int64_t* key, void* stream);
/* integer companion of cdseg_randn, the same Philox4x32-10 stream: out[4 t + i] = word i of counter (t, offset) under
 * key seed, reduced modulo *bound_dev (device int32, if given) or bound (0: the raw 32-bit word) */
int cdseg_rand_int(int64_t* out, long n, uint64_t seed, uint64_t offset, const int32_t* bound_dev, uint32_t bound,
                   void* stream);

/* ------------------------------------------------------------------ evaluator
 * ref: engines/hooks/evaluator.py:132-140 (pointops.knn_query(1, ...) label transfer), utils/misc.py:52-65 (IoU counts).
 * Exact 1-NN of every query among the reference points of the same batch element (lowest index on ties, like the
 * reference's brute-force scan, libs/pointops/src/knn_query/knn_query_cuda_kernel.cu:60-104), found through a uniform
 * grid: origin (3 host floats) <= every reference coordinate, cell = grid cell size.  offsets: cumulative ends (nb).
 * idx (m) int32, dist2 (m) float or NULL. */
/* k nearest neighbours (round 5; ref: libs/pointops/functions/query.py:7-24 KNNQuery, src/knn_query/knn_query_cuda_kernel.cu:
 * 60-104 - the neighbourhood query of the reference's other backbones, off the CDSegNet path, SURVEY finding 2): idx (m, k)
 * int32 ascending by (squared distance, index), -1 placeholders when the batch element has fewer than k points; dist2 (m, k)
 * SQUARED distances (the reference's Python wrapper takes the square root), 1e10 placeholders, or NULL.  k <= 64
 * (CDSEG_ERR_UNSUPPORTED beyond); workspace cdseg_knn1_ws_bytes(n); other arguments as cdseg_knn1. */
int cdseg_knn(const float* ref_xyz, const int32_t* ref_offset, long n, const float* qry_xyz, const int32_t* qry_offset,
              long m, int nb, int k, const float* origin, float cell, int32_t* idx, float* dist2, void* ws, size_t ws_bytes,
              void* stream);
size_t cdseg_knn1_ws_bytes(long n);
int cdseg_knn1(const float* ref_xyz, const int32_t* ref_offset, long n, const float* qry_xyz, const int32_t* qry_offset,
               long m, int nb, const float* origin, float cell, int32_t* idx, float* dist2, void* ws, size_t ws_bytes,
               void* stream);
/* out (3,k) int64: per-class intersection, prediction and target counts over rows with target != ignore_index;
 * pred_idx (n) or NULL: row i is predicted pred[pred_idx[i]] (no sentinel: every entry names an element of pred). */
int cdseg_iou_counts(const int32_t* pred, const int32_t* pred_idx, const int32_t* target, long n, int k, int ignore_index,
                     int64_t* out, void* stream);

/* ------------------------------------------------------------------ fused MLP (ref: ptv3.py:299-322, :423-427)
 * x (n, ldx) fp32 += fc2(GELU(fc1(h))), h (n, ldh); xc (n, ldxc) = typed copy of the new x or NULL.  The 4C hidden
 * activation stays in LDS.  Supported: dtype bf16, channels 32, 64 or 128 (hidden = 4 * channels); else
 * CDSEG_ERR_UNSUPPORTED (callers fall back to two cdseg_gemm launches). */
int cdseg_mlp_fused(const void* h, int ldh, const void* w1, const float* b1, const void* w2, const float* b2, float* x,
                    int ldx, void* xc, int ldxc, long n, int channels, int dtype, void* stream);

/* Block tail after attention in ONE launch (ptv3.py:416-427): x += proj(o); h = LayerNorm(x); x += fc2(GELU(fc1(h)));
 * xc = typed copy of x.  o (n, ldo); the updated residual rows stay in LDS while the MLP runs, h never exists in HBM.
 * Supported: bf16, channels 32 or 64; else CDSEG_ERR_UNSUPPORTED. */
int cdseg_attn_tail_fused(const void* o, int ldo, const void* wp, const float* bp, const float* ln_g, const float* ln_b,
                          float ln_eps, const void* w1, const float* b1, const void* w2, const float* b2, float* x, int ldx,
                          void* xc, int ldxc, long n, int channels, int dtype, void* stream);

/* Block head after the sparse conv in ONE launch (ptv3.py:401-414): x += LN_cpe(y Wl^T + bl) [+ colbias];
 * h = LN1(x); qkv (n, ldqkv) = h Wqkv^T + bqkv.  y (n, ldy) = conv output; h never exists in HBM.
 * qkv_flags: 0, or CDSEG_ATTN_V_BF16 = write the v third of qkv as bfloat16 whatever the build's 16-bit type is (pass the
 * same flag to cdseg_attention_ex; a no-op in the bfloat16 build).
 * Supported: bf16, channels 32 or 64; else CDSEG_ERR_UNSUPPORTED. */
int cdseg_cpe_head_fused(const void* y, int ldy, const void* wl, const float* bl, const float* lnp_g, const float* lnp_b,
                         float* x, int ldx, const float* colbias, const float* ln1_g, const float* ln1_b, float eps,
                         const void* wqkv, const float* bqkv, void* qkv, int ldqkv, long n, int channels, int dtype,
                         int qkv_flags, void* stream);

/* ------------------------------------------------------------------ 3x3x3 submanifold conv, wide stages
 * ref: spconv.SubMConv3d call sites ptv3.py:356-362 (the CPE conv of every Block).  y (n, ldy) bf16 =
 * bias + sum_o x[nbr[o, i]] W_o^T for C_in = C_out = channels in {32, 64}, bf16: weights stationary in LDS, gathered rows
 * loaded straight into MFMA fragments (csrc/conv.hip).  wimg = fragment-order image of the (C, 27*C) weight, built once
 * per weight tensor by cdseg_subm_conv3_pack into a caller-owned buffer of cdseg_subm_conv3_wimg_bytes(channels) bytes.
 * nbr: OFFSET-MAJOR (27, n) kernel map.  Other shapes / dtypes: CDSEG_ERR_UNSUPPORTED (use cdseg_gemm with nbr). */
size_t cdseg_subm_conv3_wimg_bytes(int channels);
int cdseg_subm_conv3_pack(const void* w, int channels, void* wimg, void* stream);
int cdseg_subm_conv3(const void* x, int ldx, const void* wimg, const float* bias, const int32_t* nbr_kmajor, long n,
                     int channels, void* y, int ldy, void* stream);

/* ------------------------------------------------------------------ stem (k = 5) without a materialised kernel map
 * ref: ptv3.py:633-663 (Embedding: SubMConv3d(c_in -> 32, k = 5, bias = False) + BatchNorm1d(eps 1e-3) + GELU).
 * The <= 125 neighbours of a point are enumerated through the next coarser level (27 parent cells x <= 8 children);
 * bf16 operands, fp32 accumulation (csrc/stem.hip).  x8 (n, 8) bf16 rows in physical order (channels zero-padded),
 * wimg = cdseg_stem5_pack image (MFMA fragment order, cdseg_stem5_wimg_bytes) of the (32, 125 * 8) 16-bit weight, scale / shift = folded BatchNorm, grid (n, 3),
 * cluster (n) parent of every point, parent_nbr3 (27, m) offset-major 3x3x3 map of the parent level,
 * child_info (m) from cdseg_child_info(fine z-codes, children runs).  out (n, 32) fp32, out2 (n, 32) bf16 or NULL. */
int cdseg_child_info(const int64_t* zcode_sorted, const int32_t* seg_start, long m, int64_t* info, void* stream);
size_t cdseg_stem5_wimg_bytes(void);
int cdseg_stem5_pack(const void* w, void* wimg, void* stream);
int cdseg_stem5(const void* x8, const void* wimg, const float* scale, const float* shift, const int32_t* grid,
                const int32_t* cluster, const int32_t* parent_nbr3, const int64_t* child_info, long n, long m, int depth,
                float* out, void* out2, void* stream);

/* ------------------------------------------------------------------ Block head / tail on weight images (16-bit trunk)
 * Same contracts as cdseg_cpe_head_fused / cdseg_attn_tail_fused (ptv3.py:401-427), two machine mappings chosen by the
 * channel count:
 *   C = 32 / 64   (csrc/blockrr.hip) all weights of the kernel resident in LDS as MFMA fragments, a wave owns 32 points,
 *                 the activations never leave registers;
 *   C = 128 / 256 (csrc/deep.hip) the activations of a 128- (or 32-) row tile resident in LDS for the whole chain of products,
 *                 the weights streamed L2 -> registers: a wave owns 32 output channels of every product, its fragments are
 *                 stored in the image in the order it consumes them.
 * Images: cdseg_block_rr_img_bytes(C, 0 = head | 1 = tail) bytes; cdseg_block_rr_pack builds them once per Block from the
 * 16-bit row-major weights (head: cpe linear (C,C), qkv (3C,C); tail: proj (C,C), fc1 (4C,C), fc2 (C,4C)); either image
 * pointer may be NULL.  Other channel counts: CDSEG_ERR_UNSUPPORTED (cdseg_gemm + cdseg_layernorm sequences). */
size_t cdseg_block_rr_img_bytes(int channels, int which);
int cdseg_block_rr_pack(int channels, const void* wl, const void* wqkv, void* head_img, const void* wp, const void* w1,
                        const void* w2, void* tail_img, void* stream);
int cdseg_cpe_head_rr(const void* y, int ldy, const void* head_img, const float* bl, const float* lnp_g, const float* lnp_b,
                      float* x, int ldx, const float* colbias, const float* ln1_g, const float* ln1_b, float eps,
                      const float* bqkv, void* qkv, int ldqkv, long n, int channels, int qkv_flags /* as above; deep stages only */,
                      void* stream);
int cdseg_attn_tail_rr(const void* o, int ldo, const void* tail_img, const float* bp, const float* ln_g, const float* ln_b,
                       float eps, const float* b1, const float* b2, float* x, int ldx, void* xc, int ldxc, long n,
                       int channels, void* stream);
/* The tail with a say in what it writes (cdseg_attn_tail_rr is this call with flags 0 and no logit arguments).  The tail is
 * bound by HBM traffic: 4 C bytes of x and 2 C of xc per row are a third each of what it moves.
 *   flags & CDSEG_BLOCK_X_DEAD: the caller will not read x after this call; its contents are UNSPECIFIED on return.  The
 *     C = 32 / 64 kernel then leaves the rows as it read them and stores xc alone, bit-identical to the unflagged call; the
 *     deep-stage tails (C >= 128) write x as always.
 *   logits != NULL (C = 64): neither x nor xc is written (xc may be NULL); the kernel forms the segmentation head on the
 *     final fp32 row it holds in registers, logits[out_idx ? out_idx[row] : row][k] = sum_c head_w[k][c] x[c] + head_b[k]
 *     (head_w (num_classes, C) fp32 row-major, head_b (num_classes) fp32 or NULL, out_idx (n) as in cdseg_gemm_args: a
 *     negative entry writes the row nowhere), operands and accumulation in fp32.  It needs num_classes % 4 == 0, the head's
 *     weights in what the tail's workgroup has left of 80 KB of LDS (num_classes <= 20 at C = 64), logits 16-byte aligned and
 *     ld_logits % 4 == 0; anything else is CDSEG_ERR_UNSUPPORTED before any launch, nothing written.
 * Route record (cdseg_route_read): the kernel id stays tail_rr_kernel<C>; aux says what the launch left unwritten. */
#define CDSEG_BLOCK_X_DEAD 1
#define CDSEG_TAIL_AUX_X_SKIPPED 1 /* aux bit 0: the fp32 rows of x were not stored */
#define CDSEG_TAIL_AUX_LOGITS 2    /* aux bit 1: the launch wrote the logits and neither x (bit 0 is set too) nor xc */
int cdseg_attn_tail_rr_ex(const void* o, int ldo, const void* tail_img, const float* bp, const float* ln_g, const float* ln_b,
                          float eps, const float* b1, const float* b2, float* x, int ldx, void* xc, int ldxc, long n,
                          int channels, int flags, float* logits, int ld_logits, const float* head_w, const float* head_b,
                          const int32_t* out_idx, int num_classes, void* stream);
/* Deep stages only (C = 128 / 256 / 512): the same two launches with the residual rows READ from one buffer (x / x_in) and
 * WRITTEN to another (x_out / x; they may alias, which gives the in-place forms above).  With distinct buffers, launches of
 * few rows (a single scene's deep stages: 32-row tiles on a fraction of the CUs) cut a tile's weight stream over several
 * workgroups - the head one per q / k / v column block, the tail by MLP hidden chunks through the fp32 workspace `ws`
 * (>= 4 * n * C * 4 bytes for the four-way split, 16-byte aligned; NULL / smaller: fewer or no splits) and a fixed-order
 * reduce launch.  Results do not depend on scheduling; they differ from the unsplit form by fp32 summation order only.
 * (ref: the Block's cpe linear + norms + qkv, ptv3.py:401-414, and proj + norm2 + MLP, ptv3.py:416-427) */
int cdseg_cpe_head_rr2(const void* y, int ldy, const void* head_img, const float* bl, const float* lnp_g, const float* lnp_b,
                       const float* x, int ldx, float* x_out, int ldx_out, const float* colbias, const float* ln1_g,
                       const float* ln1_b, float eps, const float* bqkv, void* qkv, int ldqkv, long n, int channels,
                       int qkv_flags, void* stream);
int cdseg_attn_tail_rr2(const void* o, int ldo, const void* tail_img, const float* bp, const float* ln_g, const float* ln_b,
                        float eps, const float* b1, const float* b2, const float* x_in, int ldx_in, float* x, int ldx, void* xc,
                        int ldxc, long n, int channels, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ native Block executor
 * One PTv3 Block (ref: ptv3.py:399-428, eval mode) per call: the library issues every launch of the
 * block itself, carving its temporaries from the caller's scratch buffer: sparse-conv CPE, then for the 16-bit trunk with
 * C = 32 / 64 the fused head (cdseg_cpe_head_fused), window attention and the fused tail (cdseg_attn_tail_rr), with
 * C = 128 / 256 and head_img / tail_img given the deep-stage head and tail (cdseg_cpe_head_rr / cdseg_attn_tail_rr);
 * otherwise Linear+LayerNorms, QKV, attention, proj, MLP as separate launches.
 * Replaces ~10 host round trips through the binding by one.  Weights are described once (cdseg_block_desc), the per-scene tensors per call
 * (cdseg_block_io). */
typedef struct cdseg_block_desc {
  int dtype;       /* compute dtype T of weights / operand activations */
  int channels;    /* C */
  int heads;       /* C / 16 */
  int hidden;      /* MLP hidden width */
  float attn_scale;
  float ln_eps;
  const void* cpe_conv_w;  /* (C, 27*C) T */
  const float* cpe_conv_b;
  const void* cpe_lin_w;   /* (C, C) T */
  const float* cpe_lin_b;
  const float* cpe_ln_g;
  const float* cpe_ln_b;
  const float* norm1_g;
  const float* norm1_b;
  const void* qkv_w;       /* (3C, C) T */
  const float* qkv_b;
  const void* proj_w;      /* (C, C) T */
  const float* proj_b;
  const float* norm2_g;
  const float* norm2_b;
  const void* fc1_w;       /* (hidden, C) T */
  const float* fc1_b;
  const void* fc2_w;       /* (C, hidden) T */
  const float* fc2_b;
  const void* cpe_conv_wimg; /* cdseg_subm_conv3_pack image of cpe_conv_w, or NULL: the conv runs on cdseg_gemm */
  const void* head_img;      /* cdseg_block_rr_pack images (C = 32 / 64 / 128 / 256), or NULL: the unfused / tile-fused launches */
  const void* tail_img;
  int attn_flags;            /* CDSEG_ATTN_Q_PRESCALED when qkv_w / qkv_b (and the images built from them) carry
                                attn_scale * log2(e) in their q rows (the engine folds it at load time) */
} cdseg_block_desc;

typedef struct cdseg_block_io {
  long n;                  /* points at this stage */
  float* x;                /* (n, C) fp32 residual stream, updated in place */
  const void* xc_in;       /* (n, C) T: CPE conv input (sparse_conv_feat of the reference) */
  void* xc_out;            /* (n, C) T: shadow copy of the block output (may alias x when T is fp32) */
  const float* tbias;      /* (C) timestep bias or NULL */
  const int32_t* nbr;      /* (27, n) OFFSET-MAJOR kernel map of the stage (cdseg_nbr_table with kmajor = 1) */
  const int32_t* gidx;     /* attention slot plan of the block's curve */
  const int32_t* widx;
  const int32_t* patch_start;
  int num_patches;
  int max_len;
  void* scratch;           /* >= cdseg_block_scratch_bytes(desc, n) */
  size_t scratch_bytes;
  unsigned long long* sat_counter; /* NULL, or (diagnostic, IEEE-half build): += clamped values seen in this Block's 16-bit
                                      buffers that reach memory (cdseg_count_saturated); costs a few extra launches */
  /* What the caller reads of the Block's outputs (trailing fields, all zero = everything, as before they existed; see
   * cdseg_attn_tail_rr_ex).  flags & CDSEG_BLOCK_X_DEAD: x is not read after this call and is UNSPECIFIED on return; ignored
   * when xc_out aliases x (there is no second copy), honoured by the C = 32 / 64 register-resident tail, ignored by every other
   * path.  logits .. ld_logits: the Block is the model's last and its tail writes the segmentation logits INSTEAD of x and
   * xc_out, which are then both unspecified (xc_out must still be a valid pointer; the saturation diagnostic skips it).  Only
   * the register-resident tail can: CDSEG_ERR_UNSUPPORTED, before any launch of the Block, when this call would take another
   * path or the head does not fit (cdseg_attn_tail_rr_ex) - the caller then runs the Block without them and the head itself. */
  int flags;
  float* logits;           /* (rows, ld_logits) fp32 or NULL */
  const float* head_w;     /* (num_classes, C) fp32 row-major */
  const float* head_b;     /* (num_classes) fp32 or NULL */
  const int32_t* out_idx;  /* (n) or NULL: Block row -> logits row */
  int num_classes;
  int ld_logits;
} cdseg_block_io;

size_t cdseg_block_scratch_bytes(const cdseg_block_desc* desc, long n);
int cdseg_block_forward(const cdseg_block_desc* desc, const cdseg_block_io* io, void* stream);

/* ------------------------------------------------------------------ native plan builder (round 6)
 * ref: models/utils/structure.py:47-102 (Point.serialization), ptv3.py:188-250 (padding plan), :477-505 (pooling structure).
 * The integer side of one forward - (batch | z) sort, level-0 codes, all pooled levels, links, 3x3x3 kernel maps, curve orders,
 * padding tables, slot plans - in TWO library calls around the forward's one host read (the pooled sizes), written into two
 * caller-owned arenas (int32 / int64 elements; every item starts on a 256-byte boundary).  Same kernels, same results as the
 * per-op entry points above (tests/test_gpu_e2e.py::test_native_plan_equals_per_op_plan); exists because a single scene's
 * plan phase was bound by ~40 binding round trips, not by the device (csrc/plan.hip).
 * Level indices: 0 = the input resolution, 1 .. nlev the pooled levels in ascending cumulative pooling depth. */
#define CDSEG_PLAN_MAX_LEVELS 8
#define CDSEG_PLAN_MAX_LINKS 16
#define CDSEG_PLAN_MAX_PADS 4
typedef struct cdseg_plan_spec {
  int nlev;            /* pooled levels (1 .. 8) */
  int cum[9];          /* cumulative pooling depth per level index, cum[0] = 0, strictly ascending */
  int ncurve;          /* curves other than z in use (0 .. 3) */
  int curve_rows[3];   /* their rows of the (4, n) code array: 1 = z-trans, 2 = hilbert, 3 = hilbert-trans */
  int nslot_curve;     /* curves that get slot plans (1 .. 4) */
  int slot_curve[4];   /* -1 = z (identity order), else an index into curve_rows */
  int nlink;           /* links a -> b between POOLED levels (1 <= a < b); the (0, l) links come out of the pooling pass.
                          Must contain (l, l + 1) for every pooled level l whose parent is one octree step up */
  int link_a[CDSEG_PLAN_MAX_LINKS];
  int link_b[CDSEG_PLAN_MAX_LINKS];
  int npad;            /* padding keys (1 .. 4) */
  int pad_patch[CDSEG_PLAN_MAX_PADS]; /* patch size */
  int pad_flash[CDSEG_PLAN_MAX_PADS]; /* enable_flash: K = patch size; else K = min(smallest batch element, patch size) */
} cdseg_plan_spec;

typedef struct cdseg_plan_begin_io {
  const void* grid;        /* (n, 3) int32 | int64 voxel coordinates, caller's point order */
  int grid_elem_bytes;
  const int64_t* offset;   /* (nb) cumulative batch offsets */
  int nb;
  long n;
  int depth;               /* serialization depth (structure.py:66) */
  int end_bit;             /* significant bits of the (batch | z) code */
  int32_t* i32;            /* arenas: cdseg_plan_begin_layout */
  int64_t* i64;
  void* ws;
  size_t ws_bytes;
  int64_t* gmax_host;      /* PINNED host word <- max(grid), or NULL */
  int32_t* meta_host;      /* PINNED host ints <- cdseg_pool_levels' meta (nlev * (1 + nb) + 1), or NULL */
} cdseg_plan_begin_io;

/* off_out[13]: offsets (elements) of batch, perm0, grid0, bat0, last_idx, cluster (nlev, n), seg_start (nlev, n + 1), meta,
 * orders0 (ncurve, n) in the int32 arena, then gmax, zcode, zcode_sorted, code0 (4, n) in the int64 arena.
 * totals_out[3]: int32 elements, int64 elements, workspace bytes. */
int cdseg_plan_begin_layout(const cdseg_plan_spec* spec, long n, int nb, long* off_out, long* totals_out);
/* phase 0: everything up to the two asynchronous host copies; phase 1: the level-0 orders of the non-z curves (one sort) -
 * independent of the host read, so the caller records its event between the phases and waits for it after phase 1 is queued */
int cdseg_plan_begin(const cdseg_plan_spec* spec, const cdseg_plan_begin_io* io, int phase, void* stream);

typedef struct cdseg_plan_finish_io {
  long n;
  int nb;
  int depth;
  const long* m_host;      /* (nlev) pooled sizes, from meta */
  const int* offs_host;    /* (nlev + 1, nb + 1) batch offsets of every level index, level 0 first */
  const int32_t* grid0;    /* items of the begin arena */
  const int32_t* bat0;
  const int64_t* code0;
  const int32_t* cluster;
  const int32_t* seg;
  const int32_t* orders0;
  int32_t* i32;            /* arenas: cdseg_plan_finish_layout */
  int64_t* i64;
  void* ws;
  size_t ws_bytes;
  int32_t* pads_host;      /* PINNED staging buffer for the padding tables (>= info_out[3] ints), free again once the call's
                              copy has run */
} cdseg_plan_finish_io;

/* off_out (element offsets), in this order: per pooled level l = 1 .. nlev: grid (int32 arena), batch (int32), code4 (int64);
 * per link: cluster, seg_start (int32); per level 0 .. nlev: nbr3 (27, m_l) offset-major (int32); per level 0 .. nlev:
 * child_info (int64) or -1; the coarse-order base (int32: level l / curve c at base + ncurve * sum_{1 <= l' < l} m_l' + c * m_l);
 * per (level 0 .. nlev, pad key): offs, offs_pad, patch_start (int32); slot gidx base, slot widx base (int32: the plan of
 * (level, pad key, slot curve), in that nesting, starts at the sum of the n_pad of the plans before it).
 * info_out: int32 elements, int64 elements, workspace bytes, padding-table ints, padding-table base; then per (level, pad key):
 * K, n_pad, patches, longest patch, sum of squared patch lengths (a double's bits). */
int cdseg_plan_finish_layout(const cdseg_plan_spec* spec, long n, int nb, const long* m_host, const int* offs_host,
                             long* off_out, long* info_out);
int cdseg_plan_finish(const cdseg_plan_spec* spec, const cdseg_plan_finish_io* io, void* stream);

/* ------------------------------------------------------------------ training path (exact fp32; the attention core also in 16 bits)
 * ref: pointcept/models/default.py:424-493 (training forward), pointcept/engines/train.py:216-271 (loss.backward());
 *      what autograd differentiates: ptv3.py:246-296 (SerializedAttention core), ptv3.py:399-428 (Block tail).
 * cdseg_attention_bwd: gradients of cdseg_attention's inputs.  dout (rows, H*16) is the gradient of its output; dq / dk /
 *   dv are ACCUMULATED into (+=, the caller zeroes them) at the gathered rows - a point that the padding plan put into
 *   two slots collects both (the backward of the reference's `qkv[order]` gather); slots without an output row (widx -1)
 *   receive no output gradient but still act as keys.  num_slots = patch_start[num_patches]; max_len = the longest patch,
 *   <= 1024 (the patch-head lives in LDS: longer -> CDSEG_ERR_UNSUPPORTED).  ws: cdseg_attention_bwd_ws_bytes (one size,
 *   sufficient for either dtype).  dtype is that of q, k, v and dout; dq, dk, dv are fp32 in both forms:
 *     CDSEG_F32   exact fp32 (the backward of the parity mode's forward).
 *     CDSEG_BF16  the build's 16-bit type: the recompute-P backward of the 16-bit forward (flags 0) on the 16-bit matrix
 *                 pipe.  Differentiates what that forward computes: q' = q * fp32(scale * log2 e) rounded once to the
 *                 16-bit type (the rounding counts as the identity), s' = q'.k, P = exp2(s' - m') / l.  The row statistics
 *                 (m', l, D = sum_j P dP) are recomputed here in fp32 with the exact row maximum; P and dS = P (dP - D) are
 *                 rounded to the 16-bit type as MFMA operands only; all accumulators are fp32.  dout is not clamped and dS
 *                 is converted without saturation (half build): a gradient beyond the 16-bit range arrives as inf / NaN.
 *   Alignment (CDSEG_ERR_ARG otherwise): every pointer 16-byte aligned; ldq, ldk, ldv, lddo (in elements) multiples of 4
 *   (CDSEG_F32) or of 8 (CDSEG_BF16), i.e. 16-byte rows; lddq, lddk, lddv multiples of 4; every one of the seven strides
 *   at least the row, num_heads * 16 elements.
 * cdseg_layernorm_bwd: dx (=, or += when accumulate) for y = LayerNorm(x) * gamma + beta; optional dgamma / dbeta (+=).
 *   CDSEG_ERR_ARG: a NULL x, gamma, dy or dx, a pointer that is not 4-byte aligned, or ldx, lddy or lddx < c (scalar
 *   accesses: any stride from c on, odd ones included).
 * cdseg_gelu_bwd: dx = dy * d/du GELU(u) on the pre-activation u (erf form, torch.nn.GELU()).
 * cdseg_linear_wgrad: dw[n][k] += sum_m dy[m][n] * x[row(m)][k] and (db != NULL) db[n] += sum_m dy[m][n], fp32; row(m) = m,
 *   or xidx[m] with -1 = skip: ONE kernel offset of a submanifold conv (xidx = that offset's row of the offset-major kernel
 *   map, dw = the offset's (Cout, Cin) slice of the (Cout, 27, Cin) weight, lddw = 27 * Cin; ref: spconv.SubMConv3d weight
 *   gradient, ptv3.py:356-362).  n, k multiples of 16.  Accumulates (the caller zeroes dw / db); partial sums are added
 *   with fp32 atomics (summation order not fixed).  The DATA gradient of a Linear / of the conv needs no entry point of
 *   its own: it is cdseg_gemm on the transposed weight / on the mirrored, transposed kernel (W'[ci][o][co] = W[co][26-o][ci])
 *   with the same kernel map.
 *   CDSEG_ERR_ARG: a NULL x, dy or dw, a pointer that is not 4-byte aligned, or a stride shorter than its row: ldx < k,
 *   lddy < n, lddw < k (cdseg_conv_wgrad: ldx < cin, lddy < cout; its dw is contiguous).  Any stride from the row length on
 *   is taken, odd ones included (scalar accesses). */
size_t cdseg_attention_bwd_ws_bytes(long num_slots, int num_heads);
int cdseg_attention_bwd(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const int32_t* q_gidx,
                        const int32_t* kv_gidx, const int32_t* widx, const int32_t* patch_start, int num_patches,
                        int num_heads, long num_slots, int max_len, float scale, const void* dout, int lddo, void* dq,
                        void* dk, void* dv, int lddq, int lddk, int lddv, int dtype, void* ws, size_t ws_bytes, void* stream);
int cdseg_layernorm_bwd(const float* x, int ldx, const float* gamma, float eps, const float* dy, int lddy, float* dx, int lddx,
                        int accumulate, float* dgamma, float* dbeta, long m, int c, void* stream);
int cdseg_gelu_bwd(const float* u, const float* dy, float* dx, long n, void* stream);
int cdseg_linear_wgrad(const float* x, int ldx, const int32_t* xidx, const float* dy, int lddy, long m, int k, int n, float* dw,
                       int lddw, float* db, void* stream);
/* all kvol offsets of a submanifold conv in one launch: dw (cout, kvol, cin) += ..., db (cout) += column sums of dy;
 * nbr_kmajor: the (kvol, m) offset-major kernel map */
int cdseg_conv_wgrad(const float* x, int ldx, const int32_t* nbr_kmajor, int kvol, const float* dy, int lddy, long m, int cin,
                     int cout, float* dw, float* db, void* stream);
/* The same two weight gradients on 16-bit operands (training under AMP, train_precision "fp16-amp" / "bf16-amp"): x and dy
 * are of the build's 16-bit type (bfloat16, or IEEE half in the half build), dw / db stay fp32 and are accumulated into.
 * Semantics, row(m), the offset-major map and the (cout, kvol, cin) layout are those of the fp32 forms above.  Products of
 * 16-bit values are exact and every sum is fp32 (v_mfma_f32_32x32x16 accumulators, fp32 atomics for the partial tiles, order
 * not fixed): no partial sum is rounded to 16 bits.  An inf / NaN in dy (a scaled gradient beyond half's range, cast
 * without saturation) arrives in the dw rows and the db entry of its column, where a GradScaler finds it.
 * Row chunks staged row-major in LDS, both operands read with ds_read_b64_tr_b16; a chunk of 64 rows in which the offset
 * has no live neighbour is skipped.
 *   CDSEG_ERR_ARG: a pointer that is not 16-byte aligned, ldx / lddy (in elements) not a multiple of 8, or a stride
 *   shorter than its row (ldx < k, lddy < n, lddw < k; lddw is in fp32 elements and need not be a multiple of anything).
 *   CDSEG_ERR_UNSUPPORTED: n, k (cin, cout) not multiples of 16 (a 16-wide shape runs as a zero-padded 32-wide tile).
 *   m <= 0: CDSEG_OK, nothing written. */
int cdseg_linear_wgrad16(const void* x, int ldx, const int32_t* xidx, const void* dy, int lddy, long m, int k, int n, float* dw,
                         int lddw, float* db, void* stream);
int cdseg_conv_wgrad16(const void* x, int ldx, const int32_t* nbr_kmajor, int kvol, const void* dy, int lddy, long m, int cin,
                       int cout, float* dw, float* db, void* stream);

/* ------------------------------------------------------------------ dropout (training only: attn_drop, proj_drop)
 * ref: ptv3.py:282-288, :1038-1047 (flash-attention's dropout_p = attn_drop), :293-294, :1052-1053 (proj_drop),
 *      :316-322 (MLP.drop).  The masks are this library's own; they are not torch's nor flash-attention's.
 *
 * The mask.  A dropout site is a pair (seed, offset).  Its random bytes are words of the cdseg_rand_int stream of that
 * pair: W(t) = the four 32-bit words cdseg_rand_int(out, 4, seed, offset, NULL, 0) would write at out[4 t .. 4 t + 3], i.e.
 * Philox4x32-10 under key (seed low, seed high) at counter (t low, t high, offset low, offset high).  Byte b of a word is
 * (word >> 8 b) & 255.
 *   threshold  T = floor(256 * (1 - rate) + 1/2), computed in double, and at least 1.  An element is KEPT iff its byte < T
 *              and kept values are multiplied by 256 / T (rounded to fp32): the effective keep probability is T / 256, the
 *              8-bit granularity of flash-attention.  A rate below 1/512 has T = 256: nothing is dropped and the factor is 1
 *              (the attention entry points then run cdseg_attention / cdseg_attention_bwd themselves).  A rate above
 *              1 - 1/512 keeps T = 1.  A rate outside [0, 1) (or NaN) is CDSEG_ERR_ARG.
 *   attention  element (patch p, head h, query slot i, key slot j), slots counted from the start of the patch (i, j < 1024,
 *              h < 65536):  t = (j >> 2) | (i >> 2) << 8 | h << 16 | p << 32,  word i & 3,  byte j & 3.
 *              One call is a 4 x 4 block of the (query, key) plane.  A lane of every kernel holds, per tile, either four
 *              consecutive keys of one query (one word) or four consecutive queries of one key (the same byte of the four
 *              words), so one call feeds four accumulator elements in the forward and in all four backward kernels; more
 *              per call would serve one orientation and starve the other.  (The 16-bit kernels' lanes hold four such
 *              blocks per tile and share them with the three other lanes of their quad: one call per lane for 16 elements.)
 *   element    element (row r, column c) of the (m, c) tensor as passed (r < 2^32):
 *              t = (c >> 4) | r << 32,  word (c >> 2) & 3,  byte c & 3  - 16 consecutive columns of a row per call.
 * The decision depends on (seed, offset, p, h, i, j) - or (seed, offset, r, c) - and on nothing else: not on the tile order,
 * the wave count or the kernel variant, not on the dtype or the build, not on forward or backward.
 *
 * cdseg_attention_drop: cdseg_attention with O = ((M / keep) o softmax(scale Q K^T)) V, M the mask above and keep = T / 256;
 *   dtype CDSEG_F32, or CDSEG_BF16 (the build's 16-bit type, flags 0: q' = q * fp32(scale log2 e) rounded once).  The softmax
 *   denominator runs over all keys, dropped or not.  A padding-duplicate slot (widx -1) is a key like any other with mask
 *   elements of its own.  16-bit form: fp32 statistics with the exact row maximum; (M / keep) o P is rounded to the 16-bit
 *   type once, as the MFMA operand; fp32 accumulator; the output is rounded as cdseg_attention's.
 * cdseg_attention_drop_bwd: cdseg_attention_bwd for that forward (same workspace, cdseg_attention_bwd_ws_bytes):
 *   dV = ((M/keep) o P)^T dO,  dP = (dO V^T) o (M/keep),  D = sum_j P dP,  dS = P (dP - D),  dQ = scale dS K,  dK = scale dS^T Q.
 *   Rounding and accumulation as cdseg_attention_bwd: fp32 statistics, dout never clamped, (M/keep) o P and dS are the 16-bit
 *   MFMA operands and dS is converted without saturation (half build).
 *   Both: CDSEG_ERR_ARG for a bad rate, max_len > 1024, num_heads > 65535, a NULL operand, a pointer or a row (ld * element
 *   size; gradient rows: lddq, lddk, lddv multiples of 4) that is not 16-byte aligned; CDSEG_ERR_WORKSPACE as cdseg_attention_bwd.
 * cdseg_dropout: y = x o M / keep on an (m, c) fp32 tensor with row strides ldx, ldy >= c (elements); y may be x.  16-byte
 *   accesses when x, y are 16-byte aligned and ldx, ldy are multiples of 4, scalar ones otherwise (and on a ragged last group).
 *   It is its own backward: dx = cdseg_dropout(dy) with the same (seed, offset).  CDSEG_ERR_ARG: a bad rate, a NULL or not
 *   4-byte aligned pointer, ld < c, m >= 2^32. */
int cdseg_attention_drop(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const int32_t* q_gidx,
                         const int32_t* kv_gidx, const int32_t* widx, const int32_t* patch_start, int num_patches, int num_heads,
                         int max_len, float scale, void* out, int ldo, int dtype, double rate, uint64_t seed, uint64_t offset,
                         void* stream);
int cdseg_attention_drop_bwd(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const int32_t* q_gidx,
                             const int32_t* kv_gidx, const int32_t* widx, const int32_t* patch_start, int num_patches,
                             int num_heads, long num_slots, int max_len, float scale, const void* dout, int lddo, void* dq,
                             void* dk, void* dv, int lddq, int lddk, int lddv, int dtype, void* ws, size_t ws_bytes, double rate,
                             uint64_t seed, uint64_t offset, void* stream);
int cdseg_dropout(const float* x, int ldx, float* y, int ldy, long m, int c, double rate, uint64_t seed, uint64_t offset,
                  void* stream);

/* ------------------------------------------------------------------ deterministic training (fixed-order gradient reductions)
 * Opt-in forms of the reductions above whose fp32 summation order is FIXED, so that two runs of a training step give the
 * same bits.  The default entry points are unchanged.  Contract of the order:
 *   weight gradient   same tiling, main loop and row partition as the default form (dtype CDSEG_F32: the fp32 kernel,
 *                     CDSEG_BF16: the 16-bit kernel of this build).  Split s of the rows (cdseg_wgrad_partition) leaves its
 *                     partial dW tile and db partial in the workspace with plain stores (a split without live rows stores
 *                     zeros); a second launch computes  t = p[0]; t += p[1]; ... by ascending split index  and then
 *                     dw = dw + t, db = db + t_b: ONE add onto the existing content (accumulate-into, as above).
 *   LayerNorm         dx as the default form.  A 64-row block sums dgamma / dbeta as the default form does (per-wave
 *                     registers, the fixed 4-wave tree) and stores its partial row; a second launch adds the rows by
 *                     ascending block index, then dgamma = dgamma + t, dbeta = dbeta + t.  c <= 512, wider rows:
 *                     CDSEG_ERR_UNSUPPORTED (the default form handles them with per-element atomics).
 *   segment sum       out[j] = sum_i src[i], i = seg_start[j] .. seg_start[j + 1] - 1 ascending (out is overwritten; an empty
 *                     run gives 0): the backward of the unpooling gather child[cluster], whose children are contiguous.
 *                     CDSEG_ERR_ARG: a NULL src, seg_start or out, src / out / seg_start not 4-byte aligned, ld < c or
 *                     ldo < c (scalar accesses: any stride from c on, odd ones included).
 * No block waits for another; the library allocates nothing.  Status codes, checked before any launch:
 *   CDSEG_ERR_WORKSPACE    ws NULL or ws_bytes below the matching _ws_bytes query.
 *   CDSEG_ERR_ARG          CDSEG_BF16: as the 16-bit forms above (16-byte aligned pointers, ldx / lddy multiples of 8);
 *                          CDSEG_F32: a NULL or not 4-byte aligned operand; ws not 16-byte aligned (LayerNorm: 4-byte);
 *                          a stride shorter than its row, as in the default forms (ldx < k, lddy < n, lddw < k; LayerNorm:
 *                          ldx, lddy, lddx < c).
 *   CDSEG_ERR_UNSUPPORTED  another dtype; n, k (cin, cout) not multiples of 16.
 * The partition query is host only: the launch rule is a function of (m, n, k, kvol, dtype) alone (kvol = 1: the Linear form)
 * and never asks the device.  It returns the rows per split (the last split may be shorter) and the number of splits. */
int cdseg_wgrad_partition(long m, int n, int k, int kvol, int dtype, long* rows_per_split, int* splits);
size_t cdseg_wgrad_det_ws_bytes(long m, int n, int k, int kvol, int dtype);
int cdseg_linear_wgrad_det(const void* x, int ldx, const int32_t* xidx, const void* dy, int lddy, long m, int k, int n, float* dw,
                           int lddw, float* db, int dtype, void* ws, size_t ws_bytes, void* stream);
int cdseg_conv_wgrad_det(const void* x, int ldx, const int32_t* nbr_kmajor, int kvol, const void* dy, int lddy, long m, int cin,
                         int cout, float* dw, float* db, int dtype, void* ws, size_t ws_bytes, void* stream);
size_t cdseg_layernorm_bwd_det_ws_bytes(long m, int c);
int cdseg_layernorm_bwd_det(const float* x, int ldx, const float* gamma, float eps, const float* dy, int lddy, float* dx, int lddx,
                            int accumulate, float* dgamma, float* dbeta, long m, int c, void* ws, size_t ws_bytes, void* stream);
int cdseg_segment_sum(const float* src, int ld, const int32_t* seg_start, long m, int c, float* out, int ldo, void* stream);

/* ------------------------------------------------------------------ fused segmentation loss (csrc/loss.hip)
 * ref: losses/misc.py:95-132 (CrossEntropyLoss, reduction "mean"), losses/lovasz.py:118-165, 210-265 (multi-class
 * Lovasz-Softmax over the classes present, whole batch).  logits (n, c) fp32 with row stride ldl, labels (n) int64.
 *   valid rows: label != ignore_index (n_valid of them);  p = softmax(logits) per row, fp32
 *   CE = -(1 / n_valid) sum_valid log p[i, y_i]
 *   per present class c (a distinct label among the valid rows, P of them): fg_i = [y_i == c], err_i = |fg_i - p[i, c]| over
 *     the valid rows, sorted by err DESCENDING, TIES BY ASCENDING ROW INDEX (the reference leaves the tie order to an unstable
 *     sort; this rule makes the gradient a function of the input);  F_k / B_k = inclusive foreground / background counts,
 *     T = sum fg, jac_k = 1 - (T - F_k) / (T + B_k), d_0 = jac_0, d_k = jac_k - jac_{k-1}, L_c = sum_k err_(k) d_k
 *   Lovasz = (1 / P) sum_c L_c
 *   backward (jac is a constant, as in the reference): coef[i, c] = -+ d_rank(i, c) / P (- on foreground rows),
 *     dCE / dlogit[i, j] = (p_ij - [j == y_i]) / n_valid,  dLovasz / dlogit[i, j] = p_ij (coef_ij - sum_k coef_ik p_ik);
 *     ignored rows get zeros.
 * Two phases around the caller's ONE host read:
 *   phase 0  hist (c + 1 int32, device) <- rows per class over the valid rows; hist[c] = labels outside [0, c) that are not
 *            ignore_index (a caller error).  Needs logits / labels / hist only.
 *   phase 1  hist_host = the caller's host copy of hist.  out[0] = CE, out[1] = Lovasz (device floats);
 *            coef (n, P) fp32, row stride P: column r = the r-th present class in ascending class order; rows of ignored
 *            points are not written.  ws from cdseg_seg_loss_ws_bytes(n, c) (sized for P = c), 16-byte aligned.
 * cdseg_seg_loss_bwd: dlogits (n, c; row stride lddl) = g_ce[0] * dCE + g_lovasz[0] * dLovasz, one launch that recomputes p;
 *   g_ce / g_lovasz are DEVICE floats (NULL = 0), hist_host and coef as in phase 1.
 * Every float sum runs in an order fixed by the shape (no float atomics): equal inputs give equal bits.
 * Status codes, checked before any launch:
 *   CDSEG_ERR_ARG          NULL / misaligned pointer, n <= 0, c <= 0, ld < c, another phase; hist_host with hist_host[c] != 0,
 *                          counts beyond n or NO valid row (the empty batch has no fused form: nan / 0 are the caller's)
 *   CDSEG_ERR_UNSUPPORTED  n >= 2^24 or c > 256 (the 64-bit sort key: 8 bits class rank, 31 bits error, 24 bits row, 1 bit fg)
 *   CDSEG_ERR_WORKSPACE    ws NULL, ws_bytes below the query, or (phase 1) below what the sort of the n x P keys needs.
 *   CDSEG_ERR_LAUNCH       (phase 1, before any launch) the sort's storage query failed - no device.
 * cdseg_seg_loss_ws_bytes asks rocPRIM on the current device; without a device the sort's share cannot be sized and is left
 * out (a lower bound). */
size_t cdseg_seg_loss_ws_bytes(long n, int c);
int cdseg_seg_loss_fwd(const float* logits, int ldl, const int64_t* labels, long n, int c, long ignore_index, int phase,
                       int32_t* hist, const int32_t* hist_host, float* out, float* coef, void* ws, size_t ws_bytes,
                       void* stream);
int cdseg_seg_loss_bwd(const float* logits, int ldl, const int64_t* labels, long n, int c, long ignore_index,
                       const int32_t* hist_host, const float* coef, const float* g_ce, const float* g_lovasz, float* dlogits,
                       int lddl, void* stream);

/* ------------------------------------------------------------------ train-mode BatchNorm + GELU, pooling maximum (csrc/norm.hip)
 * ref: nn.BatchNorm1d (training) -> nn.GELU at the stems, SerializedPooling.norm and both projections of SerializedUnpooling
 * (ptv3.py:464-555, 597-663), nn.SyncBatchNorm (engines/train.py:275-276), torch_scatter.segment_csr(reduce = "max") and its
 * arg-max backward (ptv3.py:510-515).  fp32 tensors (rows, c) with a row stride; per channel j over the m rows:
 *   stats   = [sum_i x_ij (c), sum_i x_ij^2 (c), m]  in fp64: 2 c + 1 doubles.  Buffers of several row shards (ranks) merge by
 *             plain addition; fp64 sums of fp32 data keep E[x^2] - mean^2 safe.
 *   mean_j  = stats[j] / n, var_j = max((n stats[c + j] - stats[j]^2) / n^2, 0) with n = stats[2 c] (read on the device; both
 *             products are carried exactly, so the difference loses nothing beyond the rounding the sums carry),
 *   invstd_j = 1 / sqrt(var_j + eps), all in fp64 and rounded to fp32 once; the running buffers (each may be NULL) are updated
 *             in place like nn.BatchNorm1d: r = (1 - momentum) r + momentum v, v = mean for running_mean and the UNBIASED
 *             variance var n / (n - 1) for running_var (n <= 1: var itself; the caller refuses that case).
 *   x_hat   = (x - mean) invstd,  z = fma(gamma, x_hat, beta),  y = GELU(z) = z erfc(-z / sqrt 2) / 2; every element-wise
 *             expression here and in the backward is evaluated in fp64 from the fp32 operands and rounded to fp32 once
 *   backward: g = dy GELU'(z) with z and x_hat recomputed from x (nothing but x, mean, invstd is kept),
 *             gsums = [sum_i g_ij (c), sum_i g_ij x_hat_ij (c)] in fp64: 2 c doubles (dbeta and dgamma, mergeable like stats),
 *             dx = gamma invstd (g - gsums[j] / n - x_hat gsums[c + j] / n), gsums and n = count[0] (fp64) read on the device:
 *             under SyncBN the caller passes the merged ones.  A non-finite dy reaches dx.
 * Summation order: block b of the partition owns the rows [b rows_per_block, (b + 1) rows_per_block); inside a block a lane
 * adds its rows by ascending index and the block's row slots are added by ascending slot; the block partials (in ws) are
 * added by a second launch as t = p[0]; t += p[1]; ... by ascending block index.  No float atomics: equal inputs give equal
 * bits, on every device.  The partition query is host only and a function of (m, c) alone.
 * Pooling maximum: out[j] = max over the rows seg_start[j] .. seg_start[j + 1] - 1 of y (runs are not empty), bit for bit
 * what the segment maximum above gives with scale 1, shift 0 and no activation; arg[j] (int32) = the FIRST row, ascending,
 * that holds the maximum (-1 for a run of NaNs only).  Backward over the n fine rows, every element written exactly once:
 *   dy[i] = arg[cluster[i]] == i ? dout[cluster[i]] : 0   per channel (no zero fill, no atomics).
 * Status codes, checked before any launch; m = 0 (n = 0) returns CDSEG_OK without one:
 *   CDSEG_ERR_UNSUPPORTED  c not a multiple of 16 in [16, 512]; 2^31 rows or more (pooling maximum: arg is int32).
 *   CDSEG_ERR_ARG          a NULL operand; an fp32 / int32 (rows, c) tensor or per-channel vector that is not 16-byte aligned
 *                          (every lane moves 16 bytes); a row stride below c or not a multiple of 4; an fp64 buffer not
 *                          8-byte aligned; m < 0; eps < 0; momentum outside [0, 1]; ws not 16-byte aligned.
 *   CDSEG_ERR_WORKSPACE    ws NULL or ws_bytes below the query. */
int cdseg_bn_partition(long m, int c, long* rows_per_block, int* blocks);
size_t cdseg_bn_ws_bytes(long m, int c);
int cdseg_bn_stats(const float* x, int ldx, long m, int c, double* stats, void* ws, size_t ws_bytes, void* stream);
int cdseg_bn_finish(const double* stats, int c, double eps, double momentum, float* mean, float* invstd, float* running_mean,
                    float* running_var, void* stream);
int cdseg_bn_gelu_fwd(const float* x, int ldx, long m, int c, const float* mean, const float* invstd, const float* gamma,
                      const float* beta, float* y, int ldy, void* stream);
int cdseg_bn_gelu_bwd_sums(const float* x, int ldx, const float* dy, int lddy, long m, int c, const float* mean,
                           const float* invstd, const float* gamma, const float* beta, double* gsums, void* ws, size_t ws_bytes,
                           void* stream);
int cdseg_bn_gelu_bwd_dx(const float* x, int ldx, const float* dy, int lddy, long m, int c, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, const double* gsums, const double* count, float* dx, int lddx,
                         void* stream);
int cdseg_segment_max_arg(const float* y, int ldy, const int32_t* seg_start, long m, int c, float* out, int ldo, int32_t* arg,
                          int lda, void* stream);
int cdseg_segment_max_bwd(const float* dout, int lddo, const int32_t* arg, int lda, const int32_t* cluster, long n, int c,
                          float* dy, int lddy, void* stream);

/* ------------------------------------------------------------------ gate of the Feature Fusion Module (csrc/fusion.hip)
 * ref: CrossBlock, ptv3.py:1196-1206: q_point.feat = q_shortcut + feat_scale * attn, or (1 - feat_scale) * q_shortcut +
 * feat_scale * attn, with attn behind DropPath.  Contiguous fp32 (rows, c) tensors; s = q_shortcut, a = the projected
 * attention output, m (rows) = the per-row DropPath factor mask / keep (NULL = 1), alpha and gamma (c) = the per-channel
 * factors the caller derives from the mode (a scalar mode passes a broadcast vector; alpha = 1 or 1 - gamma):
 *   forward   y[r][j] = alpha[j] s[r][j] + gamma[j] m[r] a[r][j]       (a NULL, then m NULL too: y = alpha s).  y may be s.
 *   backward  ds = alpha dy,  da = gamma m dy  (ds may be dy), and sums (2 c doubles) = [sum_r dy m a (c), sum_r dy s (c)]:
 *             the gradient of every mode's feat_scale is a host expression of the two (d gamma = sums[j], d alpha = sums[c + j]).
 * Every element-wise expression is evaluated in fp64 from the fp32 operands and rounded to fp32 once; the column sums are
 * accumulated and returned in fp64.  Two paths, chosen per call: with c a multiple of 4 and every tensor and per-channel vector
 * 16-byte aligned every lane moves 16 bytes; any other width or alignment takes a scalar path with the same arithmetic.
 * Summation order: block b owns rows_per_block consecutive rows (64 at least, 256 blocks at most: a function of rows alone);
 * on the 16-byte path a lane adds its rows by ascending index and the block's row slots are added by ascending slot, as in the
 * BatchNorm sums above, on the scalar path one thread adds a column's rows of the block by ascending index; the block partials
 * (in ws, cdseg_fuse_gate_ws_bytes) are added by a second launch by ascending block index.  No float atomics: equal inputs on
 * the same path give equal bits.  Nothing outside y / ds, da, sums and ws_bytes of ws is written.
 * Status codes, checked before any launch; rows = 0 returns CDSEG_OK without one:
 *   CDSEG_ERR_UNSUPPORTED  c outside [1, 512].
 *   CDSEG_ERR_ARG          a NULL operand other than m (and a in the forward); m without a; a tensor or vector that is not
 *                          4-byte aligned; sums not 8-byte, ws not 16-byte aligned; rows < 0.
 *   CDSEG_ERR_WORKSPACE    ws NULL or ws_bytes below the query. */
size_t cdseg_fuse_gate_ws_bytes(long rows, int c);
int cdseg_fuse_gate_fwd(const float* s, const float* a, const float* m, const float* alpha, const float* gamma, float* y,
                        long rows, int c, void* stream);
int cdseg_fuse_gate_bwd(const float* dy, const float* s, const float* a, const float* m, const float* alpha, const float* gamma,
                        float* ds, float* da, double* sums, long rows, int c, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ skip-connection options (csrc/skip.hip)
 * ref: SerializedUnpooling.forward, ptv3.py:607-626, and freeU / Fourier_filter, :42-100.  The reference scales the skip
 * feature by f, filters it over ALL N rows of the batch (FreeU) and merges it with the unpooled child.  Its 2-D FFT mask is
 * constant along the channel frequencies and scales the row frequencies 0 and -1 by s, so that the real part it keeps is, per
 * channel j and REFERENCE row m (theta_m = 2 pi m / N):
 *   y[m][j] = x[m][j] + k (S0_j + A_j cos theta_m + B_j sin theta_m),        k = (float32(s) - 1) / N   (fp64, rounded once)
 *   S0_j = sum_m x[m][j],   A_j = sum_m x[m][j] cos theta_m,   B_j = sum_m x[m][j] sin theta_m
 * The operator is I + k P with P symmetric: the backward is the same two calls on the gradient.
 *   ref_of_row (n) int32   physical row -> reference row (NULL = identity); its values enter arithmetic only.  n_total = N.
 *   cdseg_skip_stats       stats (3 c doubles, on the device) = [S0 A B] of x: (n, c), fp32 or the build's 16-bit type
 *                          (dtype), row stride ldx.  cos / sin in fp64 (sincospi(2 m / N)), sums in fp64 in an order fixed by
 *                          (n, c) and the path: chunk b of cdseg_skip_partition owns rows_per_chunk consecutive rows (64 at
 *                          least, 256 chunks at most), a lane adds its rows by ascending index, the row slots of a block by
 *                          ascending slot, and a finish launch adds the chunk partials (in ws): by ascending chunk index
 *                          inside each of 16 segments of ceil(chunks / 16) consecutive chunks, then the segment sums by
 *                          ascending segment (one chain over 256 partials is bound by the latency of its loads).  No float
 *                          atomics, no host read: equal inputs on the same path give equal bits.
 *   cdseg_skip_fold        u (3 cout doubles) = [W S0, W A, W B] for a (cout, cin) matrix W (dtype, row stride ldw): what the
 *                          filter adds behind a Linear that reads the filtered feature (proj_cat of the 'cat' mode).  fp64,
 *                          fixed order.
 *   cdseg_skip_merge       in place on the fp32 stream x (n, c), row stride ldx; every part may be absent:
 *                            x[r][j] = f (x[r][j] + k (S0_j + A_j cos theta_r + B_j sin theta_r)) + child[cluster[r]][j]
 *                            folded != 0 (stats holds u, x carries f already):
 *                            x[r][j] = x[r][j] + f k (u0_j + u1_j cos theta_r + u2_j sin theta_r) + child[cluster[r]][j]
 *                          stats NULL: f x + child[cluster]; child NULL (then cluster NULL): the scaled / filtered skip alone.
 *                          Evaluated in fp64 from the fp32 operands, rounded to fp32 once.  child: fp32 (n_child, c), row
 *                          stride ldchild; cluster (n) int32 in [0, n_child).
 * Two paths, chosen per call: c a multiple of 4 with operands and row strides aligned for 4 elements per access (16 bytes of
 * fp32, 8 of the 16-bit type), else a scalar path with the same arithmetic.  LDS only for the block's reduction, no scratch.
 * Nothing outside stats / u / x and ws_bytes of ws is written.
 * Status codes, checked before any launch; n = 0 returns CDSEG_OK without one:
 *   CDSEG_ERR_UNSUPPORTED  c (cin, cout) outside [1, 512]; 2^31 rows or more.
 *   CDSEG_ERR_ARG          a NULL x / stats / u / w; dtype neither CDSEG_F32 nor CDSEG_BF16; a row stride below the width; a
 *                          pointer not aligned to its element (stats, u: 8 bytes; ws: 16); n < 0; n_total < n with a filter;
 *                          folded without stats; child without cluster or with n_child <= 0, cluster without child; NaN f or s.
 *   CDSEG_ERR_WORKSPACE    ws NULL or ws_bytes below the query. */
int cdseg_skip_partition(long n, int c, long* rows_per_chunk, int* chunks);
size_t cdseg_skip_stats_ws_bytes(long n, int c);
int cdseg_skip_stats(const void* x, int dtype, int ldx, long n, int c, const int32_t* ref_of_row, long n_total, double* stats,
                     void* ws, size_t ws_bytes, void* stream);
int cdseg_skip_fold(const void* w, int dtype, int ldw, int cout, int cin, const double* stats, double* u, void* stream);
int cdseg_skip_merge(float* x, int ldx, long n, int c, const double* stats, int folded, double s, long n_total, double f,
                     const int32_t* ref_of_row, const float* child, int ldchild, const int32_t* cluster, long n_child, void* stream);

/* ------------------------------------------------------------------ fused optimizer step (csrc/optim.hip)
 * ref: engines/train.py:216-271 (run_step: scaler.unscale_, clip_grad_norm_, scaler.step(optimizer)) on torch.optim.AdamW.
 * One tensor table describes the parameters; a work list cuts them into chunks of at most CDSEG_OPT_CHUNK elements (a
 * chunk never spans two tensors), one 256-thread block per chunk, grid-strided beyond 2048 blocks.
 *   tensor table   host array of `count` entries.  p, m, v: fp32, updated in place; g: fp32, READ ONLY; step: the tensor's
 *                  step counter, ONE device float; p16: the 16-bit copy of p in THIS BUILD's 16-bit type (NULL = none);
 *                  group: index into the group array; flags: CDSEG_OPT_CLIP = g counts towards the clipped norm and is
 *                  clipped, CDSEG_OPT_SKIP = the tensor takes no part in this call (no gradient: nothing of it is read or
 *                  written, its pointers must still be valid addresses).  Every entry validates and copies the table into
 *                  the caller's workspace with ONE host-to-device copy on the caller's stream; after it returns the library
 *                  holds no host pointer.  The copy is hipMemcpyAsync: from PAGEABLE host memory the runtime stages the
 *                  bytes before the call returns, so the caller may rewrite the table at once (as cdseg_plan_finish's pad
 *                  table); a caller that passes PINNED memory must keep the table unchanged until the stream has passed
 *                  the copy.
 *   groups         host array, passed on BY VALUE (at most CDSEG_OPT_MAX_GROUPS).  Doubles: 1 - beta2 formed from a float
 *                  beta2 = 0.999 is off by 1.3e-5 relative; the kernel forms every derived constant in fp64 and rounds once.
 *   chunk list     cdseg_opt_chunks (host only; a function of the sizes alone): chunks_host[2 k] = tensor index,
 *                  chunks_host[2 k + 1] = start element, tensors and starts ascending; chunks_host NULL = count only.
 *                  The caller uploads the list once; the entries below take the DEVICE copy (chunks_dev) and check that
 *                  nchunks is the count of the table's sizes.  A list entry that points outside the table is never followed.
 * cdseg_grad_norm: one read of the gradients.  inv_scale = fp32(1 / double(grad_scale[0])) (grad_scale: device float, NULL =
 *   1), as GradScaler.unscale_ forms it.  Per chunk: a lane adds (g inv_scale)^2 over its elements by ascending index in
 *   fp32, the lanes go through the fixed 64-wide wave tree and the block's waves by ascending wave index in fp64; the block
 *   stores its partial (0 for a tensor without CDSEG_OPT_CLIP) and its non-finite flag (any inf / nan in the raw g, over ALL
 *   tensors that take part) with plain stores.  A second, single-block launch adds the partials by ascending chunk index
 *   (lane t the chunks [t L, (t + 1) L), L = ceil(nchunks / 256), then lane 0 the 256 lane sums by ascending lane), fp64.
 *   out (3 device floats): out[0] = norm, out[1] = clip_coef = min(1, max_norm / (norm + 1e-6)) in fp32 (torch's
 *   clip_grad_norm_), out[2] = 1 if a gradient is non-finite else 0.  Equal inputs give equal bits.
 * cdseg_adamw_step: a first launch advances step[0] += 1 of every tensor that takes part; the main launch, per element
 *     g' = (g * inv_scale) * clip_coef      (each factor only where its pointer is given; clip_coef only with CDSEG_OPT_CLIP)
 *     m  = fma(1 - beta1, g', beta1 * m)
 *     v  = fma((1 - beta2) * g', g', beta2 * v)
 *     p  = fma(-lr / (1 - beta1^t), m / (sqrt(v) / sqrt(1 - beta2^t) + eps), p * (1 - lr * weight_decay))
 *     p16 = cast16(p)                       (the rounding of cdseg_cast of this build: saturating in the IEEE-half build)
 *   every operation rounded once in fp32 (correctly rounded division and square root, no contraction beyond the fma written
 *   here); t = step[0] after the advance; the constants are formed in fp64 once per block and tensor and rounded to fp32.
 *   grad_scale, found_inf, clip_coef: device floats (each may be NULL), never read on the host.  With found_inf[0] != 0
 *   NOTHING is written: p, m, v, p16 and step keep their bits.  found_inf is the CALLER's flag (GradScaler.step produces it
 *   with a pass of its own over every gradient before it calls the optimizer); out[2] of cdseg_grad_norm is not consulted.  16-byte loads / stores where p, g, m, v and p16 of a tensor
 *   are 16-byte aligned, a scalar path otherwise (uniform per block); same bits on either path.
 * Status codes, checked before any launch or copy:
 *   CDSEG_ERR_ARG          NULL table / groups / chunks_dev / out; count <= 0; an entry with a NULL or not 4-byte aligned
 *                          p / g / m / v / step, an odd p16, n <= 0, unknown flag bits, a group index outside [0, ngroups);
 *                          ngroups <= 0; lr, eps, weight_decay < 0 or a beta outside [0, 1); max_norm < 0; nchunks that is not
 *                          the chunk count of the table; a scale / flag / coefficient pointer not 4-byte aligned; ws not
 *                          16-byte aligned.
 *   CDSEG_ERR_UNSUPPORTED  n >= 2^31 (chunk starts are int32); more than CDSEG_OPT_MAX_GROUPS groups.
 *   CDSEG_ERR_WORKSPACE    ws NULL or ws_bytes below cdseg_opt_ws_bytes(count, nchunks). */
#define CDSEG_OPT_CHUNK 8192
#define CDSEG_OPT_MAX_GROUPS 16
#define CDSEG_OPT_CLIP 1
#define CDSEG_OPT_SKIP 2
typedef struct cdseg_opt_tensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  void* p16;
  float* step;
  long n;
  int group;
  int flags;
} cdseg_opt_tensor;
typedef struct cdseg_opt_group {
  double lr;
  double beta1;
  double beta2;
  double eps;
  double weight_decay;
} cdseg_opt_group;
int cdseg_opt_chunks(const long* n_host, int count, int32_t* chunks_host, long* nchunks);
size_t cdseg_opt_ws_bytes(int count, long nchunks);
int cdseg_grad_norm(const cdseg_opt_tensor* tensors_host, int count, const int32_t* chunks_dev, long nchunks,
                    const float* grad_scale, float max_norm, float* out, void* ws, size_t ws_bytes, void* stream);
int cdseg_adamw_step(const cdseg_opt_tensor* tensors_host, int count, const cdseg_opt_group* groups_host, int ngroups,
                     const int32_t* chunks_dev, long nchunks, const float* grad_scale, const float* found_inf,
                     const float* clip_coef, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ native training Block (csrc/trainblock.hip)
 * One PTv3 Block (ref: ptv3.py:399-428) of the TRAINING step in two host calls: the forward keeps what the backward reads
 * in a tape, the backward writes the input gradients and the 18 parameter gradients.  The launches are those of the
 * autograd graph (cdsegnet_amd/train_graph.py) through the same entry points - the dense and gathered GEMM, LayerNorm and its
 * backward, the attention core and its backward, the Linear / conv weight gradients - plus the row kernels below for what that
 * graph leaves to torch (residual adds, stochastic-depth masks, GELU, the per-scene timestep rows and their column sums, casts).
 *
 *   x0 = x_in + LN_cpe(Linear(SubMConv3d(x_conv))) [+ t_rows[scene(row)]]
 *   x1 = x0 + mask1[row] * proj(attention(qkv(LN1(x0))))
 *   x_out = x1 + mask2[row] * fc2(GELU(fc1(LN2(x1))))
 *
 * mm_dtype CDSEG_BF16: every Linear / conv operand is rounded ONCE to the build's 16-bit type (saturating in the half build),
 * sums and the residual stream are fp32, every gradient that becomes an operand is cast WITHOUT saturation (an inf stays an
 * inf for a GradScaler).  attn_dtype CDSEG_BF16: the attention core on 16-bit q / k / v, fp32 dq / dk / dv.
 * param[]: the 18 fp32 parameter tensors in the order of the CDSEG_TB_* indices; weights are (out, in) row-major, the conv
 * kernel (C, 27, C).  shadow16[]: optional current 16-bit copies of the six matrices (conv, cpe Linear, qkv, proj, fc1, fc2; NULL:
 * cdseg_train_block_prepare makes them).  derived: buffer of the size cdseg_train_block_bytes reports, filled by
 * cdseg_train_block_prepare in ONE launch - the six transposed Linear weights, the mirrored, transposed conv kernel
 * W'[ci][o][co] = W[co][26-o][ci], in mm_dtype, and with mm_dtype CDSEG_BF16 the 16-bit forward weights where no shadow copy is
 * given.  Call it again whenever a weight changes.
 * cdseg_train_block_bytes: host only, a function of the shape alone; every size is a multiple of 256.  The gradient slab holds the
 * 18 gradients (fp32, parameter order) at the byte offsets cdseg_train_block_grad_offsets reports (each a multiple of 256); the
 * backward zeroes it with one memset.  slots = patch_start_host[num_patches].
 * Checked before the first launch (CDSEG_ERR_ARG): a NULL descriptor / io / required pointer, channels or hidden not a multiple
 * of 16, channels != 16 * heads, max_len > CDSEG_MAX_PATCH, a pointer that is not 16-byte aligned, a tape or scratch below
 * the reported size, a dtype other than CDSEG_F32 / CDSEG_BF16.  n <= 0: CDSEG_OK, nothing launched. */
#define CDSEG_TB_CONV_W 0
#define CDSEG_TB_CONV_B 1
#define CDSEG_TB_CPE_W 2
#define CDSEG_TB_CPE_B 3
#define CDSEG_TB_CPE_LN_G 4
#define CDSEG_TB_CPE_LN_B 5
#define CDSEG_TB_NORM1_G 6
#define CDSEG_TB_NORM1_B 7
#define CDSEG_TB_QKV_W 8
#define CDSEG_TB_QKV_B 9
#define CDSEG_TB_PROJ_W 10
#define CDSEG_TB_PROJ_B 11
#define CDSEG_TB_NORM2_G 12
#define CDSEG_TB_NORM2_B 13
#define CDSEG_TB_FC1_W 14
#define CDSEG_TB_FC1_B 15
#define CDSEG_TB_FC2_W 16
#define CDSEG_TB_FC2_B 17
#define CDSEG_TB_PARAMS 18
typedef struct cdseg_train_block_desc {
  int channels, heads, hidden;
  float attn_scale;
  float eps_cpe, eps_norm1, eps_norm2;
  int mm_dtype, attn_dtype;
  int deterministic;       /* parameter gradients through the _det entry points (fixed summation order) */
  const float* param[18];
  const void* shadow16[6]; /* conv, cpe Linear, qkv, proj, fc1, fc2: the build's 16-bit type, or NULL */
  void* derived;
  size_t derived_bytes;
} cdseg_train_block_desc;
typedef struct cdseg_train_block_io {
  long n;
  const float* x_in;          /* (n, C) */
  const float* x_conv;        /* (n, C): what the CPE conv reads; may be x_in */
  const float* t_rows;        /* (num_scenes, C) or NULL: per-scene timestep rows */
  const int32_t* scene_offs;  /* (num_scenes + 1) row offsets of the scenes (required with t_rows) */
  int num_scenes;
  const float* mask1;         /* (n) or NULL: stochastic-depth row mask of the attention branch, already / keep */
  const float* mask2;         /* (n) or NULL: of the MLP branch */
  const int32_t* nbr;         /* (27, n) offset-major kernel map */
  const int32_t* gidx;
  const int32_t* widx;
  const int32_t* patch_start; /* (num_patches + 1) */
  int num_patches, max_len;
  long num_slots;             /* patch_start_host[num_patches] */
  void* tape;
  size_t tape_bytes;
  void* scratch;
  size_t scratch_bytes;
  float* x_out;               /* (n, C) */
  /* The row level above the voxels (a Mix3D batch trained on every point): all zero / NULL = one row per voxel, the executor
   * above launch for launch.  Otherwise the n rows are in voxel order, the rows of a voxel contiguous, and the sparse conv takes
   * the voxel as its unit: nbr describes n_conv voxels, the whole CPE (conv, Linear, LayerNorm) runs on the first row of every
   * voxel and row i adds the CPE term of voxel row_vox[i].  Backward: a voxel's CPE gradient is the sum over its run in
   * ascending row order, the conv's data gradient lands on the run's first row (the other rows of dx_conv are zero).
   * Tape and scratch keep their sizes (they are sized by n >= n_conv).  CDSEG_ERR_ARG before any launch: n_conv outside
   * [1, n], one of the two pointers without the other or without n_conv, a pointer that is not 4-byte aligned. */
  long n_conv;
  const int32_t* row_vox;     /* (n): voxel of a row, ascending */
  const int32_t* row_start;   /* (n_conv + 1): first row of every voxel's run, row_start[n_conv] = n */
} cdseg_train_block_io;
int cdseg_train_block_bytes(const cdseg_train_block_desc* desc, long n, long slots, size_t* tape, size_t* scratch,
                            size_t* derived, size_t* grads);
int cdseg_train_block_grad_offsets(const cdseg_train_block_desc* desc, size_t* offsets18_host);
int cdseg_train_block_prepare(const cdseg_train_block_desc* desc, void* stream);
int cdseg_train_block_forward(const cdseg_train_block_desc* desc, const cdseg_train_block_io* io, void* stream);
/* dy (n, C) -> dx_in (n, C), dx_conv (n, C; NULL when io->x_conv == io->x_in: the conv's data gradient is added into dx_in),
 * dt_rows (num_scenes, C; with io->t_rows), grad_slab.  io: the forward's, tape included. */
int cdseg_train_block_backward(const cdseg_train_block_desc* desc, const cdseg_train_block_io* io, const float* dy,
                               float* dx_in, float* dx_conv, float* dt_rows, void* grad_slab, void* stream);
/* The row kernels of the executor on their own (rows of c fp32 values, c a multiple of 4, contiguous rows, 16-byte aligned
 * pointers; out_dtype CDSEG_F32 or CDSEG_BF16).  Multiply and add are rounded separately (no contraction).
 *   residual          out = x + mask[row] * a + t_rows[scene(row)]   (a, mask, t_rows optional; fp32 out; out may be x)
 *   scale_cast        out = cast(mask[row] * dy), WITHOUT saturation (mask NULL: the plain non-saturating cast)
 *   add_layernorm     x1 = x + mask[row] * a;  h = LayerNorm(x1) * gamma + beta in out_dtype (saturating), c <= 2048
 *   gelu_fwd          g = GELU(u) (erf form) in out_dtype (saturating)
 *   gelu_bwd_cast     du = dg * GELU'(u) in out_dtype WITHOUT saturation */
int cdseg_residual(const float* x, const float* a, const float* mask, const float* t_rows, const int32_t* scene_offs,
                   int num_scenes, float* out, long n, int c, void* stream);
/* The row kernels of the row level (io->n_conv above; row_vox (n), row_start (nv + 1) as there):
 *   gather_first      out[v] = cast(x[row_start[v]]) in out_dtype (saturating), nv rows
 *   residual_rows     out[i] = x[i] + a[row_vox[i]] + t_rows[scene(i)]   (a: nv rows; t_rows optional; out may be x)
 *   run_sum           out[v] = 0 + dx[row_start[v]] + ... + dx[row_start[v + 1] - 1], ascending
 *   scatter_first     accumulate: dx[row_start[v]] += g[v], other rows untouched; else dx[i] = g[row_vox[i]] on the first row of
 *                     a run and 0 on the others (all n rows written) */
int cdseg_gather_first(const float* x, const int32_t* row_start, void* out, int out_dtype, long nv, int c, void* stream);
int cdseg_residual_rows(const float* x, const float* a, const int32_t* row_vox, const float* t_rows, const int32_t* scene_offs,
                        int num_scenes, float* out, long n, int c, void* stream);
int cdseg_run_sum(const float* dx, const int32_t* row_start, float* out, long nv, int c, void* stream);
int cdseg_scatter_first(const float* g, const int32_t* row_vox, const int32_t* row_start, float* dx, int accumulate, long n, int c,
                        void* stream);
int cdseg_scale_cast(const float* dy, const float* mask, void* out, int out_dtype, long n, int c, void* stream);
int cdseg_add_layernorm(const float* x, const float* a, const float* mask, const float* gamma, const float* beta, float eps,
                        float* x1, void* h, int out_dtype, long n, int c, void* stream);
int cdseg_gelu_fwd(const float* u, void* g, int out_dtype, long count, void* stream);
int cdseg_gelu_bwd_cast(const float* u, const float* dg, void* du, int out_dtype, long count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CDSEG_H */
