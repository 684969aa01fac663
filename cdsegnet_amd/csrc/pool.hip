// Serialized pooling of the wide stages in ONE launch (gfx950, 16-bit trunk):
//
//   out[m] = act(scale * max_{i in children(m)} round16(W x_i + b) + shift)        ref: ptv3.py:506-515, 548-551
//            (SerializedPooling: proj Linear -> torch_scatter.segment_csr(reduce="max") -> BatchNorm (folded) -> GELU)
//
// As two launches (cdseg_gemm, cdseg_segment_max) the projected rows make a round trip through HBM: 960 k x 64 16-bit
// values written and read back (246 MB) to produce 446 k pooled rows - 90 + 84 us on the first pooling of the benchmark
// forward.  Here the projection of 16 children at a time stays on the CU:
//   * the children of a pooled row are contiguous (points are in (batch | z) order, a pooled cell is a code prefix), so
//     a wave takes 16 CONSECUTIVE pooled rows and walks their children 16 at a time;
//   * W is resident in LDS as MFMA A fragments (4 - 16 KB); the product is computed transposed (D^T = W X^T,
//     v_mfma_f32_16x16x32) with the output channels permuted inside the image so that lane (j, q) ends up with the
//     COUT / 4 consecutive channels q * COUT / 4 .. of child j (the register-resident layout of blockrr.hip);
//   * the 16 x COUT projected values are rounded to the 16-bit type (what the two-launch path stores: max and rounding
//     commute, the results are bit-identical to max over the stored rows) and parked in a per-wave LDS strip; lane
//     (p, q) then folds the rows of ITS pooled row m0 + p into a running fp32 maximum - a loop over at most 16 strip
//     rows, no cross-lane traffic, clusters that straddle two strips just continue in the next one;
//   * epilogue per pooled row: folded BatchNorm, GELU (erf), fp32 row + its 16-bit copy, 64 - 128 contiguous bytes per lane.
// HBM traffic = the fine rows once + the pooled rows once.
#include <atomic>
#include <type_traits>

#include "common.h"
#include "route.h"

namespace {

struct PoolP {
  const bf16_t* x; const uint4* wimg; const float* bias; const int32_t* seg; const float* scale; const float* shift;
  float* out; bf16_t* out2;
  long m;  // pooled rows
  int ldx, ldo, ldo2, act;
};

constexpr int PL_WAVES = 8;
constexpr int POOL_FOLD_WALK = 1, POOL_FOLD_SCAN = 2;
// the scan fold from a mean run length of POOL_SCAN_RATIO children per pooled row on (n_fine >= POOL_SCAN_RATIO * m).
// Measured crossover (tools/pool_fold_crossover.py, half build, 24 scenes; walk / scan in us):
//   32 -> 64, 2.88 M rows:   ratio 2: 257 / 270   4: 164 / 208   8: 178 / 172   16: 349 / 172
//   64 -> 128, 1.34 M rows:  ratio 2: 350 / 342   4: 197 / 213   8: 204 / 186   16: 349 / 174
// the scan costs the same VALU work per 16 children whatever the runs, the walk grows with the run length: they cross between
// 7 and 8.  The n-branch's one-step poolings (2.2 and 3.9 children) keep the walk, the c-branch's two-step one (8.4) scans.
constexpr long POOL_SCAN_RATIO = 8;

// DPP controls (one DPP row = the 16 child lanes of a q group)
constexpr int DPP_QUAD_1032 = 0xB1, DPP_QUAD_2301 = 0x4E, DPP_ROW_SHR0 = 0x110, DPP_ROW_ROR1 = 0x121, DPP_ROW_MIRROR = 0x140,
              DPP_ROW_HALF_MIRROR = 0x141;
// (old = the lane's own value: a lane without a source inside its row keeps it)
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false); }
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

template <int CIN, int COUT>
struct PoolCfg {
  static constexpr int KS = CIN / 32, OT = COUT / 16, QI = CIN / 4, QO = COUT / 4;
  static constexpr int W_BYTES = CIN * COUT * 2;
  static constexpr int ROW = COUT * 2 + 16;             // strip row pitch in bytes (+16: bank spread)
  static constexpr int STRIP = 16 * ROW;                // one wave's strip
  static constexpr int PAR = 3 * COUT * 4;              // bias, scale, shift
  static constexpr int LDS = W_BYTES + PL_WAVES * STRIP + PAR;
};

// the chunks of one wave (the weight image and the parameters are in LDS).  SCAN = false: the strip walk; true: the
// segmented maximum across the 16 child lanes of a step (below)
template <int CIN, int COUT, bool SCAN>
__device__ __forceinline__ void pool_chunks(const PoolP& p, char* smem) {
  using K = PoolCfg<CIN, COUT>;
  constexpr int KS = K::KS, OT = K::OT, QO = K::QO;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, q = lane >> 4;
  const uint4* W = reinterpret_cast<const uint4*>(smem);  // OT x KS fragments
  char* strip = smem + K::W_BYTES + wave * K::STRIP;
  const float* pr = reinterpret_cast<const float*>(smem + K::W_BYTES + PL_WAVES * K::STRIP);
  // 32 -> 64: the four weight fragments stay in registers for the lifetime of the wave; 64 -> 128 (16 fragments = 64
  // registers next to 32 running maxima) re-reads them from LDS per strip
  // (the scan spends its registers on the 16 - 32 values it scans in place: always from LDS)
  constexpr bool KEEPW = OT * KS <= 4 && !SCAN;
  uint4 wkeep[KEEPW ? OT : 1][KS];
  if constexpr (KEEPW) {
#pragma unroll
    for (int t = 0; t < OT; ++t)
#pragma unroll
      for (int s = 0; s < KS; ++s) wkeep[t][s] = W[(t * KS + s) * 64 + lane];
  }

  const long chunks = (p.m + 15) / 16;
  for (long chunk = (long)blockIdx.x * PL_WAVES + wave; chunk < chunks; chunk += (long)gridDim.x * PL_WAVES) {
    const long m0 = chunk * 16;
    const long mrow = m0 + j;  // this lane's pooled row (lanes q = 0..3 share it, COUT / 4 channels each)
    const bool valid = mrow < p.m;
    const int s0 = p.seg[valid ? mrow : p.m], s1 = p.seg[valid ? mrow + 1 : p.m];
    const int f0 = __builtin_amdgcn_readfirstlane(s0);
    const long mend = m0 + 16 < p.m ? m0 + 16 : p.m;
    const int f1 = p.seg[mend];  // (wave uniform)
    float mx[QO];  // walk: the running maximum of this lane's pooled row; scan: the values of child f + j, scanned in place
#pragma unroll
    for (int c = 0; c < QO; ++c) mx[c] = -INFINITY;
    int done = 0;       // scan: runs of this chunk that ended in earlier steps (wave uniform)
    bool open = false;  // scan: the run of the previous step's last child goes on in this step (wave uniform)
    // the rows of strip f + 16 are requested while strip f is multiplied and folded (rows past the chunk: duplicates of
    // its last child - never folded, they lie outside every [s0, s1))
    auto fetch = [&](int f, bf16x8_t (&dst)[KS]) {
      int row = f + j;
      row = row < f1 ? row : f1 - 1;
#pragma unroll
      for (int s = 0; s < KS; ++s) dst[s] = *reinterpret_cast<const bf16x8_t*>(p.x + (long)row * p.ldx + 32 * s + 8 * q);
    };
    bf16x8_t xf[KS];
    fetch(f0, xf);
#pragma unroll 1
    for (int f = f0; f < f1; f += 16) {
      bf16x8_t xn[KS];
      fetch(f + 16 < f1 ? f + 16 : f, xn);
      int lo = lane;  // opaque per strip: keeps the weight-fragment reads of the 64 -> 128 form inside the loop
      asm volatile("" : "+v"(lo));
      // projected values of child j, channels q * QO .. + QO - 1, rounded to the 16-bit type -> strip row j (walk) or
      // mx[] (scan)
      if constexpr (SCAN) {
        // one output tile at a time (the registers go to the values scanned in place).  mx[] still holds the scanned values of
        // the previous step: a run that came in from there has its maximum so far in lane 15 of each row, child 0 takes it
#pragma unroll
        for (int t = 0; t < OT; ++t) {
          f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < KS; ++s) a = mfma_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, W[(t * KS + s) * 64 + lo]), xf[s], a);
          a += *reinterpret_cast<const f32x4_t*>(pr + q * QO + 4 * t);
          float n4[4];
          unpack_bf16x2(pack_bf16x2(a[0], a[1]), n4[0], n4[1]);
          unpack_bf16x2(pack_bf16x2(a[2], a[3]), n4[2], n4[3]);
          if (open) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float c = fmaxf(n4[e], dpp_f<DPP_ROW_ROR1>(mx[4 * t + e]));
              n4[e] = j == 0 ? c : n4[e];
            }
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) mx[4 * t + e] = n4[e];
          asm volatile("" : "+v"(mx[4 * t]), "+v"(mx[4 * t + 1]), "+v"(mx[4 * t + 2]), "+v"(mx[4 * t + 3]));  // (tile by tile)
        }
      }
#pragma unroll
      for (int t = 0; t < (SCAN ? 0 : OT); t += 2) {
        // (bias added behind the product, like the GEMM's epilogue: bit-identical projected values)
        f32x4_t a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        uint4 w0[KS], w1[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          w0[s] = KEEPW ? wkeep[KEEPW ? t : 0][s] : W[(t * KS + s) * 64 + lo];
          w1[s] = KEEPW ? wkeep[KEEPW ? t + 1 : 0][s] : W[((t + 1) * KS + s) * 64 + lo];
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          a = mfma_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w0[s]), xf[s], a);
          b = mfma_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w1[s]), xf[s], b);
        }
        a += *reinterpret_cast<const f32x4_t*>(pr + q * QO + 4 * t);
        b += *reinterpret_cast<const f32x4_t*>(pr + q * QO + 4 * t + 4);
        uint4 u;
        u.x = pack_bf16x2(a[0], a[1]); u.y = pack_bf16x2(a[2], a[3]);
        u.z = pack_bf16x2(b[0], b[1]); u.w = pack_bf16x2(b[2], b[3]);
        *reinterpret_cast<uint4*>(strip + j * K::ROW + (q * QO + 4 * t) * 2) = u;
      }
      if constexpr (SCAN) {
        // ends: bit e = child f + e is the last one of its run (every run holds at least one child, so the ends of a step are
        // distinct children).  Each owner lane sets the bit of its own run, an OR over the 16 lanes of the DPP row gives the
        // step's mask to every lane
        int eb = s1 - 1 - f;
        eb = (valid && (unsigned)eb < 16u) ? 1 << eb : 0;
        eb |= dpp_i<DPP_ROW_MIRROR>(eb);
        eb |= dpp_i<DPP_ROW_HALF_MIRROR>(eb);
        eb |= dpp_i<DPP_QUAD_1032>(eb);
        eb |= dpp_i<DPP_QUAD_2301>(eb);
        const int ends = __builtin_amdgcn_readfirstlane(eb);
        // segmented inclusive maximum along the row: child j takes child j - d where no run ends in [j - d, j)
        auto step = [&](auto dc) {
          constexpr int d = decltype(dc)::value;
          const bool take = j >= d && ((ends >> (j - d)) & ((1 << d) - 1)) == 0;
#pragma unroll
          for (int c = 0; c < QO; ++c) {
            const float t = fmaxf(mx[c], dpp_f<DPP_ROW_SHR0 + d>(mx[c]));
            mx[c] = take ? t : mx[c];
          }
        };
        step(std::integral_constant<int, 1>{});
        step(std::integral_constant<int, 2>{});
        step(std::integral_constant<int, 4>{});
        step(std::integral_constant<int, 8>{});
        // the last child of a run holds the run's maximum: parked (the 16-bit values they are) in the strip row of its
        // pooled row, the done-th run of the chunk plus the ends in front of it
        if ((ends >> j) & 1) {
          const int r = done + __builtin_popcount(ends & ((1 << j) - 1));
          char* dst = strip + r * K::ROW + q * QO * 2;
#pragma unroll
          for (int c8 = 0; c8 < QO / 8; ++c8) {
            uint4 u;
            u.x = pack_bf16x2(mx[8 * c8], mx[8 * c8 + 1]); u.y = pack_bf16x2(mx[8 * c8 + 2], mx[8 * c8 + 3]);
            u.z = pack_bf16x2(mx[8 * c8 + 4], mx[8 * c8 + 5]); u.w = pack_bf16x2(mx[8 * c8 + 6], mx[8 * c8 + 7]);
            *reinterpret_cast<uint4*>(dst + c8 * 16) = u;
          }
        }
        done += __builtin_popcount(ends);
        open = !((ends >> 15) & 1);
#pragma unroll
        for (int s = 0; s < KS; ++s) xf[s] = xn[s];
        continue;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      // fold this lane's children that sit in the strip
      const int a0 = (s0 > f ? s0 : f) - f, a1 = (s1 < f + 16 ? s1 : f + 16) - f;
      for (int r = a0; r < a1; ++r) {
        const char* src = strip + r * K::ROW + q * QO * 2;
#pragma unroll
        for (int c8 = 0; c8 < QO / 8; ++c8) {
          const uint4 u = *reinterpret_cast<const uint4*>(src + c8 * 16);
          const uint32_t w4[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float v0, v1;
            unpack_bf16x2(w4[e], v0, v1);
            mx[8 * c8 + 2 * e] = fmaxf(mx[8 * c8 + 2 * e], v0);
            mx[8 * c8 + 2 * e + 1] = fmaxf(mx[8 * c8 + 2 * e + 1], v1);
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // the strip is rewritten by the next 16 children
#pragma unroll
      for (int s = 0; s < KS; ++s) xf[s] = xn[s];
    }
    if constexpr (SCAN) {
      // strip row j now holds the maximum of pooled row m0 + j: back to the owner lanes, as the walk leaves them
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const char* src = strip + j * K::ROW + q * QO * 2;
#pragma unroll
      for (int c8 = 0; c8 < QO / 8; ++c8) {
        const uint4 u = *reinterpret_cast<const uint4*>(src + c8 * 16);
        unpack_bf16x2(u.x, mx[8 * c8], mx[8 * c8 + 1]);
        unpack_bf16x2(u.y, mx[8 * c8 + 2], mx[8 * c8 + 3]);
        unpack_bf16x2(u.z, mx[8 * c8 + 4], mx[8 * c8 + 5]);
        unpack_bf16x2(u.w, mx[8 * c8 + 6], mx[8 * c8 + 7]);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // the strip is rewritten by the next chunk
    }
    if (valid) {
      float* o = p.out + mrow * p.ldo + q * QO;
#pragma unroll
      for (int c4 = 0; c4 < QO / 4; ++c4) {
        const f32x4_t sc = *reinterpret_cast<const f32x4_t*>(pr + COUT + q * QO + 4 * c4);
        const f32x4_t sh = *reinterpret_cast<const f32x4_t*>(pr + 2 * COUT + q * QO + 4 * c4);
        f32x4_t v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = __builtin_fmaf(mx[4 * c4 + r], sc[r], sh[r]);  // (the expression of segment_max_kernel, bit for bit)
          if (p.act == CDSEG_ACT_GELU) v[r] = gelu_erf(v[r]);
        }
        *reinterpret_cast<f32x4_t*>(o + 4 * c4) = v;
        if (p.out2) {
          uint2 u;
          u.x = pack_bf16x2(v[0], v[1]);
          u.y = pack_bf16x2(v[2], v[3]);
          *reinterpret_cast<uint2*>(p.out2 + mrow * p.ldo2 + q * QO + 4 * c4) = u;
        }
      }
    }
  }
}

// (one kernel per fold: the walk keeps the 80 / 90 registers, 3 and 2 blocks per CU, it has on its own)
template <int CIN, int COUT, bool SCAN>
__global__ __launch_bounds__(PL_WAVES * 64) void pool_fused_kernel(PoolP p) {
  using K = PoolCfg<CIN, COUT>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  {
    uint4* d = reinterpret_cast<uint4*>(smem);
    for (int u = tid; u < K::W_BYTES / 16; u += PL_WAVES * 64) d[u] = p.wimg[u];
    float* pr = reinterpret_cast<float*>(smem + K::W_BYTES + PL_WAVES * K::STRIP);
    for (int c = tid; c < COUT; c += PL_WAVES * 64) {
      pr[c] = p.bias ? p.bias[c] : 0.f;
      pr[COUT + c] = p.scale ? p.scale[c] : 1.f;
      pr[2 * COUT + c] = p.shift ? p.shift[c] : 0.f;
    }
  }
  __syncthreads();
  pool_chunks<CIN, COUT, SCAN>(p, smem);
}

// fragment image of W (COUT, CIN) row-major: 16-byte unit (ot * KS + s) * 64 + lane, lane = 16 q + i:
//   W[(i >> 2) * (COUT / 4) + 4 ot + (i & 3)][32 s + 8 q + 0..7]      (input channels in natural k-slot order: the fp32 sums
//   of a product are then the GEMM kernel's, bit for bit)
// (MFMA A operand; output row i lands in lane group i >> 2, register i & 3: lane (j, q) holds channels q * COUT / 4 + 4 ot + r)
__global__ void pool_pack_kernel(const bf16_t* __restrict__ w, uint4* __restrict__ img, int cin, int cout) {
  const int KS = cin / 32;
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= (cout / 16) * KS * 64) return;
  const int lane = u & 63, s = (u >> 6) % KS, ot = (u >> 6) / KS;
  const int q = lane >> 4, i = lane & 15;
  const long row = (i >> 2) * (cout / 4) + ot * 4 + (i & 3);
  img[u] = *reinterpret_cast<const uint4*>(w + row * cin + 32 * s + 8 * q);
}

template <int CIN, int COUT, bool SCAN>
int launch_pool(const PoolP& p, int fold_asked, hipStream_t s) {
  using K = PoolCfg<CIN, COUT>;
  static std::atomic<bool> attr_done{false};  // (a concurrent first call sets the attribute twice: harmless)
  if (!attr_done) {
    if (hipFuncSetAttribute((const void*)pool_fused_kernel<CIN, COUT, SCAN>, hipFuncAttributeMaxDynamicSharedMemorySize, K::LDS) != hipSuccess)
      return CDSEG_ERR_LAUNCH;
    attr_done = true;
  }
  const long chunks = (p.m + 15) / 16;
  long blocks = (chunks + PL_WAVES - 1) / PL_WAVES;
  const int per_cu = K::LDS > 80 * 1024 ? 1 : (K::LDS > 52 * 1024 ? 2 : 3);
  if (blocks > 256 * per_cu) blocks = 256 * per_cu;
  // fix: the fold taken; aux: the fold asked for (POOL_FOLD_AUTO = the rule decided)
  cdseg_route_rec(cdseg_route_template_id<CDSEG_RF_POOL, CIN, COUT, SCAN ? 1 : 0>(), 16, COUT, 1, SCAN ? POOL_FOLD_SCAN : POOL_FOLD_WALK, 0,
                  CDSEG_BF16 << CDSEG_ROUTE_F_CT_SHIFT, fold_asked);
  hipLaunchKernelGGL((pool_fused_kernel<CIN, COUT, SCAN>), dim3((unsigned)blocks), dim3(PL_WAVES * 64), K::LDS, s, p);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

bool pool_supported(int cin, int cout) { return (cin == 32 && cout == 64) || (cin == 64 && cout == 128); }

std::atomic<int> g_pool_fold{0};

}  // namespace

extern "C" int cdseg_pool_fused_fold(int fold) {
  if (fold < 0 || fold > POOL_FOLD_SCAN) return CDSEG_ERR_ARG;
  return g_pool_fold.exchange(fold);
}

extern "C" size_t cdseg_pool_fused_img_bytes(int cin, int cout) { return pool_supported(cin, cout) ? (size_t)cin * cout * 2 : 0; }

extern "C" int cdseg_pool_fused_pack(const void* w, int cin, int cout, void* wimg, void* stream) {
  if (!w || !wimg || (((uintptr_t)w | (uintptr_t)wimg) & 15)) return CDSEG_ERR_ARG;
  if (!pool_supported(cin, cout)) return CDSEG_ERR_UNSUPPORTED;
  const int units = (cout / 16) * (cin / 32) * 64;
  hipLaunchKernelGGL(pool_pack_kernel, dim3((units + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w, (uint4*)wimg, cin,
                     cout);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

namespace {

// n_fine: the rows of x (= seg_start[m]) where the caller knows them, else -1
int pool_fused_impl(const void* x, int ldx, long n_fine, const void* wimg, const float* bias, const int32_t* seg_start, long m,
                    const float* scale, const float* shift, int act, float* out, int ldo, void* out2, int ldo2, int cin, int cout,
                    void* stream) {
  if (m <= 0) return CDSEG_OK;
  if (!x || !wimg || !seg_start || !out) return CDSEG_ERR_ARG;
  if (!pool_supported(cin, cout) || (act != CDSEG_ACT_NONE && act != CDSEG_ACT_GELU)) return CDSEG_ERR_UNSUPPORTED;
  if ((ldx & 7) || (ldo & 3) || (out2 && (ldo2 & 3)) || (((uintptr_t)x | (uintptr_t)wimg | (uintptr_t)out) & 15) ||
      (out2 && (((uintptr_t)out2) & 7)) || (bias && (((uintptr_t)bias) & 15)) || (scale && (((uintptr_t)scale) & 15)) ||
      (shift && (((uintptr_t)shift) & 15)) || (!scale != !shift))
    return CDSEG_ERR_ARG;
  PoolP p;
  p.x = (const bf16_t*)x; p.wimg = (const uint4*)wimg; p.bias = bias; p.seg = seg_start; p.scale = scale; p.shift = shift;
  p.out = out; p.out2 = (bf16_t*)out2; p.m = m; p.ldx = ldx; p.ldo = ldo; p.ldo2 = ldo2; p.act = act;
  const int fold = g_pool_fold.load(std::memory_order_relaxed);
  const bool scan = fold ? fold == POOL_FOLD_SCAN : n_fine >= POOL_SCAN_RATIO * m;
  hipStream_t s = (hipStream_t)stream;
  if (cin == 32) return scan ? launch_pool<32, 64, true>(p, fold, s) : launch_pool<32, 64, false>(p, fold, s);
  return scan ? launch_pool<64, 128, true>(p, fold, s) : launch_pool<64, 128, false>(p, fold, s);
}

}  // namespace

extern "C" int cdseg_pool_fused(const void* x, int ldx, const void* wimg, const float* bias, const int32_t* seg_start, long m,
                                const float* scale, const float* shift, int act, float* out, int ldo, void* out2, int ldo2,
                                int cin, int cout, void* stream) {
  return pool_fused_impl(x, ldx, -1, wimg, bias, seg_start, m, scale, shift, act, out, ldo, out2, ldo2, cin, cout, stream);
}

// PRECONDITION: every run holds at least one row (seg_start strictly increasing).  The scan fold finds a run's end at child
// seg_start[m + 1] - 1: an empty run would put its end on the previous run's last child and the pooled rows behind it would
// take each other's maxima, silently (nothing is read or written out of bounds).  The walk tolerates empty runs; this entry may
// pick the scan, so its callers must not pass any.
extern "C" int cdseg_pool_fused_n(const void* x, int ldx, long n_fine, const void* wimg, const float* bias, const int32_t* seg_start,
                                  long m, const float* scale, const float* shift, int act, float* out, int ldo, void* out2,
                                  int ldo2, int cin, int cout, void* stream) {
  return pool_fused_impl(x, ldx, n_fine, wimg, bias, seg_start, m, scale, shift, act, out, ldo, out2, ldo2, cin, cout, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// SerializedUnpooling of the wide decoder stages, mode "add", in ONE launch (ref: ptv3.py:597-630):
//
//   s      = act(scale_s * (Ws parent_i + bs) + shift_s)                      the skip branch, per fine row i
//   x[i]   = s + act(scale_p * (Wp coarse_m + bp) + shift_p),  m = the coarse row whose run holds i
//   xc[i]  = round16(s)                                                      (the PRE-add skip: what the next CPE conv reads)
//
// As two cdseg_gemm launches the projected coarse rows go to HBM as fp32 and come back through a gather, once per fine
// row.  The children of a coarse row are the contiguous run seg[m] .. seg[m + 1] the pooling walked, so here a wave takes 16
// CONSECUTIVE coarse rows, projects them once into a per-wave fp32 LDS strip and then walks their fine rows 16 at a time:
// skip product, epilogue, add of the owner's strip row, stores.  Both weight images stay in LDS; the products are computed
// transposed (D^T = W X^T) with the input channels in natural k order and the epilogue is cdseg_gemm's expression by
// expression, so x and xc are the two launches' bit for bit.  The output channels keep the MFMA order (tile t, lane group q:
// channels 16 t + 4 q .. + 3): a store instruction writes 64 contiguous bytes of x per row.
// The owner of fine row f + j inside a step: the runs ended so far plus the run ends among the step's children in front of
// it (the `ends` mask of the pooling's scan fold).
namespace {

struct UnpoolP {
  const bf16_t* xs; const bf16_t* xp; const uint4* wimg_s; const uint4* wimg_p;
  const float* bias_s; const float* scale_s; const float* shift_s; const float* bias_p; const float* scale_p; const float* shift_p;
  const int32_t* seg; float* out; bf16_t* out2;
  long m;  // coarse rows
  int ldxs, ldp, ldo, ldo2, act;
};

template <int KS, int KP>  // input channels of the skip / the child projection; 64 output channels
struct UnpoolCfg {
  static constexpr int C = 64, OT = C / 16, SS = KS / 32, SP = KP / 32;
  static constexpr int WS_BYTES = KS * C * 2, WP_BYTES = KP * C * 2;
  static constexpr int ROW = C * 4 + 16;      // strip row pitch in bytes (+16: bank spread)
  static constexpr int STRIP = 16 * ROW;      // one wave's strip
  static constexpr int PAR = 6 * C * 4;       // bias, scale, shift of the skip, then of the child projection
  static constexpr int LDS = WS_BYTES + WP_BYTES + PL_WAVES * STRIP + PAR;
};

// one 16-row product D^T = W X^T and cdseg_gemm's epilogue up to the activation: v[t] = channels 16 t + 4 q .. + 3 of row j
template <int S, int OT>
__device__ __forceinline__ void unpool_project(const uint4* W, const bf16x8_t (&x)[S], const float* par, int lane, int q, int act,
                                               f32x4_t (&v)[OT]) {
  constexpr int C = 16 * OT;
#pragma unroll
  for (int t = 0; t < OT; ++t) {
    f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < S; ++s) a = mfma_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, W[(t * S + s) * 64 + lane]), x[s], a);
    const f32x4_t b = *reinterpret_cast<const f32x4_t*>(par + 16 * t + 4 * q);
    const f32x4_t sc = *reinterpret_cast<const f32x4_t*>(par + C + 16 * t + 4 * q);
    const f32x4_t sh = *reinterpret_cast<const f32x4_t*>(par + 2 * C + 16 * t + 4 * q);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float y = a[r] + b[r];
      y = y * sc[r] + sh[r];  // (as written in gemm.hip's epilogue4)
      if (act == CDSEG_ACT_GELU) y = gelu_erf(y);
      v[t][r] = y;
    }
  }
}

template <int KS, int KP>
__global__ __launch_bounds__(PL_WAVES * 64) void unpool_fused_kernel(UnpoolP p) {
  using K = UnpoolCfg<KS, KP>;
  constexpr int C = K::C, OT = K::OT, SS = K::SS, SP = K::SP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, q = lane >> 4;
  {
    uint4* d = reinterpret_cast<uint4*>(smem);
    for (int u = tid; u < K::WS_BYTES / 16; u += PL_WAVES * 64) d[u] = p.wimg_s[u];
    d = reinterpret_cast<uint4*>(smem + K::WS_BYTES);
    for (int u = tid; u < K::WP_BYTES / 16; u += PL_WAVES * 64) d[u] = p.wimg_p[u];
    float* pr = reinterpret_cast<float*>(smem + K::WS_BYTES + K::WP_BYTES + PL_WAVES * K::STRIP);
    for (int c = tid; c < C; c += PL_WAVES * 64) {
      pr[c] = p.bias_s ? p.bias_s[c] : 0.f;
      pr[C + c] = p.scale_s ? p.scale_s[c] : 1.f;
      pr[2 * C + c] = p.shift_s ? p.shift_s[c] : 0.f;
      pr[3 * C + c] = p.bias_p ? p.bias_p[c] : 0.f;
      pr[4 * C + c] = p.scale_p ? p.scale_p[c] : 1.f;
      pr[5 * C + c] = p.shift_p ? p.shift_p[c] : 0.f;
    }
  }
  __syncthreads();
  const uint4* Ws = reinterpret_cast<const uint4*>(smem);
  const uint4* Wp = reinterpret_cast<const uint4*>(smem + K::WS_BYTES);
  char* strip = smem + K::WS_BYTES + K::WP_BYTES + wave * K::STRIP;
  const float* pr = reinterpret_cast<const float*>(smem + K::WS_BYTES + K::WP_BYTES + PL_WAVES * K::STRIP);

  const long chunks = (p.m + 15) / 16;
  for (long chunk = (long)blockIdx.x * PL_WAVES + wave; chunk < chunks; chunk += (long)gridDim.x * PL_WAVES) {
    const long m0 = chunk * 16;
    const long mrow = m0 + j;  // this lane's coarse row (lanes q = 0..3 share it)
    const bool valid = mrow < p.m;
    const int s1 = p.seg[valid ? mrow + 1 : p.m];
    const int f0 = p.seg[m0];  // (wave uniform)
    const long mend = m0 + 16 < p.m ? m0 + 16 : p.m;
    const int f1 = p.seg[mend];  // (wave uniform)
    auto fetch = [&](int f, bf16x8_t (&dst)[SS]) {
      int row = f + j;
      row = row < f1 ? row : f1 - 1;
#pragma unroll
      for (int s = 0; s < SS; ++s) dst[s] = *reinterpret_cast<const bf16x8_t*>(p.xs + (long)row * p.ldxs + 32 * s + 8 * q);
    };
    bf16x8_t xf[SS];
    if (f0 < f1) fetch(f0, xf);
    {
      // the 16 coarse rows, projected once -> strip row j (rows past m: a copy of the last one, no fine row owns them)
      bf16x8_t xp[SP];
      const long row = valid ? mrow : p.m - 1;
#pragma unroll
      for (int s = 0; s < SP; ++s) xp[s] = *reinterpret_cast<const bf16x8_t*>(p.xp + row * p.ldp + 32 * s + 8 * q);
      f32x4_t v[OT];
      unpool_project<SP, OT>(Wp, xp, pr + 3 * C, lane, q, p.act, v);
#pragma unroll
      for (int t = 0; t < OT; ++t) *reinterpret_cast<f32x4_t*>(strip + j * K::ROW + (16 * t + 4 * q) * 4) = v[t];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    int done = 0;  // runs of this chunk that ended in earlier steps (wave uniform)
#pragma unroll 1
    for (int f = f0; f < f1; f += 16) {
      bf16x8_t xn[SS];
      fetch(f + 16 < f1 ? f + 16 : f, xn);
      int lo = lane;  // opaque per step: keeps the weight-fragment reads inside the loop
      asm volatile("" : "+v"(lo));
      // ends: bit e = fine row f + e is the last one of its run (see the pooling's scan fold)
      int eb = s1 - 1 - f;
      eb = (valid && (unsigned)eb < 16u) ? 1 << eb : 0;
      eb |= dpp_i<DPP_ROW_MIRROR>(eb);
      eb |= dpp_i<DPP_ROW_HALF_MIRROR>(eb);
      eb |= dpp_i<DPP_QUAD_1032>(eb);
      eb |= dpp_i<DPP_QUAD_2301>(eb);
      const int ends = __builtin_amdgcn_readfirstlane(eb);
      int owner = done + __builtin_popcount(ends & ((1 << j) - 1));
      owner = owner < 15 ? owner : 15;  // (rows past f1 count the ends in front of them: never stored)
      f32x4_t v[OT];
      unpool_project<SS, OT>(Ws, xf, pr, lo, q, p.act, v);
      const long row = (long)f + j;
      if (row < f1) {
        float* o = p.out + row * p.ldo + 4 * q;
        bf16_t* o2 = p.out2 + row * p.ldo2 + 4 * q;
        const char* src = strip + owner * K::ROW + 16 * q;
#pragma unroll
        for (int t = 0; t < OT; ++t) {
          uint2 u;
          u.x = pack_bf16x2(v[t][0], v[t][1]);
          u.y = pack_bf16x2(v[t][2], v[t][3]);
          *reinterpret_cast<uint2*>(o2 + 16 * t) = u;
          const f32x4_t c = *reinterpret_cast<const f32x4_t*>(src + 64 * t);
          *reinterpret_cast<f32x4_t*>(o + 16 * t) = v[t] + c;
        }
      }
      done += __builtin_popcount(ends);
#pragma unroll
      for (int s = 0; s < SS; ++s) xf[s] = xn[s];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // the strip is rewritten by the next chunk
  }
}

// fragment image of W (64, CIN) row-major in MFMA order: 16-byte unit (ot * S + s) * 64 + lane, lane = 16 q + i:
//   W[16 ot + i][32 s + 8 q + 0..7]
__global__ void unpool_pack_kernel(const bf16_t* __restrict__ w, uint4* __restrict__ img, int cin, int cout) {
  const int S = cin / 32;
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= (cout / 16) * S * 64) return;
  const int lane = u & 63, s = (u >> 6) % S, ot = (u >> 6) / S;
  const int q = lane >> 4, i = lane & 15;
  img[u] = *reinterpret_cast<const uint4*>(w + (long)(16 * ot + i) * cin + 32 * s + 8 * q);
}

template <int KS, int KP>
int launch_unpool(const UnpoolP& p, hipStream_t s) {
  using K = UnpoolCfg<KS, KP>;
  static std::atomic<bool> attr_done{false};  // (a concurrent first call sets the attribute twice: harmless)
  if (!attr_done) {
    if (hipFuncSetAttribute((const void*)unpool_fused_kernel<KS, KP>, hipFuncAttributeMaxDynamicSharedMemorySize, K::LDS) != hipSuccess)
      return CDSEG_ERR_LAUNCH;
    attr_done = true;
  }
  const long chunks = (p.m + 15) / 16;
  long blocks = (chunks + PL_WAVES - 1) / PL_WAVES;
  const int per_cu = K::LDS > 80 * 1024 ? 1 : (K::LDS > 52 * 1024 ? 2 : 3);
  if (blocks > 256 * per_cu) blocks = 256 * per_cu;
  cdseg_route_rec(cdseg_route_template_id<CDSEG_RF_UNPOOL, KS, KP>(), 16, 64, 1, 0, 0, CDSEG_BF16 << CDSEG_ROUTE_F_CT_SHIFT, 0);
  hipLaunchKernelGGL((unpool_fused_kernel<KS, KP>), dim3((unsigned)blocks), dim3(PL_WAVES * 64), K::LDS, s, p);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

bool unpool_supported(int k_skip, int k_child, int c) { return c == 64 && ((k_skip == 32 && k_child == 64) || (k_skip == 64 && k_child == 128)); }

}  // namespace

extern "C" size_t cdseg_unpool_fused_img_bytes(int cin, int cout) {
  return cout == 64 && (cin == 32 || cin == 64 || cin == 128) ? (size_t)cin * cout * 2 : 0;
}

extern "C" int cdseg_unpool_fused_pack(const void* w, int cin, int cout, void* wimg, void* stream) {
  if (!w || !wimg || (((uintptr_t)w | (uintptr_t)wimg) & 15)) return CDSEG_ERR_ARG;
  if (!cdseg_unpool_fused_img_bytes(cin, cout)) return CDSEG_ERR_UNSUPPORTED;
  const int units = (cout / 16) * (cin / 32) * 64;
  hipLaunchKernelGGL(unpool_pack_kernel, dim3((units + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w, (uint4*)wimg,
                     cin, cout);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

// PRECONDITION: every run holds at least one row (seg_start strictly increasing), as for cdseg_pool_fused_n: the owner of a
// fine row is counted from the run ends in front of it, an empty run would shift the owners of the rows behind it.
extern "C" int cdseg_unpool_fused(const void* skip_x, int ld_skip, const void* wimg_skip, const float* bias_skip,
                                  const float* scale_skip, const float* shift_skip, const void* coarse_x, int ld_coarse,
                                  const void* wimg_child, const float* bias_child, const float* scale_child,
                                  const float* shift_child, const int32_t* seg_start, long m, int act, float* out, int ldo,
                                  void* out2, int ldo2, int k_skip, int k_child, int c, void* stream) {
  if (m <= 0) return CDSEG_OK;
  if (!skip_x || !wimg_skip || !coarse_x || !wimg_child || !seg_start || !out || !out2) return CDSEG_ERR_ARG;
  if (!unpool_supported(k_skip, k_child, c) || (act != CDSEG_ACT_NONE && act != CDSEG_ACT_GELU)) return CDSEG_ERR_UNSUPPORTED;
  auto mis = [](const void* ptr, int a) { return ptr && (((uintptr_t)ptr) & (a - 1)); };
  if ((ld_skip & 7) || (ld_coarse & 7) || (ldo & 3) || (ldo2 & 3) || mis(skip_x, 16) || mis(coarse_x, 16) || mis(wimg_skip, 16) ||
      mis(wimg_child, 16) || mis(out, 16) || mis(out2, 8) || mis(bias_skip, 16) || mis(scale_skip, 16) || mis(shift_skip, 16) ||
      mis(bias_child, 16) || mis(scale_child, 16) || mis(shift_child, 16) || (!scale_skip != !shift_skip) ||
      (!scale_child != !shift_child))
    return CDSEG_ERR_ARG;
  UnpoolP p;
  p.xs = (const bf16_t*)skip_x; p.xp = (const bf16_t*)coarse_x; p.wimg_s = (const uint4*)wimg_skip; p.wimg_p = (const uint4*)wimg_child;
  p.bias_s = bias_skip; p.scale_s = scale_skip; p.shift_s = shift_skip;
  p.bias_p = bias_child; p.scale_p = scale_child; p.shift_p = shift_child;
  p.seg = seg_start; p.out = out; p.out2 = (bf16_t*)out2; p.m = m;
  p.ldxs = ld_skip; p.ldp = ld_coarse; p.ldo = ldo; p.ldo2 = ldo2; p.act = act;
  hipStream_t s = (hipStream_t)stream;
  if (k_skip == 32) return launch_unpool<32, 64>(p, s);
  return launch_unpool<64, 128>(p, s);
}
