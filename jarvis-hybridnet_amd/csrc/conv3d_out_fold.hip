// V2V output layer with the last two residual closings applied on load.
//
// The tail of V2VNet.forward (jarvis/hybridnet/v2vnet.py:27-43,75-83,98-102) is, per voxel,
//   skip = relu(IN(r_skip) + f1)                        closing pass of skip_res1
//   d1   = relu(IN(r_dec) + relu(IN(u0))) + skip        closing pass of decoder_res1
//   out  = W d1 + b                                     output_layer (1 x 1 x 1)
// with r_skip / r_dec the raw second convolutions of the two residual blocks, u0 the raw decoder_upsample1 output and
// f1 the materialised front_layers.1 output.  `skip` has one reader (the second pass) and `d1` has one reader (the
// output layer), each touching a voxel once: as three launches the two tensors are written and read back only to carry
// a value from one elementwise pass to the next.  This kernel reads the four inputs and writes `out`.
//
// Bit-equal to the three launches by construction:
//   * mean / rstd of the three statistics slots exactly as norm_apply_kernel derives them (elementwise.hip: fp64,
//     norm_coef_over_count of operand_load.h), one (slot, channel) per thread, shared through LDS;
//   * the elementwise part term for term what norm_apply_kernel evaluates (subtract, multiply, add, max; the build
//     contracts nothing);
//   * the contraction in the order of conv_mfma_kernel: voxels as A, weights as B (the packed operand of
//     pack_conv_weights as it is), per 8-channel step one v_mfma_f32_16x16x4_f32 over the channels 8 k8 + {0, 2, 4, 6}
//     and one over 8 k8 + {1, 3, 5, 7}, steps in ascending order from a zero accumulator, bias added afterwards.
//
// Form (conv_pw_direct.hip's): a wave owns 16-voxel row blocks, operands go from registers, no barrier after the
// prologue.  A lane (p = lane & 15, kq = lane >> 4) loads the 16-byte words u of voxel p, channels 16 u + 4 kq .. + 3 (a
// wave instruction reads 64 contiguous bytes per voxel), evaluates d1 for them, and the A operands -- lane (p, kq) needs
// the channel pair 8 k8 + 2 kq, + 1 -- come out of a 4 x 4 exchange between the four lane rows of a voxel: two
// v_permlane16_swap + two v_permlane32_swap per word.  The flagship's instantiation (six 8-channel steps) keeps the loads
// of the next row block in flight while the current one is multiplied (PF); every other channel count takes the plain
// load / compute loop at three waves per SIMD.  PF is instantiated for six steps ONLY: the five-step PF instantiation
// (J = 17..20) returned zeros in output channel 13 on the MI355X while the same source without PF is bit-equal; the cause
// was not found in the source or in the generated code, so that instantiation does not exist, and
// tests/test_hip_v2v_fold.py runs every instantiation that does.
#include "conv_mfma.h"

namespace jh {

namespace {
typedef float of4 __attribute__((ext_vector_type(4)));
typedef unsigned ou4 __attribute__((ext_vector_type(4)));

// The inputs of one launch.  Statistics: [T][Cp][kStatW] each.
struct OutFoldArgs {
  const float *r_dec, *u0, *r_skip, *f1;
  const double *st_dec, *st_u0, *st_skip;
  const float *w, *bias;
  float* y;
  int P, Cp, cout_p, cout_p16;
};

// K8: 8-channel steps (Cp / 8), NCB: column blocks of 16 output channels, PF: keep the next row block's loads in flight
// (the launcher: K8 == 6 only, see above)
template <int K8, int NCB, bool PF>
__global__ __launch_bounds__(256, 2) void conv3d_out_fold_kernel(const OutFoldArgs a, int rb_per_wave) {
  constexpr int KW = (K8 + 1) / 2;                 // 16-channel words per voxel (the last one half used when K8 is odd)
  __shared__ __attribute__((aligned(16))) float nrm_s[3][2][64];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int px = lane & 15, kq = lane >> 4;
  const int n = blockIdx.y;
  const int P = a.P, Cp = a.Cp;

  // ---- mean / rstd of the three normalised operands: thread (slot, c), norm_apply_kernel's expressions
  if (tid < 3 * Cp) {
    const int slot = tid / Cp, c = tid - slot * Cp;
    const double* base = slot == 0 ? a.st_dec : (slot == 1 ? a.st_u0 : a.st_skip);
    const NormCoef k = norm_coef_over_count(base + ((size_t)n * Cp + c) * kStatW, P);
    nrm_s[slot][0][c] = k.mean;
    nrm_s[slot][1][c] = k.rstd;
  }
  __syncthreads();                                 // the only barrier: waves are independent from here on
  const int nrb = P >> 4;
  const int rb0 = (blockIdx.x * 4 + wave) * rb_per_wave;
  const int rb1 = min(nrb, rb0 + rb_per_wave);
  if (rb0 >= nrb) return;

  of4 mu[3][KW], rs[3][KW];
#pragma unroll
  for (int u = 0; u < KW; ++u) {
    const bool in = 16 * u + 4 * kq < Cp;
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) {
      mu[sl][u] = in ? *reinterpret_cast<const of4*>(&nrm_s[sl][0][16 * u + 4 * kq]) : (of4){0.f, 0.f, 0.f, 0.f};
      rs[sl][u] = in ? *reinterpret_cast<const of4*>(&nrm_s[sl][1][16 * u + 4 * kq]) : (of4){1.f, 1.f, 1.f, 1.f};
    }
  }

  // ---- weights: the B operand of conv_mfma_kernel as packed ([k8][cb][64 lanes][2]), for the wave's life
  float2 bw[K8][NCB];
#pragma unroll
  for (int k8 = 0; k8 < K8; ++k8)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
      bw[k8][cb] = *reinterpret_cast<const float2*>(a.w + ((size_t)(k8 * NCB + cb) * 64 + lane) * 2);

  // ---- addressing: each tensor's frame set as a buffer; a lane's word u of voxel px of a row block
  const size_t img = (size_t)n * P * Cp;
  const int img_bytes = (int)((size_t)P * Cp * 4);
  const __amdgpu_buffer_rsrc_t rs_dec = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.r_dec + img), 0, img_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_u0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.u0 + img), 0, img_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_skip = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.r_skip + img), 0, img_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_f1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.f1 + img), 0, img_bytes, 0x00020000);
  int xoff[KW];
#pragma unroll
  for (int u = 0; u < KW; ++u)
    xoff[u] = 16 * u + 4 * kq < Cp ? (px * Cp + 16 * u + 4 * kq) * 4 : (int)0x80000000;     // past the tensor: reads 0
  const int xrb = 16 * Cp * 4;                      // bytes per row block
  // output: the accumulator holds 4 voxels x 1 channel per lane; after the lane-quad transpose (conv_epilogue's) a lane
  // holds voxel 4 kq + j, channels 16 cb + (px & ~3) .. + 3: one 16-byte store
  const int j = lane & 3;
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(
      a.y + (size_t)n * P * a.cout_p, 0, (int)((size_t)P * a.cout_p * 4), 0x00020000);
  int yoff[NCB];
  float bv[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    const int c0 = 16 * cb + (px & ~3), ch = 16 * cb + px;
    yoff[cb] = c0 < a.cout_p ? ((kq * 4 + j) * a.cout_p + c0) * 4 : (int)0x80000000;       // pad column blocks: dropped
    bv[cb] = (a.bias && ch < a.cout_p16) ? a.bias[ch] : 0.f;
  }
  const int yrb = 16 * a.cout_p * 4;

  struct Row { of4 d[KW], u[KW], s[KW], f[KW]; };
  auto load = [&](int rb, Row& r) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < KW; ++u) {
      r.d[u] = __builtin_bit_cast(of4, __builtin_amdgcn_raw_buffer_load_b128(rs_dec, xoff[u], rb * xrb, 0));
      r.u[u] = __builtin_bit_cast(of4, __builtin_amdgcn_raw_buffer_load_b128(rs_u0, xoff[u], rb * xrb, 0));
      r.s[u] = __builtin_bit_cast(of4, __builtin_amdgcn_raw_buffer_load_b128(rs_skip, xoff[u], rb * xrb, 0));
      r.f[u] = __builtin_bit_cast(of4, __builtin_amdgcn_raw_buffer_load_b128(rs_f1, xoff[u], rb * xrb, 0));
    }
  };
  auto compute = [&](int rb, const Row& r) __attribute__((always_inline)) {
    float2 av[2 * KW];                              // A operands: channel pair 8 k8 + 2 kq, + 1 of voxel px
#pragma unroll
    for (int u = 0; u < KW; ++u) {
      // norm_apply_kernel<ACT_RELU, true, true, true, true> (decoder_res1) with, as its r2, what
      // norm_apply_kernel<ACT_RELU, true, false, true> (skip_res1) stores
      of4 t = (r.d[u] - mu[0][u]) * rs[0][u];
      of4 e = (r.u[u] - mu[1][u]) * rs[1][u];
      of4 s = (r.s[u] - mu[2][u]) * rs[2][u];
#pragma unroll
      for (int i = 0; i < 4; ++i) e[i] = fmaxf(e[i], 0.f);
      t += e;
      s += r.f[u];
#pragma unroll
      for (int i = 0; i < 4; ++i) { t[i] = fmaxf(t[i], 0.f); s[i] = fmaxf(s[i], 0.f); }
      const of4 d1 = t + s;
      // lane row kq holds the pairs (16 u + 4 kq, + 1) and (+ 2, + 3); row kq = 2 a + b needs, for step 2 u + m, the pair
      // b of row 2 m + a: exchange (row bit 0 <-> pair), then (row bit 1 <-> pair)
      const auto x0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(d1[0]), __float_as_uint(d1[2]), false, false);
      const auto x1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(d1[1]), __float_as_uint(d1[3]), false, false);
      const auto z0 = __builtin_amdgcn_permlane32_swap(x0[0], x0[1], false, false);
      const auto z1 = __builtin_amdgcn_permlane32_swap(x1[0], x1[1], false, false);
      av[2 * u] = make_float2(__uint_as_float(z0[0]), __uint_as_float(z1[0]));
      av[2 * u + 1] = make_float2(__uint_as_float(z0[1]), __uint_as_float(z1[1]));
    }
    f32x4 acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) acc[cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k8 = 0; k8 < K8; ++k8) {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
        acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[k8].x, bw[k8][cb].x, acc[cb], 0, 0, 0);
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
        acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[k8].y, bw[k8][cb].y, acc[cb], 0, 0, 0);
    }
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = acc[cb][i] + bv[cb];
      {
        float x, y;
        x = (j & 1) ? v[0] : v[1]; y = quad_xor1(x); if (j & 1) v[0] = y; else v[1] = y;
        x = (j & 1) ? v[2] : v[3]; y = quad_xor1(x); if (j & 1) v[2] = y; else v[3] = y;
        x = (j & 2) ? v[0] : v[2]; y = quad_xor2(x); if (j & 2) v[0] = y; else v[2] = y;
        x = (j & 2) ? v[1] : v[3]; y = quad_xor2(x); if (j & 2) v[1] = y; else v[3] = y;
      }
      const of4 o = (of4){v[0], v[1], v[2], v[3]};
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(ou4, o), yrs, yoff[cb], rb * yrb, 0);
    }
  };

  if constexpr (PF) {
    Row ra, rb_;
    int rb = rb0;
    load(rb, ra);
    while (true) {
      if (rb + 1 < rb1) load(rb + 1, rb_);
      compute(rb, ra);
      if (++rb >= rb1) break;
      if (rb + 1 < rb1) load(rb + 1, ra);
      compute(rb, rb_);
      if (++rb >= rb1) break;
    }
  } else {
    for (int rb = rb0; rb < rb1; ++rb) {
      Row r;
      load(rb, r);
      compute(rb, r);
    }
  }
}
}  // namespace

// Shapes the kernel takes: at most 64 input channels (2 J <= 64: eight 8-channel steps, two column blocks) and a whole
// number of 16-voxel row blocks per frame set ((G / 2)^3 a multiple of 16, i.e. G a multiple of 8).  A function of
// (J, G) only.
bool v2v_fold_shape(int J, int G) {
  return J >= 1 && J <= 32 && G >= 8 && G % 8 == 0;
}

// ... and whether a plan built NOW folds (JH_V2V_FOLD, default on; read at every call like the knobs of conv_layer.hip:
// plans of both settings live in one process)
bool v2v_fold_applies(int J, int G) {
  const char* e = getenv("JH_V2V_FOLD");
  return (e ? atoi(e) : 1) != 0 && v2v_fold_shape(J, G);
}

int launch_conv3d_out_fold(const ConvWeights& w, const Act& r_dec, const double* st_dec, const float* u0,
                           const double* st_u0, const float* r_skip, const double* st_skip, const float* f1,
                           const Act& y, hipStream_t s) {
  const size_t P = r_dec.pixels();
  JH_REQUIRE(w.layout == WeightLayout::Plain && w.cin_p == r_dec.Cp && w.cout_p16 == round_up(y.C, 16) && w.bias,
             "output fold: the packed weights of the 1 x 1 x 1 layer");
  JH_REQUIRE(r_dec.Cp <= 64 && w.cout_p16 <= 32 && (r_dec.Cp > 32) == (w.cout_p16 > 16) && P % 16 == 0 &&
             P * r_dec.Cp * 4 < ((size_t)1 << 31), "output fold: shape (v2v_fold_shape)");
  JH_REQUIRE(y.N == r_dec.N && y.pixels() == P && y.Cp == cpad(y.C) && st_dec && st_u0 && st_skip && u0 && r_skip && f1,
             "output fold: operands");
  OutFoldArgs a;
  a.r_dec = r_dec.p; a.u0 = u0; a.r_skip = r_skip; a.f1 = f1;
  a.st_dec = st_dec; a.st_u0 = st_u0; a.st_skip = st_skip;
  a.w = w.w; a.bias = w.bias; a.y = y.p;
  a.P = (int)P; a.Cp = r_dec.Cp; a.cout_p = y.Cp; a.cout_p16 = w.cout_p16;
  const int nrb = (int)(P / 16);
  // row blocks per wave: up to 16, to amortise the prologue (fp64 mean / rstd, weights), but never fewer waves than
  // fill the chip -- a single frame set spreads one row block per wave (no sums here: the blocking is free to depend on
  // the batch)
  const int rbw = (int)std::max<long>(1, std::min<long>(16, (long)nrb * r_dec.N / 4096));
  const dim3 grid((nrb + 4 * rbw - 1) / (4 * rbw), r_dec.N);
  const int k8 = a.Cp / 8;
#define JH_OF(K8V, NCBV)                                                                                       \
  if (k8 == K8V) {                                                                                             \
    hipLaunchKernelGGL((conv3d_out_fold_kernel<K8V, NCBV, (K8V == 6)>), grid, dim3(256), 0, s, a, rbw);        \
    JH_CHECK_HIP(hipGetLastError());                                                                           \
    return 0;                                                                                                  \
  }
  JH_OF(1, 1) JH_OF(2, 1) JH_OF(3, 1) JH_OF(4, 1) JH_OF(5, 2) JH_OF(6, 2) JH_OF(7, 2) JH_OF(8, 2)
#undef JH_OF
  JH_REQUIRE(false, "output fold: no kernel for this channel count");
}

}  // namespace jh
