// ConvTranspose2d(k = 4, s = 2, p = 1) with all four output parities in ONE workgroup:
// nn.ConvTranspose2d of the keypoint head, jarvis/efficienttrack/model.py:90-96.
//
// Output (2y + py, 2x + px) is a 2 x 2-tap convolution of the input: even parities read inputs
// {y - 1, y}, odd ones {y, y + 1} (conv_host.hip: deconv2d_k4s2p1_desc).  The general kernel
// (conv_mfma.h) runs the four parities as four workgroups, each of which stages (nearly) the
// same input patch.  The layer is bound by the non-matrix instructions of staging, so here ONE
// workgroup stages the 10 x 18 halo patch of an 8 x 16 tile of INPUT pixels once and produces
// the 16 x 32 output pixels of all four parities from it:
//
//   for each of the 3 x 3 window positions (r, s):       A rows from LDS, once
//     for each parity (py, px) with r - py, s - px in {0, 1}:    (1, 2 or 4 of them: 16 in all)
//       MFMAs with that parity's packed weights of tap (r - py, s - px)
//
// i.e. a quarter of the staging work and 9 instead of 16 A-operand reads per channel step for
// the same 16 (parity, tap) MFMA groups.  Per parity the taps are visited in the order of the
// general kernel and the per-workgroup statistics cover the same pixels, so outputs and fused
// statistics are bit-identical to it.
//
// Operand layout ("paired"): in an fp32 MFMA stream every LDS read costs ~24 cycles and every
// global load ~36 cycles of issue whatever its width (tools/mfma_valu_coissue.hip), against 32 per
// MFMA, so both operands are read 16 bytes at a time: the patch keeps the channels of two
// consecutive 8-channel steps interleaved per lane quarter ([kq][step parity][2]), the weights are
// packed as [tap][step pair][column block][lane][4] (WeightLayout::ChannelPaired) --
// one ds_read_b128 / global_load_dwordx4 feeds four MFMAs instead of two.
//
// WINDOW FORM (deconv4_window_kernel, layers without fused statistics and without a gate: the
// keypoint head).  Padding every parity to 16-column blocks by itself costs J = 23 a quarter of
// its MFMAs (4 x 32 columns for 4 x 23).  Pair the outputs the other way: 2 wy - 1 with 2 wy.
// Both read exactly the inputs {wy - 1, wy}:
//
//   output 2 wy     (even parity of y = wy):      input wy - 1 -> kernel tap 3,  wy -> tap 1
//   output 2 wy - 1 (odd parity of y = wy - 1):   input wy - 1 -> kernel tap 2,  wy -> tap 0
//
// so the layer is ONE stride-1 2 x 2 convolution over windows (wy, wx) with 4 cout_p output
// columns, column = sub * cout_p + channel, sub = 2 sy + sx for output (2 wy - 1 + sy,
// 2 wx - 1 + sx): 96 columns = 6 blocks at J = 23 instead of 8, 4 A-row reads per channel step
// instead of 9, a 9 x 17 patch instead of 10 x 18.  Window tap (ty, tx) is tap (ty, tx) of the
// parity each output belongs to, so per output the products are accumulated in the order
// [channel pass][tap][8-channel step][k] of the four-parity kernel: bit-identical to it.
//
// Interior workgroups own the 8 x 16 tiles of the windows [0, H) x [0, W).  The windows wy = H
// (W + 1 of them, the corner included) and wx = W (H of them) give output row 2H - 1 and output
// column 2W - 1; their taps on the far side read nothing but zeros.  They form a 1-D list
// e = 0 .. W + H, 128 per EDGE workgroup of the same launch (grid x = tiles + ceil((H + W + 1) / 128)),
// staged as a line of input pixels -- row H - 1 from x = -1 to W, then column W - 1 from y = -1 to
// H - 1 -- in which row window e reads positions e, e + 1 and column window e reads e + 1, e + 2.  An edge workgroup
// runs three taps, (0, 0), (0, 1), (1, 0), the latter two with a zero slot for the windows of the
// other kind.  Outputs -1 and 2H / 2W are never stored; every element has exactly one writer.
//
// MFMAs per image at 64 x 64, 64 channels, J = 23: four-parity 32 workgroups x 2 passes x 16
// groups x 128 = 131 072; window form 32 x 2 x 4 taps x 384 = 98 304 interior + 2 x 2 x 3 x 384 =
// 4 608 edge = 0.785 of it.
#include <atomic>
#include <type_traits>
#include "conv_mfma.h"

namespace jh {

namespace {
constexpr int kDTY = 8, kDTX = 16, kDPY = kDTY + 2, kDPX = kDTX + 2, kDNPIX = kDPY * kDPX;
constexpr int kDSPAD = 4;
}  // namespace

// Staging shared by both kernels (as the PF kernels of conv_mfma.h: items addressed once, zero padding = out-of-range
// buffer loads, the next channel pass's loads in flight under this pass's MFMAs; InstanceNorm / activation on load).
// mean / rstd of image n's input channels into nrm[0 .. 2 cin_p)
__device__ __forceinline__ void deconv4_load_norm(const ConvArgs& a, float* nrm, int n, int tid) {
  if (a.in_stats) norm_table_fill(NormTable::MeanRstd, nrm, a.cin_p, a.in_stats, n, a.cin_p, a.in_inv, tid, 256);
}

// NPIX patch pixels of KC8 * 8 channels per pass; `map(pix, &iy, &ix)` says which input pixel a patch pixel is
// (false, or a pixel outside the image: zeros)
template <int KC8, int NPIX>
struct Deconv4Stage {
  static constexpr int KC = KC8 * 8, S2 = (KC + kDSPAD) / 2, Q4 = KC / 4, ITER = (NPIX * Q4 + 255) / 256;
  static_assert(256 % Q4 == 0, "one channel quad per thread");
  typedef float cf4 __attribute__((ext_vector_type(4)));
  float4 pf[ITER];
  int pvo[ITER];
  __amdgpu_buffer_rsrc_t xrs;
  int tid, c4;

  template <class Map>
  __device__ __forceinline__ void init(const ConvArgs& a, const float* xin, int tid_, Map map) {
    tid = tid_;
    c4 = tid % Q4;
    xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xin), 0, (int)((size_t)a.Hin * a.Win * a.in_px * 4),
                                            0x00020000);
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int pix = tid / Q4 + it * (256 / Q4);
      int iy = 0, ix = 0;
      const bool ok = map(pix, &iy, &ix) && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win;
      pvo[it] = ok ? ((iy * a.Win + ix) * a.in_px + c4 * 4) * 4 : (int)0x80000000;
    }
  }
  __device__ __forceinline__ void issue(const ConvArgs& a, int c0) {
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int off = (c0 + c4 * 4 < a.in_px) ? pvo[it] : (int)0x80000000;
      const cf4 v = __builtin_bit_cast(cf4, __builtin_amdgcn_raw_buffer_load_b128(xrs, off, c0 * 4, 0));
      pf[it] = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
  template <int MODE>
  __device__ __forceinline__ void commit_mode(const ConvArgs& a, const float* nrm, float2* lds2, int c0) {
    float4 mu = make_float4(0.f, 0.f, 0.f, 0.f), rs = make_float4(1.f, 1.f, 1.f, 1.f);
    const int cc = min(c0 + c4 * 4, a.cin_p - 4);      // (clamped: such items are 0 anyway)
    if (MODE != 0) {
      mu = *reinterpret_cast<const float4*>(nrm + cc);
      rs = *reinterpret_cast<const float4*>(nrm + a.cin_p + cc);
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int pix = tid / Q4 + it * (256 / Q4);
      if (pix < NPIX) {
        float4 v = pf[it];
        if (MODE != 0) {
          const float m = (pvo[it] < 0 || c0 + c4 * 4 >= a.in_px) ? 0.f : 1.f;
          v = act4(norm_sub4(v, mu, rs), mode_act(MODE));
          v.x *= m; v.y *= m; v.z *= m; v.w *= m;
        }
        // quad c4 = channels of step c4 / 2, lane quarters 2 (c4 & 1) and + 1; slot of
        // (step, quarter) inside its 16-channel pair: quarter * 2 + step parity
        float2* dst = lds2 + pix * S2 + (c4 >> 2) * 8 + (c4 & 1) * 4 + ((c4 >> 1) & 1);
        dst[0] = make_float2(v.x, v.y);
        dst[2] = make_float2(v.z, v.w);
      }
    }
  }
  // the pass's items from registers to the patch in LDS
  __device__ __forceinline__ void commit(const ConvArgs& a, const float* nrm, float2* lds2, int c0) {
    dispatch_mode(operand_mode(a.in_stats, a.in_act), [&](auto mode_c) __attribute__((always_inline)) {
      commit_mode<decltype(mode_c)::value>(a, nrm, lds2, c0);
    });
  }
};

// TR: layers without fused statistics issue the MFMAs with swapped operands (conv_epilogue_tr)
template <int NRP, int KC8, bool TR>
__global__ __launch_bounds__(256) void deconv4_fused_kernel(const ConvArgs a) {
  constexpr int MR = 2, NR = 4 * NRP;
  constexpr int KC = KC8 * 8, S = KC + kDSPAD, S2 = S / 2, KP = KC8 / 2;
  static_assert(KC8 % 2 == 0 && S2 % 2 == 0, "paired operand layout");
  extern __shared__ __attribute__((aligned(16))) float lds_all[];
  float* nrm = lds_all;                         // [cin_p] mean, [cin_p] rstd (optional)
  float* lds = lds_all + a.nrm_floats;          // halo patch [180][S]
  float2* lds2 = reinterpret_cast<float2*>(lds);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mrow = lane & 15, kq = lane >> 4;
  const int tiles_x = (a.Win + kDTX - 1) / kDTX;
  const BlockId bid = xcd_block();
  const int tile_x = bid.x % tiles_x, tile_y = bid.x / tiles_x;
  const int n = bid.z;
  const int oy0 = tile_y * kDTY, ox0 = tile_x * kDTX;          // in input pixels
  const int iy0 = oy0 - 1, ix0 = ox0 - 1;

  int abase[MR];
#pragma unroll
  for (int mr = 0; mr < MR; ++mr) {
    const int p = (wave * MR + mr) * 16 + mrow;
    abase[mr] = ((p / kDTX) * kDPX + p % kDTX) * S2 + kq * 2;          // (float2 units, 16-byte aligned)
  }
  f32x4 acc[MR][NR];                            // [row block][parity * NRP + column block]
#pragma unroll
  for (int mr = 0; mr < MR; ++mr)
#pragma unroll
    for (int nr = 0; nr < NR; ++nr) acc[mr][nr] = (f32x4){0.f, 0.f, 0.f, 0.f};

  deconv4_load_norm(a, nrm, n, tid);
  const float* __restrict__ xin = a.x + (size_t)n * a.Hin * a.Win * a.in_px;
  const int nkc8_total = a.cin_p >> 3;
  const float4* __restrict__ wbase = reinterpret_cast<const float4*>(a.w);
  const unsigned ulane = lane;
  const int tap_stride = (nkc8_total >> 1) * NRP * 64;     // float4 units (launcher: cout_p16 = 16 NRP)
  const int phase_stride4 = (int)(a.phase_stride >> 2);

  Deconv4Stage<KC8, kDNPIX> st;
  st.init(a, xin, tid, [&](int pix, int* iy, int* ix) {
    *iy = iy0 + pix / kDPX; *ix = ix0 + pix % kDPX;
    return pix < kDNPIX;
  });
  st.issue(a, 0);

  for (int c0 = 0; c0 < a.cin_p; c0 += KC) {
    __syncthreads();
    st.commit(a, nrm, lds2, c0);
    __syncthreads();
    if (c0 + KC < a.cin_p) st.issue(a, c0 + KC);

    int koff[KP];
#pragma unroll
    for (int k8 = 0; k8 < KP; ++k8) koff[k8] = min((c0 >> 4) + k8, (nkc8_total >> 1) - 1) * NRP * 64;
    // the 16 (window position, parity) groups in window order; the weights of group g + 1 are
    // requested before the MFMAs of group g
    auto wptr = [&](int g) __attribute__((always_inline)) -> const float4* {
      // g -> (r, s, py, px) by enumeration (compile-time after unrolling)
      int idx = 0;
      for (int r = 0; r < 3; ++r)
        for (int s = 0; s < 3; ++s)
          for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) {
              const int ty = r - py, tx = s - px;
              if (ty < 0 || ty > 1 || tx < 0 || tx > 1) continue;
              if (idx == g) return wbase + (size_t)(py * 2 + px) * phase_stride4 + (ty * 2 + tx) * tap_stride;
              ++idx;
            }
      return wbase;
    };
    // Pinned software pipeline (left alone the compiler sinks every weight load to a few MFMAs
    // before its use, far less than an L2 round trip): the weights of group g + 2 and the A rows of
    // the next window position are requested BEFORE the 32 MFMAs of group g, and the scheduling
    // barriers keep them there.
    float4 bq[3][KP][NRP];
#pragma unroll
    for (int g0 = 0; g0 < 2; ++g0) {
      const float4* w0 = wptr(g0) + ulane;
#pragma unroll
      for (int k8 = 0; k8 < KP; ++k8)
#pragma unroll
        for (int nr = 0; nr < NRP; ++nr) bq[g0][k8][nr] = w0[koff[k8] + nr * 64];
    }
    float4 an[KP][MR];
#pragma unroll
    for (int k8 = 0; k8 < KP; ++k8)
#pragma unroll
      for (int mr = 0; mr < MR; ++mr) an[k8][mr] = *reinterpret_cast<const float4*>(lds2 + abase[mr] + k8 * 8);
    int g = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        float4 ac[KP][MR];
#pragma unroll
        for (int k8 = 0; k8 < KP; ++k8)
#pragma unroll
          for (int mr = 0; mr < MR; ++mr) ac[k8][mr] = an[k8][mr];
        if (r * 3 + s + 1 < 9) {
          const int r1 = (r * 3 + s + 1) / 3, s1 = (r * 3 + s + 1) % 3;
#pragma unroll
          for (int k8 = 0; k8 < KP; ++k8)
#pragma unroll
            for (int mr = 0; mr < MR; ++mr)
              an[k8][mr] = *reinterpret_cast<const float4*>(lds2 + abase[mr] + (r1 * kDPX + s1) * S2 + k8 * 8);
        }
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
          for (int px = 0; px < 2; ++px) {
            const int ty = r - py, tx = s - px;
            if (ty < 0 || ty > 1 || tx < 0 || tx > 1) continue;
            if (g + 2 < 16) {
              const float4* wn = wptr(g + 2) + ulane;
#pragma unroll
              for (int k8 = 0; k8 < KP; ++k8)
#pragma unroll
                for (int nr = 0; nr < NRP; ++nr) bq[(g + 2) % 3][k8][nr] = wn[koff[k8] + nr * 64];
            }
            __builtin_amdgcn_sched_barrier(0);
            const int ph = py * 2 + px;
#pragma unroll
            for (int k8 = 0; k8 < KP; ++k8) {
              // x, y: the even 8-channel step; z, w: the odd one (the order of the unpaired kernels)
#define JH_D4_STEP(C)                                                                                          \
  _Pragma("unroll") for (int mr = 0; mr < MR; ++mr) _Pragma("unroll") for (int nr = 0; nr < NRP; ++nr)       \
    acc[mr][ph * NRP + nr] = TR ? __builtin_amdgcn_mfma_f32_16x16x4f32(bq[g % 3][k8][nr].C, ac[k8][mr].C,    \
                                                                       acc[mr][ph * NRP + nr], 0, 0, 0)       \
                                : __builtin_amdgcn_mfma_f32_16x16x4f32(ac[k8][mr].C, bq[g % 3][k8][nr].C,    \
                                                                       acc[mr][ph * NRP + nr], 0, 0, 0);
              JH_D4_STEP(x) JH_D4_STEP(y) JH_D4_STEP(z) JH_D4_STEP(w)
#undef JH_D4_STEP
            }
            __builtin_amdgcn_sched_barrier(0);
            ++g;
          }
      }
  }

  // ---- epilogue, one parity at a time
  __syncthreads();
  EpilogueArgs e;
  e.y = a.y + (size_t)n * a.Hy * a.Wy * a.cout_p;
  e.bias = a.bias;
  e.stats = a.stats ? a.stats + (size_t)n * a.cout_p * kStatW : nullptr;
  e.Dout = 1; e.Hout = a.Hin; e.Wout = a.Win; e.Hy = a.Hy; e.Wy = a.Wy;
  e.cout_p = a.cout_p; e.cout_p16 = a.cout_p16; e.os = 2; e.osz = 2; e.offz = 0;
  const bool full = oy0 + kDTY <= a.Hin && ox0 + kDTX <= a.Win;
#pragma unroll
  for (int ph = 0; ph < 4; ++ph) {
    f32x4 pa[MR][NRP];
#pragma unroll
    for (int mr = 0; mr < MR; ++mr)
#pragma unroll
      for (int nr = 0; nr < NRP; ++nr) pa[mr][nr] = acc[mr][ph * NRP + nr];
    e.offy = ph >> 1; e.offx = ph & 1;
    if constexpr (TR) {
      if (full) conv_epilogue_tr<MR, NRP, kDTY, kDTX, true>(pa, e, 0, 0, oy0, ox0, tid);
      else conv_epilogue_tr<MR, NRP, kDTY, kDTX, false>(pa, e, 0, 0, oy0, ox0, tid);
    } else {
      if (full) conv_epilogue<MR, NRP, kDTY, kDTX, 4, true>(pa, e, lds, 0, 0, oy0, ox0, tid);
      else conv_epilogue<MR, NRP, kDTY, kDTX>(pa, e, lds, 0, 0, oy0, ox0, tid);
      if (e.stats && ph < 3) __syncthreads();   // the reduction scratch is reused
    }
  }
}

template <int NRP, int KC8, bool TR>
static int launch_deconv4_tr(const ConvArgs& a, hipStream_t s) {
  size_t lds = (size_t)kDNPIX * (KC8 * 8 + kDSPAD) * sizeof(float);
  const size_t red = (size_t)4 * 4 * 16 * 2 * sizeof(double);
  if (lds < red) lds = red;
  lds += (size_t)a.nrm_floats * sizeof(float);
  auto kern = deconv4_fused_kernel<NRP, KC8, TR>;
  const int tiles = ((a.Hin + kDTY - 1) / kDTY) * ((a.Win + kDTX - 1) / kDTX);
  hipLaunchKernelGGL(kern, dim3(tiles, 1, a.N), dim3(256), lds, s, a);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}

template <int NRP, int KC8>
static int launch_deconv4_inst(const ConvArgs& a, hipStream_t s) {
  if (!a.stats) return launch_deconv4_tr<NRP, KC8, true>(a, s);
  return launch_deconv4_tr<NRP, KC8, false>(a, s);
}

// ------------------------------------------------------------------------------ window form
namespace {
constexpr int kWPY = kDTY + 1, kWPX = kDTX + 1, kWNPIX = kWPY * kWPX;     // 9 x 17 halo patch
constexpr int kWELINE = 130, kWEZERO = kWELINE, kWENPIX = kWELINE + 1;      // edge line + the zero slot
constexpr int kWLDSPIX = kWNPIX > kWENPIX ? kWNPIX : kWENPIX;
}  // namespace

// NB: column blocks of 16 over the 4 cout_p columns (even); EDGE: the 1-D list of edge windows (unit: which 128 of
// them); interior: the 8 x 16 tile of windows that starts at (wy0, wx0)
template <int NB, int KC8, bool EDGE>
__device__ __forceinline__ void deconv4_window_body(const ConvArgs& a, const int n, const int unit, const int wy0,
                                                    const int wx0) {
  constexpr int MR = 2, NT = EDGE ? 3 : 4, NCH = NB / 2, NG = NT * NCH;
  constexpr int KC = KC8 * 8, S = KC + kDSPAD, S2 = S / 2, KP = KC8 / 2;
  constexpr int NPIX = EDGE ? kWENPIX : kWNPIX;
  static_assert(KC8 % 2 == 0 && S2 % 2 == 0 && NB % 2 == 0, "paired operand layout, column blocks in twos");
  extern __shared__ __attribute__((aligned(16))) float lds_all[];
  float* nrm = lds_all;                         // [cin_p] mean, [cin_p] rstd (optional)
  float* lds = lds_all + a.nrm_floats;          // patch [NPIX][S]
  float2* lds2 = reinterpret_cast<float2*>(lds);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mrow = lane & 15, kq = lane >> 4;
  const int H = a.Hin, W = a.Win;
  const int e0 = unit * 128;                                                                       // first edge window

  // A rows of (tap, row block), float2 units, 16-byte aligned
  int arow[NT][MR];
#pragma unroll
  for (int mr = 0; mr < MR; ++mr) {
    const int p = (wave * MR + mr) * 16 + mrow;
    if (EDGE) {
      const int e = e0 + p;
      const bool rw = e <= W, cw = !rw && e <= W + H;
      arow[0][mr] = (rw ? p : (cw ? p + 1 : kWEZERO)) * S2 + kq * 2;
      arow[1][mr] = (rw ? p + 1 : kWEZERO) * S2 + kq * 2;
      arow[2][mr] = (cw ? p + 2 : kWEZERO) * S2 + kq * 2;
    } else {
#pragma unroll
      for (int t = 0; t < NT; ++t)
        arow[t][mr] = ((p / kDTX + (t >> 1)) * kWPX + p % kDTX + (t & 1)) * S2 + kq * 2;
    }
  }
  f32x4 acc[MR][NB];
#pragma unroll
  for (int mr = 0; mr < MR; ++mr)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[mr][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};

  deconv4_load_norm(a, nrm, n, tid);
  const float* __restrict__ xin = a.x + (size_t)n * H * W * a.in_px;
  const int npair = ((a.cin_p >> 3) + 1) >> 1;             // (cin_p % 16 == 8: the last pair's odd step is zeros)
  const float4* __restrict__ wbase = reinterpret_cast<const float4*>(a.w);
  const unsigned ulane = lane;
  const int tap_stride = npair * NB * 64;                  // float4 units

  Deconv4Stage<KC8, NPIX> st;
  st.init(a, xin, tid, [&](int pix, int* iy, int* ix) {
    if (EDGE) {
      const int pos = e0 + pix;                 // row H - 1 from x = -1 to W, then column W - 1 from y = -1 to H - 1
      const bool row = pos <= W + 1;
      *iy = row ? H - 1 : pos - W - 3;
      *ix = row ? pos - 1 : W - 1;
      return pix < kWELINE;                     // (the slot behind the line stays zero)
    }
    *iy = wy0 - 1 + pix / kWPX; *ix = wx0 - 1 + pix % kWPX;
    return pix < kWNPIX;
  });
  st.issue(a, 0);

  for (int c0 = 0; c0 < a.cin_p; c0 += KC) {
    __syncthreads();
    st.commit(a, nrm, lds2, c0);
    __syncthreads();
    if (c0 + KC < a.cin_p) st.issue(a, c0 + KC);

    int koff[KP];
#pragma unroll
    for (int k8 = 0; k8 < KP; ++k8) koff[k8] = min((c0 >> 4) + k8, npair - 1) * NB * 64;
    // groups g = (tap, two column blocks) in that order, 32 MFMAs each; pinned pipeline as in
    // deconv4_fused_kernel: weights two groups ahead, A rows one tap ahead
    auto wptr = [&](int g) __attribute__((always_inline)) -> const float4* {
      // (tap g / NCH: the edge taps (0, 0), (0, 1), (1, 0) are the first three of the four)
      return wbase + (g / NCH) * tap_stride + (g % NCH) * 128;
    };
    float4 bq[3][KP][2];
#pragma unroll
    for (int g0 = 0; g0 < 2 && g0 < NG; ++g0) {
      const float4* w0 = wptr(g0) + ulane;
#pragma unroll
      for (int k8 = 0; k8 < KP; ++k8)
#pragma unroll
        for (int nr = 0; nr < 2; ++nr) bq[g0][k8][nr] = w0[koff[k8] + nr * 64];
    }
    float4 an[KP][MR];
#pragma unroll
    for (int k8 = 0; k8 < KP; ++k8)
#pragma unroll
      for (int mr = 0; mr < MR; ++mr) an[k8][mr] = *reinterpret_cast<const float4*>(lds2 + arow[0][mr] + k8 * 8);
    int g = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      float4 ac[KP][MR];
#pragma unroll
      for (int k8 = 0; k8 < KP; ++k8)
#pragma unroll
        for (int mr = 0; mr < MR; ++mr) ac[k8][mr] = an[k8][mr];
      if (t + 1 < NT) {
#pragma unroll
        for (int k8 = 0; k8 < KP; ++k8)
#pragma unroll
          for (int mr = 0; mr < MR; ++mr)
            an[k8][mr] = *reinterpret_cast<const float4*>(lds2 + arow[t + 1 < NT ? t + 1 : t][mr] + k8 * 8);
      }
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        if (g + 2 < NG) {
          const float4* wn = wptr(g + 2) + ulane;
#pragma unroll
          for (int k8 = 0; k8 < KP; ++k8)
#pragma unroll
            for (int nr = 0; nr < 2; ++nr) bq[(g + 2) % 3][k8][nr] = wn[koff[k8] + nr * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k8 = 0; k8 < KP; ++k8) {
          // x, y: the even 8-channel step; z, w: the odd one
#define JH_D4W_STEP(C)                                                                                         \
  _Pragma("unroll") for (int mr = 0; mr < MR; ++mr) _Pragma("unroll") for (int nr = 0; nr < 2; ++nr)          \
    acc[mr][ch * 2 + nr] = __builtin_amdgcn_mfma_f32_16x16x4f32(bq[g % 3][k8][nr].C, ac[k8][mr].C,            \
                                                                acc[mr][ch * 2 + nr], 0, 0, 0);
          JH_D4W_STEP(x) JH_D4W_STEP(y) JH_D4W_STEP(z) JH_D4W_STEP(w)
#undef JH_D4W_STEP
        }
        __builtin_amdgcn_sched_barrier(0);
        ++g;
      }
    }
  }

  // ---- epilogue (swapped operands: a lane holds four consecutive columns of window lane & 15)
  float* __restrict__ y = a.y + (size_t)n * a.Hy * a.Wy * a.cout_p;
  const int cp = a.cout_p;
#pragma unroll
  for (int mr = 0; mr < MR; ++mr) {
    const int p = (wave * MR + mr) * 16 + mrow;
    int wy, wx;
    bool ok;
    if (EDGE) {
      const int e = e0 + p;
      const bool rw = e <= W;
      wy = rw ? H : e - W - 1; wx = rw ? e : W;
      ok = e <= W + H;
    } else {
      wy = wy0 + p / kDTX; wx = wx0 + p % kDTX;
      ok = wy < H && wx < W;
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int c = nb * 16 + kq * 4;
      const int sub = (c >= cp) + (c >= 2 * cp) + (c >= 3 * cp);     // (cout_p % 8 == 0: a lane's four columns share it)
      const int ch = c - sub * cp;
      const int oy = 2 * wy - 1 + (sub >> 1), ox = 2 * wx - 1 + (sub & 1);
      f32x4 v = acc[mr][nb];
      if (a.bias) v += *reinterpret_cast<const f32x4*>(a.bias + min(ch, a.cout_p16 - 4));
      if (ok && c < 4 * cp && (unsigned)oy < (unsigned)a.Hy && (unsigned)ox < (unsigned)a.Wy)
        *reinterpret_cast<f32x4*>(y + ((size_t)oy * a.Wy + ox) * cp + ch) = v;
    }
  }
}

template <int NB, int KC8>
__global__ __launch_bounds__(256) void deconv4_window_kernel(const ConvArgs a) {
  const BlockId bid = xcd_block();
  const int H = a.Hin, W = a.Win;
  const int tiles_x = (W + kDTX - 1) / kDTX;
  const int tiles = ((H + kDTY - 1) / kDTY) * tiles_x;
  const bool edge = (int)bid.x >= tiles;
  const int unit = edge ? (int)bid.x - tiles : (int)bid.x;
  int wy0 = (unit / tiles_x) * kDTY, wx0 = (unit % tiles_x) * kDTX;                                // first window
  if (a.box) {
    // BOX (ConvArgs::box): only the stored pixels [x0, x1] x [y0, y1] of image n have a reader.  Output pixel p
    // belongs to window (p + 1) / 2, so the box is the windows [wlo, whi] of either axis, and the interior tiles are
    // laid from its first window instead of from window 0: a tile that starts behind the box's last interior window
    // has nothing to do and ends here, before it stages anything.  A tile's origin is clamped so that it never
    // leaves the image -- two tiles may then overlap, and an output is the same bits whichever tile computes it
    // (its products and their order do not depend on where in a tile its window sits).  The edge workgroups run
    // only where the box reaches output row 2H - 1 or column 2W - 1.  (n is uniform: one scalar 16-byte load.)
    const int4 b = a.box[bid.z];
    const int wx_lo = (b.x + 1) >> 1, wy_lo = (b.y + 1) >> 1, wx_hi = (b.z + 1) >> 1, wy_hi = (b.w + 1) >> 1;
    if (edge) {
      if (wy_hi < H && wx_hi < W) return;
    } else {
      wy0 += wy_lo; wx0 += wx_lo;
      if (wy0 > min(wy_hi, H - 1) || wx0 > min(wx_hi, W - 1)) return;
      wy0 = min(wy0, max(H - kDTY, 0)); wx0 = min(wx0, max(W - kDTX, 0));
    }
  }
  if (!edge) deconv4_window_body<NB, KC8, false>(a, bid.z, unit, wy0, wx0);
  else deconv4_window_body<NB, KC8, true>(a, bid.z, unit, 0, 0);
}

// (test-only: how tests/test_hip_deconv4_window.py tells which form a call took; under graph capture it counts
// captures, not replays)
static std::atomic<long> g_window_launches{0};
long deconv4_window_launches() { return g_window_launches.load(); }

// Channels per LDS pass of the window form: those of the form it replaces (the pass is part of the
// order of accumulation) -- deconv4_fused_kernel's where that kernel takes the layer, else the
// general four-phase path's pick_kc8; 0 where that is an odd number of 8-channel steps.
// (conv_launch_2d_k2 takes the 8 x 8 geometry for images up to 8 wide: pick_kc8 reads the geometry only through
// the LDS budget, and the patch of either geometry fits it at every pass size -- 153 x 36 floats = 22 KB of 40 --
// so the pass is the same for both; tests/test_hip_deconv4_window.py has an 88-channel shape 8 wide.)
static_assert(ConvGeom<2, 2, 1, 1, kDTY, kDTX>::NPIX * (32 + 4) * sizeof(float) <= kConvLdsBudget &&
              ConvGeom<2, 2, 1, 1, 8, 8>::NPIX <= ConvGeom<2, 2, 1, 1, kDTY, kDTX>::NPIX,
              "the general path's pass size must not depend on its tile geometry");
static int deconv4_window_kc8(int cin_p) {
  if (cin_p % 16 == 0) return cin_p % 32 == 0 ? 4 : 2;
  const int k = pick_kc8(cin_p, &ConvGeom<2, 2, 1, 1, kDTY, kDTX>::lds_bytes, kConvLdsBudget);
  return k % 2 == 0 ? k : 0;
}

// Layers the window form takes when they run without statistics and gate: fewer column blocks over
// 4 cout_p than four times over cout_p16.  wide: also cout 25..32, 8 blocks in either form
bool deconv4_window_eligible(int cin_p, int cout_p, bool wide) {
  const int nbw = (4 * cout_p + 15) / 16;
  return (nbw == 2 || nbw == 6 || (wide && nbw == 8)) && cin_p % 8 == 0 && deconv4_window_kc8(cin_p) != 0;
}

template <int NB, int KC8>
static int launch_deconv4_window_inst(const ConvArgs& a, hipStream_t s) {
  const size_t lds = (size_t)kWLDSPIX * (KC8 * 8 + kDSPAD) * sizeof(float) + (size_t)a.nrm_floats * sizeof(float);
  const int tiles = ((a.Hin + kDTY - 1) / kDTY) * ((a.Win + kDTX - 1) / kDTX);
  const int edge = (a.Hin + a.Win + 1 + 127) / 128;
  hipLaunchKernelGGL((deconv4_window_kernel<NB, KC8>), dim3(tiles + edge, 1, a.N), dim3(256), lds, s, a);
  JH_CHECK_HIP(hipGetLastError());
  ++g_window_launches;
  return 0;
}

int launch_deconv4_window(const ConvArgs& a, hipStream_t s) {
  const int nb = (4 * a.cout_p + 15) / 16, kc8 = deconv4_window_kc8(a.cin_p);
  JH_REQUIRE(a.layout == WeightLayout::Window && a.nphase == 4 && !a.stats && !a.gate && !a.se.pool &&
             deconv4_window_eligible(a.cin_p, a.cout_p, true), "not a layer of the window form");
  JH_REQUIRE((long)a.Hin * a.Win * a.in_px < (1L << 29) && (long)a.Hy * a.Wy * a.cout_p < (1L << 31),
             "image too large for the window form's 32-bit offsets");
  if (nb == 8 && kc8 == 4) return launch_deconv4_window_inst<8, 4>(a, s);
  if (nb == 8 && kc8 == 2) return launch_deconv4_window_inst<8, 2>(a, s);
  if (nb == 6 && kc8 == 4) return launch_deconv4_window_inst<6, 4>(a, s);
  if (nb == 6 && kc8 == 2) return launch_deconv4_window_inst<6, 2>(a, s);
  if (nb == 2 && kc8 == 4) return launch_deconv4_window_inst<2, 4>(a, s);
  return launch_deconv4_window_inst<2, 2>(a, s);
}

// Layers this kernel takes (their weights are then packed in the paired layout)
bool deconv4_eligible(int cin_p, int cout_p16) {
  return cout_p16 <= 32 && cin_p % 16 == 0;
}

int launch_deconv4_fused(const ConvArgs& a, hipStream_t s) {
  const int nrp = a.cout_p16 / 16;
  // (conv_weight_layout, csrc/conv_layer.hip, decided with deconv4_eligible)
  JH_REQUIRE(a.layout == WeightLayout::ChannelPaired && !a.gate && nrp <= 2 && a.nphase == 4,
             "not a layer of the fused four-parity kernel");
  const int kc8 = a.cin_p % 32 == 0 ? 4 : 2;
  if (nrp == 2 && kc8 == 4) return launch_deconv4_inst<2, 4>(a, s);
  if (nrp == 2 && kc8 == 2) return launch_deconv4_inst<2, 2>(a, s);
  if (nrp == 1 && kc8 == 4) return launch_deconv4_inst<1, 4>(a, s);
  return launch_deconv4_inst<1, 2>(a, s);
}

}  // namespace jh
