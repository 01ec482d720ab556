// Arguments of the fused BiFPN node kernels (csrc/bifpn_node.hip, csrc/bifpn_rows*.hip); which kernel runs a node and
// how it is launched: csrc/node_layer.h.
#pragma once
#include "jh_common.h"

namespace jh {

struct NodeArgs {
  const float* in[3];
  const double* st[3];     // statistics of in[i] (sum, sumsq per (n,c)) or nullptr
  float inv_cnt[3];        // 1 / pixels the statistics were taken over
  int mode[3];
  float w[3];
  int n_in, act;
  const float* dw;         // [9][Cp]
  const float* pw;         // packed [Cp/8][cout_p16/16][64][2]
  const float* bias;       // [cout_p16]
  float* y;                // raw output [N][H][W][cout_p]
  double* stats;           // [N][cout_p][2]
  int N, H, W, Cp, cout_p, cout_p16, cf;   // cf = channels per halo chunk (multiple of 4)
  int blds = 0;            // pointwise weights staged in LDS behind the operand tile
  int alias = 0;           // operand tile written over the halo tile (single channel chunk)
  float* y_pool = nullptr; // row-streaming forms (NodeChoice::pool): also the 2x2-max-pooled raw output [N][H/2][W/2][cout_p]
  int reserved = 0;        // unused: keeps sizeof(NodeArgs), and with it the offsets of the row kernels' scalar arguments
};

#if defined(__HIPCC__)
constexpr int kNodeTY = 8, kNodeTX = 16, kNodePY = 10, kNodePX = 18, kNodeNRG = 4;

// Fetch of one channel quad of input k at output pixel (oy, ox) of the node: `b` is the
// (uniform) base of image n of that input at ITS resolution, offsets are 32-bit.
__device__ __forceinline__ float4 node_fetch_n(const float* b, int mode, int oy, int ox, int H, int W,
                                               int Cp, int c) {
  if (mode == FUSE_SAME) return *reinterpret_cast<const float4*>(b + ((oy * W + ox) * Cp + c));
  if (mode == FUSE_UP2)
    return *reinterpret_cast<const float4*>(b + (((oy >> 1) * (W >> 1) + (ox >> 1)) * Cp + c));
  if (mode == FUSE_UP4)
    return *reinterpret_cast<const float4*>(b + (((oy >> 2) * (W >> 2) + (ox >> 2)) * Cp + c));
  const int w = W * 2;                // FUSE_POOL2 (max commutes with the monotone IN map)
  const float* s = b + ((oy * 2 * w + ox * 2) * Cp + c);
  const float4 a0 = *reinterpret_cast<const float4*>(s);
  const float4 a1 = *reinterpret_cast<const float4*>(s + Cp);
  const float4 a2 = *reinterpret_cast<const float4*>(s + w * Cp);
  const float4 a3 = *reinterpret_cast<const float4*>(s + w * Cp + Cp);
  return make_float4(fmaxf(fmaxf(a0.x, a1.x), fmaxf(a2.x, a3.x)), fmaxf(fmaxf(a0.y, a1.y), fmaxf(a2.y, a3.y)),
                     fmaxf(fmaxf(a0.z, a1.z), fmaxf(a2.z, a3.z)), fmaxf(fmaxf(a0.w, a1.w), fmaxf(a2.w, a3.w)));
}
__device__ __forceinline__ size_t node_plane(int mode, int H, int W) {
  if (mode == FUSE_SAME) return (size_t)H * W;
  if (mode == FUSE_UP2) return (size_t)(H >> 1) * (W >> 1);
  if (mode == FUSE_UP4) return (size_t)(H >> 2) * (W >> 2);
  return (size_t)H * W * 4;
}

#endif

}  // namespace jh
