// choose_node(): the one place that maps a fused BiFPN node to a kernel form, a row segmentation and a launch shape
// (csrc/node_layer.h).  Host code only; the kernels are in bifpn_node.hip and bifpn_rows{,_ps,_wg}.hip.
#include <algorithm>

#include "bifpn_node.h"
#include "node_layer.h"

namespace jh {

NodeUse node_use(const NodeArgs& a, NodeBatchClass cls, bool want_pool) {
  NodeUse u;
  u.Cp = a.Cp; u.cout_p = a.cout_p; u.cout_p16 = a.cout_p16; u.N = a.N; u.H = a.H; u.W = a.W;
  u.n_in = a.n_in; u.act = a.act; u.cls = cls; u.want_pool = want_pool;
  for (int i = 0; i < 3; ++i) u.mode[i] = a.mode[i];
  return u;
}

std::string node_choice_name(const NodeChoice& c) {
  switch (c.form) {
    case NodeForm::RowsWave: return "rows_wave";
    case NodeForm::RowsPairs: return "rows_pairs";
    case NodeForm::RowsWg: return "rows_wg";
    default: return "tile";
  }
}

static int node_variant(const NodeUse& u, NodeVariant* v) {
  const int m1 = u.mode[1], m2 = u.mode[2];
  JH_REQUIRE(u.mode[0] == FUSE_SAME, "first input of a node is at the node's own level");
  if (u.n_in == 2 && m1 == FUSE_UP2) *v = NodeVariant::Up2;
  else if (u.n_in == 2 && m1 == FUSE_POOL2) *v = NodeVariant::Pool2;
  else if (u.n_in == 2 && m1 == FUSE_SAME) *v = NodeVariant::Same2;
  else if (u.n_in == 3 && m1 == FUSE_SAME && m2 == FUSE_POOL2) *v = NodeVariant::SamePool2;
  else if (u.n_in == 3 && m1 == FUSE_UP2 && m2 == FUSE_UP4) *v = NodeVariant::Up2Up4;
  else if (u.n_in == 3 && m1 == FUSE_SAME && m2 == FUSE_SAME) *v = NodeVariant::Same3;
  else JH_REQUIRE(false, "unsupported BiFPN node variant");
  return 0;
}

// The tile form's LDS layout: per-channel head (statistics, depthwise weights), halo tile, operand tile, and either the
// pointwise weights or the epilogue's fp64 partials behind it.
static int tile_layout(const NodeUse& u, NodeChoice* c) {
  const size_t head = ((size_t)3 * u.Cp * 2 + (size_t)9 * u.Cp) * sizeof(float);
  const size_t at_bytes = (size_t)128 * (u.Cp + 4) * sizeof(float);
  const size_t red = (size_t)8 * kNodeNRG * 16 * 2 * sizeof(double);   // conv_epilogue: fp64 partials
  const size_t halo_px = (size_t)kNodePY * kNodePX * sizeof(float);
  // preferred: the whole channel range in one halo chunk, operand tile aliased onto it
  // (3 workgroups per CU for the 56-channel pyramid of the small model)
  const size_t b_bytes = (size_t)(u.Cp / 8) * (u.cout_p16 / 16) * 128 * sizeof(float);
  c->blds = (b_bytes <= 16 * 1024) ? 1 : 0;        // 512 threads x 32 bytes
  c->lds = head + std::max(halo_px * u.Cp, at_bytes + (c->blds ? b_bytes : red));
  c->cf = u.Cp;
  c->alias = 1;
  if (u.Cp > 64 || u.Cp < 32 || c->lds > 54 * 1024) {
    // fallback: separate operand tile, halo chunked to the LDS budget
    c->alias = 0;
    c->blds = 0;
    size_t budget = 78 * 1024;
    const size_t fixed = head + at_bytes;
    if (fixed + halo_px * 12 > budget) budget = 156 * 1024;
    int cf = std::min(u.Cp, 64);          // the depthwise rounds handle <= 16 channel quads
    while (cf > 8 && fixed + halo_px * cf > budget) cf -= 4;
    c->cf = cf;
    c->lds = fixed + halo_px * cf;
    JH_REQUIRE(halo_px * cf >= red, "halo chunk too small");
  }
  JH_REQUIRE(c->lds <= 160 * 1024, "BiFPN node does not fit LDS");
  const int tiles = ((u.H + kNodeTY - 1) / kNodeTY) * ((u.W + kNodeTX - 1) / kNodeTX);
  c->grid = dim3(tiles, u.N);
  c->block = dim3(512);
  return 0;
}

int choose_node(const NodeUse& u, NodeChoice* out) {
  NodeChoice c;
  if (node_variant(u, &c.variant)) return 1;
  const NodeVariant v = c.variant;
  const bool below8 = u.cls == NodeBatchClass::Below8, atleast8 = u.cls == NodeBatchClass::AtLeast8;
  const int Cp16 = round_up(u.Cp, 16);

  // ---- form
  // 88 channels, class >= 8, a level whose width is no multiple of 16 (or below 16): the one-wave / pair forms need
  // whole 16-pixel strips, the tile kernel's path for more than 64 channels is slow whatever the level -- the workgroup
  // form masks the last strip's pixels past the row end.  The reference's DEFAULT geometry (320-pixel images: levels
  // 80 / 40 / 20 / 10 / 5) has four of its five levels here.
  const bool ragged88 = u.Cp == 88 && atleast8 && (u.W % 16 != 0 || u.W < 16);
  // Workgroup form: 160 channels (the large model) in every class but the tile-only one; 88 channels on ragged levels
  // and -- with short segments -- at time batches below 8, where one wave per strip is far too slow per row for a few
  // images (at bench scale it is the faster form there).  As many output channels as input channels, no padding.
  const bool wg = (u.Cp == 160 || (u.Cp == 88 && (below8 || ragged88))) && u.cout_p == u.Cp && u.cout_p16 == Cp16;
  // One wave per strip / pairs: the 56-channel (small model) or 88-channel (medium) pyramid.
  bool rows = wg || (!below8 && (u.Cp == 56 || u.Cp == 88));
  // (time batches below 8: the 56-channel pyramid keeps the tile form, 13 us per node for one frame set; the wide
  //  pyramids' tile path costs 35-130 us per node whatever the level.  JH_NODE_ROWS=0: never a row form)
  if (JH_ENV_KNOB("JH_NODE_ROWS") == 0) rows = false;
  // as many output column blocks as the input has
  if (u.cout_p16 != Cp16) rows = false;
  if (wg) {
    // the workgroup form masks the pixels past the row end of its last strip: every level down to 2 x 2
    if (u.W < 2 || u.H < 2) rows = false;
  } else if (u.W % 16 != 0 || u.W < (u.Cp >= 88 ? 16 : 32) || u.H < 16) {
    // (88 channels: also the 16-pixel-wide level -- one strip per image -- because the tile kernel's path for more than
    //  64 channels is slow there, 0.10 ms per launch against 0.05; at 56 channels the tile kernel wins below 32 pixels)
    rows = false;
  }
  // (one wave per workgroup walking >= 10 rows: below ~2048 strips the chip is not filled and the tile form wins)
  if (u.cls == NodeBatchClass::ByLaunchSize && ((u.W + 15) / 16) * ((u.H + 7) / 8) * u.N < 2048) rows = false;
  // no max-pooled input; up-sampled inputs of whole pixels; two same-level inputs in the workgroup form only
  if (v == NodeVariant::Up2) rows = rows && u.W % 2 == 0 && u.H % 2 == 0;
  else if (v == NodeVariant::Up2Up4) rows = rows && u.W % 4 == 0 && u.H % 4 == 0;
  else if (v == NodeVariant::Same2) rows = rows && wg;
  else if (v != NodeVariant::Same3) rows = false;

  if (!rows) {
    c.form = NodeForm::Tile;
    if (tile_layout(u, &c)) return 1;
    *out = c;
    return 0;
  }
  JH_REQUIRE(u.act == ACT_SILU || (u.act == ACT_NONE && (v == NodeVariant::Up2 || v == NodeVariant::Up2Up4)),
             "row-streaming node: activation");

  // ---- rows per workgroup: a function of the node and of the time-batch class ONLY -- the float partial sums of the
  // statistics are taken per strip segment, so the segmentation must not depend on how many images a launch carries
  // (bit-equal results for any number of cameras per rank).  Measured at 384 images, one wave per strip (P3 two-input
  // node: 8 rows 240 us, 16: 205, 32: 191; P4: 8: 74, 16: 66, 32: 71; three-input head: 16: 221, 32: 223; three
  // same-level inputs at P4: 8: 116, 16: 99): half the image height, 16 / 8 rows for the head.
  int seg_rows = v != NodeVariant::Up2Up4 ? std::max(8, u.H / 2) : (u.H >= 64 ? 16 : 8);
  if (wg) {
    c.form = NodeForm::RowsWg;
    c.strips = (u.W + 15) / 16;
    // Time batches below 8 (the single-frame caller among them: few images, a node is a latency chain of its rows):
    // short segments -- measured per node with one 12-camera frame set, 88 / 160 channels, us: 64-row levels 16 rows
    // 33 / 62 (8: 41 / 72, 4: 50 / 79, 32: 53 / 103); 32-row levels 4 rows 18 / 29 (8: 22 / 38, 2: 26 / 42); 16 rows
    // and below 2 rows 13 / 21 (4: 15 / 26, 8: 21 / 37).
    if (below8) seg_rows = u.H >= 64 ? 16 : (u.H >= 32 ? 4 : 2);
    // Otherwise, levels of 32 pixels and more: ONE segment per strip -- the workgroup's prologue (its waves' weight
    // slices, the statistics' fp64 arithmetic, two warm-up rows) is paid once per 64 rows instead of per 16 or 32:
    // measured at 160 channels, 384 images: P3 node 1.218 -> 1.133 ms, head 1.270 -> 1.024, P4 0.331 -> 0.292 /
    // 0.431 -> 0.389; the 16-pixel levels keep 8 rows, 0.106 against 0.112 with 16.
    // (88 channels on a ragged level keep half-image segments: 192 images x 3 strips of a 40-pixel level are 576
    //  workgroups on 512 slots with one segment per strip)
    else if (u.H >= 32 && !ragged88) seg_rows = u.H;
  } else {
    c.form = NodeForm::RowsWave;
    c.strips = u.W / 16;
    // 88 channels, producer / consumer pairs: four items per 512-thread workgroup, so fewer and longer segments fill
    // the chip better -- measured at 384 images: 32-row segments at the 32-pixel levels 0.155 -> 0.140 / 0.188 ->
    // 0.167 ms, the three-input head at 64 pixels 0.445 -> 0.397 with 32 rows instead of 16; the 16-pixel levels keep
    // 8 rows: 0.051 against 0.078 with one segment per image.
    if (u.Cp == 88 && u.H >= 32) {
      seg_rows = 32;
      // (the pairs of a workgroup must walk the same number of rows: a level that is no multiple of 32 -- 80 x 80 in
      //  the reference's DEFAULT 320-pixel geometry -- takes its largest even divisor up to 40 that leaves two
      //  segments; with 32 it fell back to the one-wave form at 1.4x the time per pixel)
      if (u.H % 32 != 0)
        for (int d = std::min(40, u.H / 2) & ~1; d >= 8; d -= 2)
          if (u.H % d == 0) { seg_rows = d; break; }
    }
  }
  seg_rows = (seg_rows + 1) & ~1;                // (even: the kernels' row loops are unrolled by two on row parity)
  if (seg_rows > u.H) seg_rows = u.H;
  c.seg_rows = seg_rows;
  c.segs = (u.H + seg_rows - 1) / seg_rows;
  // 88 channels at bench scale: producer / consumer wave pairs -- the same arithmetic per output value and the same
  // segmentation as one wave per strip, so the results are bit-equal.  Every pair of a workgroup must walk the same
  // number of rows, and the items must fill whole workgroups.
  const long items = (long)c.strips * c.segs * u.N;
  const int per_wg = bifpn_rows_ps_geo(88).items;
  if (!wg && u.Cp == 88 && u.cout_p == 88 && u.H % seg_rows == 0 && seg_rows % 2 == 0 && items % per_wg == 0)
    c.form = NodeForm::RowsPairs;

  // ---- pooled output: the two-input form can write the 2x2-max-pooled raw output on the side, so that the bottom-up
  // node of the next level reads a same-resolution tensor with THIS node's statistics; the workgroup form also from
  // three same-level inputs, so the bottom-up pass stays in a row form one level further down.
  // (an even width too: with an odd one the lane of the last pixel of a row would own pooled column W / 2, which is
  //  the first pixel of the NEXT pooled row -- across a segment border another workgroup's)
  c.pool = u.want_pool && u.act == ACT_SILU && u.cout_p == u.Cp && u.H % 2 == 0 && u.W % 2 == 0 &&
           (u.n_in == 2 || (wg && v == NodeVariant::Same3));
  JH_REQUIRE(!(c.pool && v == NodeVariant::Same2), "row-streaming node: pooled output of two same-level inputs");

  // ---- launch shape
  const NodeKernelGeo g = c.form == NodeForm::RowsWg      ? bifpn_rows_wg_geo(u.Cp)
                          : c.form == NodeForm::RowsPairs ? bifpn_rows_ps_geo(u.Cp)
                                                          : bifpn_rows_geo(u.Cp);
  c.grid = c.form == NodeForm::RowsPairs ? dim3((unsigned)(items / per_wg)) : dim3(c.strips * c.segs, u.N);
  c.block = dim3(g.block);
  c.lds = g.lds;
  *out = c;
  return 0;
}

}  // namespace jh
