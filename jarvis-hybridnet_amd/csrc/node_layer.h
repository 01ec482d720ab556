// One fused BiFPN node: which kernel form runs it, how its rows are segmented, and its launch.
//
// Every caller that runs a node -- the network plan (EffTrackPlan::node) and the single-operator entry point
// (jh_op_bifpn_node) -- describes the node (NodeUse), asks choose_node() once and hands the answer to
// launch_bifpn_node() with the kernel argument.  The rules that map a node to a form, a segmentation and a launch
// shape live in choose_node() and nowhere else (by channels, level and time-batch class only).
#pragma once
#include <string>
#include "jh_common.h"

namespace jh {

struct NodeArgs;            // the kernel argument (csrc/bifpn_node.h)

// The predictor's time-batch class.  A predictor sets it from its time batch ALONE (not from the number of cameras it
// owns), so that a camera-sharded rank and the single-GPU run of the same time batch launch the same kernels and stay
// bit-equal.  ByLaunchSize: the stand-alone operator, a row form only where the launch fills the chip.
enum class NodeBatchClass { ByLaunchSize = 0, Below8 = 1, AtLeast8 = 2 };

// Everything the rules of choose_node() read (channel counts padded as the plan pads them).
struct NodeUse {
  int Cp = 0, cout_p = 0, cout_p16 = 0, N = 0, H = 0, W = 0;
  int n_in = 0, mode[3] = {0, 0, 0}, act = 0;
  NodeBatchClass cls = NodeBatchClass::ByLaunchSize;
  bool want_pool = false;   // the caller could use the 2x2-max-pooled raw output, if the form can write it
};

NodeUse node_use(const NodeArgs& a, NodeBatchClass cls, bool want_pool);   // shape, inputs and activation from `a`

enum class NodeForm {
  Tile,        // 8 x 16 pixels per workgroup (bifpn_node.hip)
  RowsWave,    // one wave per 16-pixel strip (bifpn_rows.hip)
  RowsPairs,   // producer / consumer wave pairs (bifpn_rows_ps.hip)
  RowsWg,      // one workgroup per strip (bifpn_rows_wg.hip)
};
// The fusions that exist; the first input is always at the node's own level.
enum class NodeVariant {
  Up2,         // + x2 up-sampled
  Up2Up4,      // + x2 and x4 up-sampled (the head)
  Same3,       // + two more same-level inputs (bottom-up node whose finer input arrives pooled)
  Same2,       // + one more same-level input (the coarsest level's bottom-up node)
  Pool2,       // + 2x2-max-pooled
  SamePool2,   // + same level + 2x2-max-pooled
};

struct NodeChoice {
  NodeForm form = NodeForm::Tile;
  NodeVariant variant = NodeVariant::Up2;
  bool pool = false;                      // the form can and will write NodeArgs::y_pool
  int seg_rows = 0, strips = 0, segs = 0; // row forms: rows per strip segment, strips per row, segments per strip
  dim3 grid, block;
  size_t lds = 0;
  int blds = 0, alias = 0, cf = 0;        // tile form: NodeArgs::blds / alias / cf
};

// Pure host arithmetic; 0, or 1 with the error text set (unsupported variant, activation or pooled request, a node that
// fits no form).  Reads JH_NODE_ROWS (0: the tile form everywhere) once per process.
int choose_node(const NodeUse& u, NodeChoice* out);
// "tile", "rows_wave", "rows_pairs", "rows_wg"
std::string node_choice_name(const NodeChoice& c);

// `a` as the kernels read it (a.y_pool given exactly when c.pool); blds / alias / cf are taken from the choice.
int launch_bifpn_node(const NodeArgs& a, const NodeChoice& c, hipStream_t s);

// Each form's launcher and launch geometry, next to its kernel templates.
struct NodeKernelGeo { int block; size_t lds; int items; };   // items: (strip, segment) items per workgroup
NodeKernelGeo bifpn_rows_geo(int Cp);         // csrc/bifpn_rows.hip
NodeKernelGeo bifpn_rows_ps_geo(int Cp);      // csrc/bifpn_rows_ps.hip
NodeKernelGeo bifpn_rows_wg_geo(int Cp);      // csrc/bifpn_rows_wg.hip
int launch_bifpn_rows(const NodeArgs& a, const NodeChoice& c, hipStream_t s);
int launch_bifpn_rows_ps(const NodeArgs& a, const NodeChoice& c, hipStream_t s);
int launch_bifpn_rows_wg(const NodeArgs& a, const NodeChoice& c, hipStream_t s);

#if defined(__HIPCC__)
// Launch of one kernel instantiation with the choice's grid, block and dynamic LDS; the first launch of an
// instantiation that needs more than 64 KB raises its limit.
template <auto Kern, typename... Args>
int launch_node_kernel(const NodeChoice& c, hipStream_t s, const Args&... args) {
  static bool big = false;
  if (c.lds > 64 * 1024 && !big) {
    JH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     160 * 1024));
    big = true;
  }
  hipLaunchKernelGGL(Kern, c.grid, c.block, c.lds, s, args...);
  JH_CHECK_HIP(hipGetLastError());
  return 0;
}
#endif

}  // namespace jh
