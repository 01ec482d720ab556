// One convolution layer: which kernel form runs it, how its weights are packed, and its launch.
//
// Every caller that runs a (transposed) convolution -- the network plans (Plan::add_conv) and the single-operator
// entry points (jh_op_conv, jh_op_conv_operand) -- describes how the layer is used (ConvUse), makes a ConvLayer from
// that and launches it.  The rules that map a use to a kernel form live in choose_conv() and nowhere else.
#pragma once
#include <string>
#include <vector>
#include "jh_common.h"

namespace jh {

enum class ConvForm {
  Mfma,            // fp32 MFMA implicit GEMM (conv_mfma.h, deconv4.hip, conv_pw_direct.hip), weights in a WeightLayout
  Wino,            // 3x3x3 stride 1: Winograd F(2x2,3x3) x direct z (conv3d_wino.hip, conv3d_wino_pw.hip)
  WinoBf16x3,      // ... the same layers on the bf16 matrix cores with split operands (conv3d_bf16x3.hip)
  ConvBf16x3,      // dense k x k convolutions with the generic split-bf16 kernel (conv_bf16x3.h)
  Deconv4Bf16x3,   // the keypoint head's ConvTranspose2d k4 s2 p1, split bf16 (deconv4_bf16x3.hip)
  DeconvC1,        // ConvTranspose2d k4 s2 p1 with one output channel on the vector ALUs (deconv_c1.hip)
};

enum class ConvGate { None = 0, Tensor = 1, Recipe = 2 };   // multiplicative gate on the input: (N, cin_p) tensor / SeGate

// How a layer is used: everything the rules of choose_conv() read.
struct ConvUse {
  ConvDesc desc;                  // (its latency_class is that of the layer's launches)
  bool transposed = false;        // weights in ConvTranspose layout (cin, cout, k..)
  bool has_bias = false;
  bool want_stats = false;        // the launches accumulate the fused InstanceNorm statistics of the output
  ConvGate gate = ConvGate::None;
  int precision = 0;              // 0 fp32, 1 bf16x3, 2 bf16x3_wide (include/jarvis_hip.h)
  int in_px = 0;                  // floats per input pixel in memory (Act::Cp); 0: cpad(cin)
};

struct ConvChoice {
  ConvForm form = ConvForm::Mfma;
  WeightLayout layout = WeightLayout::Plain;   // of the Mfma form
  int wino_variant = 0;                        // of the Wino form: 4 persistent, 0 one role per workgroup
};
// Pure host arithmetic.  Reads JH_WINO, JH_WINO_PW and JH_DECONV4_WINDOW afresh at every call: a process may make layers
// of either form.
ConvChoice choose_conv(const ConvUse& u);
// "mfma" + "" / "_paired" / "_tappair" / "_window", "wino", "wino_bf16x3", "conv_bf16x3", "deconv4_bf16x3", "deconv_c1"
std::string conv_choice_name(const ConvChoice& c);

// THE HEAD'S BOX.  A layer whose output has one reader that reads part of it may be given that part as a
// per-image box (ConvArgs::box).  The two rules are here and nowhere else:
//  * which layers can use a box: the window form of ConvTranspose2d k4 s2 p1 -- the four-parity kernel and the general
//    path keep computing everything;
//  * which calls of a 3D predictor may give its keypoint head one: those in which the voxel gather of the same call is
//    the ONLY reader of the heat maps (head_box_allowed: anything else that reads them keeps the full map).
// JH_HEAD_ROI=0, read when the plan is built (EffTrackPlan::build), gives no layer a box: the previous dispatch.
bool conv_takes_box(const ConvChoice& c);
bool head_roi_knob();        // JH_HEAD_ROI as it stands now (unset: on)
// The call forms of a 3D predictor.  Forward: the whole-path forward, launched by the predictor itself (plain
// launches or its own graph; camera mask, given joint mask, caller-supplied centres and centre keyframes included).
// Staged: jh_predictor_stage_keypoints*, whose heat maps are the caller's (heat_dev, the exchange of the
// camera-sharded path).  Hybridnet: jh_predictor_hybridnet_forward, which can export them.  Captured: a whole-path
// forward on a stream the CALLER is capturing -- its launches run again at every replay, without the predictor's
// host code, which then cannot know that its own heat maps are complete only inside the boxes (jh_predictor::
// heat_boxed): no box.
enum class HeatCall { Forward = 0, Staged = 1, Hybridnet = 2, Captured = 3 };
// Only the plain Forward, and not with the joint-mask consensus in force (it scans whole heat maps), on a
// camera-sharded predictor (the heat maps leave the rank) or in a plan built with want_res1.
bool head_box_allowed(HeatCall kind, bool consensus, bool sharded, bool want_res1);

// [channels][taps] -> [taps][Cp], pad channels zero: the weight order of the vector-ALU kernels (depthwise, deconv_c1)
std::vector<float> taps_major(const float* w, int channels, int taps, int Cp);

// Owns the layer's device memory: packed weights, bias, and the Winograd tile table of its output volume.
struct ConvLayer {
  ConvLayer() = default;
  ConvLayer(const ConvLayer&) = delete;
  ConvLayer& operator=(const ConvLayer&) = delete;
  ~ConvLayer();

  ConvChoice choice;
  ConvDesc desc{};
  ConvWeights w;                   // DeconvC1: w.w is the [16 taps][in_px] tap-major table
  int* wino_tiles = nullptr;       // wino_tables() of the output volume (Wino form, volumes with remainder strips)
  size_t table_bytes = 0;

  // gate / se: only the Mfma form takes one.  stats: nullptr or the layer's fused statistics.
  // box: ConvArgs::box, only for a layer that takes_box()
  int launch(const Act& x, const Act& y, const float* gate, double* stats, const InNorm& in, const SeGate* se,
             hipStream_t s, const int4* box = nullptr) const;
  bool takes_box() const { return conv_takes_box(choice); }
  std::string profile_name(int out_w) const;
  // weights and tile table (the bias vector, cout_p16 floats, is not counted)
  size_t device_bytes() const { return w.phase_stride * desc.nphase * sizeof(float) + table_bytes; }
};

// w_host / b_host: torch layout (b_host given exactly when u.has_bias); D, H, W: extent of the output.
int make_conv_layer(const ConvUse& u, const float* w_host, const float* b_host, int D, int H, int W, ConvLayer* out);

}  // namespace jh
