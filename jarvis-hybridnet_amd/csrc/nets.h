// Launch plans of the two networks on the hot path.
//
// A plan is built once per (weights, input shape): activations are allocated,
// weights are repacked into MFMA operand order, and the forward pass becomes a
// flat list of kernel launches on one stream with no host synchronisation and
// no allocation, so a caller may capture it into a hipGraph.
#pragma once
#include <deque>
#include <functional>
#include <map>
#include <string>
#include <vector>
#include "jh_common.h"
#include "conv_layer.h"
#include "node_layer.h"
#include "preprocess.h"

namespace jh {

typedef std::map<std::string, std::vector<float>> ParamMap;

// Common machinery: owned device buffers, a zero-initialised scratch arena for
// InstanceNorm statistics / SE pools, and the recorded launch list.
class Plan {
 public:
  ~Plan();
  int run(hipStream_t s);
  size_t launches() const { return ops_.size(); }
  size_t device_bytes() const { return bytes_; }
  // Precision of the convolutions this plan builds (0 fp32, 1 bf16x3, 2 bf16x3_wide; include/jarvis_hip.h):
  // the process default (jh_set_precision / JH_PRECISION) at construction; an owner with its own setting
  // (jh_predictor_config::precision) overrides it before build().
  int precision = precision_mode();
  // Least tensor bytes per workgroup of the InstanceNorm / pooled-sum passes (launch_norm_apply): part of the pooled
  // sums' arithmetic, so -- like the BiFPN nodes' form -- a function of the predictor's time-batch class only (64 KB
  // for time batches >= 8, 0 = small blocks for single frame sets); set before build().
  int norm_block_kb = 0;

 protected:
  int alloc(void** p, size_t bytes);
  int new_act(int N, int D, int H, int W, int C, Act* out);
  size_t scratch(size_t doubles);           // offset into the zeroed arena
  int finish();                             // allocate the arena
  double* sc(size_t off) const { return arena_ + off; }
  int upload(const std::vector<float>& host, float** dev);
  int get(const ParamMap& pm, const std::string& key, size_t numel, const float** out);

  struct Op { std::function<int(hipStream_t)> fn; std::string name; double flops, bytes; };
  std::vector<Op> ops_;
  void push(const std::string& name, double flops, double bytes, std::function<int(hipStream_t)> fn) {
    ops_.push_back(Op{std::move(fn), name, flops, bytes});
  }
  std::vector<void*> owned_;
  std::deque<ConvLayer> layers_;            // the convolution layers (add_conv); a deque: the ops hold pointers
  std::vector<ConvWeights> convs_;          // pointwise weights of the fused BiFPN nodes
  double* arena_ = nullptr;
  size_t arena_doubles_ = 0;
  size_t bytes_ = 0;

  // building blocks shared by both networks
  int add_conv(const ParamMap& pm, const ConvDesc& d, const std::string& wkey,
               const std::string& bkey, bool transposed, const Act& x, const Act& y,
               const float* gate, bool want_stats, size_t* stats_off, long in_stats_off = -1,
               float in_inv = 0.f, int in_act = 0, const SeGate* se = nullptr, long se_pool_off = -1,
               const int4* const* box_cell = nullptr);   // box_cell: where every launch reads its ConvArgs::box from
  void add_norm(const Act& x, size_t stats_off, int act, const float* r1, const float* r2,
                float* y, long pool_off, long r1_stats_off = -1);
};

// A tensor as consumers see it: the raw conv output plus the statistics the
// InstanceNorm that follows it needs (st < 0: already normalised / no norm).
struct Ref {
  Act a;
  long st = -1;
  float inv = 0.f;       // 1 / pixels the statistics were accumulated over
  int act = 0;           // activation that follows that InstanceNorm (ACT_*)
};

class EffTrackPlan : public Plan {
 public:
  // size: 0 small, 1 medium, 2 large.  N images of H x W (multiples of 64).
  // want_res1: also compute res1 = final_conv1(first_conv(..)) (model.py:128), which the
  // inference path never reads (hybridnet/model.py:57-58, jarvis3D.py:147)
  int build(const ParamMap& pm, const std::string& prefix, int size, int J, int N, int H, int W,
            bool want_res1 = false);
  // Pre-processing fused into the stem convolution (small model's vector-ALU stem only): when
  // stem_fusable, a caller may set stem_src.mode to 1 (resize) / 2 (crop) before run(); `input` is then
  // never read.  mode 0 (default): the stem reads `input`.
  bool stem_fusable = false;
  StemSource stem_src;
  // algorithmic bytes of the (fused) stem launch for the profiler: taps read from the frames + stem output
  void set_stem_traffic(double bytes);
  int stem_channels() const { return stem_ch_; }
  // The time-batch class that choose_node() (csrc/node_layer.h) reads for every BiFPN node of this plan, set before
  // build().  A predictor sets it from its time batch ALONE (not from the number of cameras it owns), so that a
  // camera-sharded rank and the single-GPU run of the same time batch launch the same kernels and stay bit-equal
  // (SURVEY 8e); ByLaunchSize: by the number of workgroups of the launch, as the stand-alone operator does.
  NodeBatchClass node_class = NodeBatchClass::ByLaunchSize;
  Act input;     // [N][H][W][8]   normalised image, channel-last
  Act heat;      // [N][H/2][W/2][Jp]  res2 (ConvTranspose output)
  Act res1;      // [N][H/4][W/4][Jp]  final_conv1 output (only with want_res1)
  int J = 0;
  int stem_op_ = -1, stem_ch_ = 16;
  // The head's box (conv_layer.h has the rules).  head_takes_box: the head is a layer that can use one and
  // JH_HEAD_ROI was not 0 when the plan was built.  head_box: [N] boxes in device memory that the NEXT run()'s head
  // launch reads (ConvArgs::box), or nullptr = the full map; a caller sets it before run(), as it sets stem_src.
  bool head_takes_box = false;
  const int4* head_box = nullptr;
  // The head's launch alone, without a box, on the operand the last run() left: completes a boxed heat map to exactly
  // what a box-less run() writes.
  int run_head(hipStream_t s);

 private:
  int mbconv(const ParamMap& pm, const std::string& p, int stage, int k, int stride, int cin,
             int cout, int expand, Ref* x, Ref* out);
  void materialise(Ref* x);
  int lateral(const ParamMap& pm, const std::string& p, int cout, const Ref& x, Ref* out);
  int pool(const Ref& x, Ref* out);
  int node(const ParamMap& pm, const std::string& conv_prefix, int n_in, const Ref* ins,
           const int* modes, const float* w, int act, const Act& like, int cout, Ref* out,
           Ref* pooled = nullptr);   // pooled: also MaxPool2d(2,2) of the raw output, if NodeChoice::pool (else a.p = 0)
};

class V2VPlan : public Plan {
 public:
  int build(const ParamMap& pm, const std::string& prefix, int J, int T, int G);
  Act input;     // [T][G][G][G][Jp]   reprojected volume / 255
  Act output;    // [T][G/2]^3[Jp]

 private:
  // x_stats >= 0: x is a raw conv output whose InstanceNorm + ReLU the block applies on load
  // raw_stats != nullptr: the block stops behind its second convolution -- *out is that convolution's raw output,
  // *raw_stats its statistics -- and the reader applies the closing relu(IN(out) + x) on load (the output fold)
  int res_block(const ParamMap& pm, const std::string& p, int c, const Act& x, const float* extra,
                Act* out, long x_stats = -1, size_t* raw_stats = nullptr);
};

}  // namespace jh
