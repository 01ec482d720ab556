// Plan builders: EfficientTrack 2D network and V2V 3D network.
//
// Architecture restated from the reference (cited per function); the weights
// are consumed under the reference's own state-dict keys.
#include <cmath>
#include <cstring>
#include <cstdlib>
#include "nets.h"
#include "bifpn_node.h"

namespace jh {

// -------------------------------------------------------------------- Profiler
Profiler& profiler() {
  static Profiler p;
  return p;
}
void Profiler::begin(const std::string& name, double flops, double bytes, hipStream_t s) {
  ProfRec r{name, flops, bytes, nullptr, nullptr, 0.f};
  (void)hipEventCreate(&r.e0);
  (void)hipEventCreate(&r.e1);
  (void)hipEventRecord(r.e0, s);
  recs.push_back(r);
}
void Profiler::end(hipStream_t s) { (void)hipEventRecord(recs.back().e1, s); }
int Profiler::finish() {
  JH_CHECK_HIP(hipDeviceSynchronize());
  for (auto& r : recs) {
    if (!r.e0) continue;
    JH_CHECK_HIP(hipEventElapsedTime(&r.ms, r.e0, r.e1));
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
    r.e0 = r.e1 = nullptr;
  }
  return 0;
}

// ------------------------------------------------------------------------ Plan
Plan::~Plan() {
  for (void* p : owned_) (void)hipFree(p);
  for (auto& c : convs_) free_conv_weights(&c);
}

int Plan::alloc(void** p, size_t bytes) {
  JH_CHECK_HIP(hipMalloc(p, bytes));
  owned_.push_back(*p);
  bytes_ += bytes;
  return 0;
}

int Plan::new_act(int N, int D, int H, int W, int C, Act* out) {
  out->N = N; out->D = D; out->H = H; out->W = W; out->C = C; out->Cp = cpad(C);
  if (alloc(reinterpret_cast<void**>(&out->p), out->bytes())) return 1;
  // pad channels must hold zeros from the start
  JH_CHECK_HIP(hipMemset(out->p, 0, out->bytes()));
  return 0;
}

size_t Plan::scratch(size_t doubles) {
  const size_t off = arena_doubles_;
  arena_doubles_ += (doubles + 7) / 8 * 8;
  return off;
}

int Plan::finish() {
  if (arena_doubles_ == 0) arena_doubles_ = 8;
  return alloc(reinterpret_cast<void**>(&arena_), arena_doubles_ * sizeof(double));
}

static int g_precision = [] {
  const char* e = getenv("JH_PRECISION");
  if (!e) return 0;
  return std::string(e) == "bf16x3" ? 1 : (std::string(e) == "bf16x3_wide" ? 2 : 0);
}();
int precision_mode() { return g_precision; }
void set_precision_mode(int m) { g_precision = m; }

int Plan::run(hipStream_t s) {
  if (launch_zero(arena_, arena_doubles_ * sizeof(double), s)) return 1;
  Profiler& pf = profiler();
  for (auto& op : ops_) {
    if (pf.on) pf.begin(op.name, op.flops, op.bytes, s);
    if (op.fn(s)) return 1;
    if (pf.on) pf.end(s);
  }
  return 0;
}

int Plan::upload(const std::vector<float>& host, float** dev) {
  if (alloc(reinterpret_cast<void**>(dev), host.size() * sizeof(float))) return 1;
  JH_CHECK_HIP(hipMemcpy(*dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}

int Plan::get(const ParamMap& pm, const std::string& key, size_t numel, const float** out) {
  auto it = pm.find(key);
  JH_REQUIRE(it != pm.end(), "missing parameter " + key);
  JH_REQUIRE(it->second.size() == numel, "wrong element count for parameter " + key);
  *out = it->second.data();
  return 0;
}

int Plan::add_conv(const ParamMap& pm, const ConvDesc& d, const std::string& wkey,
                   const std::string& bkey, bool transposed, const Act& x, const Act& y,
                   const float* gate, bool want_stats, size_t* stats_off, long in_stats_off,
                   float in_inv, int in_act, const SeGate* se, long se_pool_off, const int4* const* box_cell) {
  size_t taps;
  if (d.ostride > 1) taps = (d.nd == 2) ? 16 : 8;
  else taps = (size_t)d.k * d.k * (d.nd == 3 ? d.k : 1);
  const float *w = nullptr, *b = nullptr;
  if (get(pm, wkey, (size_t)d.cin * d.cout * taps, &w)) return 1;
  if (!bkey.empty() && get(pm, bkey, d.cout, &b)) return 1;
  // which kernel form runs the layer, and in which weight layout: choose_conv (csrc/conv_layer.hip)
  ConvUse use;
  use.desc = d; use.desc.latency_class = norm_block_kb == 0 ? 1 : 0;   // (the plan's time-batch class, set before build())
  use.transposed = transposed; use.has_bias = b != nullptr; use.want_stats = want_stats;
  use.gate = se ? ConvGate::Recipe : (gate ? ConvGate::Tensor : ConvGate::None);
  use.precision = precision;
  use.in_px = x.Cp;
  layers_.emplace_back();
  const ConvLayer* layer = &layers_.back();
  if (make_conv_layer(use, w, b, y.D, y.H, y.W, &layers_.back())) return 1;
  bytes_ += layer->device_bytes();
  size_t off = 0;
  if (want_stats) {
    off = scratch((size_t)y.N * y.Cp * kStatW);
    if (stats_off) *stats_off = off;
  }
  // algorithmic work: 2*MAC over the real (unpadded) channels; bytes = one read of
  // the input, one write of the output, one read of the weights
  const double opix = (double)y.N * y.pixels();
  const double taps_per_out = (d.ostride > 1) ? (double)taps / d.nphase : (double)taps;
  const double flops = 2.0 * opix * d.cin * d.cout * taps_per_out;
  // (the one-channel vector-ALU kernel keeps its weights in registers and stores whole padded pixels)
  const double bytes = layer->choice.form == ConvForm::DeconvC1
      ? 4.0 * x.N * (x.pixels() * d.cin + (double)y.pixels() * y.Cp)
      : 4.0 * ((double)x.N * x.pixels() * d.cin + opix * d.cout + (double)d.cin * d.cout * taps);
  push(layer->profile_name(y.W), flops, bytes,
       [this, layer, x, y, gate, want_stats, off, in_stats_off, in_inv, in_act, sev = se ? *se : SeGate(),
        se_pool_off, box_cell](hipStream_t s) {
    InNorm in;
    if (in_stats_off >= 0) { in.stats = sc((size_t)in_stats_off); in.inv = in_inv; in.act = in_act; }
    SeGate seg = sev;
    if (se_pool_off >= 0) seg.pool = sc((size_t)se_pool_off);
    return layer->launch(x, y, gate, want_stats ? sc(off) : nullptr, in, se_pool_off >= 0 ? &seg : nullptr, s,
                         box_cell ? *box_cell : nullptr);
  });
  return 0;
}

void Plan::add_norm(const Act& x, size_t stats_off, int act, const float* r1, const float* r2,
                    float* y, long pool_off, long r1_stats_off) {
  const double el = (double)x.N * x.pixels() * x.C;
  // (bytes: one read of x and of each residual operand, one write of y -- none for the pooled-sums-only form)
  push("norm_apply", 8.0 * el, 4.0 * el * (1 + (y ? 1 : 0) + (r1 ? 1 : 0) + (r2 ? 1 : 0)),
       [this, x, stats_off, act, r1, r2, y, pool_off, r1_stats_off](hipStream_t s) {
    return launch_norm_apply(x, sc(stats_off), act, r1, r2, y,
                             pool_off >= 0 ? sc((size_t)pool_off) : nullptr, s,
                             r1_stats_off >= 0 ? sc((size_t)r1_stats_off) : nullptr, norm_block_kb);
  });
}

// ---------------------------------------------------------------- EfficientTrack
namespace {
struct SizeSpec { double width, depth; int fpn, cells, head; };
// jarvis/efficienttrack/model.py:34-51, utils.py:152-155
const SizeSpec kSizes[3] = {{0.5, 0.5, 56, 3, 64}, {1.0, 1.0, 88, 4, 88}, {1.1, 1.2, 160, 6, 160}};
// jarvis/efficienttrack/utils.py:267-272: kernel, repeats, in, out, expand, stride
const int kStages[7][6] = {{3, 1, 32, 16, 1, 1}, {3, 2, 16, 24, 6, 2}, {5, 2, 24, 40, 6, 2},
                           {3, 3, 40, 80, 6, 2}, {5, 3, 80, 112, 6, 1}, {5, 4, 112, 192, 6, 2},
                           {3, 1, 192, 320, 6, 1}};
struct Block { int stage, k, stride, cin, cout, expand; };

int scale_ch(int c, double width) {       // utils.py:76-96 (divisor 8)
  const double f = c * width;
  int o = std::max(8, (int)(f + 4) / 8 * 8);
  if (o < 0.9 * f) o += 8;
  return o;
}

// trunk after the cut behind the last stride-16 block; taps before the 2nd..4th
// stride-2 block (efficientnet.py:156-173, model.py:515-533)
void trunk(int size, int* stem, std::vector<Block>* blocks, int taps[3]) {
  const SizeSpec& s = kSizes[size];
  std::vector<Block> all;
  for (int st = 0; st < 7; ++st) {
    const int cin = scale_ch(kStages[st][2], s.width), cout = scale_ch(kStages[st][3], s.width);
    const int rep = (int)std::ceil(s.depth * kStages[st][1]);
    for (int r = 0; r < rep; ++r)
      all.push_back({st, kStages[st][0], r == 0 ? kStages[st][5] : 1, r == 0 ? cin : cout, cout,
                     kStages[st][4]});
  }
  int seen = 0, nt = 0;
  for (size_t i = 0; i < all.size() && nt < 3; ++i)
    if (all[i].stride == 2 && seen++ >= 1) taps[nt++] = (int)i - 1;
  blocks->assign(all.begin(), all.begin() + taps[2] + 1);
  *stem = scale_ch(32, s.width);
}

// relu(p) / (sum + eps), model.py:309-311 (float arithmetic like the reference)
void fuse_weights(const float* p, int n, float* w) {
  float r[3], sum = 0.f;
  for (int i = 0; i < n; ++i) { r[i] = p[i] > 0.f ? p[i] : 0.f; sum += r[i]; }
  for (int i = 0; i < n; ++i) w[i] = r[i] / (sum + 1e-4f);
}
}  // namespace

// MBConvBlock.forward, efficientnet.py:90-123
// Write IN(+act) of a "raw + statistics" tensor in place, for consumers that cannot apply
// it on load (depthwise kernels, residual adds).
void EffTrackPlan::materialise(Ref* x) {
  if (x->st < 0) return;
  add_norm(x->a, (size_t)x->st, x->act, nullptr, nullptr, x->a.p, -1);
  x->st = -1;
}

// The input may still be "raw + statistics" (stem, or a block without a skip connection):
// the block's first dense conv then applies that InstanceNorm(+act) while it stages its
// operand.  The output is returned the same way when the block has no skip connection.
int EffTrackPlan::mbconv(const ParamMap& pm, const std::string& p, int stage, int k, int stride,
                         int cin, int cout, int expand, Ref* xin, Ref* outr) {
  const bool skip = (stride == 1 && cin == cout);
  // (in place: the caller's Ref is updated so that later readers of the same tensor,
  // e.g. the BiFPN laterals, do not normalise it a second time)
  if (skip || (stage >= 4 && expand == 1)) materialise(xin);
  const Ref xr = *xin;
  const Act& x = xr.a;
  Act* out = &outr->a;
  const int mid = cin * expand;
  const int squeeze = std::max(1, (int)(cin * 0.25));
  const int Ho = (x.H + 2 * (k / 2) - k) / stride + 1, Wo = (x.W + 2 * (k / 2) - k) / stride + 1;
  Act raw;
  if (new_act(x.N, 1, Ho, Wo, mid, &raw)) return 1;
  size_t st1 = 0;
  // squeeze-excite pooled sums: [N][Cp][kLimbs].  Depthwise blocks whose image is one 16 x 16 tile get them from
  // the depthwise launch itself (the workgroup owns the whole image of its channels); everything else from a
  // pooled-sums-only pass over the raw tensor.
  const size_t pool = scratch((size_t)raw.N * raw.Cp * kLimbs);
  bool pooled = false;
  if (stage < 4) {
    // "fused" path: one dense k x k conv; _expand_conv is never executed
    if (add_conv(pm, conv_desc(2, k, stride, k / 2, cin, mid), p + "_depthwise_conv.weight", "",
                 false, x, raw, nullptr, true, &st1, xr.st, xr.inv, xr.act)) return 1;
  } else {
    Act e = x;
    if (expand != 1) {
      if (new_act(x.N, 1, x.H, x.W, mid, &e)) return 1;
      if (add_conv(pm, conv_desc(2, 1, 1, 0, cin, mid), p + "_expand_conv.weight", "", false, x, e,
                   nullptr, false, nullptr, xr.st, xr.inv, xr.act)) return 1;
    }
    JH_REQUIRE(stride == 1, "depthwise stages are stride 1");
    const float* w = nullptr;
    if (get(pm, p + "_depthwise_conv.weight", (size_t)mid * k * k, &w)) return 1;
    float* wd = nullptr;
    if (upload(taps_major(w, mid, k * k, raw.Cp), &wd)) return 1;
    st1 = scratch((size_t)raw.N * raw.Cp * kStatW);
    pooled = depthwise_can_pool(Ho, Wo);
    push(std::string("depthwise_k") + std::to_string(k) + (pooled ? "pool" : ""), 2.0 * raw.N * raw.pixels() * mid * k * k,
         8.0 * raw.N * raw.pixels() * mid, [this, e, wd, k, raw, st1, pool, pooled](hipStream_t s) {
      return launch_depthwise(e, wd, k, raw.p, sc(st1), s, pooled ? sc(pool) : nullptr);
    });
  }
  // _gn1 + swish: only its per-(n,c) pooled sums (squeeze-excite) are computed here; the
  // normalised tensor itself is never written -- the project conv re-applies
  // InstanceNorm + SiLU (+ the SE gate) while it stages its operand
  if (!pooled) add_norm(raw, st1, ACT_SILU, nullptr, nullptr, nullptr, (long)pool);
  // squeeze-excite gate
  const float *wr, *br, *we, *be;
  if (get(pm, p + "_se_reduce.weight", (size_t)squeeze * mid, &wr)) return 1;
  if (get(pm, p + "_se_reduce.bias", squeeze, &br)) return 1;
  if (get(pm, p + "_se_expand.weight", (size_t)mid * squeeze, &we)) return 1;
  if (get(pm, p + "_se_expand.bias", mid, &be)) return 1;
  float *dwr, *dbr, *dwe, *dbe, *gate = nullptr;
  if (upload(std::vector<float>(wr, wr + (size_t)squeeze * mid), &dwr)) return 1;
  if (upload(std::vector<float>(br, br + squeeze), &dbr)) return 1;
  if (upload(std::vector<float>(we, we + (size_t)mid * squeeze), &dwe)) return 1;
  if (upload(std::vector<float>(be, be + mid), &dbe)) return 1;
  const float inv_hw = 1.f / (float)(Ho * Wo);
  // Small batches (the single-frame-set call: 12 images, launch-latency-bound): the gate -- two tiny fully
  // connected layers per image -- is computed by the project convolution's own prologue from the pooled
  // sums, with the arithmetic of se_gate_kernel, bit for bit: 14 launches less per forward.  At bench
  // scale the serial prologue in every project-conv workgroup costs more than the launches (1950-1969
  // against 1973-1985 frames/s), so large batches keep the stand-alone se_gate launch.
  const bool se_fused = raw.N <= 32;
  SeGate seg;
  seg.wr = dwr; seg.br = dbr; seg.we = dwe; seg.be = dbe; seg.C = mid; seg.S = squeeze; seg.inv_hw = inv_hw;
  if (!se_fused) {
    if (alloc(reinterpret_cast<void**>(&gate), (size_t)raw.N * raw.Cp * sizeof(float))) return 1;
    push("se_gate", 4.0 * raw.N * mid * squeeze, 8.0 * raw.N * mid,
         [this, pool, raw, mid, squeeze, inv_hw, dwr, dbr, dwe, dbe, gate](hipStream_t s) {
      return launch_se_gate(sc(pool), raw.N, mid, raw.Cp, squeeze, inv_hw, dwr, dbr, dwe, dbe, gate, s);
    });
  }
  // project (gate applied while staging the operand) + _gn2 (+ skip)
  if (new_act(x.N, 1, Ho, Wo, cout, out)) return 1;
  size_t st2 = 0;
  if (add_conv(pm, conv_desc(2, 1, 1, 0, mid, cout), p + "_project_conv.weight", "", false, raw,
               *out, gate, true, &st2, (long)st1, 1.f / (float)(Ho * Wo), ACT_SILU,
               se_fused ? &seg : nullptr, se_fused ? (long)pool : -1)) return 1;
  if (skip) {
    add_norm(*out, st2, ACT_NONE, x.p, nullptr, out->p, -1);
    outr->st = -1;
  } else {                                  // _gn2 is applied by the consumers on load
    outr->st = (long)st2;
    outr->inv = 1.f / (float)(Ho * Wo);
    outr->act = ACT_NONE;
  }
  return 0;
}

// 1x1 conv + bias; its InstanceNorm (model.py:404-425) is applied by the consumers
// from the fused statistics
int EffTrackPlan::lateral(const ParamMap& pm, const std::string& p, int cout, const Ref& xr,
                          Ref* out) {
  const Act& x = xr.a;
  if (new_act(x.N, 1, x.H, x.W, cout, &out->a)) return 1;
  size_t st = 0;
  if (add_conv(pm, conv_desc(2, 1, 1, 0, x.C, cout), p + ".0.weight", p + ".0.bias", false, x,
               out->a, nullptr, true, &st, xr.st, xr.inv, xr.act)) return 1;
  out->st = (long)st;
  out->inv = 1.f / (float)(x.H * x.W);
  return 0;
}

// MaxPool2d(2,2) of a not-yet-normalised tensor: max commutes with the (monotone)
// InstanceNorm map, so the pooled raw tensor keeps the producer's statistics.
int EffTrackPlan::pool(const Ref& x, Ref* out) {
  if (new_act(x.a.N, 1, x.a.H / 2, x.a.W / 2, x.a.C, &out->a)) return 1;
  out->st = x.st;
  out->inv = x.inv;
  const Act a = x.a, o = out->a;
  push("maxpool2", 0, 5.0 * o.N * o.pixels() * o.C * 4,
       [a, o](hipStream_t s) { return launch_maxpool2(a, o.p, s); });
  return 0;
}

// One fused BiFPN node (csrc/bifpn_node.hip): weighted fusion of normalised inputs
// + activation + SeparableConvBlock (depthwise 3x3, pointwise 1x1 + bias); the
// block's InstanceNorm is again left to the consumers.
int EffTrackPlan::node(const ParamMap& pm, const std::string& cp, int n_in, const Ref* ins,
                       const int* modes, const float* w, int act, const Act& like, int cout,
                       Ref* out, Ref* pooled) {
  const int cin = like.C;
  const float* dwh = nullptr;
  if (get(pm, cp + "depthwise_conv.weight", (size_t)cin * 9, &dwh)) return 1;
  float* dwd = nullptr;
  if (upload(taps_major(dwh, cin, 9, like.Cp), &dwd)) return 1;
  const float *pwh = nullptr, *bh = nullptr;
  if (get(pm, cp + "pointwise_conv.weight", (size_t)cin * cout, &pwh)) return 1;
  if (get(pm, cp + "pointwise_conv.bias", cout, &bh)) return 1;
  ConvWeights cw;
  if (pack_conv_weights(conv_desc(2, 1, 1, 0, cin, cout), pwh, bh, false, WeightLayout::Plain, &cw)) return 1;
  convs_.push_back(cw);
  if (new_act(like.N, 1, like.H, like.W, cout, &out->a)) return 1;
  const size_t st = scratch((size_t)like.N * out->a.Cp * kStatW);
  out->st = (long)st;
  out->inv = 1.f / (float)(like.H * like.W);
  NodeArgs a{};
  a.n_in = n_in; a.act = act;
  long sts[3] = {-1, -1, -1};
  double bytes = 4.0 * like.N * like.pixels() * cout;
  for (int i = 0; i < n_in; ++i) {
    a.in[i] = ins[i].a.p; a.mode[i] = modes[i]; a.w[i] = w[i]; a.inv_cnt[i] = ins[i].inv;
    sts[i] = ins[i].st;
    bytes += 4.0 * ins[i].a.N * ins[i].a.pixels() * cin;
  }
  a.dw = dwd; a.pw = cw.w; a.bias = cw.bias; a.y = out->a.p;
  a.N = like.N; a.H = like.H; a.W = like.W; a.Cp = like.Cp;
  a.cout_p = out->a.Cp; a.cout_p16 = cw.cout_p16;
  // form, segmentation and launch shape: decided here, once (csrc/node_layer.hip)
  NodeChoice choice;
  if (choose_node(node_use(a, node_class, pooled != nullptr), &choice)) return 1;
  if (pooled) {
    // a row form can write the 2x2-max-pooled raw output on the side: the bottom-up node of the next level then reads
    // a same-resolution tensor with THIS node's statistics
    pooled->a = Act{};
    if (choice.pool) {
      if (new_act(like.N, 1, like.H / 2, like.W / 2, cout, &pooled->a)) return 1;
      pooled->st = (long)st; pooled->inv = out->inv; pooled->act = out->act;
      a.y_pool = pooled->a.p;
      bytes += 4.0 * like.N * pooled->a.pixels() * cout;
    }
  }
  const double px = (double)like.N * like.pixels();
  char nm[64];
  snprintf(nm, sizeof nm, "bifpn_node_%dx%d@%d", cin, cout, like.W);
  const long s0 = sts[0], s1 = sts[1], s2 = sts[2];
  push(nm, 2.0 * px * cin * (9.0 + cout), bytes, [this, a, choice, s0, s1, s2, st](hipStream_t s) {
    NodeArgs b = a;
    b.st[0] = s0 >= 0 ? sc((size_t)s0) : nullptr;
    b.st[1] = s1 >= 0 ? sc((size_t)s1) : nullptr;
    b.st[2] = s2 >= 0 ? sc((size_t)s2) : nullptr;
    b.stats = sc(st);
    return launch_bifpn_node(b, choice, s);
  });
  return 0;
}

void EffTrackPlan::set_stem_traffic(double bytes) {
  if (stem_op_ >= 0 && stem_op_ < (int)ops_.size()) ops_[stem_op_].bytes = bytes;
}

// EfficientTrackBackbone.forward, model.py:114-130 (res2 branch only: the
// final_conv1 branch is dead on the inference path, model.py:57-58 / jarvis3D.py:147)
int EffTrackPlan::build(const ParamMap& pm, const std::string& pre, int size, int joints, int N,
                        int H, int W, bool want_res1) {
  JH_REQUIRE(size >= 0 && size < 3, "model size");
  JH_REQUIRE(H % 64 == 0 && W % 64 == 0, "image side must be a multiple of 64");
  const SizeSpec& ss = kSizes[size];
  J = joints;
  int stem, taps[3];
  std::vector<Block> blocks;
  trunk(size, &stem, &blocks, taps);

  if (new_act(N, 1, H, W, 3, &input)) return 1;
  input.Cp = 4;          // one float4 per pixel; the stem conv zero-fills its K padding while staging
  // stem conv + IN + swish (efficientnet.py:150-152, model.py:536-538)
  Ref x;
  if (new_act(N, 1, H / 2, W / 2, stem, &x.a)) return 1;
  size_t st = 0;
  const std::string bb = pre + "backbone_net.model.";
  JH_REQUIRE(stem == 16 || stem == 32, "stem channels");
  // the 3 -> 16 (small) / 3 -> 32 (medium, large) stem runs on the vector ALUs (csrc/stem.hip): K = 27 is
  // too little matrix work per workgroup for the MFMA kernel, and the pre-processing fuses into it
  const float* wh = nullptr;
  if (get(pm, bb + "_conv_stem.weight", (size_t)stem * 27, &wh)) return 1;
  std::vector<float> packed(27 * stem);
  pack_stem_weights(wh, packed.data(), stem);
  float* wd = nullptr;
  if (upload(packed, &wd)) return 1;
  st = scratch((size_t)N * stem * kStatW);
  const Act xin = input, xo = x.a;
  const double opix = (double)N * xo.pixels();
  // (named by FAMILY: this layer runs on the vector ALUs and is HBM-bound on the frame rows it fetches; its
  //  algorithmic bytes depend on what feeds it -- set_stem_traffic() -- so bench.py prices it against HBM)
  stem_op_ = (int)ops_.size();
  stem_ch_ = stem;
  push("stem_conv_k3s2_3x" + std::to_string(stem) + "@" + std::to_string(xo.W), 2.0 * opix * 27 * stem,
       4.0 * ((double)N * xin.pixels() * 3 + opix * stem + 27 * stem),
       [this, xin, xo, wd, st](hipStream_t s) {
         if (stem_src.mode) return launch_stem_conv_src(stem_src, xin, wd, xo, sc(st), s);
         return launch_stem_conv(xin, wd, xo, sc(st), s);
       });
  // JH_STEM_FUSE=0: the stand-alone resize / crop kernels feed the stem instead (read at plan build time, so a
  // process may build plans of both forms)
  const char* fuse = getenv("JH_STEM_FUSE");
  stem_fusable = !(fuse && atoi(fuse) == 0);
  // the stem's InstanceNorm + swish is applied by the first block's conv on load
  x.st = (long)st;
  x.inv = 1.f / (float)((H / 2) * (W / 2));
  x.act = ACT_SILU;
  std::vector<Ref> outs(blocks.size() + 1);
  outs[0] = x;
  for (size_t i = 0; i < blocks.size(); ++i) {
    const Block& b = blocks[i];
    if (mbconv(pm, bb + "_blocks." + std::to_string(i) + ".", b.stage, b.k, b.stride, b.cin,
               b.cout, b.expand, &outs[i], &outs[i + 1])) return 1;
  }
  Ref feats[3];
  for (int f = 0; f < 3; ++f) {
    JH_REQUIRE(taps[f] >= 0 && taps[f] < (int)blocks.size(), "feature taps");
    feats[f] = outs[taps[f] + 1];
  }

  // BiFPN cells (model.py:301-353, 446-504).  Every tensor inside the pyramid is
  // kept as "raw conv output + statistics"; the fused node kernel normalises on load.
  const int Wf = ss.fpn;
  Ref p3, p4, p5, p6, p7;
  for (int cell = 0; cell < ss.cells; ++cell) {
    const std::string p = pre + "bifpn." + std::to_string(cell) + ".";
    Ref p3_in, p4_in, p5_in, p6_in, p7_in, p4_in2, p5_in2;
    if (cell == 0) {
      Ref t6;
      if (lateral(pm, p + "p5_to_p6", Wf, feats[2], &t6)) return 1;
      if (pool(t6, &p6_in)) return 1;
      if (pool(p6_in, &p7_in)) return 1;
      if (lateral(pm, p + "p3_down_channel", Wf, feats[0], &p3_in)) return 1;
      if (lateral(pm, p + "p4_down_channel", Wf, feats[1], &p4_in)) return 1;
      if (lateral(pm, p + "p5_down_channel", Wf, feats[2], &p5_in)) return 1;
      if (lateral(pm, p + "p4_down_channel_2", Wf, feats[1], &p4_in2)) return 1;
      if (lateral(pm, p + "p5_down_channel_2", Wf, feats[2], &p5_in2)) return 1;
    } else {
      p3_in = p3; p4_in = p4; p5_in = p5; p6_in = p6; p7_in = p7;
      p4_in2 = p4; p5_in2 = p5;
    }
    auto fnode = [&](const char* wname, int n_in, const Ref* ins, const int* modes, const Ref& like,
                     const char* conv, Ref* out, Ref* pooled = nullptr) -> int {
      const float* wp = nullptr;
      if (get(pm, p + wname, n_in, &wp)) return 1;
      float w[3];
      fuse_weights(wp, n_in, w);
      return node(pm, p + conv + ".", n_in, ins, modes, w, ACT_SILU, like.a, Wf, out, pooled);
    };
    const int m_up[2] = {FUSE_SAME, FUSE_UP2};
    const int m_dn3[3] = {FUSE_SAME, FUSE_SAME, FUSE_POOL2};
    const int m_dn2[2] = {FUSE_SAME, FUSE_POOL2};
    Ref p6_up, p5_up, p4_up, p3_out, p4_out, p5_out, p6_out, p7_out;
    { const Ref in[2] = {p6_in, p7_in}; if (fnode("p6_w1", 2, in, m_up, p6_in, "conv6_up", &p6_up)) return 1; }
    { const Ref in[2] = {p5_in, p6_up}; if (fnode("p5_w1", 2, in, m_up, p5_in, "conv5_up", &p5_up)) return 1; }
    { const Ref in[2] = {p4_in, p5_up}; if (fnode("p4_w1", 2, in, m_up, p4_in, "conv4_up", &p4_up)) return 1; }
    Ref p3_pool;
    { const Ref in[2] = {p3_in, p4_up}; if (fnode("p3_w1", 2, in, m_up, p3_in, "conv3_up", &p3_out, &p3_pool)) return 1; }
    const int m_same3[3] = {FUSE_SAME, FUSE_SAME, FUSE_SAME};
    Ref p4_pool;
    if (p3_pool.a.p) {          // (time batches: P3's node wrote its pooled output, all three inputs at P4's resolution)
      const Ref in[3] = {p4_in2, p4_up, p3_pool};
      if (fnode("p4_w2", 3, in, m_same3, p4_in2, "conv4_down", &p4_out, &p4_pool)) return 1;
    } else {
      const Ref in[3] = {p4_in2, p4_up, p3_out};
      if (fnode("p4_w2", 3, in, m_dn3, p4_in2, "conv4_down", &p4_out)) return 1;
    }
    // the head reads p3, p4, p5 of the last cell only: its p6 / p7 outputs are dead
    const bool more = cell + 1 < ss.cells;
    Ref p5_pool, p6_pool;
    if (p4_pool.a.p) {          // (wide pyramids: P4's bottom-up node wrote its pooled output too, and so on down)
      const Ref in[3] = {p5_in2, p5_up, p4_pool};
      if (fnode("p5_w2", 3, in, m_same3, p5_in2, "conv5_down", &p5_out, more ? &p5_pool : nullptr)) return 1;
    } else {
      const Ref in[3] = {p5_in2, p5_up, p4_out};
      if (fnode("p5_w2", 3, in, m_dn3, p5_in2, "conv5_down", &p5_out)) return 1;
    }
    if (more) {
      if (p5_pool.a.p) {
        const Ref in[3] = {p6_in, p6_up, p5_pool};
        if (fnode("p6_w2", 3, in, m_same3, p6_in, "conv6_down", &p6_out, &p6_pool)) return 1;
      } else {
        const Ref in[3] = {p6_in, p6_up, p5_out};
        if (fnode("p6_w2", 3, in, m_dn3, p6_in, "conv6_down", &p6_out)) return 1;
      }
      if (p6_pool.a.p) {
        const int m_same2[2] = {FUSE_SAME, FUSE_SAME};
        const Ref in[2] = {p7_in, p6_pool};
        if (fnode("p7_w2", 2, in, m_same2, p7_in, "conv7_down", &p7_out)) return 1;
      } else {
        const Ref in[2] = {p7_in, p6_out};
        if (fnode("p7_w2", 2, in, m_dn2, p7_in, "conv7_down", &p7_out)) return 1;
      }
    }
    p3 = p3_out; p4 = p4_out; p5 = p5_out; p6 = p6_out; p7 = p7_out;
  }

  // head: softplus-normalised 3-way fusion + first_conv as one fused node (model.py:119-127)
  const float* wc = nullptr;
  if (get(pm, pre + "weights_cat", 3, &wc)) return 1;
  float w[3], sum = 0.f;
  for (int i = 0; i < 3; ++i) { w[i] = wc[i] > 20.f ? wc[i] : log1pf(expf(wc[i])); sum += w[i]; }
  for (int i = 0; i < 3; ++i) w[i] = w[i] / (sum + 0.0001f);
  const Ref hin[3] = {p3, p4, p5};
  const int hmodes[3] = {FUSE_SAME, FUSE_UP2, FUSE_UP4};
  Ref mid;
  if (node(pm, pre + "first_conv.", 3, hin, hmodes, w, ACT_NONE, p3.a, ss.head, &mid)) return 1;
  // first_conv's InstanceNorm is applied by deconv1 while it stages its operand
  if (new_act(N, 1, mid.a.H * 2, mid.a.W * 2, J, &heat)) return 1;
  if (want_res1) {     // res1 = final_conv1(res1), model.py:128 (3x3, no bias, no norm)
    if (new_act(N, 1, mid.a.H, mid.a.W, J, &res1)) return 1;
    if (add_conv(pm, conv_desc(2, 3, 1, 1, ss.head, J), pre + "final_conv1.weight", "", false, mid.a,
                 res1, nullptr, false, nullptr, mid.st, mid.inv, ACT_NONE)) return 1;
  }
  // (J == 1, the CenterDetect head: the one-channel vector-ALU form)
  // (the head's launches read their box through head_box; JH_HEAD_ROI=0, read here: no box ever)
  if (add_conv(pm, deconv2d_k4s2p1_desc(ss.head, J), pre + "deconv1.weight", "", true, mid.a, heat,
               nullptr, false, nullptr, mid.st, mid.inv, ACT_NONE, nullptr, -1, &head_box)) return 1;
  head_takes_box = layers_.back().takes_box() && !want_res1 && head_roi_knob();
  return finish();
}

int EffTrackPlan::run_head(hipStream_t s) {
  const int4* const box = head_box;
  head_box = nullptr;
  Op& op = ops_.back();                         // (the head is the plan's last launch)
  Profiler& pf = profiler();
  if (pf.on) pf.begin(op.name, op.flops, op.bytes, s);
  const int rc = op.fn(s);
  head_box = box;
  if (rc) return 1;
  if (pf.on) pf.end(s);
  return 0;
}

// ------------------------------------------------------------------------- V2V
// Res3DBlock.forward, v2vnet.py:27-43: relu(IN(conv(relu(IN(conv(x))))) + x)
// `extra`, when set, is added after the final relu (the encoder/decoder skip sum).
int V2VPlan::res_block(const ParamMap& pm, const std::string& p, int c, const Act& x,
                       const float* extra, Act* out, long x_stats, size_t* raw_stats) {
  Act a;
  if (new_act(x.N, x.D, x.H, x.W, c, &a)) return 1;
  size_t s1 = 0, s2 = 0;
  const float inv = 1.f / (float)(x.D * x.H * x.W);
  if (add_conv(pm, conv_desc(3, 3, 1, 1, c, c), p + "res_branch.0.weight", p + "res_branch.0.bias",
               false, x, a, nullptr, true, &s1, x_stats, inv, ACT_RELU)) return 1;
  // the InstanceNorm + ReLU between the two convs is applied by the second conv on load
  if (new_act(x.N, x.D, x.H, x.W, c, out)) return 1;
  if (add_conv(pm, conv_desc(3, 3, 1, 1, c, c), p + "res_branch.3.weight", p + "res_branch.3.bias",
               false, a, *out, nullptr, true, &s2, (long)s1, 1.f / (float)(x.D * x.H * x.W),
               ACT_RELU)) return 1;
  if (raw_stats) { *raw_stats = s2; return 0; }     // closed by the reader (V2VPlan::build: the output fold)
  add_norm(*out, s2, ACT_RELU, x.p, extra, out->p, -1, x_stats);
  return 0;
}

// V2VNet.forward, v2vnet.py:98-102 with EncoderDecorder.forward :75-83 inlined
int V2VPlan::build(const ParamMap& pm, const std::string& pre, int J, int T, int G) {
  JH_REQUIRE(G % 4 == 0, "grid size must be a multiple of 4");
  const int Gh = G / 2, Gq = G / 4;
  if (new_act(T, G, G, G, J, &input)) return 1;
  Act f0, f1, skip, e0, e1, u0, d1;
  size_t st = 0;
  if (new_act(T, Gh, Gh, Gh, 2 * J, &f0)) return 1;
  if (add_conv(pm, conv_desc(3, 3, 2, 1, J, 2 * J), pre + "front_layers.0.block.0.weight",
               pre + "front_layers.0.block.0.bias", false, input, f0, nullptr, true, &st)) return 1;
  // The stage-entry tensors (f0, e0, u0) stay RAW: their InstanceNorm + ReLU is applied on load by the two
  // readers, the residual block's first convolution and its closing relu(IN(conv2) + x) pass
  // (rounds 1-2 materialised them with a pass of their own).
  if (res_block(pm, pre + "front_layers.1.", 2 * J, f0, nullptr, &f1, (long)st)) return 1;
  const std::string e = pre + "encoder_decoder.";
  // skip_res1 (three launches) depends on f1 only and is read again by decoder_res1's closing pass.  Running it as a
  // side branch on a second stream next to encoder_pool1 .. decoder_upsample1 was measured on the single-frame forward,
  // where the V2V stage is a chain of 47-us launches: 2.089 ms with the branch against 2.059 without (medium 3.68 /
  // 3.59) -- each of these kernels already spreads over the chip, the two chains only take turns.  The side-stream
  // machinery was removed after that measurement: a plan is one chain on the caller's stream.
  // The output fold (csrc/conv3d_out_fold.hip; JH_V2V_FOLD=0: off): skip_res1 and decoder_res1 stop behind their second
  // convolutions and the output layer applies both closing passes on load -- `skip` and `d1` then hold raw tensors and
  // two norm_apply launches are gone.  Decided from (J, G) and the knob, never from T.
  const bool fold = v2v_fold_applies(J, G);
  size_t st_skip = 0, st_dec = 0;
  if (res_block(pm, e + "skip_res1.", 2 * J, f1, nullptr, &skip, -1, fold ? &st_skip : nullptr)) return 1;
  if (new_act(T, Gq, Gq, Gq, 4 * J, &e0)) return 1;
  if (add_conv(pm, conv_desc(3, 2, 2, 0, 2 * J, 4 * J), e + "encoder_pool1.block.0.weight",
               e + "encoder_pool1.block.0.bias", false, f1, e0, nullptr, true, &st)) return 1;
  if (res_block(pm, e + "mid_res.", 4 * J, e0, nullptr, &e1, (long)st)) return 1;
  if (new_act(T, Gh, Gh, Gh, 2 * J, &u0)) return 1;
  if (add_conv(pm, deconv3d_k2s2_desc(4 * J, 2 * J), e + "decoder_upsample1.block.0.weight",
               e + "decoder_upsample1.block.0.bias", true, e1, u0, nullptr, true, &st)) return 1;
  const size_t st_u0 = st;
  if (res_block(pm, e + "decoder_res1.", 2 * J, u0, skip.p, &d1, (long)st, fold ? &st_dec : nullptr)) return 1;   // ... + res1
  if (new_act(T, Gh, Gh, Gh, J, &output)) return 1;
  if (!fold) {
    if (add_conv(pm, conv_desc(3, 1, 1, 0, 2 * J, J), pre + "output_layer.weight",
                 pre + "output_layer.bias", false, d1, output, nullptr, false, nullptr)) return 1;
    return finish();
  }
  // the layer's weights as add_conv packs them (the MFMA form's Plain layout, at every precision); the launch is the fold's
  const float *w = nullptr, *b = nullptr;
  if (get(pm, pre + "output_layer.weight", (size_t)2 * J * J, &w)) return 1;
  if (get(pm, pre + "output_layer.bias", J, &b)) return 1;
  ConvUse use;
  use.desc = conv_desc(3, 1, 1, 0, 2 * J, J);
  use.has_bias = true; use.precision = precision; use.in_px = d1.Cp;
  layers_.emplace_back();
  const ConvLayer* layer = &layers_.back();
  if (make_conv_layer(use, w, b, Gh, Gh, Gh, &layers_.back())) return 1;
  JH_REQUIRE(layer->choice.form == ConvForm::Mfma && layer->choice.layout == WeightLayout::Plain,
             "output fold: the 1 x 1 x 1 layer's weight layout");
  bytes_ += layer->device_bytes();
  // algorithmic work of the layer; bytes: four reads of the padded 2 J-channel tensors, one write of the output, the weights
  const double vox = (double)T * d1.pixels();
  char nm[96];
  snprintf(nm, sizeof nm, "conv3d_k1s1fold_%dx%d@%d", 2 * J, J, Gh);
  push(nm, 2.0 * vox * 2 * J * J, 4.0 * (vox * (4.0 * d1.Cp + output.Cp) + 2.0 * J * J),
       [this, layer, d1, u0, skip, f1, st_dec, st_u0, st_skip](hipStream_t s) {
    return launch_conv3d_out_fold(layer->w, d1, sc(st_dec), u0.p, sc(st_u0), skip.p, sc(st_skip), f1.p, output, s);
  });
  return finish();
}

}  // namespace jh
