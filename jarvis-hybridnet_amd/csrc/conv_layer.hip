// One convolution layer (conv_layer.h): the rules that pick its kernel form, its weight packing, its launch.  Host only.
#include <cstdlib>
#include "conv_layer.h"
#include "conv_mfma.h"
#include "conv3d_wino.h"

namespace jh {

// A knob as it stands NOW (not JH_ENV_KNOB, which reads once per process): layers of both settings in one process.
static int knob_now(const char* name, int unset) {
  const char* e = getenv(name);
  return e ? atoi(e) : unset;
}

// The weight layout of the MFMA form.
static WeightLayout conv_weight_layout(const ConvUse& u) {
  const ConvDesc& d = u.desc;
  const int cin_p = cpad(d.cin), cout_p = cpad(d.cout), cout_p16 = round_up(d.cout, 16);
  // stride-2 3D convs: two taps per 16-byte weight word (conv_mfma.h, TAPPAIR)
  if (d.nd == 3 && d.k == 3 && d.stride == 2 && d.ostride == 1) return WeightLayout::TapPaired;
  if (d.nd == 2 && d.ostride > 1) {
    // ConvTranspose2d k4 s2 p1 without statistics and gate: the window form of csrc/deconv4.hip, one 2 x 2 convolution
    // over the 4 cout_p columns (output sub-position, channel) of a window.  JH_DECONV4_WINDOW=0: the four-parity
    // forms; =2: also the layers of 8 column blocks in either form, cout 25..32 (the measurement knob of DESIGN 3.8a)
    const int wmode = knob_now("JH_DECONV4_WINDOW", 1);
    if (!u.want_stats && u.gate == ConvGate::None && wmode != 0 && deconv4_window_eligible(cin_p, cout_p, wmode >= 2))
      return WeightLayout::Window;
    // the fused four-parity kernel reads both operands 16 bytes at a time: two 8-channel steps per lane word
    if (deconv4_eligible(cin_p, cout_p16)) return WeightLayout::ChannelPaired;
  }
  return WeightLayout::Plain;
}

ConvChoice choose_conv(const ConvUse& u) {
  const ConvDesc& d = u.desc;
  const bool ungated = u.gate == ConvGate::None;
  // a ConvTranspose2d k4 s2 p1 as the heads use it: no bias, no fused statistics, no gate
  const bool bare_deconv2d = d.nd == 2 && d.ostride > 1 && u.transposed && !u.has_bias && !u.want_stats && ungated;
  const int in_px = u.in_px ? u.in_px : cpad(d.cin);
  const auto form = [](ConvForm f, int wino_variant = 0) { return ConvChoice{f, WeightLayout::Plain, wino_variant}; };
  // one output channel (the CenterDetect head): vector-ALU kernel instead of a 16-wide MFMA column block, at every
  // precision
  if (bare_deconv2d && d.cout == 1) return form(ConvForm::DeconvC1);
  // 3x3x3 stride-1 convs (the V2V residual blocks) run as Winograd F(2x2,3x3) x direct z (JH_WINO=0: direct), in the
  // persistent wave-specialised form (JH_WINO_PW=0: one role per workgroup); at precision bf16x3 and above, the same
  // layers on the bf16 matrix cores with split operands
  if (d.nd == 3 && d.k == 3 && d.stride == 1 && d.ostride == 1 && d.phase[0].pad[2] == 1 && !u.transposed && ungated &&
      knob_now("JH_WINO", 1) != 0)
    return form(u.precision >= 1 ? ConvForm::WinoBf16x3 : ConvForm::Wino, knob_now("JH_WINO_PW", 1) != 0 ? 4 : 0);
  // ... and the keypoint head's ConvTranspose2d
  if (bare_deconv2d && u.precision >= 1 && deconv4_bf16x3_eligible(d.cout)) return form(ConvForm::Deconv4Bf16x3);
  // ... and the dense k x k convolutions with a generic split-bf16 kernel (no gate; the 3-channel network input, one
  // float4 per pixel, keeps its own kernels).  Level 1 (bf16x3) takes the 3D one (V2V's stride-2 front convolution);
  // the 2D trunk convolutions only at level 2 (bf16x3_wide): split, they move the keypoints by up to 7.6e-4 mm on the
  // fixture cases, which leaves no margin under the 1e-3 mm bar.
  if (!u.transposed && ungated && conv_bf16x3_eligible(d) && in_px == cpad(d.cin) &&
      (u.precision == 2 || (u.precision == 1 && d.nd == 3)))
    return form(ConvForm::ConvBf16x3);
  return ConvChoice{ConvForm::Mfma, conv_weight_layout(u), 0};
}

bool conv_takes_box(const ConvChoice& c) { return c.form == ConvForm::Mfma && c.layout == WeightLayout::Window; }

bool head_roi_knob() { return knob_now("JH_HEAD_ROI", 1) != 0; }

bool head_box_allowed(HeatCall kind, bool consensus, bool sharded, bool want_res1) {
  return kind == HeatCall::Forward && !consensus && !sharded && !want_res1;
}

std::string conv_choice_name(const ConvChoice& c) {
  static const char* const forms[] = {"mfma", "wino", "wino_bf16x3", "conv_bf16x3", "deconv4_bf16x3", "deconv_c1"};
  static const char* const layouts[] = {"", "_paired", "_tappair", "_window"};
  return std::string(forms[(int)c.form]) + (c.form == ConvForm::Mfma ? layouts[(int)c.layout] : "");
}

std::vector<float> taps_major(const float* w, int channels, int taps, int Cp) {
  std::vector<float> wt((size_t)taps * Cp, 0.f);
  for (int c = 0; c < channels; ++c)
    for (int t = 0; t < taps; ++t) wt[(size_t)t * Cp + c] = w[(size_t)c * taps + t];
  return wt;
}

ConvLayer::~ConvLayer() {
  free_conv_weights(&w);
  if (wino_tiles) (void)hipFree(wino_tiles);
}

int make_conv_layer(const ConvUse& u, const float* w_host, const float* b_host, int D, int H, int W, ConvLayer* out) {
  const ConvDesc& d = u.desc;
  JH_REQUIRE(w_host && (b_host != nullptr) == u.has_bias, "conv layer weights / bias");
  const ConvChoice c = out->choice = choose_conv(u);
  const int in_px = u.in_px ? u.in_px : cpad(d.cin);
  out->desc = d;
  switch (c.form) {
    case ConvForm::DeconvC1: {
      const std::vector<float> wt = taps_major(w_host, d.cin, 16, in_px);
      out->w.phase_stride = wt.size() / d.nphase;
      return upload_conv_weights(wt.data(), wt.size() * sizeof(float), nullptr, 0, &out->w);
    }
    case ConvForm::ConvBf16x3: return pack_conv_bf16x3_weights(d, w_host, b_host, &out->w);
    case ConvForm::Deconv4Bf16x3: return pack_deconv4_bf16x3_weights(d.cin, d.cout, w_host, &out->w);
    case ConvForm::WinoBf16x3: return pack_bf16x3_weights(d.cin, d.cout, w_host, b_host, &out->w);
    case ConvForm::Mfma: return pack_conv_weights(d, w_host, b_host, u.transposed, c.layout, &out->w);
    case ConvForm::Wino: break;
  }
  if (pack_wino_weights(d.cin, d.cout, w_host, b_host, &out->w)) return 1;
  // Winograd on a volume with remainder strips (e.g. 36^3 / 18^3 of the shipped 72^3 grid): the persistent kernel's
  // tables, built and uploaded here, when the layer is made -- never under stream capture (csrc/conv3d_wino.h)
  const std::vector<int> tt = wino_tables(D, H, W, in_px);
  if (tt.empty()) return 0;
  out->table_bytes = tt.size() * sizeof(int);
  JH_CHECK_HIP(hipMalloc(&out->wino_tiles, out->table_bytes));
  JH_CHECK_HIP(hipMemcpy(out->wino_tiles, tt.data(), out->table_bytes, hipMemcpyHostToDevice));
  return 0;
}

int ConvLayer::launch(const Act& x, const Act& y, const float* gate, double* stats, const InNorm& in, const SeGate* se,
                      hipStream_t s, const int4* box) const {
  JH_REQUIRE(choice.form == ConvForm::Mfma || (!gate && !(se && se->pool)), "only the MFMA form takes a gate");
  JH_REQUIRE(!box || takes_box(), "only the window form takes a box");
  switch (choice.form) {
    case ConvForm::DeconvC1: return launch_deconv_c1(x, in.stats, in.inv, in.act, w.w, y, s);
    case ConvForm::ConvBf16x3: return launch_conv_bf16x3(desc, w, x, y, stats, s, &in);
    case ConvForm::Deconv4Bf16x3: return launch_deconv4_bf16x3(w, x, y, s, &in);
    case ConvForm::WinoBf16x3: return launch_conv3d_bf16x3(w, x, y, stats, s, &in);
    case ConvForm::Wino: return launch_conv3d_wino(w, x, y, stats, s, &in, choice.wino_variant, wino_tiles);
    case ConvForm::Mfma: return launch_conv(desc, w, x, y, gate, stats, s, &in, se, box);
  }
  JH_REQUIRE(false, "conv form");
}

std::string ConvLayer::profile_name(int out_w) const {
  if (choice.form == ConvForm::DeconvC1) return "deconv_k4s2T_c1";
  const ConvDesc& d = desc;
  const bool up = d.ostride > 1;
  const bool split = choice.form == ConvForm::WinoBf16x3 || choice.form == ConvForm::ConvBf16x3;
  const char* tag = up ? (choice.form == ConvForm::Deconv4Bf16x3 ? "Tbf16x3" : "T")
                       : (split ? "bf16x3" : (choice.form == ConvForm::Wino ? "wino" : ""));
  char nm[96];
  snprintf(nm, sizeof nm, "conv%dd_k%ds%d%s_%dx%d@%d", d.nd, up ? (d.nd == 2 ? 4 : 2) : d.k, up ? 2 : d.stride, tag,
           d.cin, d.cout, out_w);
  return nm;
}

}  // namespace jh
